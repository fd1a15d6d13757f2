"""Host side of the sigmoid router (CPU): model.MoE's config checks, the C entries' refusals, and the
default configuration still taking the softmax path."""
import types

import pytest
import torch


def _moe(monkeypatch, **over):
    monkeypatch.setenv("DEVICE", "cpu")
    from picotron_amd import model as M
    d = dict(hidden_size=128, intermediate_size=128, num_experts=8, num_experts_per_tok=2)
    d.update(over)
    return M.MoE(types.SimpleNamespace(**d))


@pytest.mark.parametrize("over", [
    dict(n_group=3, topk_group=1),                          # n_group does not divide num_experts
    dict(n_group=2, topk_group=3),                          # topk_group > n_group
    dict(n_group=4, topk_group=1, num_experts_per_tok=3),   # k > topk_group * num_experts / n_group
    dict(n_group=8, topk_group=8),                          # groups of one expert
    dict(moe_scoring_func="tanh"),
    dict(moe_scoring_func="softmax", n_group=2, topk_group=1),
])
def test_invalid_router_configs_raise(monkeypatch, over):
    with pytest.raises(ValueError, match="n_group|moe_scoring_func"):
        _moe(monkeypatch, **{"moe_scoring_func": "sigmoid", **over})


def test_default_config_passes_no_router_variant(monkeypatch):
    from picotron_amd import functional as FN
    seen = []
    monkeypatch.setattr(FN.MoEFunction, "apply", lambda *a: (seen.append(a), (a[0], torch.zeros(())))[1])
    plain = _moe(monkeypatch)
    x = torch.zeros(2, 4, 128)
    plain(x, x)
    assert len(seen[0]) == 11 and seen[0][10] is None and not list(plain.buffers())
    sig = _moe(monkeypatch, moe_scoring_func="sigmoid", n_group=2, topk_group=1, routed_scaling_factor=2.5,
               moe_bias_update_rate=1e-3, n_shared_experts=2)
    r = sig.router_variant()
    assert (r.n_group, r.topk_group, r.scale) == (2, 1, 2.5) and r.bias is sig.e_score_correction_bias and r.load is sig.load
    assert sig.eval().router_variant().load is None   # evaluation does not steer the bias
    assert set(sig.state_dict()) >= {"e_score_correction_bias", "shared_experts.down_proj.weight"} and "load" not in sig.state_dict()
    assert tuple(sig.shared_experts.gate_proj.weight.shape) == (256, 128)
    assert sig.to(torch.bfloat16).e_score_correction_bias.dtype == torch.float32 and sig.router.weight.dtype == torch.bfloat16


def test_abi_refusals_without_a_device():
    from picotron_amd import _C
    lib = _C.load_library()
    P, EINVAL, EUNSUP = 0x10000, -1, -3

    def route(logits=P, ldl=64, T=16, E=64, k=6, G=8, Kg=3, idx=P, bias=P, load=None):
        return lib.pt_moe_route_sigmoid(logits, ldl, bias, T, E, k, G, Kg, 1, 2.5, idx, P, P, P, P, load, P, None)
    assert route(logits=None) == EINVAL and route(idx=None) == EINVAL and route(T=0) == EINVAL
    assert route(G=0) == EINVAL and route(Kg=0) == EINVAL and route(ldl=63) == EINVAL
    assert route(E=256, ldl=256) == EUNSUP and route(k=9) == EUNSUP                  # the preamble's limits
    assert route(G=7) == EUNSUP and route(G=32, Kg=16) == EUNSUP and route(Kg=9) == EUNSUP
    assert route(G=64, Kg=64) == EUNSUP and route(E=16, ldl=16, G=8, Kg=2, k=6) == EUNSUP and route(G=16, Kg=1, k=5) == EUNSUP
    assert route(E=129, ldl=8) == EUNSUP                                             # the limits before ldl

    def bwd(dgate=P, gate=P, dl=P, ldl=64, T=16, E=64, k=6):
        return lib.pt_moe_route_sigmoid_bwd(dgate, P, P, gate, P, None, 1, 2.5, dl, ldl, T, E, k, None)
    assert bwd(dgate=None) == EINVAL and bwd(gate=None) == EINVAL and bwd(dl=None) == EINVAL and bwd(k=0) == EINVAL
    assert bwd(E=130, ldl=130) == EUNSUP and bwd(k=9) == EUNSUP and bwd(ldl=32) == EINVAL
    assert lib.pt_moe_bias_update(None, P, 8, 1e-3, None) == EINVAL and lib.pt_moe_bias_update(P, None, 8, 1e-3, None) == EINVAL
    assert lib.pt_moe_bias_update(P, P, 0, 1e-3, None) == EINVAL and lib.pt_moe_bias_update(P, P, 129, 1e-3, None) == EUNSUP
