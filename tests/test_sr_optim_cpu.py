"""The host side of optim.AdamW(stochastic_rounding=True) without a kernel: the constructor's checks, the kinds
and the batching of a step, stream ids that stay put, the seed in the state dict, loading plain-bf16 state into
a stochastic-rounding optimizer and back, the refusal of f32 master state, and the entries' argument checks."""
import copy

import pytest
import torch

from tests.test_master_weights_cpu import _aligned, _hand_state, _params

BF16, F32 = torch.bfloat16, torch.float32


def test_constructor_validation():
    from picotron_amd.optim import AdamW
    p = [torch.nn.Parameter(torch.zeros(8, dtype=BF16))]
    with pytest.raises(ValueError, match="one or the other"):
        AdamW(p, stochastic_rounding=True, master_weights=True)
    with pytest.raises(ValueError, match="stochastic_rounding=True"):   # the adjusted text names both ways out
        AdamW(p, use_main_grad=True)
    for seed in (-1, 1 << 64, 0.5):
        with pytest.raises(ValueError, match="sr_seed"):
            AdamW(p, stochastic_rounding=True, sr_seed=seed)
    a = AdamW(p)
    assert a.stochastic_rounding is False and "sr_seed" not in a.param_groups[0]   # the default is what it was
    b = AdamW(p, stochastic_rounding=True)
    assert b.stochastic_rounding is True and b.param_groups[0]["sr_seed"] == 0 and not b.master_weights
    c = AdamW(p, stochastic_rounding=True, sr_seed=(1 << 64) - 1, use_main_grad=True, max_grad_norm=1.0)
    assert (c.param_groups[0]["sr_seed"], c.use_main_grad, c.max_grad_norm) == ((1 << 64) - 1, True, 1.0)


def _mixed():
    shapes = [64, 24, 40, 16, 32]
    ps = [torch.nn.Parameter(_aligned(n, BF16)) for n in shapes]
    ps.append(torch.nn.Parameter(_aligned(8, BF16, off=1)))     # an unaligned view
    pf = torch.nn.Parameter(_aligned(12, F32))                  # an f32 parameter: the ordinary path
    return ps, pf


def test_batches_kinds_and_stream_ids():
    from picotron_amd import optim
    ps, pf = _mixed()
    opt = optim.AdamW([dict(params=ps[:2] + [pf]), dict(params=ps[2:], sr_seed=77)], lr=1e-3, stochastic_rounding=True,
                      sr_seed=5, use_main_grad=True)
    position = {id(p): i for i, p in enumerate(ps[:2] + [pf] + ps[2:])}   # what state_dict() numbers them
    for p in ps[:2] + [ps[5], pf]:
        p.grad = _aligned(p.numel(), p.dtype)
    ps[2].main_grad = _aligned(40, F32)
    ps[3].main_grad = _aligned(16, F32)
    ps[3].grad = _aligned(16, BF16)                             # ignored: main_grad wins
    # ps[4] has no gradient this step: it keeps its stream id all the same
    got = {}
    for gi, group in enumerate(opt.param_groups):
        for sc, kind, items in opt._batches(group):
            key = (gi, kind, items[0][1].dtype)
            assert key not in got
            got[key] = (sc, items)
    assert sorted(got, key=str) == sorted([(0, optim.SR_MULTI, BF16), (0, optim.SINGLE, F32), (1, optim.SR_MULTI, F32),
                                           (1, optim.SR_SINGLE, BF16)], key=str)
    for (gi, kind, _), (sc, items) in got.items():
        if kind == optim.SINGLE:
            assert "seed" not in sc and len(items[0]) == 4 and items[0][0] is pf
            continue
        assert sc["seed"] == (5, 77)[gi] and sc["step"] == 1 and isinstance(sc["step"], int)
        for p, g, m, v, stream in items:
            assert stream == position[id(p)] and isinstance(stream, int)
            assert m.dtype == v.dtype == BF16 and "master_param" not in opt.state[p]   # the plain recipe's state
    assert [it[0] is p for it, p in zip(got[(1, optim.SR_MULTI, F32)][1], (ps[2], ps[3]))] == [True, True]
    assert got[(1, optim.SR_MULTI, F32)][1][1][1] is ps[3].main_grad
    assert got[(1, optim.SR_SINGLE, BF16)][1][0][0] is ps[5] and ps[5].data_ptr() % 16 == 2
    # second step: ps[4] joins one step behind, in a batch of its own, with the id of its position
    ps[4].grad = _aligned(32, BF16)
    steps = sorted((sc["step"], [it[4] for it in items]) for sc, kind, items in opt._batches(opt.param_groups[1])
                   if kind == optim.SR_MULTI and items[0][1].dtype == BF16)
    assert steps == [(1, [position[id(ps[4])]])]
    f32 = [(sc["step"], [it[4] for it in items]) for sc, kind, items in opt._batches(opt.param_groups[1])
           if kind == optim.SR_MULTI and items[0][1].dtype == F32]
    assert f32 == [(3, [position[id(ps[2])], position[id(ps[3])]])]


def test_seed_travels_in_the_state_dict():
    from picotron_amd.optim import AdamW
    params = _params()
    opt = AdamW(params, stochastic_rounding=True, sr_seed=1234567890123)
    sd = copy.deepcopy(opt.state_dict())
    assert sd["param_groups"][0]["sr_seed"] == 1234567890123
    other = AdamW(params, stochastic_rounding=True, sr_seed=1)
    other.load_state_dict(sd)
    assert other.param_groups[0]["sr_seed"] == 1234567890123
    for p in params:
        p.grad = torch.zeros_like(p)
    seeds = {sc.get("seed") for sc, kind, _ in other._batches(other.param_groups[0]) if kind.startswith("sr")}
    assert seeds == {1234567890123}


def test_load_state_dict_across_modes():
    from picotron_amd import optim
    params = _params()
    plain, sr = optim.AdamW(params), optim.AdamW(params, stochastic_rounding=True, sr_seed=9)
    bf16_state = {"state": _hand_state(params, False), "param_groups": copy.deepcopy(plain.state_dict()["param_groups"])}
    sr.load_state_dict(copy.deepcopy(bf16_state))            # plain -> SR: the state as it is
    for i, p in enumerate(params):
        st = sr.state[p]
        assert st["step"].item() == 2.0 and "master_param" not in st
        for k in ("exp_avg", "exp_avg_sq"):
            assert st[k].dtype == p.dtype and torch.equal(st[k], bf16_state["state"][i][k])
    for p in params:
        p.grad = torch.zeros_like(p)
    for sc, kind, _ in sr._batches(sr.param_groups[0]):      # the saved groups had no seed: the constructor's holds
        if kind.startswith("sr"):
            assert sc["seed"] == 9 and sc["step"] == 3
    sr_state = copy.deepcopy(sr.state_dict())                # SR -> plain
    plain.load_state_dict(sr_state)
    assert plain.state[params[0]]["exp_avg"].dtype == BF16 and plain.state[params[0]]["step"].item() == 3.0
    kinds = sorted(kind for _, kind, _ in plain._batches(plain.param_groups[0]))
    assert not any(k.startswith("sr") for k in kinds)
    f32_state = {"state": _hand_state(params, True), "param_groups": copy.deepcopy(sr_state["param_groups"])}
    fresh = optim.AdamW(params, stochastic_rounding=True)
    with pytest.raises(ValueError, match="master_weights=True"):   # f32 master state is refused as it is today
        fresh.load_state_dict(f32_state)
    assert len(fresh.state) == 0


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """PT_EINVAL (-1) from the host-side checks: no device is touched (there is none here)."""
    from picotron_amd import _C
    lib = _C.load_library()
    sc = (0.999, 0.1, 0.999, 0.001, 0.03, 1e-8, -3e-4)
    one = 16   # any non-null address: the checks return before it is read
    assert lib.pt_adamw_sr_step_multi(one, one, 1, 1, 0, *sc, 1, 2, 0, None) == -1              # step 0
    assert lib.pt_adamw_sr_step_multi(one, one, 1, 1, 2, *sc, 1, 2, 1, None) == -1              # grad dtype
    assert lib.pt_adamw_sr_step_multi(None, one, 1, 1, 0, *sc, 1, 2, 1, None) == -1
    assert lib.pt_adamw_sr_step_multi(one, one, 1, 0, 1, *sc, 1, 2, 1, None) == 0               # nothing to do
    assert lib.pt_adamw_sr_step_multi(one, one, 1, 0, 1, *sc, 1, 2, 0, None) == -1              # ... but checked first
    assert lib.pt_adamw_sr_step_multi_clip(one, one, 1, 1, 0, *sc, 1, 2, 1, None, 1.0, None, None) == -1
    assert lib.pt_adamw_sr_step_multi_clip(one, one, 1, 1, 0, *sc, 1, 2, 1, one, 0.0, None, None) == -1
    assert lib.pt_adamw_sr_step(one, one, one, one, 8, 0, *sc, 1, 2, 1, 1 << 30, None) == -1    # stream id
    assert lib.pt_adamw_sr_step(one, one, one, one, 8, 0, *sc, 1, 2, 1, -1, None) == -1
    assert lib.pt_adamw_sr_step(one, one, one, one, 8, 0, *sc, 1, 2, 0, 5, None) == -1
    assert lib.pt_adamw_sr_step(one, one, one, one, 8, 2, *sc, 1, 2, 1, 5, None) == -1
    assert lib.pt_adamw_sr_step(one, one, one, one, 0, 1, *sc, 1, 2, 1, 5, None) == 0
    assert lib.pt_adamw_sr_step_clip(one, one, one, one, 8, 0, *sc, 1, 2, 1, 5, one, 0.0, None, None) == -1
    assert lib.pt_grad_sq_sr_multi(one, one, 1, 1, 5, 1.0, 0, one, one, None) == -1
    assert lib.pt_grad_sq_sr_multi(one, one, 1, 1, 0, 1.0, 0, None, one, None) == -1
    assert lib.pt_sr_cast_bf16(one, one, 8, 1, 2, 1, 0, 3, None) == -1
    assert lib.pt_sr_cast_bf16(one, one, 8, 1, 2, 0, 0, 0, None) == -1
    assert lib.pt_sr_cast_bf16(one, one, 8, 1, 2, 1, 1 << 30, 0, None) == -1
    assert lib.pt_sr_cast_bf16(one, one, 0, 1, 2, 1, 0, 2, None) == 0
