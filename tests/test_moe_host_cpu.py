"""Host side of the mixture-of-experts layer (CPU): the capacity formula, the Muon / AdamW parameter
split, every refusal, the wrappers' argument checks and the ABI's return codes -- nothing here
touches a device."""
import types

import pytest
import torch

from picotron_amd import process_group_manager as pgm


def _config(**over):
    d = dict(hidden_size=128, intermediate_size=128, num_attention_heads=2, num_key_value_heads=2, vocab_size=256,
             rms_norm_eps=1e-5, rope_theta=10000.0, num_hidden_layers=2, max_position_embeddings=64)
    d.update(over)
    return types.SimpleNamespace(**d)


@pytest.fixture
def cpu_model(monkeypatch):
    monkeypatch.setenv("DEVICE", "cpu")

    def build(**over):
        from picotron_amd import model as M
        return M.Llama(_config(**over))
    return build


@pytest.fixture
def grid(monkeypatch):
    """A process grid of the given sizes without torch.distributed."""
    def set_(tp=1, cp=1, pp=1, dp=1):
        m = types.SimpleNamespace(tp_world_size=tp, cp_world_size=cp, pp_world_size=pp, dp_world_size=dp,
                                  cp_dp_world_size=cp * dp, tp_rank=0, cp_rank=0, pp_rank=0, dp_rank=0,
                                  pp_is_first_stage=True, pp_is_last_stage=pp == 1, tp_group=None, cp_group=None,
                                  cp_dp_group=None)
        monkeypatch.setattr(pgm, "process_group_manager", m)
        return m
    return set_


def test_moe_capacity_values_and_clamps():
    from picotron_amd.kernels import moe_capacity
    assert moe_capacity(4096, 8, 2, 1.25) == 1280
    assert moe_capacity(4096, 64, 8, 1.25) == 640
    assert moe_capacity(1000, 8, 2, 1.0) == 256            # ceil64(250)
    assert moe_capacity(192, 8, 2, 1.0) == 64              # the lower clamp: max(64, ceil64(48))
    assert moe_capacity(16, 128, 8, 1.25) == 64            # both clamps meet: ceil64(16) = 64
    assert moe_capacity(192, 8, 2, 4.0) == 192             # cf = E / k: ceil64(T), dropless
    assert moe_capacity(192, 8, 2, 100.0) == 192           # the upper clamp
    assert moe_capacity(1000, 8, 2, 4.0) == 1024           # ceil64(T)
    assert moe_capacity(1, 1, 1, 1.0) == 64
    assert moe_capacity(4096, 60, 4, 1.25) == 384          # ceil(341.33) = 342 -> 384
    for T, E, k, cf in ((1000, 8, 2, 1.25), (63, 60, 4, 1.0), (4096, 128, 8, 2.0)):
        C = moe_capacity(T, E, k, cf)
        assert C % 64 == 0 and 64 <= C <= -(-T // 64) * 64
    for bad in ((0, 8, 2, 1.0), (10, 8, 9, 1.0), (10, 8, 0, 1.0), (10, 8, 2, 0.0), (10, 8, 2, float("inf"))):
        with pytest.raises(ValueError):
            moe_capacity(*bad)


def test_split_muon_params_moe_and_dense(cpu_model):
    from picotron_amd import optim
    moe = cpu_model(num_experts=4, num_experts_per_tok=2, moe_intermediate_size=64)
    names = {id(p): n for n, p in moe.named_parameters()}
    mats, rest = optim.split_muon_params(moe)
    mat_names, rest_names = [names[id(p)] for p in mats], [names[id(p)] for p in rest]
    for layer in range(2):
        for e in range(4):
            for w in ("gate_proj", "up_proj", "down_proj"):
                assert f"decoder_layers.{layer}.mlp.experts.{e}.{w}.weight" in mat_names
        assert f"decoder_layers.{layer}.mlp.router.weight" in rest_names
        assert f"decoder_layers.{layer}.post_attention_layernorm.weight" in rest_names
    assert len(mats) + len(rest) == len(list(moe.parameters()))
    assert all(p.dim() == 2 for p in mats)
    assert tuple(moe.decoder_layers[0].mlp.experts[0].gate_proj.weight.shape) == (64, 128)
    assert tuple(moe.decoder_layers[0].mlp.router.weight.shape) == (4, 128)
    # dense: exactly the seven projections per layer, as before
    dense = cpu_model()
    dn = {id(p): n for n, p in dense.named_parameters()}
    mats, rest = optim.split_muon_params(dense)
    assert [dn[id(p)] for p in mats] == [n for n, _ in dense.named_parameters()
                                         if "decoder_layers." in n and "norm" not in n]
    assert len(mats) == 14 and [dn[id(p)] for p in rest] == [n for n, p in dense.named_parameters()
                                                               if not ("decoder_layers." in n and "norm" not in n)]


def test_dense_config_builds_the_dense_layer(cpu_model):
    from picotron_amd import model as M
    for over in ({}, {"num_experts": 0}, {"num_experts": None}):
        m = cpu_model(**over)
        assert all(type(l.mlp) is M.MLP for l in m.decoder_layers)
        assert not any("router" in n or "experts" in n for n, _ in m.named_parameters())
    moe = cpu_model(num_experts=8)
    mlp = moe.decoder_layers[1].mlp
    assert isinstance(mlp, M.MoE) and (mlp.num_experts, mlp.top_k, mlp.capacity_factor, mlp.norm_topk_prob) == (8, 2, 1.25, True)
    assert tuple(mlp.experts[7].down_proj.weight.shape) == (128, 128)   # moe_intermediate_size defaults to intermediate_size
    over = cpu_model(num_experts=8, num_experts_per_tok=4, moe_capacity_factor=2.0, norm_topk_prob=False).decoder_layers[0].mlp
    assert (over.top_k, over.capacity_factor, over.norm_topk_prob) == (4, 2.0, False)
    for bad in ({"num_experts": 129}, {"num_experts": 4, "num_experts_per_tok": 5}, {"num_experts": 16, "num_experts_per_tok": 9},
                {"num_experts": 4, "moe_intermediate_size": 96}):
        with pytest.raises(ValueError):
            cpu_model(**bad)


@pytest.mark.parametrize("sizes,word", [({"tp": 2}, "tensor"), ({"cp": 2}, "context"), ({"pp": 2}, "pipeline")])
def test_moe_refuses_model_parallel_grids(cpu_model, grid, sizes, word):
    grid(**sizes)
    with pytest.raises(NotImplementedError, match=word):
        cpu_model(num_experts=4)
    cpu_model()   # dense models build on the same grid


def test_parallel_engines_refuse_a_moe_model(cpu_model, grid):
    from picotron_amd import train
    from picotron_amd.context_parallel import context_parallel
    from picotron_amd.pipeline_parallel.pipeline_parallel import PipelineParallel
    from picotron_amd.tensor_parallel.tensor_parallel import apply_tensor_parallel
    grid()
    moe = cpu_model(num_experts=4)
    with pytest.raises(NotImplementedError, match="mixture-of-experts"):
        apply_tensor_parallel(moe)           # tensor and sequence parallelism (one entry enables both)
    with pytest.raises(NotImplementedError, match="mixture-of-experts"):
        PipelineParallel(moe, moe.model_config)
    with pytest.raises(NotImplementedError, match="mixture-of-experts"):
        train.GraphedTrainStep(moe, None, "cpu")
    grid(cp=2)
    with pytest.raises(NotImplementedError, match="mixture-of-experts"):
        context_parallel.apply_context_parallel(moe)
    grid()
    assert context_parallel.apply_context_parallel(moe) is moe   # cp = 1 changes nothing


def test_train_step_keyword_defaults_and_checks(cpu_model, grid):
    import inspect
    from picotron_amd import train
    sig = inspect.signature(train.train_step)
    assert sig.parameters["moe_aux_loss"].default == 0.0
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="moe_aux_loss"):
            train.train_step(None, types.SimpleNamespace(grad_acc_steps=1), "cpu", moe_aux_loss=bad)
    inner = types.SimpleNamespace(decoder_layers=[], moe_aux_loss=None)
    assert train._moe_module(inner) is inner
    assert train._moe_module(types.SimpleNamespace(module=inner)) is inner   # through a DP wrapper


def test_wrapper_argument_checks_come_before_the_device():
    """Wrong shapes / dtypes / sizes raise ValueError before any library call."""
    from picotron_amd import kernels as K
    bf = torch.bfloat16
    with pytest.raises(ValueError):
        K.moe_route(torch.zeros(4, 8), 2)                                   # not bf16 / not on a device
    with pytest.raises(ValueError):
        K.moe_plan(torch.zeros(4, 2, dtype=torch.int64), 8, 64)             # idx must be int32
    with pytest.raises(ValueError):
        K.moe_dispatch(torch.zeros(4, 64, dtype=bf), torch.zeros(64, dtype=torch.int32), 2)
    with pytest.raises(ValueError):
        K.moe_combine(torch.zeros(64, 64, dtype=bf), torch.zeros(4, 2, dtype=torch.int32))
    with pytest.raises(ValueError):
        K.moe_combine_bwd(torch.zeros(4, 64, dtype=bf), torch.zeros(64, 64, dtype=bf), torch.zeros(4, 2, dtype=torch.int32),
                          torch.zeros(64, dtype=torch.int32), torch.zeros(4, 2))
    with pytest.raises(ValueError):
        K.moe_route_bwd(torch.zeros(4, 2), torch.zeros(4, 8), torch.zeros(4, 2, dtype=torch.int32),
                        torch.zeros(8, dtype=torch.int32))


def test_abi_argument_errors_return_codes_without_a_device():
    """Every pt_moe_* entry validates on the host: PT_EINVAL -1, PT_EALIGN -2, PT_EUNSUPPORTED -3.
    The pointers are never dereferenced (dummy, suitably aligned addresses)."""
    from picotron_amd import _C
    lib = _C.load_library()
    P, ODD = 0x10000, 0x10002
    EINVAL, EALIGN, EUNSUP = -1, -2, -3
    assert lib.pt_moe_plan_block() == 1024
    assert lib.pt_moe_route_workspace(4096, 8) == 2 * 256 * 8
    assert lib.pt_moe_route_workspace(0, 8) == EINVAL and lib.pt_moe_route_workspace(16, 129) == EUNSUP
    assert lib.pt_moe_plan_workspace(4096, 8, 2) == 9 * 8
    assert lib.pt_moe_plan_workspace(4096, 8, 9) == EUNSUP

    def route(logits=P, ldl=8, T=16, E=8, k=2, idx=P):
        return lib.pt_moe_route(logits, ldl, T, E, k, 1, idx, P, P, P, P, P, None)
    assert route(logits=None) == EINVAL and route(idx=None) == EINVAL and route(T=0) == EINVAL and route(k=0) == EINVAL
    assert route(E=129, ldl=129) == EUNSUP and route(k=9, E=16, ldl=16) == EUNSUP and route(k=3, E=2) == EUNSUP
    assert route(ldl=7) == EINVAL

    def plan(idx=P, T=16, E=8, k=2, C=64, ws=P):
        return lib.pt_moe_plan(idx, T, E, k, C, P, P, ws, None)
    assert plan(idx=None) == EINVAL and plan(ws=None) == EINVAL and plan(C=0) == EINVAL and plan(T=-1) == EINVAL
    assert plan(E=200) == EUNSUP and plan(k=9, E=16) == EUNSUP and plan(T=2 ** 31, k=1) == EUNSUP

    def dispatch(x=P, ldx=64, xe=P, ldxe=64, T=16, k=2, R=512, H=64):
        return lib.pt_moe_dispatch(x, ldx, P, xe, ldxe, T, k, R, H, None)
    assert dispatch(x=None) == EINVAL and dispatch(R=0) == EINVAL and dispatch(H=0) == EINVAL
    assert dispatch(H=72, ldx=72, ldxe=72) == EUNSUP and dispatch(k=9) == EUNSUP
    assert dispatch(x=ODD) == EALIGN and dispatch(ldx=68) == EALIGN and dispatch(ldxe=32) == EALIGN

    def combine(ye=P, slot=P, res=None, ldr=0, y=P, ldy=64, H=64, k=2):
        return lib.pt_moe_combine(ye, 64, slot, None, res, ldr, y, ldy, 16, k, 512, H, None)
    assert combine(ye=None) == EINVAL and combine(slot=None) == EINVAL and combine(y=None) == EINVAL
    assert combine(H=100) == EUNSUP and combine(k=9) == EUNSUP
    assert combine(y=ODD) == EALIGN and combine(res=ODD, ldr=64) == EALIGN and combine(res=P, ldr=60) == EALIGN

    def combine_bwd(dy=P, gate=P, dye=P, lddye=64, dgate=P, H=64):
        return lib.pt_moe_combine_bwd(dy, 64, P, 64, P, P, gate, dye, lddye, dgate, 16, 2, 512, H, None)
    assert combine_bwd(dy=None) == EINVAL and combine_bwd(gate=None) == EINVAL and combine_bwd(dgate=None) == EINVAL
    assert combine_bwd(H=32) == EUNSUP and combine_bwd(dye=ODD) == EALIGN and combine_bwd(lddye=66) == EALIGN

    def route_bwd(dgate=P, dl=P, ldl=8, T=16, E=8, k=2):
        return lib.pt_moe_route_bwd(dgate, P, P, P, None, 1, dl, ldl, T, E, k, None)
    assert route_bwd(dgate=None) == EINVAL and route_bwd(dl=None) == EINVAL and route_bwd(T=0) == EINVAL
    assert route_bwd(E=130, ldl=130) == EUNSUP and route_bwd(k=9, E=16, ldl=16) == EUNSUP and route_bwd(ldl=4) == EINVAL
