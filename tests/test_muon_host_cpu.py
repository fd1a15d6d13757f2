"""Muon's host side without a GPU: the parameter split, the refusals, the learning-rate adjustment,
the grouping plan and the ABI declarations."""
import os
import re
import types

import pytest
import torch

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _toy(qk_norm=False):
    from picotron_amd.model import Llama
    cfg = types.SimpleNamespace(hidden_size=128, intermediate_size=192, num_attention_heads=2, num_key_value_heads=1,
                                vocab_size=96, rms_norm_eps=1e-5, rope_theta=10000.0, num_hidden_layers=2,
                                max_position_embeddings=32)
    if qk_norm:
        cfg.qk_norm = True
    return Llama(cfg)


@pytest.fixture(autouse=True)
def _grid(monkeypatch):
    from picotron_amd import process_group_manager as pgm
    monkeypatch.setenv("DEVICE", "cpu")   # the model's RoPE tables
    pgm.setup_process_group_manager(1, 1, 1, 1)
    yield
    pgm.setup_process_group_manager(1, 1, 1, 1)


def test_split_by_name():
    from picotron_amd.optim import split_muon_params
    model = _toy()
    names = {id(p): n for n, p in model.named_parameters()}
    matrices, rest = split_muon_params(model)
    got = sorted(names[id(p)] for p in matrices)
    want = sorted(f"decoder_layers.{i}.{m}.weight" for i in range(2) for m in
                  ("attention.q_proj", "attention.k_proj", "attention.v_proj", "attention.out_proj", "mlp.gate_proj",
                   "mlp.up_proj", "mlp.down_proj"))
    assert got == want
    rest_names = sorted(names[id(p)] for p in rest)
    assert "embedding.weight" in rest_names and "final_proj.weight" in rest_names and "final_norm.weight" in rest_names
    assert all("layernorm" in n or n in ("embedding.weight", "final_proj.weight", "final_norm.weight")
               for n in rest_names), rest_names
    assert len(matrices) + len(rest) == len(names) and all(p.dim() == 2 for p in matrices)


def test_split_keeps_qk_norm_weights_on_adamw():
    from picotron_amd.optim import split_muon_params
    model = _toy(qk_norm=True)
    names = {id(p): n for n, p in model.named_parameters()}
    norm_names = [n for n in names.values() if "q_norm" in n or "k_norm" in n]
    matrices, rest = split_muon_params(model)
    rest_names = {names[id(p)] for p in rest}
    assert all(n in rest_names for n in norm_names)
    assert not any("norm" in names[id(p)] for p in matrices)


def test_refusals():
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.optim import Muon, MuonAdamW
    with pytest.raises(ValueError, match="2D"):
        Muon([torch.nn.Parameter(torch.zeros(8, dtype=BF))])
    with pytest.raises(ValueError, match="2D"):
        Muon([torch.nn.Parameter(torch.zeros(2, 4, 4, dtype=BF))])
    with pytest.raises(NotImplementedError, match="f32"):
        Muon([torch.nn.Parameter(torch.zeros(8, 8))])
    with pytest.raises(ValueError):
        Muon([torch.nn.Parameter(torch.zeros(8, 8, dtype=torch.float16))])
    with pytest.raises(ValueError):
        Muon([torch.nn.Parameter(torch.zeros(8, 8, dtype=BF))], adjust_lr_fn="other")
    shard = torch.nn.Parameter(torch.zeros(8, 8, dtype=BF))
    shard.tensor_model_parallel = True
    Muon([shard])   # tp = 1: the mark means nothing
    pgm.current().tp_world_size = 2
    try:
        with pytest.raises(NotImplementedError, match="tensor-parallel"):
            Muon([shard])
        Muon([torch.nn.Parameter(torch.zeros(8, 8, dtype=BF))])   # a replicated matrix is fine
    finally:
        pgm.setup_process_group_manager(1, 1, 1, 1)
    with pytest.raises(ValueError, match="max_grad_norm"):
        MuonAdamW(([shard], []), adamw=dict(max_grad_norm=1.0))


def test_constructor_matches_torch():
    from picotron_amd.optim import Muon
    p = torch.nn.Parameter(torch.zeros(8, 16, dtype=BF))
    ours, theirs = Muon([p]), torch.optim.Muon([torch.nn.Parameter(torch.zeros(8, 16, dtype=BF))])
    a, b = ours.param_groups[0], theirs.param_groups[0]
    assert sorted(a) == sorted(b)
    for k in a:
        if k != "params":
            assert a[k] == b[k], k
    theirs.load_state_dict(ours.state_dict())
    ours.load_state_dict(theirs.state_dict())


def test_param_groups_are_concatenated():
    from picotron_amd.optim import MuonAdamW
    model = _toy().to(BF)
    opt = MuonAdamW(model, muon=dict(lr=0.02), adamw=dict(lr=3e-4))
    assert [g["lr"] for g in opt.param_groups] == [0.02, 3e-4]
    for g in opt.param_groups:   # an LR scheduler's write reaches the owners
        g["lr"] *= 0.5
    assert opt.muon.param_groups[0]["lr"] == 0.01 and opt.adamw.param_groups[0]["lr"] == 1.5e-4
    sd = opt.state_dict()
    assert sorted(sd) == ["adamw", "muon"]
    opt.load_state_dict(sd)


@pytest.mark.parametrize("fn", [None, "original", "match_rms_adamw"])
def test_lr_ratio_against_torch(fn):
    from torch.optim._muon import _adjust_lr
    from picotron_amd import kernels as K
    from tests import _muon_ref as M
    for shape in ((64, 64), (2048, 8192), (8192, 2048), (72, 40), (512, 2048)):
        want = _adjust_lr(0.02, fn, torch.Size(shape))
        assert 0.02 * K.muon_lr_ratio(fn, shape) == pytest.approx(want, rel=1e-15)
        assert M.lr_ratio(fn, shape) == K.muon_lr_ratio(fn, shape)
    with pytest.raises(ValueError):
        K.muon_lr_ratio("other", (8, 8))


def test_group_plan_is_pure():
    from picotron_amd import kernels as K
    shapes = [(64, 128)] * 5 + [(128, 64)] + [(64, 128)] * 4 + [(256, 256)] * 4
    plan = K.muon_group_plan(shapes)
    assert plan == K.muon_group_plan(list(shapes))
    assert plan == [((64, 128), [0, 1, 2, 3]), ((64, 128), [4, 6, 7, 8]), ((64, 128), [9]), ((128, 64), [5]),
                    ((256, 256), [10, 11, 12, 13])]
    assert all(1 <= len(idx) <= K.MUON_GROUP for _, idx in plan)
    assert sorted(i for _, idx in plan for i in idx) == list(range(len(shapes)))
    assert K.muon_group_plan([]) == []


def test_abi_declares_and_binds_the_muon_entries():
    from picotron_amd import _C
    txt = open(os.path.join(ROOT, "include", "picotron_hip.h")).read()
    declared = sorted(set(re.findall(r"^int\s+(pt_muon_\w+)\s*\(", txt, flags=re.M)))
    assert declared == sorted(n for n in _C.SIGNATURES if n.startswith("pt_muon_"))
    assert len(declared) == 8
    lib = _C.load_library()
    for n in declared:
        assert hasattr(lib, n), n
    assert lib.pt_muon_block_chunks() == 2048
    # argument errors come back as codes before anything is launched
    assert lib.pt_muon_momentum(None, None, 0, 0, 0, 0.05, 0.95, 1, None, None, None) == -1
    assert lib.pt_muon_poly(None, None, None, 0, 64, 1.0, 1.0, 1.0, None) == -1
    assert lib.pt_muon_apply(None, None, 0, 0, 1.0, 0.1, None) == -1
