"""Every measurement switch's non-default form (picotron_amd/switches.py) through the whole GPU path,
against the CPU oracle: a 2-layer Llama (T = 2 x 1024 tokens, H 1024, I 4096 or 2048, d 64, GQA 16 / 8
heads) at shapes where the switched launches are taken -- the fused RoPE / SwiGLU epilogues and the
split-K halves forced on by their thresholds (tools/switch_kernels.py traces, per case, the launches
that differ: profiles/r05/switch_kernels_r05k.txt) -- with loss, logits and every parameter gradient within north_star's bf16
tolerance (norm-relative 2e-2), as test_model_gpu.test_llama_loss_and_grads_match_oracle.  The
oracle (oracle/picotron_oracle.py) runs once for all cases on the same bf16 weights and tokens.

Each case also asserts that its form was taken (FORM): the kernel calls functional.py makes are recorded
(tests/_model_ref.py, names and result kinds only) and compared with the pinned table -- which calls must
and must not appear, how many dual launches ran, how many dX came back as split-K halves -- so that a
threshold drifting away from these shapes fails here instead of silently testing the default path twice.
A switch that acts below that layer is pinned where it acts: the pure decision function the launch calls
(kernels.hq_form / wgrad_ksplit / swiglu_dx_ksplit) at this model's shapes, or the library's variant
register for the native switches.  The per-element check of every stage under these forms is
tests/test_model_stages_gpu.py."""
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import picotron_oracle as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TOL = 2e-2
# two shapes: "a" (I 4096: the split-K halves, the few-tile forms at M = 2048) and "b" (I 2048: the
# SwiGLU-backward dX in K-slices needs (T / 256) (I / 256) <= 64)
CONFIGS = {"a": dict(S=1024, H=1024, I=4096, nh=16, nkv=8, V=2048), "b": dict(S=1024, H=1024, I=2048, nh=16, nkv=8, V=2048)}
# the switch forms the default path does not take (switches.DEFAULTS holds the defaults), each as the
# overrides on top of FORCE; the order is that of tools/switch_kernels.py, which traces what each changes
CASES = [("a", {})] + [("a", {k: v}) for k, v in (
    ("fuse", 0), ("norm_defer", 0), ("ce_stats", 0), ("dual_qkv", 0), ("dual_gu", 0), ("gu_splitk", 0), ("ksplit", 0),
    ("splitk2", 0), ("dual", 0), ("norm_splitk", 0), ("fuse_delta", 0), ("attn_pair", 0), ("gemm_mix", 0))] + [
    ("b", {}), ("b", dict(swiglu_splitk=0)),
]
# (gemm_kh, the K-halves tile 14 for 256x128 launches at K >= 4096, is not reached at shapes this
# small: test_kernels_gpu.py covers gemm_kh = 0 on the launch directly)
# thresholds lowered so that these shapes take the fused / split launches the switches choose between
FORCE = dict(rope_fuse_min_tiles=0, swiglu_fuse_min_tiles=0, splitk2_min=2048)


# case id -> what the recorder must show: must / never (call names), count {name: n}, parts (dX results that are
# split-K halves, 2 layers), decide (a callable on (kernels, T, H, I, V) that must hold inside the override),
# native (the library's variant register must read 0), spy (the number of kernels.attn_delta calls: the separate
# delta pass that attn_bwd makes itself when fuse_delta = 0)
FORM = {
    "a-default": dict(must=("linear_fwd_rope", "linear_swiglu_fwd", "linear_ce_stats", "cross_entropy_loss_lse_stats",
                            "rmsnorm_colsum_batch"),
                      never=("rope_", "swiglu_fwd", "swiglu_bwd", "linear_dgrad_swiglu", "linear_wgrad_grouped"),
                      count={"linear_dgrad_dual": 6}, parts=4, spy=0,
                      decide=lambda K, T, H, I, V: K.hq_form([(V, H, T)]) == 1 and K.wgrad_ksplit([(H, I, T)]) == 4),
    "a-fuse0": dict(must=("rope_", "swiglu_fwd", "swiglu_bwd"), never=("linear_fwd_rope", "linear_swiglu_fwd"),
                    count={"rope_": 4, "linear_dgrad_dual": 4}, parts=4),
    "a-norm_defer0": dict(never=("rmsnorm_colsum_batch",), count={"linear_dgrad_dual": 6}, parts=4),
    "a-ce_stats0": dict(must=("cross_entropy_loss_lse",), never=("linear_ce_stats", "cross_entropy_loss_lse_stats"), parts=4),
    "a-dual_qkv0": dict(count={"linear_dgrad_dual": 4, "linear_wgrad_grouped": 2}, parts=2),
    "a-dual_gu0": dict(never=("linear_wgrad_grouped", "_splitk_halves"), count={"linear_dgrad_dual": 4, "linear_wgrad": 3}, parts=2),
    "a-gu_splitk0": dict(never=("_splitk_halves",), count={"linear_dgrad_dual": 6}, parts=2),
    "a-ksplit0": dict(count={"linear_dgrad_dual": 6}, parts=4,
                      decide=lambda K, T, H, I, V: K.hq_form([(V, H, T)]) == 0 and K.wgrad_ksplit([(H, I, T)]) == 1),
    "a-splitk20": dict(count={"linear_dgrad_dual": 6}, parts=0),
    "a-dual0": dict(must=("linear_dgrad_swiglu",), never=("linear_dgrad_dual",), count={"linear_wgrad_grouped": 6}, parts=0),
    "a-norm_splitk0": dict(count={"linear_dgrad_dual": 6}, parts=0),
    "a-fuse_delta0": dict(spy=2, parts=4),
    "a-attn_pair0": dict(native="attn_pair", parts=4),
    "a-gemm_mix0": dict(native="gemm_mix", parts=4),
    "b-default": dict(count={"linear_dgrad_dual": 6}, parts=4, decide=lambda K, T, H, I, V: K.swiglu_dx_ksplit(T, I, H) == 2),
    "b-swiglu_splitk0": dict(count={"linear_dgrad_dual": 6}, parts=4, decide=lambda K, T, H, I, V: K.swiglu_dx_ksplit(T, I, H) == 1),
}


def assert_form(cid, rec, cfg, T, deltas):
    """The recorded calls are those of the form `cid` (FORM); called inside the case's override."""
    from picotron_amd import _C
    from picotron_amd import kernels as K
    want = FORM[cid]
    names = rec.names()
    for n in want.get("must", ()):
        assert n in names, f"{cid}: no K.{n} call was recorded: the form was not taken ({sorted(set(names))})"
    for n in want.get("never", ()):
        assert n not in names, f"{cid}: K.{n} was called: the form was not taken"
    for n, k in want.get("count", {}).items():
        assert names.count(n) == k, f"{cid}: {names.count(n)} K.{n} calls, the form makes {k}"
    parts = sum(1 for c in rec.calls if c.name in ("linear_dgrad_dual", "linear_dgrad") and c.result == "Parts")
    assert parts == want["parts"], f"{cid}: {parts} dX came back as split-K halves, the form makes {want['parts']}"
    assert not any(c.name == "linear_dgrad_dual" and c.result == "NoneType" for c in rec.calls), f"{cid}: a dual launch was refused"
    if "decide" in want:
        assert want["decide"](K, T, cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size), f"{cid}: the launch's decision function"
    if "spy" in want:
        assert deltas == want["spy"], f"{cid}: {deltas} separate attn_delta passes, the form makes {want['spy']}"
    if "native" in want:
        assert _C.load_library().pt_get_variant(want["native"].encode()) == 0, f"{cid}: the library's variant register"


def case_id(case):
    cfg, kw = case
    return cfg + ("-" + "-".join(f"{k}{v}" for k, v in kw.items()) if kw else "-default")


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def build(name):
    """The 2-layer Llama of shape `name` on cuda:0 (bf16, seeded) and its tokens."""
    import os
    os.environ.update(DEVICE="cuda", LOCAL_RANK="0", CONTEXT_PARALLEL="0", FLASH_ATTEN="1")
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.model import Llama
    pgm.setup_process_group_manager(1, 1, 1, 1)
    torch.manual_seed(0)
    c = CONFIGS[name]
    cfg = types.SimpleNamespace(hidden_size=c["H"], intermediate_size=c["I"], num_attention_heads=c["nh"],
                                num_key_value_heads=c["nkv"], vocab_size=c["V"], rms_norm_eps=1e-5, rope_theta=10000.0,
                                num_hidden_layers=2, max_position_embeddings=c["S"])
    with torch.device("cuda"):
        model = Llama(cfg)
    model.to(BF)
    ids = torch.randint(0, c["V"], (2, c["S"] + 1), generator=torch.Generator().manual_seed(3))
    return model, cfg, ids


@pytest.fixture(scope="module")
def models():
    import os
    old = {k: os.environ.get(k) for k in ("DEVICE", "LOCAL_RANK", "CONTEXT_PARALLEL", "FLASH_ATTEN")}
    cache = {}

    def get(name):
        if name not in cache:
            model, cfg, ids = build(name)
            p = {k: v.detach().float().cpu().requires_grad_(True) for k, v in model.named_parameters()}
            cos, sin = O.get_cos_sin(ids.shape[1] - 1, cfg.hidden_size // cfg.num_attention_heads, base=10000.0)
            lr = O.llama_forward(ids[:, :-1], p, dict(vars(cfg)), cos.float(), sin.float(),
                                 norm=O.rmsnorm_flash_semantics)
            loss_r = F.cross_entropy(lr.reshape(-1, cfg.vocab_size), ids[:, 1:].reshape(-1))
            loss_r.backward()
            cache[name] = (model, cfg, ids, dict(loss=loss_r.item(), logits=lr.detach(),
                                                 grads={k: v.grad for k, v in p.items()}))
        return cache[name]
    yield get
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def run(model, cfg, ids):
    from picotron_amd import functional as FN   # (FN.K is looked up at call time: a recorder placed over it is used)
    model.zero_grad(set_to_none=True)
    logits = model(ids[:, :-1].cuda())
    loss = FN.cross_entropy(logits.view(-1, cfg.vocab_size), ids[:, 1:].reshape(-1).cuda())
    loss.backward()
    torch.cuda.synchronize()
    return loss.float().item(), logits.detach().float().cpu(), {n: q.grad.float().cpu() for n, q in model.named_parameters()}


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_switch_form_matches_oracle(models, case):
    from picotron_amd import switches
    name, over = case
    model, cfg, ids, ref = models(name)
    assert all(k in switches.DEFAULTS for k in over)
    from tests import _model_ref as M
    assert set(FORM) == {case_id(c) for c in CASES}
    from picotron_amd import kernels as K
    deltas, real = [], K.attn_delta
    K.attn_delta = lambda *a, **kw: (deltas.append(1), real(*a, **kw))[1]
    try:
        with switches.override(**FORCE, **over), M.recording(clone=False) as rec:
            loss, logits, grads = run(model, cfg, ids)
            assert_form(case_id(case), rec, cfg, ids.shape[0] * (ids.shape[1] - 1), len(deltas))
    finally:
        K.attn_delta = real
    assert abs(loss - ref["loss"]) < TOL * abs(ref["loss"]), (over, loss, ref["loss"])
    assert rel(logits, ref["logits"]) < TOL, over
    for n, g in grads.items():
        assert rel(g, ref["grads"][n]) < TOL, (over, n)
