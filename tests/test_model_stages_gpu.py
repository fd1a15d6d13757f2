"""The autograd layer (picotron_amd/functional.py) stage by stage on the GPU: every kernel call of a forward +
backward is recorded (tests/_model_ref.py), and every stage of the model's math is checked per element, from
the production values of its inputs, under the bound its kernel's own conformance kit derives -- no
tolerance of this file's, no slack factor.  Fused launches are replayed as their separate kernels on the
recorded inputs and compared by bits first.

a. default path   1- and 2-layer Llama at test_model_gpu's tiny shape (B 2, S 128, H 256, I 512, heads 4 / 2 of
                  64, V 512); heads 2 / 1 of 128; LlamaRMSNorm mode (FLASH_ATTEN=0); qk_norm; a document band;
                  V 515 (the lm_head off the 64-grid, the CE padded with -inf columns).  loss / 4, ~5 % of the
                  targets ignored, norm weights away from 1.
b. switch forms   the forms reachable at the tiny shape (fuse, norm_defer, ce_stats = 0: FORMS_TINY) and, at
                  the smallest shape found at which the dual and split-K launches are taken (MID: B 2, S 256,
                  H 1024, I 1024, heads 16 / 8 of 64, V 1024, one layer), the default and every other form of
                  test_switch_forms_gpu.CASES (FORMS_MID; ce_stats and norm_defer at the tiny shape).  ksplit,
                  fuse_delta, attn_pair and gemm_mix act below the calls functional.py makes: the recorded K calls
                  are the default's, and the form is pinned where it acts -- kernels.swiglu_dx_ksplit(512, 1024,
                  1024) = 2 -> 1 under ksplit = 0 (the down dX then leaves the K-sliced reduce pass for the fused
                  epilogue: dgu_sliced False; ksplit's other decisions, kernels.hq_form and wgrad_ksplit of the
                  weight gradients, are 0 and 1 either way at T = 512: K-slices need 512 rows each), a spy on
                  kernels.attn_delta (one separate pass per layer under fuse_delta = 0, none otherwise), the
                  library's variant register for attn_pair / gemm_mix -- and every stage is checked under it.
                  What limits MID: pt_gemm_dual tiles every problem by
                  256 x 256 with each group's tile count a multiple of 8 (kernels.dual_fits) -- T I / 65536 for
                  the down dX, T H / 65536 for the gate|up and q|k|v dX, so T = 512 needs H = I = 1024 -- and
                  the split-K halves need K / 2 >= splitk2_min (lowered to 512 here: H / 2 for the forward
                  halves).  Each case first asserts the K calls that make the form (pinned in the tables), then
                  checks every stage; at MID the float64 references take about a second per layer.
c. nodes alone    AttentionFunction, MLPFunction, RMSNormFunction, AddRMSNormFunction, LinearFunction and
                  LMHeadFunction outside the fused layer: a transposed-view x, a dy that is a slice of a wider
                  buffer, need_dx false, a frozen weight in each position.
d. CE stash       with ce_stats on: CE on the returned logits, on logits.clone(), on the first of two lm_head
                  calls, after an unrelated lm_head call, on the logits' storage modified in place; which
                  forward ran is asserted from the recorder, the
                  CE stages must hold and inv_count be exact; reductions mean / sum / none, incoming gradients
                  other than 1.
e. table          test_zz_worst_ratio_table prints the worst |got - ref| / bound per form and role.

Worst |got - ref| / bound per role measured on the MI355X, over every form of this file, and the form it was
seen in (the summary test_zz_worst_ratio_table prints after the per-form table; a bf16 store reaches its half
ulp, so ratios near 1 are the bound at work, and 0.000 is a comparison by bits):
    role                     worst   in form
    a                        0.952   node attention
    ce_scale                 0.000   ce modified_in_place none
    dW                       0.960   node lm_head
    dW_d                     0.966   L2
    dW_emb                   0.000   mid gemm_mix0
    dW_g                     0.957   node mlp
    dW_g/dW_u.g              0.966   L2
    dW_g/dW_u.u              0.973   d128
    dW_lm                    0.986   llama_norm
    dW_o                     0.963   tiny ce_stats0
    dW_qkv.k                 0.974   V515
    dW_qkv.q                 0.956   docmask
    dW_qkv.v                 0.965   L2
    dW_u                     0.968   node mlp
    dgu.dg                   0.998   mid gemm_mix0
    dgu.du                   0.994   mid gemm_mix0
    dh1                      0.916   tiny norm_defer0
    dh2                      0.852   docmask
    dhf                      0.972   qk_norm
    dhh                      0.953   node mlp
    dlogits                  0.996   tiny ce_stats0
    do                       0.963   L2
    dqkv.dqkv.k              0.995   qk_norm
    dqkv.dqkv.q              0.993   qk_norm
    dqkv.dwkn                0.820   qk_norm
    dqkv.dwqn                0.552   qk_norm
    dqkv_rot                 0.996   qk_norm
    dqkv_unrot.dk            0.557   V515
    dqkv_unrot.dq            0.592   node attention
    dqkv_unrot.dv            0.515   L2
    dw                       0.926   node norm mode 0
    dx                       0.994   node add_norm mode 1
    dx.dw1                   0.960   tiny norm_defer0
    dx.dx                    0.996   mid gemm_mix0
    dxf/dwf.dwf              0.937   tiny ce_stats0
    dxf/dwf.dxf              0.996   L2
    dz.dw2                   0.948   d128
    dz.dz                    0.996   tiny ce_stats0
    gu                       0.955   node mlp
    h1/rstd1.h1              0.996   tiny ce_stats0
    h1/rstd1.rstd1           0.129   L2
    hf/rstdf.hf              0.996   d128
    hf/rstdf.rstdf           0.141   qk_norm
    hh                       0.988   node mlp
    logits                   0.951   docmask
    loss.inv_count           0.000   ce modified_in_place sum
    loss.loss                0.931   ce clone none
    m                        0.931   node mlp
    o/lse.lse                0.047   mid gemm_mix0
    o/lse.o                  0.489   mid gemm_mix0
    out                      0.981   V515
    qk                       0.996   qk_norm
    qk_normed/rstd_qk.qk_normed.k 0.994   qk_norm
    qk_normed/rstd_qk.qk_normed.q 0.995   qk_norm
    qk_normed/rstd_qk.rstd_qk.k 0.121   qk_norm
    qk_normed/rstd_qk.rstd_qk.q 0.120   qk_norm
    qkv                      0.996   L2
    qkv_raw                  0.952   L2
    row_lse                  0.083   tiny ce_stats0
    rstd                     0.145   node norm mode 1
    x0                       0.000   mid gemm_mix0
    y                        0.994   node norm mode 0
    z/h2/rstd2.h2            0.996   mid gemm_mix0
    z/h2/rstd2.rstd2         0.139   tiny ce_stats0
    z/h2/rstd2.z             0.000   mid gemm_mix0
"""
import types

import pytest
import torch

from tests import _model_ref as M
from tests import _row_ref as R

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
GA = 4


def cfg_of(layers=1, H=256, I=512, nh=4, nkv=2, V=512, S=128, **kw):
    return types.SimpleNamespace(hidden_size=H, intermediate_size=I, num_attention_heads=nh, num_key_value_heads=nkv,
                                 vocab_size=V, rms_norm_eps=1e-5, rope_theta=10000.0, num_hidden_layers=layers,
                                 max_position_embeddings=S, **kw)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("DEVICE", "cuda")
    monkeypatch.setenv("LOCAL_RANK", "0")
    monkeypatch.setenv("CONTEXT_PARALLEL", "0")
    monkeypatch.setenv("FLASH_ATTEN", "1")
    from picotron_amd import process_group_manager as pgm
    pgm.setup_process_group_manager(1, 1, 1, 1)
    torch.manual_seed(0)


def K_():
    from picotron_amd import kernels
    return kernels


def build(cfg, seed=0):
    from picotron_amd.model import Llama
    torch.manual_seed(seed)
    with torch.device("cuda"):
        model = Llama(cfg)
    model.to(BF)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "norm" in n:   # norm weights away from 1: a dropped weight must show
                p.copy_(1 + 0.1 * torch.randn_like(p))
    return model


def batch(cfg, B=2, seed=1):
    g = torch.Generator().manual_seed(seed)
    S = cfg.max_position_embeddings
    ids = torch.randint(0, cfg.vocab_size, (B, S + 1), generator=g)
    tgt = ids[:, 1:].reshape(-1).clone()
    tgt[torch.randperm(tgt.numel(), generator=g)[:max(1, tgt.numel() // 20)]] = -100   # ~5 % ignored
    return ids[:, :-1].contiguous(), tgt


def run_recorded(model, cfg, ids, tgt, ga=GA, document_ids=None):
    from picotron_amd import functional as FN
    with M.recording() as rec:
        kw = {} if document_ids is None else dict(document_ids=document_ids.cuda())
        logits = model(ids.cuda(), **kw)
        loss = FN.cross_entropy(logits.view(-1, cfg.vocab_size), tgt.cuda()) / ga
        loss.backward()
        torch.cuda.synchronize()
    return rec


def check_run(rec, model, cfg, B, form, ga=GA, mask=None, only=None):
    gloss = torch.ones((), dtype=BF) / ga
    layers, hc, h, ce_name = M.extract_model(K_(), rec.calls, model, B, cfg.max_position_embeddings, gloss, mask)
    return M.check_model(layers, hc, h, form, only), ce_name


# ------------------------------------------------------------------------------ a. the default path
DEFAULT_CASES = {
    "L1": dict(layers=1), "L2": dict(layers=2), "d128": dict(layers=1, nh=2, nkv=1), "llama_norm": dict(layers=1),
    "qk_norm": dict(layers=1, qk_norm=True), "docmask": dict(layers=1), "V515": dict(layers=1, V=515),
}


@pytest.mark.parametrize("case", list(DEFAULT_CASES))
def test_default_path_every_stage(monkeypatch, case):
    if case == "llama_norm":
        monkeypatch.setenv("FLASH_ATTEN", "0")
    cfg = cfg_of(**DEFAULT_CASES[case])
    model = build(cfg)
    ids, tgt = batch(cfg)
    doc = mask = None
    if case == "docmask":   # documents of uneven length, a boundary inside a 64-key tile and at a tile edge
        S = cfg.max_position_embeddings
        doc = torch.zeros(2, S, dtype=torch.int64)
        doc[0, 37:] = 1
        doc[0, 64:] = 2
        doc[1, 100:] = 1
        mask = (doc[:, :, None] == doc[:, None, :])[:, None] & torch.tril(torch.ones(S, S, dtype=torch.bool))
    rec = run_recorded(model, cfg, ids, tgt, document_ids=doc)
    if case == "llama_norm":   # the switch of the norm flavour was read: mode 1, not L1 again
        from picotron_amd.model import LlamaRMSNorm
        assert isinstance(model.final_norm, LlamaRMSNorm) and isinstance(model.decoder_layers[0].input_layernorm, LlamaRMSNorm)
        assert M.layer_config(model.decoder_layers[0], 2, cfg.max_position_embeddings).mode == 1 and M.head_config(model).mode == 1
        assert all(c.arg(3, "mode") == 1 for c in rec.calls if c.name == "rmsnorm_fwd")
    res, ce_name = check_run(rec, model, cfg, 2, case, mask=mask)
    assert ce_name == ("cross_entropy_loss_lse" if case == "V515" else "cross_entropy_loss_lse_stats")
    names = rec.names()
    if case == "qk_norm":
        assert "qk_norm_rope_fwd" in names and "qk_norm_bwd" in names and "linear_fwd_rope" not in names
    if case == "docmask":
        assert all(c.kwargs.get("band") is not None for c in rec.calls if c.name in ("attn_fwd", "attn_bwd"))
    qk = case == "qk_norm"
    c0 = types.SimpleNamespace(wqn=True if qk else None)
    want = {f"L{i} " + ("/".join(s.produces) or "dW_qkv") for i in range(cfg.num_hidden_layers) for s in M.layer_stages(c0)}
    want |= {"/".join(s.produces) for s in M.HEAD_FWD + M.HEAD_BWD}
    assert set(res) == want, sorted(want ^ set(res))   # every stage, forward and backward, was checked


# ------------------------------------------------------------------------------ b. the switch forms
FORCE = dict(rope_fuse_min_tiles=0, swiglu_fuse_min_tiles=0, splitk2_min=512)
# form -> (overrides, K calls that must be recorded, K calls that must not)
FORMS_TINY = {
    "fuse0": (dict(fuse=0), ("rope_", "swiglu_fwd", "swiglu_bwd"), ("linear_fwd_rope", "linear_swiglu_fwd", "linear_dgrad_swiglu")),
    "norm_defer0": (dict(norm_defer=0), (), ("rmsnorm_colsum_batch",)),
    "ce_stats0": (dict(ce_stats=0), ("cross_entropy_loss_lse",), ("linear_ce_stats", "cross_entropy_loss_lse_stats")),
}
MID = dict(layers=1, H=1024, I=1024, nh=16, nkv=8, V=1024, S=256)
FORMS_MID = {
    "default": (dict(), ("linear_dgrad_dual", "linear_fwd_rope", "linear_swiglu_fwd", "rmsnorm_colsum_batch"),
                ("linear_dgrad_swiglu", "linear_wgrad_grouped", "swiglu_bwd")),
    "swiglu_splitk0": (dict(swiglu_splitk=0), ("linear_dgrad_dual",), ("linear_dgrad_swiglu", "linear_wgrad_grouped")),
    "dual0": (dict(dual=0), ("linear_dgrad_swiglu", "linear_wgrad_grouped"), ("linear_dgrad_dual",)),
    "dual_qkv0": (dict(dual_qkv=0), ("linear_wgrad_grouped", "linear_dgrad_dual"), ("linear_dgrad_swiglu",)),
    "dual_gu0": (dict(dual_gu=0), ("linear_dgrad_dual",), ("linear_wgrad_grouped", "_splitk_halves")),
    "gu_splitk0": (dict(gu_splitk=0), ("linear_dgrad_dual",), ("linear_wgrad_grouped", "_splitk_halves")),
    "norm_splitk0": (dict(norm_splitk=0), ("linear_dgrad_dual",), ("linear_wgrad_grouped",)),
    "splitk20": (dict(splitk2=0), ("linear_dgrad_dual",), ("linear_wgrad_grouped",)),
    "fuse0": (dict(fuse=0), ("rope_", "swiglu_fwd", "swiglu_bwd", "linear_dgrad_dual"), ("linear_fwd_rope", "linear_swiglu_fwd")),
    # the switches that act below functional.py's calls: the same K calls as the default, the form pinned where it acts
    "ksplit0": (dict(ksplit=0), ("linear_dgrad_dual",), ("linear_dgrad_swiglu", "linear_wgrad_grouped")),
    "fuse_delta0": (dict(fuse_delta=0), ("linear_dgrad_dual",), ("linear_dgrad_swiglu", "linear_wgrad_grouped")),
    "attn_pair0": (dict(attn_pair=0), ("linear_dgrad_dual",), ("linear_dgrad_swiglu", "linear_wgrad_grouped")),
    "gemm_mix0": (dict(gemm_mix=0), ("linear_dgrad_dual",), ("linear_dgrad_swiglu", "linear_wgrad_grouped")),
}
# the forms whose down dX (SwiGLU backward) does not run in K-slices at MID: swiglu_dx_ksplit(512, 1024, 1024) is 2 by
# default and 1 with ksplit = 0 or swiglu_splitk = 0; without the dual launch or the fusion there is no such form
MID_UNSLICED = ("swiglu_splitk0", "ksplit0", "dual0", "fuse0")
# the native switches: the library's variant register must read 0 inside the case
MID_NATIVE = {"attn_pair0": "attn_pair", "gemm_mix0": "gemm_mix"}
# which dX roles must be a split-K pair (f32 halves handed to the norm backward) in each MID form
MID_PAIRS = {"default": ("dh2", "dh1"), "swiglu_splitk0": ("dh2", "dh1"), "dual0": (), "dual_qkv0": ("dh2",), "dual_gu0": ("dh1",),
             "gu_splitk0": ("dh1",), "norm_splitk0": (), "splitk20": (), "fuse0": ("dh2", "dh1"),
             "ksplit0": ("dh2", "dh1"), "fuse_delta0": ("dh2", "dh1"), "attn_pair0": ("dh2", "dh1"), "gemm_mix0": ("dh2", "dh1")}


@pytest.fixture(scope="module")
def mid():
    cfg = cfg_of(**MID)
    return cfg, build(cfg), batch(cfg)


def _assert_form(names, must, must_not, form):
    for n in must:
        assert n in names, f"form {form}: expected a K.{n} call; recorded {sorted(set(names))}"
    for n in must_not:
        assert n not in names, f"form {form}: K.{n} must not be called; recorded {sorted(set(names))}"


@pytest.mark.parametrize("form", list(FORMS_TINY))
def test_switch_form_stages_tiny(form):
    from picotron_amd import switches
    over, must, must_not = FORMS_TINY[form]
    cfg = cfg_of(layers=1)
    model = build(cfg)
    ids, tgt = batch(cfg)
    with switches.override(**over):
        rec = run_recorded(model, cfg, ids, tgt)
        _assert_form(rec.names(), must, must_not, form)
        check_run(rec, model, cfg, 2, "tiny " + form)


@pytest.mark.parametrize("form", list(FORMS_MID))
def test_switch_form_stages_mid(mid, form):
    from picotron_amd import switches
    over, must, must_not = FORMS_MID[form]
    cfg, model, (ids, tgt) = mid
    model.zero_grad(set_to_none=True)
    K = K_()
    deltas, real = [], K.attn_delta
    with switches.override(**FORCE, **over):
        K.attn_delta = lambda *a, **kw: (deltas.append(1), real(*a, **kw))[1]
        try:
            rec = run_recorded(model, cfg, ids, tgt)
        finally:
            K.attn_delta = real
        _assert_form(rec.names(), must, must_not, form)
        # fuse_delta = 0: attn_bwd makes the separate delta pass itself (kernels.attn_delta), once per layer
        assert len(deltas) == (1 if form == "fuse_delta0" else 0), f"form {form}: {len(deltas)} separate attn_delta passes"
        T = ids.numel()
        assert K.swiglu_dx_ksplit(T, cfg.intermediate_size, cfg.hidden_size) == (1 if form in MID_UNSLICED[:2] else 2)
        if form in MID_NATIVE:
            from picotron_amd import _C
            assert _C.load_library().pt_get_variant(MID_NATIVE[form].encode()) == 0, f"form {form}: the variant register"
        gloss = torch.ones((), dtype=BF) / GA
        layers, hc, h, _ = M.extract_model(K_(), rec.calls, model, 2, cfg.max_position_embeddings, gloss)
        r = layers[0][1]
        assert bool(r.get("dgu_sliced")) == (form not in MID_UNSLICED), f"form {form}: dgu_sliced"
        for role in ("dh2", "dh1"):
            assert isinstance(r[role], tuple) == (role in MID_PAIRS[form]), \
                f"form {form}: {role} {'must' if role in MID_PAIRS[form] else 'must not'} be a split-K pair"
        M.check_model(layers, hc, h, "mid " + form)


# ------------------------------------------------------------------------------ c. the nodes on their own
def _noncontig(t, kind):
    """The same values as t [B, S, H] behind a non-contiguous view: a transposed view, or a slice of a wider buffer."""
    if kind == "transposed":
        return t.transpose(0, 1).contiguous().transpose(0, 1)
    wide = torch.full(t.shape[:-1] + (t.shape[-1] + 24,), float("nan"), dtype=t.dtype, device=t.device)
    wide[..., 8:8 + t.shape[-1]] = t
    return wide[..., 8:8 + t.shape[-1]]


def _lin_params(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.Parameter((torch.randn(n, k, generator=g) * k ** -0.5).to(BF).cuda())


def _norm_w(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.Parameter((1 + 0.1 * torch.randn(n, generator=g)).to(BF).cuda())


def _node_io(B, S, H, Hout, xkind, dykind, need_dx, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    x = _noncontig(torch.randn(B, S, H, generator=g).to(BF).cuda(), xkind).requires_grad_(need_dx)
    dy = _noncontig(torch.randn(B, S, Hout, generator=g).to(BF).cuda(), dykind)
    assert not x.is_contiguous() and not dy.is_contiguous()
    return x, dy


NODE_IO = [("transposed", "slice", True), ("slice", "transposed", True), ("transposed", "slice", False)]


def _layer_like(B, S, nh, nkv, d, I, **w):
    base = dict(B=B, S=S, nh=nh, nkv=nkv, d=d, I=I, eps=1e-5, mode=0, mask=None, w1_grad=True, w2_grad=True, qkv_grad=True,
                wqn=None, wkn=None)
    base.update({k: M.cpu(v) for k, v in w.items()})
    return types.SimpleNamespace(**base)


@pytest.mark.parametrize("xkind,dykind,need_dx", NODE_IO)
@pytest.mark.parametrize("frozen", [None, "w"])
def test_linear_and_lm_head_nodes(xkind, dykind, need_dx, frozen):
    from picotron_amd import functional as FN
    B, S, H, N = 2, 128, 256, 512
    for node in ("linear", "lm_head"):
        w = _lin_params(N, H, 3)
        w.requires_grad_(frozen is None)
        x, dy = _node_io(B, S, H, N, xkind, dykind, need_dx)
        if not need_dx and frozen:
            continue   # nothing requires a gradient: autograd runs no backward
        with M.recording() as rec:
            y = FN.linear(x, w) if node == "linear" else FN.lm_head_linear(x, w)
            y.backward(dy)
            torch.cuda.synchronize()
        FN._CE_STATS.clear()
        tag = f"node {node}"
        assert [n for n in rec.names() if n.startswith("linear_")][0] == ("linear_fwd" if node == "linear" else "linear_ce_stats")
        x2, dy2 = M.cpu(x).reshape(B * S, H), M.cpu(dy).reshape(B * S, N)
        M._note(tag, "y", M._gemm("y", M.cpu(y).reshape(B * S, N), x2, M.cpu(w).t(), tag))
        if need_dx:
            M._note(tag, "dx", M._gemm("dx", M.cpu(x.grad).reshape(B * S, H), dy2, M.cpu(w), tag))
        else:
            assert x.grad is None and "linear_dgrad" not in rec.names()
        if frozen is None:
            M._note(tag, "dW", M._gemm("dW", M.cpu(w.grad), dy2.t().contiguous(), x2, tag))
        else:
            assert w.grad is None and "linear_wgrad" not in rec.names()


@pytest.mark.parametrize("xkind,dykind,need_dx", NODE_IO)
@pytest.mark.parametrize("frozen", [None, "w"])
@pytest.mark.parametrize("mode", [0, 1])
def test_norm_nodes(xkind, dykind, need_dx, frozen, mode):
    from picotron_amd import functional as FN
    B, S, H = 2, 128, 256
    for node in ("norm", "add_norm"):
        w = _norm_w(H, 5)
        w.requires_grad_(frozen is None)
        x, dy = _node_io(B, S, H, H, xkind, dykind, need_dx, seed=1)
        res, dz = _node_io(B, S, H, H, dykind, xkind, need_dx, seed=2)
        if not need_dx and frozen:
            continue
        tag = f"node {node} mode {mode}"
        with M.recording() as rec:
            if node == "norm":
                y = FN.RMSNormFunction.apply(x, w, 1e-5, mode)
                y.backward(dy)
                r2, dres = None, None
            else:
                y, z = FN.AddRMSNormFunction.apply(x, res, w, 1e-5, mode)
                torch.autograd.backward([y, z], [dy, dz])
                r2, dres = M.cpu(res).reshape(B * S, H), M.cpu(dz).reshape(B * S, H)
            torch.cuda.synchronize()
        x2 = M.cpu(x).reshape(B * S, H)
        fc = M.Cursor(rec.calls).next("rmsnorm_fwd", None, "y")
        rstd = M.cpu(fc.result[1].post)   # the forward's saved f32 rstd: the backward's input
        f = R.ref_norm_fwd(x2, r2, M.cpu(w), 1e-5, mode)
        M._note(tag, "rstd", R.check("rstd", rstd, f["rstd"], f["rstd_bound"], tag))
        M._note(tag, "y", R.check("y", M.cpu(y).reshape(B * S, H), f["y_ref"], f["y_bound"], tag))
        zin = x2
        if node == "add_norm":
            R.check_exact("z", M.cpu(z).reshape(B * S, H), f["z"])
            zin = f["z"]
        b = R.ref_norm_bwd(M.cpu(dy).reshape(B * S, H), zin, M.cpu(w), rstd, dres, mode)
        if need_dx:
            M._note(tag, "dx", R.check("dx", M.cpu(x.grad).reshape(B * S, H), b["dx_ref"], b["dx_bound"], tag))
            if node == "add_norm":
                assert torch.equal(x.grad, res.grad)
        else:
            assert x.grad is None
        if frozen is None:
            ev = M.norm_sink_events(rec.calls, {w.grad.data_ptr(): "w"})["w"]
            assert len(ev) == 1 and ev[0]["sink"] == 0, "one bf16 store into the fresh .grad"
            M._note(tag, "dw", M._norm_dw("dw", dict(got=M.cpu(w.grad), sink=0), b, tag))
        else:
            assert w.grad is None and "rmsnorm_colsum_batch" not in rec.names()


@pytest.mark.parametrize("xkind,dykind,need_dx", NODE_IO)
@pytest.mark.parametrize("frozen", [None, "wq", "wk", "wv", "wo"])
def test_attention_node(xkind, dykind, need_dx, frozen):
    from picotron_amd import functional as FN
    from picotron_amd.model import get_cos_sin
    B, S, nh, nkv, d = 2, 128, 4, 2, 64
    H = nh * d
    ws = dict(wq=_lin_params(nh * d, H, 1), wk=_lin_params(nkv * d, H, 2), wv=_lin_params(nkv * d, H, 3), wo=_lin_params(H, H, 4))
    if frozen:
        ws[frozen].requires_grad_(False)
    cos, sin = (t.to(device="cuda", dtype=BF) for t in get_cos_sin(S, d, base=10000.0))
    x, dy = _node_io(B, S, H, H, xkind, dykind, need_dx)
    with M.recording() as rec:
        y = FN.AttentionFunction.apply(x, ws["wq"], ws["wk"], ws["wv"], ws["wo"], cos, sin, nh, nkv, d)
        y.backward(dy)
        torch.cuda.synchronize()
    c = _layer_like(B, S, nh, nkv, d, 0, cos=cos[:S], sin=sin[:S], **ws)
    K, cur = K_(), M.Cursor(rec.calls)
    r = {"h1": M.cpu(x).reshape(B * S, H)}
    qc = cur.next(("linear_fwd_rope", "linear_fwd"), lambda k: M._is(M._first_weight(k), ws["wq"]), "qkv")
    M._bits_equal("the q|k|v GEMM reads x", qc.arg(0).pre, x.reshape(B * S, H))
    if qc.name == "linear_fwd_rope":
        raw = K.linear_fwd(qc.arg(0).pre, [ws["wq"], ws["wk"], ws["wv"]])
        r["qkv_raw"], r["qkv"] = M.cpu(raw), M.cpu(qc.result.post)
        M._bits_equal("qkv: fused vs separate", K.rope_(raw.clone(), nh + nkv, d, cos, sin, S), qc.result.post)
    else:
        r["qkv_raw"] = M.cpu(qc.result.post)
        r["qkv"] = M.cpu(cur.next("rope_", None, "qkv").arg(0).post)
    ac = cur.next("attn_fwd", None, "o")
    r["o"], r["lse"] = M.cpu(ac.result[0].post), M.cpu(ac.result[1].post)
    r["a"] = M.cpu(y).reshape(B * S, H)
    fwd = [s for s in M.LAYER_FWD if s.produces[0] in ("qkv_raw", "qkv", "o", "a")]
    M.check_stages(r, c, fwd, "node attention")
    # backward: dz := dy
    r["dz"] = M.cpu(dy).reshape(B * S, H)
    oc = cur.next("linear_dgrad", lambda k: M._is(M._first_weight(k), ws["wo"]), "do")
    r["do"] = M.cpu(oc.result.post)
    ab = cur.next("attn_bwd", None, "dqkv")
    got = torch.cat([M.cpu(ab.kwargs[k].post).reshape(B * S, -1) for k in ("dq", "dk", "dv")], 1)
    buf = torch.empty(B * S, got.shape[1], dtype=BF, device="cuda")
    K.attn_bwd(*[a.pre for a in ab.args[:6]], ab.args[6], ab.args[7], dq=M._heads(buf, c, "q"), dk=M._heads(buf, c, "k"),
               dv=M._heads(buf, c, "v"))
    r["dqkv_unrot"] = M.cpu(buf)
    K.rope_(buf, nh + nkv, d, cos, sin, S, inverse=True)
    M._bits_equal("dqkv: fused vs separate", got, buf)
    r["dqkv_rot"] = r["dqkv"] = got
    sinks = {p.grad.data_ptr(): n for n, p in ws.items() if p.grad is not None}
    wev = M.sink_events(rec.calls, sinks)
    for n, role in (("wq", "dW_q"), ("wk", "dW_k"), ("wv", "dW_v"), ("wo", "dW_o")):
        if n == frozen:
            assert ws[n].grad is None and n not in wev
        else:
            r[role] = M._sink_role(M._wsink(wev, n, 0, role))
            assert r[role]["epi"] == K.EPI_BF16
    only = ["do", "dqkv_unrot", "dqkv_rot", ""] + ([] if frozen == "wo" else ["dW_o"])
    if need_dx:
        r["dh1"] = M.cpu(x.grad).reshape(B * S, H)
        only.append("dh1")
    else:
        assert x.grad is None
    stages = [s for s in M.LAYER_BWD if (s.produces[0] if s.produces else "") in only]
    M.check_stages(r, c, stages, "node attention")


@pytest.mark.parametrize("xkind,dykind,need_dx", NODE_IO)
@pytest.mark.parametrize("frozen", [None, "wg", "wu", "wd"])
def test_mlp_node(xkind, dykind, need_dx, frozen):
    from picotron_amd import functional as FN
    B, S, H, I = 2, 128, 256, 512
    ws = dict(wg=_lin_params(I, H, 1), wu=_lin_params(I, H, 2), wd=_lin_params(H, I, 3))
    if frozen:
        ws[frozen].requires_grad_(False)
    x, dy = _node_io(B, S, H, H, xkind, dykind, need_dx)
    with M.recording() as rec:
        y = FN.MLPFunction.apply(x, ws["wg"], ws["wu"], ws["wd"])
        y.backward(dy)
        torch.cuda.synchronize()
    c = _layer_like(B, S, 4, 2, 64, I, **ws)
    K, cur = K_(), M.Cursor(rec.calls)
    r = {"h2": M.cpu(x).reshape(B * S, H), "dout": M.cpu(dy).reshape(B * S, H)}
    gc = cur.next(("linear_swiglu_fwd", "linear_fwd"), None, "gu")
    M._bits_equal("the gate|up GEMM reads x", gc.arg(0).pre, x.reshape(B * S, H))
    if gc.name == "linear_swiglu_fwd":
        gu_dev = gc.result[0].post
        r["gu"], r["hh"] = M.cpu(gu_dev), M.cpu(gc.result[1].post)
        gu2 = K.linear_fwd(gc.arg(0).pre, [ws["wg"], ws["wu"]])
        M._bits_equal("gu: fused vs separate", gu_dev, gu2)
        M._bits_equal("hh: fused vs separate", gc.result[1].post, K.swiglu_fwd(gu2[:, :I], gu2[:, I:]))
    else:
        gu_dev = gc.result.post
        r["gu"], r["hh"] = M.cpu(gu_dev), M.cpu(cur.next("swiglu_fwd", None, "hh").result.post)
    # the node's output has no residual: a plain bf16 store
    M.check_stages(r, c, [s for s in M.LAYER_FWD if s.produces[0] in ("gu", "hh")], "node mlp")
    M._note("node mlp", "m", M._gemm("m", M.cpu(y).reshape(B * S, H), r["hh"], M.cpu(ws["wd"]).t(), "node mlp"))
    dc = cur.next(("linear_dgrad_dual", "linear_dgrad_swiglu", "linear_dgrad"), None, "dgu")
    if dc.name == "linear_dgrad":
        r["dhh"] = M.cpu(dc.result.post)
        sc = cur.next("swiglu_bwd", None, "dgu")
        r["dgu"] = torch.cat([M.cpu(sc.kwargs["dg"].post), M.cpu(sc.kwargs["du"].post)], 1)
    else:
        dhh = K.linear_dgrad(dc.arg(0).pre, [ws["wd"]])
        dgu = torch.empty_like(gu_dev)
        K.swiglu_bwd(dhh, gu_dev[:, :I], gu_dev[:, I:], dg=dgu[:, :I], du=dgu[:, I:])
        M._bits_equal("dgu: fused vs separate", dc.result.post, dgu)
        r["dhh"], r["dgu"] = M.cpu(dhh), M.cpu(dgu)
    sinks = {p.grad.data_ptr(): n for n, p in ws.items() if p.grad is not None}
    wev = M.sink_events(rec.calls, sinks)
    only = ["dhh", "dgu"]
    for n, role in (("wg", "dW_g"), ("wu", "dW_u"), ("wd", "dW_d")):
        if n == frozen:
            assert ws[n].grad is None and n not in wev
        else:
            r[role] = M._sink_role(M._wsink(wev, n, 0, role))
    if frozen != "wd":
        only.append("dW_d")
    if frozen in ("wg", "wu"):   # the other half alone
        role, cols = ("dW_u", slice(I, 2 * I)) if frozen == "wg" else ("dW_g", slice(0, I))
        M._note("node mlp", role, M._wgrad(f"dW_gu ({role})", r[role], r["dgu"][:, cols], r["h2"], "node mlp"))
    else:
        only.append("dW_g")
    if need_dx:
        r["dh2"] = M.cpu(x.grad).reshape(B * S, H)
        only.append("dh2")
    else:
        assert x.grad is None
    M.check_stages(r, c, [s for s in M.LAYER_BWD if s.produces and s.produces[0] in only], "node mlp")


# ------------------------------------------------------------------------------ d. lm_head + CE stash hygiene
STATS, STREAM = "cross_entropy_loss_lse_stats", "cross_entropy_loss_lse"


def _ce_case(reduction, gscale, how):
    """lm_head + CE with the statistics on; `how` says which logits meet the CE.  Returns (roles, forward name)."""
    from picotron_amd import functional as FN
    T, H, V = 256, 256, 512
    g = torch.Generator().manual_seed(7)
    x = torch.randn(T, H, generator=g).to(BF).cuda().requires_grad_(True)
    x2 = torch.randn(T, H, generator=g).to(BF).cuda()
    w = _lin_params(V, H, 9)
    tgt = torch.randint(0, V, (T,), generator=g)
    tgt[::17] = -100
    FN._CE_STATS.clear()
    with M.recording() as rec:
        logits = FN.lm_head_linear(x, w)
        if how == "clone":
            lg = logits.clone()
        elif how == "first_of_two":
            lg, _other = logits, FN.lm_head_linear(x2, w)
        elif how == "after_unrelated":
            _other = FN.lm_head_linear(x2, w)
            del _other
            lg = logits
        elif how == "modified_in_place":   # the stash is keyed by the storage: its version counter must match
            lg = logits.detach()           # (same storage, same version counter; a leaf of its own)
            lg.mul_(0.5)
            assert lg.data_ptr() == logits.data_ptr()
            lg.requires_grad_(True)
        else:
            lg = logits
        at = len(rec.calls)
        loss = FN.cross_entropy(lg, tgt.cuda(), reduction=reduction)
        gl = (torch.full(loss.shape, gscale) * (1 + torch.arange(loss.numel()).reshape(loss.shape) % 3)).to(loss.dtype)
        loss.backward(gl.cuda())
        torch.cuda.synchronize()
    heads = [c for c in rec.calls if c.name == "linear_ce_stats"]
    assert len(heads) == (2 if how in ("first_of_two", "after_unrelated") else 1)
    r, name, _ = M.extract_ce(K_(), rec.calls, at, gloss=gl)
    if how == "modified_in_place":
        M._bits_equal("the CE read the halved logits", r["logits"], (heads[0].result[0].post.float() * 0.5).to(BF))
    else:
        M._bits_equal("the CE read the first lm_head call's logits", r["logits"], heads[0].result[0].post)
    if name == STATS:
        M._bits_equal("the statistics are those of these logits", r["stats"], heads[0].result[1].post)
    FN._CE_STATS.clear()
    return r, name


@pytest.mark.parametrize("how,want", [("returned", STATS), ("clone", STREAM), ("first_of_two", STATS), ("after_unrelated", STATS),
                                      ("modified_in_place", STREAM)])
@pytest.mark.parametrize("reduction,gscale", [("mean", 0.25), ("sum", 0.375), ("none", 0.5)])
def test_ce_stash_hygiene(how, want, reduction, gscale):
    r, name = _ce_case(reduction, gscale, how)
    assert name == want, f"CE on the {how} logits ran {name}"
    c = types.SimpleNamespace(reduction=reduction, ignore=-100)
    M.check_stages(r, c, M.CE_STAGES, f"ce {how} {reduction}")


# ------------------------------------------------------------------------------ e. the table
def test_zz_worst_ratio_table():
    print("\n" + M.worst_table())
    assert M.WORST and all(v <= 1.0 for v in M.WORST.values())
