"""Stage-by-stage conformance kit of the autograd layer (picotron_amd/functional.py): a recorder of the
kernel calls, the model's math written once as a list of stages, a teacher-forced per-element checker
built on the kernel kits' own bounds, and a CPU emulation with injectable wiring faults.

Recorder
    `Recorder(kernels)` stands in for `functional.K` (see `recording`).  Every function call is forwarded
    to the real module and logged as a `Call`: the name, the arguments with every tensor replaced by a `Rec`
    (identity = data_ptr / shape / stride / dtype, `pre` = a clone taken before the call, `post` = a clone
    taken after it, `obj` = the live tensor, so that a Parameter or a gradient sink is recognised by
    identity) and the results (`post` only).  Cloning every tensor argument before and after the call
    records the prior contents of whatever the call overwrites (`rope_`, the dq= / dk= / dv= of `attn_bwd`,
    `swiglu_bwd(dg=, du=)`, accumulating sinks, `dx=dqkv` of `qk_norm_bwd`) without a table of in-place
    arguments.  `SplitKParts` (p0, p1) and `KPair` (a, b) are recorded as `Parts` / `Pair` of their halves.
    Parameters are not cloned (no kernel call writes one).  clone=False logs only the call names and what kind
    of value came back (the "form was taken" assertions at shapes whose clones would be large).

Roles and stages
    A role is a named production value (bf16 / f32 CPU tensor) of one decoder layer or of the model's head:
    the tables of LAYER_STAGES and HEAD_STAGES name, per stage, the roles it reads and the roles it produces.
    Weight-gradient roles are dicts {got, old, epi} (+ prev = (dY, X) of the other micro-batch of a paired
    K = 2 T launch); norm weight gradients {got, old, sink}; a split-K dX is the pair (p0, p1) of its f32
    halves.

Teacher-forced check (`check_stages`)
    Every stage's float64 reference is computed from the PRODUCTION values of the roles it reads and
    compared per element with the production value of the role it produces, under the bound the kernel's
    own kit derives -- _gemm_ref.target_and_bound (the sink's prior contents as `old`), _row_ref's norm /
    CE / SwiGLU references and dw_target_bound, _attn_ref.check_out / check_lse / check_grads,
    _qk_norm_ref's references, _optim_ref's embedding expectation (by bits).  No tolerance is invented
    here and none carries a slack factor of this file's; rounding does not propagate from stage to stage,
    so a wrong operand, sink, scale or dropped term fails at the stage where it happens, and the failure
    names the role and the element.  A role that is missing is an error.
    Two bounds are compositions written down here because the kits check those kernels by bits on grid
    inputs only:
      * RoPE on arbitrary bf16 values, o1 = bf16(fma(a, c, -(b s))) (picotron_amd/csrc/rope.hip:45-46): the inner
        product b s and the fma round once each in f32, E32 = e (|b s| + |o|), then _row_ref.b16.
      * the row LSE taken from the lm_head GEMM's tile statistics: _row_ref.merge_stats' bound on the
        recorded statistics plus ref_ce_fwd's lse_bound -- each tile's (max, sum-exp) is a CE row sum over
        at most 256 stored logits, the quantity ref_ce_fwd's E_S bounds for one chunk step.
    The split-K dX pair is held to the f32-store bound on p0 + p1; the norm backward behind it takes
    bf16(f32(p0 + p1)), as include/picotron_hip.h states for pt_rmsnorm_bwd_splitk.

Fused stages (RoPE / SwiGLU in a GEMM epilogue, the SwiGLU backward in the down dX epilogue, the inverse
RoPE in the attention backward's stores, the CE statistics GEMM): the sources round the accumulator to
bf16 before the epilogue's arithmetic (picotron_amd/csrc/gemm.hip:604 `round_bf(acc)`, :299 "staged (bf16)", :437 "from
the bf16 staging, as picotron_amd/csrc/rope.hip does"; picotron_amd/csrc/attention.hip:231-232), so the claim is bit identity:
`extract_layer` / `extract_head` replay the separate kernels on the recorded inputs, compare bits, and
hand the separate form's intermediates (qkv_raw, dhh, dqkv_unrot) to the stages.  The replays run as
single-pass GEMMs (`single_pass`), like the fused launches.  One fused form has no separate form to replay: the
down dX of a dual launch in K-slices (_s_dgu_sliced says what holds it instead).

CPU emulation (`emu_model`): one decoder layer between an embedding and the head, built from the kits'
emulators (emu_gemm, emu_norm_fwd / bwd, emu_swiglu, emu_rope, _attn_ref.emu_forward / emu_backward,
emu_ce, emu_embedding_*), bf16 wherever the HIP path stores bf16; FAULTS injects the wiring mistakes the
checker must reject at the named role (tests/test_model_stage_checker_cpu.py).
"""
import contextlib
import math
import types

import torch

from tests import _attn_ref as A
from tests import _gemm_ref as G
from tests import _optim_ref as OR
from tests import _qk_norm_ref as Q
from tests import _row_ref as R

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
IGNORE = -100
WORST = {}   # (form, role) -> worst |got - ref| / bound seen in this process


# ============================================================================== recorder
class Rec:
    """One tensor of a recorded call."""
    __slots__ = ("key", "pre", "post", "obj")

    def __init__(self, t, pre):
        self.key = (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype)
        self.obj, self.pre, self.post = t, pre, None

    def same(self, other):
        return self.key == other.key


class Parts(tuple):
    """A recorded SplitKParts: (p0, p1)."""


class Pair(tuple):
    """A recorded KPair: (a, b)."""


class Call:
    def __init__(self, name, args, kwargs):
        self.name, self.args, self.kwargs, self.result = name, args, kwargs, None

    def arg(self, pos, name=None):
        if name is not None and name in self.kwargs:
            return self.kwargs[name]
        return self.args[pos] if pos is not None and pos < len(self.args) else None

    def recs(self):
        return list(_flat((self.args, self.kwargs)))


def _flat(x):
    if isinstance(x, Rec):
        yield x
    elif isinstance(x, dict):
        for v in x.values():
            yield from _flat(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            yield from _flat(v)


class Recorder:
    def __init__(self, real, clone=True):
        self._real, self._clone, self.calls = real, clone, []

    def __getattr__(self, name):
        v = getattr(self._real, name)
        if not isinstance(v, types.FunctionType):
            return v
        return lambda *a, **kw: self._run(name, v, a, kw)

    def names(self):
        return [c.name for c in self.calls]

    def _wrap(self, x, live, out=False):
        if isinstance(x, torch.Tensor):
            is_param = isinstance(x, torch.nn.Parameter)
            r = Rec(x, None if out else (x.detach() if is_param else x.detach().clone()))
            if out:
                r.post = x.detach().clone()
            elif is_param:
                r.post = r.pre
            else:
                live.append(r)
            return r
        if isinstance(x, (list, tuple)):
            return type(x)(self._wrap(e, live, out) for e in x) if type(x) in (list, tuple) else x
        if isinstance(x, dict):
            return {k: self._wrap(v, live, out) for k, v in x.items()}
        if hasattr(x, "p0") and hasattr(x, "p1"):
            return Parts((self._wrap(x.p0, live, out), self._wrap(x.p1, live, out)))
        if hasattr(x, "a") and hasattr(x, "b") and hasattr(x, "shape"):
            return Pair((self._wrap(x.a, live, out), self._wrap(x.b, live, out)))
        return x

    def _run(self, name, fn, a, kw):
        if not self._clone:
            call = Call(name, (), {})
            self.calls.append(call)
            out = fn(*a, **kw)
            call.result = "Parts" if hasattr(out, "p0") else type(out).__name__
            return out
        live = []
        call = Call(name, self._wrap(a, live), self._wrap(kw, live))
        out = fn(*a, **kw)
        for r in live:
            r.post = r.obj.detach().clone()
        call.result = self._wrap(out, [], out=True)
        self.calls.append(call)
        return out


@contextlib.contextmanager
def single_pass():
    """The replays' GEMMs as one pass over K, like the fused launches they are compared with: the split-K
    halves and the K-slices sum their f32 partials in another order (another GEMM form, not an epilogue)."""
    from picotron_amd import switches
    with switches.override(splitk2=0, ksplit=0):
        yield


@contextlib.contextmanager
def recording(clone=True):
    """functional.K replaced by a Recorder for the block; yields the recorder."""
    from picotron_amd import functional as FN
    real = FN.K
    rec = Recorder(real, clone)
    FN.K = rec
    try:
        yield rec
    finally:
        FN.K = real


# ============================================================================== helpers
def cpu(t):
    return t.detach().to("cpu")


def _note(form, role, ratio):
    if isinstance(ratio, dict):
        for k, v in ratio.items():
            _note(form, f"{role}.{k}", v)
        return
    WORST[(form, role)] = max(WORST.get((form, role), 0.0), float(ratio))


def _gemm(role, got, a, b, tag, epi=G.EPI_BF16, old=None, residual=None):
    """got [M, N] against a [M, K] . b [K, N] (production operands) through epilogue epi."""
    acc, S = G.ref_product(a, b)
    want = G.sink_dtype(epi)
    assert got.dtype == want, f"{role}: dtype {got.dtype}, the epilogue stores {want}"
    t, bound = G.target_and_bound(acc, S, a.shape[1], epi, old, residual)
    return G.check(role, got, t, bound, tag)


def parts_bf16(p):
    """bf16(f32(p0 + p1)) of a split-K pair, the dy pt_rmsnorm_bwd_splitk forms; a tensor as it is."""
    return (p[0].to(F32) + p[1].to(F32)).to(BF) if isinstance(p, (tuple, list)) else p


def _dx(role, got, dy, wcat, tag):
    """A dX role: a bf16 tensor (bf16 store) or the pair of f32 split-K halves (their sum under the f32-store
    bound of the whole product)."""
    if isinstance(got, (tuple, list)):
        acc, S = G.ref_product(dy, wcat)
        t, bound = G.target_and_bound(acc, S, dy.shape[1], G.EPI_F32)
        assert got[0].dtype == F32 and got[1].dtype == F32, f"{role}: split-K halves must be f32"
        return G.check(role, got[0].to(F64) + got[1].to(F64), t, bound, tag)
    return _gemm(role, got, dy, wcat, tag)


def _wgrad(role, sink, dy, x, tag):
    """A weight-gradient role {got, old, epi[, prev]}: dW = dY^T X (K = T, or 2 T with the other micro-batch's
    recorded operands) through the sink's epilogue onto its prior contents."""
    a, b = dy.t(), x
    epi = sink["epi"]
    old = sink["old"] if epi in (G.EPI_BF16_ACC, G.EPI_F32_ACC) else None
    if sink.get("prev") is not None and sink.get("unpaired"):
        return _wgrad_unpaired(role, sink, a.contiguous(), b, epi, old, tag)
    if sink.get("prev") is not None:
        pdy, px = sink["prev"]
        a, b = torch.cat([pdy.t(), a], 1), torch.cat([px, b], 0)
    return _gemm(role, sink["got"], a.contiguous(), b.contiguous(), tag, epi, old=old)


ACC_OF = {G.EPI_BF16: G.EPI_BF16_ACC, G.EPI_BF16_ACC: G.EPI_BF16_ACC, G.EPI_F32_ACC: G.EPI_F32_ACC}


def _wgrad_unpaired(role, sink, a, b, epi, old, tag):
    """A paired group the K-segmented 256 x 256 tile refuses (a sink whose rows are no multiple of 256:
    picotron_amd/csrc/gemm.hip args_fit) runs as kernels._wgrad_unpaired documents: the first micro-batch's half through
    the sink's epilogue, the second's accumulating onto it.  Two launches, two kit bounds: the second's with the
    first's unrounded target as `old`, plus the first's own bound carried through the add and the store."""
    pdy, px = sink["prev"]
    acc1, S1 = G.ref_product(pdy.t().contiguous(), px)
    t1, b1 = G.target_and_bound(acc1, S1, px.shape[0], epi, old)
    acc2, S2 = G.ref_product(a, b)
    t2, b2 = G.target_and_bound(acc2, S2, b.shape[0], ACC_OF[epi], old=t1)
    assert sink["got"].dtype == G.sink_dtype(epi), f"{role}: dtype {sink['got'].dtype}"
    return G.check(role, sink["got"], t2, b2 + (1 + G.U) * b1, tag)


def rope_target_bound(x, nheads, d, cos, sin, S, inverse):
    """(float64 target, bound) of pt_rope on arbitrary bf16 values; columns past nheads * d: bound 0."""
    rows = x.shape[0]
    half = d // 2
    pos = torch.arange(rows) % S
    c = cos.to(F64)[pos, :half][:, None, :]
    s = sin.to(F64)[pos, :half][:, None, :]
    if inverse:
        s = -s
    v = x[:, :nheads * d].to(F64).reshape(rows, nheads, d)
    a, b = v[..., :half], v[..., half:]
    o = torch.cat([a * c - b * s, b * c + a * s], -1)
    inner = torch.cat([(b * s).abs(), (a * s).abs()], -1)
    e32 = R.E * (inner + o.abs()) * R.SECOND
    t = x.to(F64).clone()
    bound = torch.zeros_like(t)
    t[:, :nheads * d] = o.reshape(rows, nheads * d)
    bound[:, :nheads * d] = R.b16(o, e32).reshape(rows, nheads * d)
    return t, bound


def _rope(role, got, x, c, tag, inverse):
    n = (c.nh + c.nkv) * c.d
    if got.shape[1] > n:
        R.check_exact(role + " (v columns)", got[:, n:], x[:, n:])
    t, bound = rope_target_bound(x, c.nh + c.nkv, c.d, c.cos, c.sin, c.S, inverse)
    return R.check(role, got[:, :n], t[:, :n], bound[:, :n], tag)


def _heads(t2d, c, which):
    """q / k / v of a [T, q|k|v] tensor as [B, S, heads, d]."""
    wq, wkv = c.nh * c.d, c.nkv * c.d
    lo, n, h = {"q": (0, wq, c.nh), "k": (wq, wkv, c.nkv), "v": (wq + wkv, wkv, c.nkv)}[which]
    return t2d[:, lo:lo + n].reshape(c.B, c.S, h, c.d)


def _mask(c):
    return c.mask if c.mask is not None else A.causal_mask(c.S, c.S)


def _norm_dw(role, sink, ref, tag):
    t, bound = R.dw_target_bound(ref["dw"], ref["dw_err"], sink["sink"], sink.get("old"))
    want = F32 if sink["sink"] == R.PT_DW_ACC_F32 else BF
    assert sink["got"].dtype == want, f"{role}: dtype {sink['got'].dtype}, the sink holds {want}"
    return R.check(role, sink["got"], t, bound, tag)


# ============================================================================== the stages
class Stage:
    def __init__(self, produces, reads, fn):
        self.produces, self.reads, self.fn = tuple(produces.split()), tuple(reads.split()), fn


def _s_norm1(r, c, tag):
    f = R.ref_norm_fwd(r["x"], None, c.w1, c.eps, c.mode)
    return {"rstd1": R.check("rstd1", r["rstd1"], f["rstd"], f["rstd_bound"], tag),
            "h1": R.check("h1", r["h1"], f["y_ref"], f["y_bound"], tag)}


def _s_qkv_raw(r, c, tag):
    return _gemm("qkv_raw", r["qkv_raw"], r["h1"], torch.cat([c.wq, c.wk, c.wv]).t(), tag)


def _s_qkv(r, c, tag):
    return _rope("qkv", r["qkv"], r["qkv_raw"], c, tag, False)


def _s_qk_normed(r, c, tag):
    """QK-norm: the per-head norm of the q | k heads of the raw projection (the norm-only replay of
    qk_norm_rope_fwd, whose fused output must equal that followed by pt_rope by bits) and rstd_qk."""
    T = c.B * c.S
    xq, xk = Q.split_heads(r["qkv_raw"], c.nh, c.nkv, c.d)
    yq, yk = Q.split_heads(r["qk_normed"], c.nh, c.nkv, c.d)
    rq, rk = Q.rstd_heads(r["rstd_qk"], T, c.nh, c.nkv)
    out = {}
    for nm, x, w, rs, y in (("q", xq, c.wqn, rq, yq), ("k", xk, c.wkn, rk, yk)):
        f = Q.ref_fwd(x, w, c.eps, c.mode)
        out[f"rstd_qk.{nm}"] = R.check(f"rstd_qk ({nm})", rs, f["rstd"], f["rstd_bound"], tag)
        out[f"qk_normed.{nm}"] = R.check(f"qk_normed ({nm})", y, f["y_ref"], f["y_bound"], tag)
    return out


def _s_qk(r, c, tag):
    return _rope("qk", r["qk"], r["qk_normed"], c, tag, False)


def _attn_inputs(r, c):
    if "qk" in r:
        qk = torch.cat([r["qk"], r["qkv_raw"][:, (c.nh + c.nkv) * c.d:]], 1)
        return _heads(qk, c, "q"), _heads(qk, c, "k"), _heads(qk, c, "v")
    return _heads(r["qkv"], c, "q"), _heads(r["qkv"], c, "k"), _heads(r["qkv"], c, "v")


def _s_attn(r, c, tag):
    q, k, v = _attn_inputs(r, c)
    f = A.ref_forward(q, k, v, A.scale_of(c.d), _mask(c))
    return {"o": A.check_out(r["o"], f, tag, "o"), "lse": A.check_lse(r["lse"], f.lse, tag, "lse")}


def _s_a(r, c, tag):
    return _gemm("a", r["a"], r["o"].reshape(c.B * c.S, -1), c.wo.t(), tag)


def _s_norm2(r, c, tag):
    f = R.ref_norm_fwd(r["a"], r["x"], c.w2, c.eps, c.mode)
    R.check_exact("z", r["z"], f["z"])
    return {"z": 0.0, "rstd2": R.check("rstd2", r["rstd2"], f["rstd"], f["rstd_bound"], tag),
            "h2": R.check("h2", r["h2"], f["y_ref"], f["y_bound"], tag)}


def _s_gu(r, c, tag):
    return _gemm("gu", r["gu"], r["h2"], torch.cat([c.wg, c.wu]).t(), tag)


def _s_hh(r, c, tag):
    f = R.ref_swiglu_fwd(r["gu"][:, :c.I], r["gu"][:, c.I:])
    return R.check("hh", r["hh"], f["h_ref"], f["h_bound"], tag)


def _s_out(r, c, tag):
    return _gemm("out", r["out"], r["hh"], c.wd.t(), tag, G.EPI_BF16_RES, residual=r["z"])


def _s_dhh(r, c, tag):
    return _gemm("dhh", r["dhh"], r["dout"], c.wd, tag)


def _s_dgu_sliced(r, c, tag):
    """The down dX of a dual launch in K-slices (kernels.linear_dgrad_dual, `dxs > 1`: f32 partials beside the dW
    slices; the SwiGLU backward runs in the reduce pass on dh = bf16(sum of the slices), picotron_amd/csrc/gemm.hip
    splitk_reduce_kernel<EPI_SWIGLU_BWD>): dh is never stored and its f32 sum has another order than any separate
    launch's, so there is no separate form to compare bits with.  The composition of the two kits' bounds: the
    f32 dh lies within the GEMM kit's E32 of the exact product, so bf16(dh) lies between bf16(acc - E32) and
    bf16(acc + E32) (the same value for all but the elements near a rounding boundary or cancelled to within
    E32); dg = bf16(bf16(dh u) F) and du = bf16(dh bf16(silu)) are monotone in dh, so the output lies between
    the SwiGLU kit's targets at those two ends, each widened by the kit's own bound there."""
    acc, S = G.ref_product(r["dout"], c.wd)
    e32 = r["dout"].shape[1] * 2.0 ** -23 * S
    g, u = r["gu"][:, :c.I], r["gu"][:, c.I:]
    assert bool(torch.isfinite(r["dgu"].to(F32)).all()), "dgu: non-finite values"
    ends = [R.ref_swiglu_bwd(R._bf(acc + sgn * e32).to(BF), g, u) for sgn in (-1, 1)]
    out = {}
    for k, got in (("dg", r["dgu"][:, :c.I].to(F64)), ("du", r["dgu"][:, c.I:].to(F64))):
        lo = torch.minimum(ends[0][k + "_ref"] - ends[0][k + "_bound"], ends[1][k + "_ref"] - ends[1][k + "_bound"])
        hi = torch.maximum(ends[0][k + "_ref"] + ends[0][k + "_bound"], ends[1][k + "_ref"] + ends[1][k + "_bound"])
        out[k] = R.check(f"dgu ({k}, K-sliced dh)", got, (lo + hi) / 2, (hi - lo) / 2, tag)
    return out


def _s_dgu(r, c, tag):
    if r.get("dgu_sliced"):
        return _s_dgu_sliced(r, c, tag)
    f = R.ref_swiglu_bwd(r["dhh"], r["gu"][:, :c.I], r["gu"][:, c.I:])
    return {"dg": R.check("dgu (dg)", r["dgu"][:, :c.I], f["dg_ref"], f["dg_bound"], tag),
            "du": R.check("dgu (du)", r["dgu"][:, c.I:], f["du_ref"], f["du_bound"], tag)}


def _s_dW_d(r, c, tag):
    return _wgrad("dW_d", r["dW_d"], r["dout"], r["hh"], tag)


def _s_dh2(r, c, tag):
    return _dx("dh2", r["dh2"], r["dgu"], torch.cat([c.wg, c.wu]), tag)


def _s_dW_gu(r, c, tag):
    return {"g": _wgrad("dW_gu (gate)", r["dW_g"], r["dgu"][:, :c.I], r["h2"], tag),
            "u": _wgrad("dW_gu (up)", r["dW_u"], r["dgu"][:, c.I:], r["h2"], tag)}


def _s_dz(r, c, tag):
    f = R.ref_norm_bwd(parts_bf16(r["dh2"]), r["z"], c.w2, r["rstd2"], r["dout"], c.mode)
    out = {"dz": R.check("dz", r["dz"], f["dx_ref"], f["dx_bound"], tag)}
    if c.w2_grad:
        out["dw2"] = _norm_dw("dw2", r["dw2"], f, tag)
    return out


def _s_do(r, c, tag):
    return _gemm("do", r["do"], r["dz"], c.wo, tag)


def _s_dW_o(r, c, tag):
    return _wgrad("dW_o", r["dW_o"], r["dz"], r["o"].reshape(c.B * c.S, -1), tag)


def _s_dqkv_unrot(r, c, tag):
    q, k, v = _attn_inputs(r, c)
    do = r["do"].reshape(c.B, c.S, c.nh, c.d)
    b = A.ref_backward(q, k, v, do, r["lse"], A.scale_of(c.d), _mask(c), o=r["o"])
    u = r["dqkv_unrot"]
    return A.check_grads(_heads(u, c, "q"), _heads(u, c, "k"), _heads(u, c, "v"), b, tag)


def _s_dqkv(r, c, tag):
    return _rope("dqkv", r["dqkv_rot"], r["dqkv_unrot"], c, tag, True)


def _s_dqk_norm(r, c, tag):
    """QK-norm backward in place on the q | k columns of the inverse-rotated gradient, and its two
    weight gradients."""
    T = c.B * c.S
    dq, dk = Q.split_heads(r["dqkv_rot"], c.nh, c.nkv, c.d)
    xq, xk = Q.split_heads(r["qkv_raw"], c.nh, c.nkv, c.d)
    gq, gk = Q.split_heads(r["dqkv"], c.nh, c.nkv, c.d)
    rq, rk = Q.rstd_heads(r["rstd_qk"], T, c.nh, c.nkv)
    n = (c.nh + c.nkv) * c.d
    R.check_exact("dqkv (v columns)", r["dqkv"][:, n:], r["dqkv_rot"][:, n:])
    out = {}
    for nm, dy, x, w, rs, got, role in (("q", dq, xq, c.wqn, rq, gq, "dwqn"), ("k", dk, xk, c.wkn, rk, gk, "dwkn")):
        f = Q.ref_bwd(dy, x, w, rs, c.mode)
        out[f"dqkv.{nm}"] = R.check(f"dqkv ({nm} norm backward)", got, f["dx_ref"], f["dx_bound"], tag)
        if r.get(role) is not None:
            out[role] = _norm_dw(role, r[role], f, tag)
    return out


def _s_dh1(r, c, tag):
    return _dx("dh1", r["dh1"], r["dqkv"], torch.cat([c.wq, c.wk, c.wv]), tag)


def _s_dW_qkv(r, c, tag):
    wq, wkv = c.nh * c.d, c.nkv * c.d
    out = {}
    for nm, lo, n in (("q", 0, wq), ("k", wq, wkv), ("v", wq + wkv, wkv)):
        if r.get("dW_" + nm) is not None:
            out[nm] = _wgrad(f"dW_qkv ({nm})", r["dW_" + nm], r["dqkv"][:, lo:lo + n], r["h1"], tag)
    assert out or not c.qkv_grad, "dW_qkv: no recorded call produces it"
    return out


def _s_dx(r, c, tag):
    f = R.ref_norm_bwd(parts_bf16(r["dh1"]), r["x"], c.w1, r["rstd1"], r["dz"], c.mode)
    out = {"dx": R.check("dx", r["dx"], f["dx_ref"], f["dx_bound"], tag)}
    if c.w1_grad:
        out["dw1"] = _norm_dw("dw1", r["dw1"], f, tag)
    return out


LAYER_FWD = [
    Stage("h1 rstd1", "x", _s_norm1),
    Stage("qkv_raw", "h1", _s_qkv_raw),
    Stage("qkv", "qkv_raw", _s_qkv),
    Stage("o lse", "qkv", _s_attn),
    Stage("a", "o", _s_a),
    Stage("z h2 rstd2", "a x", _s_norm2),
    Stage("gu", "h2", _s_gu),
    Stage("hh", "gu", _s_hh),
    Stage("out", "hh z", _s_out),
]
LAYER_BWD = [
    Stage("dhh", "dout", _s_dhh),
    Stage("dgu", "dhh gu", _s_dgu),
    Stage("dW_d", "dout hh", _s_dW_d),
    Stage("dh2", "dgu", _s_dh2),
    Stage("dW_g dW_u", "dgu h2", _s_dW_gu),
    Stage("dz", "dh2 z rstd2 dout", _s_dz),
    Stage("do", "dz", _s_do),
    Stage("dW_o", "dz o", _s_dW_o),
    Stage("dqkv_unrot", "do qkv o lse", _s_dqkv_unrot),
    Stage("dqkv_rot", "dqkv_unrot", _s_dqkv),
    Stage("dh1", "dqkv", _s_dh1),
    Stage("", "dqkv h1", _s_dW_qkv),
    Stage("dx", "dh1 x rstd1 dz", _s_dx),
]
# the QK-norm layer: the norm + RoPE kernel replaces the rotation, its backward follows the inverse rotation
QK_FWD = []
for _s in LAYER_FWD:
    if _s.produces == ("qkv",):
        QK_FWD += [Stage("qk_normed rstd_qk", "qkv_raw", _s_qk_normed), Stage("qk", "qk_normed", _s_qk)]
    else:
        QK_FWD.append(Stage("o lse", "qk qkv_raw", _s_attn) if _s.produces == ("o", "lse") else _s)
QK_BWD = []
for _s in LAYER_BWD:
    if _s.produces == ("dqkv_unrot",):
        _s = Stage("dqkv_unrot", "do qk qkv_raw o lse", _s_dqkv_unrot)
    QK_BWD.append(_s)
    if _s.produces == ("dqkv_rot",):
        QK_BWD.append(Stage("dqkv", "dqkv_rot qkv_raw rstd_qk", _s_dqk_norm))


def layer_stages(c, backward=True):
    qk = getattr(c, "wqn", None) is not None
    return (QK_FWD if qk else LAYER_FWD) + ((QK_BWD if qk else LAYER_BWD) if backward else [])


# ------------------------------------------------------------------------------ head and embedding
def _s_x0(r, c, tag):
    R.check_exact("x0", r["x0"], OR.emu_embedding_fwd(r["ids"], c.wemb, 0, c.wemb.shape[0]))
    return 0.0


def _s_hf(r, c, tag):
    f = R.ref_norm_fwd(r["xf"], None, c.wf, c.eps, c.mode)
    return {"rstdf": R.check("rstdf", r["rstdf"], f["rstd"], f["rstd_bound"], tag),
            "hf": R.check("hf", r["hf"], f["y_ref"], f["y_bound"], tag)}


def _s_logits(r, c, tag):
    return _gemm("logits", r["logits"], r["hf"], c.wlm.t(), tag)


def _ce_ref(r, c):
    """ref_ce_fwd of the production logits as the forward that ran read them, with the LSE bound of that
    forward: the streaming kernel's (four chunks per step), or the statistics' (see the module docstring)."""
    x, tgt = r["logits"], r["targets"]
    Vp = (x.shape[1] + 7) // 8 * 8
    f = R.ref_ce_fwd(x, tgt, c.ignore, style="fma", steps=math.ceil(Vp / 8192))
    lse_bound = f["lse_bound"]
    if r.get("stats") is not None:
        st = r["stats"].to(F64)
        _, merr = R.merge_stats(st[..., 0].t(), st[..., 1].t())
        lse_bound = merr + R.ref_ce_fwd(x, tgt, c.ignore, steps=1)["lse_bound"]
    valid = f["valid"]
    loss_bound = torch.where(valid, lse_bound + R.E * f["loss"].abs(), torch.zeros_like(lse_bound))
    return f, lse_bound, loss_bound


def _s_row_lse(r, c, tag):
    f, lse_bound, _ = _ce_ref(r, c)
    return R.check("row_lse", r["row_lse"], f["lse"], lse_bound, tag)


def _s_loss(r, c, tag):
    f, _, loss_bound = _ce_ref(r, c)
    got, rows = r["loss"], r["targets"].numel()
    count = int(f["valid"].sum())
    out = {}
    if c.reduction == "none":
        b = R.b16(f["loss"], loss_bound) if got.dtype == BF else loss_bound * R.SECOND
        R.check_exact("loss (ignored rows)", got.reshape(-1)[~f["valid"]], torch.zeros(rows - count, dtype=got.dtype))
        out["loss"] = R.check("loss", got.reshape(-1), f["loss"], b, tag)
        assert r.get("inv_count") is None, "inv_count: reduction 'none' has none"
        return out
    S, mass = f["loss"].sum(), f["loss"].abs().sum()
    n = math.ceil(rows / 1024) + 10
    if c.reduction == "sum":
        want, err, cnt = S, loss_bound.sum() + R.gamma(n) * mass, 1
    else:
        want, err, cnt = S / count, (loss_bound.sum() + (R.gamma(n) + R.HW + R.E) * mass) / count, count
    # 1.0f / (float)count is one correctly rounded f32 division (picotron_amd/csrc/cross_entropy.hip ce_mean_kernel): exact
    R.check_exact("inv_count", r["inv_count"].reshape(1), torch.tensor([1.0], dtype=F32) / torch.tensor([float(cnt)], dtype=F32))
    b = R.b16(want, err) if got.dtype == BF else err * R.SECOND
    out["loss"] = R.check("loss", got.reshape(1), want.reshape(1), b.reshape(1), tag)
    out["inv_count"] = 0.0
    return out


def ce_scale_want(r, c):
    """The f32 scale of the CE backward: the incoming gradient (per row for 'none'), times inv_count for 'mean'."""
    g = r["gloss"].to(F32)
    if c.reduction == "none":
        return g.reshape(-1)
    return g.reshape(1) * r["inv_count"].reshape(1) if c.reduction == "mean" else g.reshape(1)


def _s_ce_scale(r, c, tag):
    R.check_exact("ce_scale", r["ce_scale"].reshape(-1), ce_scale_want(r, c))
    return 0.0


def _s_dlogits(r, c, tag):
    x, tgt = r["logits"], r["targets"]
    rows = tgt.numel()
    gs = r["ce_scale"].to(F64).reshape(-1).expand(rows)
    ref, bound = R.ref_ce_bwd(x, tgt, r["row_lse"].to(F64), torch.zeros(rows, dtype=F64), gs, c.ignore, style="fma")
    got = r["dlogits"]
    ign = tgt == c.ignore
    R.check_exact("dlogits (ignored rows)", got[ign], torch.zeros(int(ign.sum()), got.shape[1], dtype=BF))
    return R.check("dlogits", got, ref, bound, tag)


def _s_dhf(r, c, tag):
    return _gemm("dhf", r["dhf"], r["dlogits"], c.wlm, tag)


def _s_dW_lm(r, c, tag):
    return _wgrad("dW_lm", r["dW_lm"], r["dlogits"], r["hf"], tag)


def _s_dxf(r, c, tag):
    f = R.ref_norm_bwd(r["dhf"], r["xf"], c.wf, r["rstdf"], None, c.mode)
    return {"dxf": R.check("dxf", r["dxf"], f["dx_ref"], f["dx_bound"], tag), "dwf": _norm_dw("dwf", r["dwf"], f, tag)}


def _s_dW_emb(r, c, tag):
    s = r["dW_emb"]
    R.check_exact("dW_emb", s["got"], OR.emu_embedding_bwd(r["ids"].reshape(-1), r["dx0"], s["old"], s["sink"], 0,
                                                            c.wemb.shape[0]))
    return 0.0


HEAD_FWD = [
    Stage("x0", "ids", _s_x0),
    Stage("hf rstdf", "xf", _s_hf),
    Stage("logits", "hf", _s_logits),
    Stage("row_lse", "logits targets", _s_row_lse),
    Stage("loss", "logits targets", _s_loss),
]
HEAD_BWD = [
    Stage("ce_scale", "gloss", _s_ce_scale),
    Stage("dlogits", "logits targets row_lse ce_scale", _s_dlogits),
    Stage("dhf", "dlogits", _s_dhf),
    Stage("dW_lm", "dlogits hf", _s_dW_lm),
    Stage("dxf dwf", "dhf xf rstdf", _s_dxf),
    Stage("dW_emb", "ids dx0", _s_dW_emb),
]
CE_STAGES = [s for s in HEAD_FWD + HEAD_BWD if s.produces[0] in ("row_lse", "loss", "ce_scale", "dlogits")]


def check_stages(roles, c, stages, form="default", only=None):
    """Run the stages over a role dictionary; `only`: the produced roles to check (None: every stage).
    Returns {role: worst ratio}; raises AssertionError naming the stage's role."""
    out = {}
    for st in stages:
        if only is not None and not set(st.produces or ("dW_qkv",)) & set(only):
            continue
        for name in st.reads + st.produces:
            if roles.get(name) is None:
                raise AssertionError(f"role {name!r}: no recorded call produces it (stage {st.fn.__name__})")
        label = "/".join(st.produces) or "dW_qkv"
        try:
            res = st.fn(roles, c, form)
        except AssertionError as e:
            raise AssertionError(f"stage {label}: {e}") from None
        _note(form, label, res)
        out[label] = res
    return out


def worst_table(full=True):
    """The worst ratios of this process: per form and role (full), then per role over every form."""
    rows = [f"    {form:<26} {role:<24} {ratio:.3f}" for (form, role), ratio in sorted(WORST.items())] if full else []
    best = {}
    for (form, role), ratio in WORST.items():
        if ratio >= best.get(role, (-1.0, ""))[0]:
            best[role] = (ratio, form)
    summary = [f"    {role:<24} {ratio:.3f}   {form}" for role, (ratio, form) in sorted(best.items())]
    return "\n".join(["    form                       role                     worst |got - ref| / bound"] + rows +
                     ["", "    role                     worst   in form"] + summary)


# ============================================================================== extraction from a trace
def _is(rec, p):
    return isinstance(rec, Rec) and rec.obj is p


def _first_weight(call):
    w = call.arg(1, "weights")
    return w[0] if isinstance(w, (list, tuple)) and w else w


class Cursor:
    def __init__(self, calls, at=0):
        self.calls, self.at = calls, at

    def next(self, names, pred=None, what=""):
        names = (names,) if isinstance(names, str) else names
        for i in range(self.at, len(self.calls)):
            c = self.calls[i]
            if c.name == "linear_dgrad_dual" and c.result is None:   # refused: the caller launched the separate forms
                continue
            if c.name in names and (pred is None or pred(c)):
                self.at = i + 1
                return c
        raise AssertionError(f"role {what!r}: no recorded call produces it (looked for {' / '.join(names)})")


def _bits_equal(what, a, b):
    a, b = cpu(a).contiguous(), cpu(b).contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype} {tuple(a.shape)} != {b.dtype} {tuple(b.shape)}"
    diff = R.ibits(a) != R.ibits(b)
    assert not bool(diff.any()), (f"{what}: the fused form differs from its separate kernels in {int(diff.sum())} of "
                                  f"{diff.numel()} elements, first at {tuple(int(i) for i in diff.nonzero()[0])}")


def sink_events(calls, sinks):
    """{parameter name: [event]} of every weight-gradient launch in the trace, in order.  sinks: {data_ptr:
    name} of the gradient buffers.  event: dict got, old, epi, dy, x (Rec or Pair; dy the column segment of the
    launch's dY that belongs to the parameter), call (index)."""
    ev = {}
    for i, c in enumerate(calls):
        if c.name == "linear_wgrad":
            jobs, epi = [(c.arg(0), c.arg(1), c.arg(2))], c.arg(3, "epilogue")
        elif c.name == "linear_wgrad_grouped":
            jobs, epi = c.arg(0), c.arg(1, "epilogue")
        elif c.name == "linear_dgrad_dual":
            if c.result is None:   # refused (the shapes do not tile): nothing was launched
                continue
            jobs, epi = c.arg(2), c.arg(3)
        else:
            continue
        epi = G.EPI_BF16 if epi is None else epi
        # a paired group with a sink off the 256-row tile runs unpaired (picotron_amd/csrc/gemm.hip args_fit, kernels._wgrad_unpaired)
        unpaired = c.name != "linear_dgrad_dual" and any(o.key[1][0] % 256 for _, _, outs in jobs for o in outs)
        for dy, x, outs in jobs:
            lo = 0
            for o in outs:
                n = o.key[1][0]
                name = sinks.get(o.key[0])
                if name is not None:
                    ev.setdefault(name, []).append(dict(got=cpu(o.post), old=cpu(o.pre), epi=epi, dy=dy, x=x, lo=lo, n=n,
                                                        call=i, unpaired=unpaired))
                lo += n
    return ev


def norm_sink_events(calls, sinks):
    """{parameter name: [event]} of the norm weight-gradient sums: rmsnorm_bwd(dw_out=) and the jobs of
    rmsnorm_colsum_batch; event: dict got, old, sink, partial (the Rec of the partial rows, or None)."""
    ev = {}
    for i, c in enumerate(calls):
        if c.name == "rmsnorm_bwd" and c.kwargs.get("dw_out") is not None:
            o = c.kwargs["dw_out"]
            jobs = [(None, o, c.kwargs.get("dw_sink", 0))]
        elif c.name == "rmsnorm_colsum_batch":
            jobs = c.arg(0)
        else:
            continue
        for part, o, sink in jobs:
            name = sinks.get(o.key[0])
            if name is not None:
                ev.setdefault(name, []).append(dict(got=cpu(o.post), old=cpu(o.pre), sink=sink, partial=part, call=i))
    return ev


def _wsink(ev, name, after, role):
    """The first weight-gradient event of parameter `name` at or after call index `after`."""
    for e in ev.get(name, []):
        if e["call"] >= after:
            return e
    raise AssertionError(f"role {role!r}: no recorded call produces it (no weight-gradient launch into {name})")


def _sink_role(e):
    out = dict(got=e["got"], old=e["old"], epi=e["epi"])
    if isinstance(e["dy"], Pair):
        lo, n = e["lo"], e["n"]
        out["prev"] = (cpu(e["dy"][0].pre)[:, lo:lo + n] if e["dy"][0].key[1][1] != n else cpu(e["dy"][0].pre),
                       cpu(e["x"][0].pre))
        out["unpaired"] = e["unpaired"]
    return out


def _norm_sink(nev, name, partial, after, role):
    """The norm weight-gradient event fed by `partial` (a Rec: the deferred sum's rows), else the first
    direct one at or after call `after`."""
    for e in nev.get(name, []):
        if partial is not None and e["partial"] is not None and e["partial"].same(partial) and e["call"] >= after:
            return dict(got=e["got"], old=e["old"], sink=e["sink"])
        if partial is None and e["partial"] is None and e["call"] >= after:
            return dict(got=e["got"], old=e["old"], sink=e["sink"])
    raise AssertionError(f"role {role!r}: no recorded call produces it (no column sum into {name})")


def _dxval(res):
    return (cpu(res[0].post), cpu(res[1].post)) if isinstance(res, Parts) else cpu(res.post)


def layer_config(layer, B, S, mask=None):
    """The constants of one decoder layer (CPU weights, tables, shape) for the stages."""
    at, mlp = layer.attention, layer.mlp
    n1 = layer.input_layernorm
    flash = hasattr(n1, "eps")
    w = lambda p: cpu(p)   # noqa: E731
    c = types.SimpleNamespace(
        B=B, S=S, nh=at.num_local_heads, nkv=at.num_local_kv_heads, d=at.head_dim, I=mlp.gate_proj.weight.shape[0],
        eps=n1.eps if flash else n1.variance_epsilon, mode=0 if flash else 1, mask=mask,
        w1=w(n1.weight), w2=w(layer.post_attention_layernorm.weight), wq=w(at.q_proj.weight), wk=w(at.k_proj.weight),
        wv=w(at.v_proj.weight), wo=w(at.out_proj.weight), wg=w(mlp.gate_proj.weight), wu=w(mlp.up_proj.weight),
        wd=w(mlp.down_proj.weight), cos=w(layer.cos)[:S].to(BF), sin=w(layer.sin)[:S].to(BF),
        w1_grad=n1.weight.requires_grad, w2_grad=layer.post_attention_layernorm.weight.requires_grad,
        qkv_grad=any(p.requires_grad for p in (at.q_proj.weight, at.k_proj.weight, at.v_proj.weight)),
        wqn=w(at.q_norm.weight) if at.qk_norm else None, wkn=w(at.k_norm.weight) if at.qk_norm else None)
    return c


def extract_layer_fwd(K, layer, cur, c):
    """The forward roles of one decoder layer from the trace at cursor `cur` (advanced past the layer)."""
    P = dict(w1=layer.input_layernorm.weight, w2=layer.post_attention_layernorm.weight)
    r = {}
    n1 = cur.next("rmsnorm_fwd", lambda k: _is(k.arg(1), P["w1"]) and k.kwargs.get("residual") is None, "h1")
    r["x"] = cpu(n1.arg(0).pre)
    r["h1"], r["rstd1"] = cpu(n1.result[0].post), cpu(n1.result[1].post)
    extract_attn_fwd(K, layer, cur, c, r, n1.result[0].post)
    n2 = cur.next("rmsnorm_fwd", lambda k: _is(k.arg(1), P["w2"]) and k.kwargs.get("residual") is not None, "h2")
    r["h2"], r["rstd2"], r["z"] = (cpu(t.post) for t in n2.result)
    extract_mlp_fwd(K, layer, cur, c, r, n2.result[0].post)
    return r


def extract_attn_fwd(K, layer, cur, c, r, h1):
    """The attention block's forward roles (qkv_raw, qkv / qk, o, lse, a) from the trace at `cur`; h1: the
    device value the q|k|v GEMM read (the replays run on it)."""
    at = layer.attention
    P = dict(wq=at.q_proj.weight, wo=at.out_proj.weight)
    qc = cur.next(("linear_fwd_rope", "linear_fwd"), lambda k: _is(_first_weight(k), P["wq"]), "qkv")
    dev = dict(h1=qc.arg(0).pre if h1 is None else h1)   # (None: the recorded input of the launch)
    ws = [at.q_proj.weight, at.k_proj.weight, at.v_proj.weight]
    if qc.name == "linear_fwd_rope":
        with single_pass():
            raw = K.linear_fwd(dev["h1"], ws)
        rot = K.rope_(raw.clone(), c.nh + c.nkv, c.d, qc.arg(2).pre, qc.arg(3).pre, c.S)
        _bits_equal("qkv: linear_fwd_rope vs linear_fwd + rope_", qc.result.post, rot)
        r["qkv_raw"], r["qkv"] = cpu(raw), cpu(qc.result.post)
    else:
        r["qkv_raw"] = cpu(qc.result.post)
        if c.wqn is not None:
            nq = cur.next("qk_norm_rope_fwd", lambda k: k.arg(0).same(qc.result), "qk")
            r["qk"], r["rstd_qk"] = cpu(nq.result[0].post), cpu(nq.result[1].post)
            _bits_equal("qkv after qk_norm_rope_fwd (the raw projection is kept)", nq.arg(0).post, qc.result.post)
            y, rs = K.qk_norm_rope_fwd(nq.arg(0).pre, c.nh, c.nkv, c.d, at.q_norm.weight, at.k_norm.weight, c.eps, c.mode,
                                       None, None, c.S)
            r["qk_normed"] = cpu(y)
            _bits_equal("rstd_qk: qk_norm_rope_fwd vs its norm-only call", nq.result[1].post, rs)
            K.rope_(y, c.nh + c.nkv, c.d, nq.arg(8).pre, nq.arg(9).pre, c.S)
            _bits_equal("qk: qk_norm_rope_fwd vs its norm-only call + rope_", nq.result[0].post, y)
        else:
            rc = cur.next("rope_", lambda k: k.arg(0).same(qc.result) and not k.kwargs.get("inverse", False), "qkv")
            r["qkv"] = cpu(rc.arg(0).post)
    ac = cur.next("attn_fwd", None, "o")
    r["o"], r["lse"] = cpu(ac.result[0].post), cpu(ac.result[1].post)
    oc = cur.next("linear_fwd", lambda k: _is(_first_weight(k), P["wo"]), "a")
    r["a"] = cpu(oc.result.post)
    return qc


def extract_mlp_fwd(K, layer, cur, c, r, h2, residual=True):
    """The MLP block's forward roles (gu, hh, out) from the trace at `cur`; h2: the device value the gate|up GEMM
    read.  residual: whether the down projection's launch carries the residual epilogue (None: either; the
    tensor-parallel forms: tests/_tp_ref.py)."""
    mlp = layer.mlp
    P = dict(wg=mlp.gate_proj.weight, wd=mlp.down_proj.weight)
    gc = cur.next(("linear_swiglu_fwd", "linear_fwd"), lambda k: _is(k.arg(1), P["wg"]) or _is(_first_weight(k), P["wg"]), "gu")
    dev = dict(h2=gc.arg(0).pre if h2 is None else h2)   # (None: the recorded input of the launch)
    if gc.name == "linear_swiglu_fwd":
        with single_pass():
            gu = K.linear_fwd(dev["h2"], [mlp.gate_proj.weight, mlp.up_proj.weight])
        hh = K.swiglu_fwd(gu[:, :c.I], gu[:, c.I:])
        _bits_equal("gu: linear_swiglu_fwd vs linear_fwd", gc.result[0].post, gu)
        _bits_equal("hh: linear_swiglu_fwd vs linear_fwd + swiglu_fwd", gc.result[1].post, hh)
        r["gu"], r["hh"] = cpu(gc.result[0].post), cpu(gc.result[1].post)
    else:
        r["gu"] = cpu(gc.result.post)
        sc = cur.next("swiglu_fwd", None, "hh")
        r["hh"] = cpu(sc.result.post)
    dc = cur.next("linear_fwd", lambda k: _is(_first_weight(k), P["wd"]) and
                  (residual is None or (k.kwargs.get("residual") is not None) == residual), "out")
    r["out"] = cpu(dc.result.post)
    r["_dev"] = dict(gu=gc.result[0].post if gc.name == "linear_swiglu_fwd" else gc.result.post)
    return gc, dc


def extract_layer_bwd(K, layer, names, cur, c, r, wev, nev, wgrads=True):
    """The backward roles of one decoder layer (its forward roles in r) from the trace at cursor `cur`.
    names: the parameters' names in the sink tables wev / nev (dict w1, w2, wq, wk, wv, wo, wg, wu, wd[, wqn, wkn]).
    wgrads=False: a micro-batch that deferred its weight-gradient GEMMs to its pair -- no dW role."""
    if not wgrads:
        wev = None
    start = cur.at
    extract_mlp_bwd(K, layer, names, cur, c, r, wev)
    n2 = cur.next("rmsnorm_bwd", lambda k: _is(k.arg(2), layer.post_attention_layernorm.weight), "dz")
    r["dz"] = cpu(n2.result[0].post)
    if c.w2_grad:
        r["dw2"] = _norm_sink(nev, names["w2"], n2.result[1] if n2.kwargs.get("defer_dw") else None, start, "dw2")
    extract_attn_bwd(K, layer, names, cur, c, r, wev, nev, start)
    n1 = cur.next("rmsnorm_bwd", lambda k: _is(k.arg(2), layer.input_layernorm.weight), "dx")
    r["dx"] = cpu(n1.result[0].post)
    if c.w1_grad:
        r["dw1"] = _norm_sink(nev, names["w1"], n1.result[1] if n1.kwargs.get("defer_dw") else None, start, "dw1")
    return r


def extract_mlp_bwd(K, layer, names, cur, c, r, wev):
    """The MLP block's backward roles (dout, dhh, dgu, dW_d, dh2, dW_g, dW_u) from the trace at `cur`; returns
    the gate|up dX call."""
    mlp = layer.mlp
    wd, wg = mlp.down_proj.weight, mlp.gate_proj.weight
    I, start = c.I, cur.at
    dc = cur.next(("linear_dgrad_dual", "linear_dgrad_swiglu", "linear_dgrad"),
                  lambda k: _is(_first_weight(k), wd) or _is(k.arg(1), wd), "dgu")
    dout = dc.arg(0).pre
    r["dout"] = cpu(dout)
    if dc.name == "linear_dgrad":
        r["dhh"] = cpu(dc.result.post)
        sc = cur.next("swiglu_bwd", None, "dgu")
        r["dgu"] = torch.cat([cpu(sc.kwargs["dg"].post), cpu(sc.kwargs["du"].post)], 1)
    else:
        dgu_rec = dc.result
        gu = r["_dev"]["gu"]
        with single_pass():
            dhh = K.linear_dgrad(dout, [wd])
        dgu = torch.empty_like(gu)
        K.swiglu_bwd(dhh, gu[:, :I], gu[:, I:], dg=dgu[:, :I], du=dgu[:, I:])
        r["dgu_sliced"] = dc.name == "linear_dgrad_dual" and K.swiglu_dx_ksplit(dout.shape[0], I, dout.shape[1]) > 1
        if not r["dgu_sliced"]:   # (K-sliced: another f32 summation order, see _s_dgu_sliced)
            _bits_equal(f"dgu: {dc.name} vs linear_dgrad + swiglu_bwd", dgu_rec.post, dgu)
        r["dhh"], r["dgu"] = cpu(dhh), cpu(dgu_rec.post)
    if wd.requires_grad and wev is not None:
        r["dW_d"] = _sink_role(_wsink(wev, names["wd"], start, "dW_d"))
    gc = cur.next(("linear_dgrad_dual", "linear_dgrad"), lambda k: _is(_first_weight(k), wg), "dh2")
    r["dh2"] = _dxval(gc.result)
    for nm, role in (("wg", "dW_g"), ("wu", "dW_u")):
        if wev is not None:
            r[role] = _sink_role(_wsink(wev, names[nm], start, role))
    return gc


def extract_attn_bwd(K, layer, names, cur, c, r, wev, nev, start=None):
    """The attention block's backward roles (do, dqkv_unrot, dqkv_rot, dqkv, dW_o, dh1, dW_q / k / v) from the
    trace at `cur`; returns the q|k|v dX call."""
    at = layer.attention
    wo, wq = at.out_proj.weight, at.q_proj.weight
    start = cur.at if start is None else start
    oc = cur.next("linear_dgrad", lambda k: _is(_first_weight(k), wo), "do")
    r.setdefault("dz", cpu(oc.arg(0).pre))   # (a block on its own: the gradient the out projection's dX read)
    r["do"] = cpu(oc.result.post)
    ab = cur.next("attn_bwd", None, "dqkv")
    got = torch.cat([cpu(ab.kwargs[k].post).reshape(c.B * c.S, -1) for k in ("dq", "dk", "dv")], 1)
    if ab.kwargs.get("rope") is not None:
        a = [x.pre for x in ab.args[:6]]
        buf = torch.empty(c.B * c.S, got.shape[1], dtype=BF, device=a[0].device)
        sh = types.SimpleNamespace(**vars(c))
        view = lambda w: _heads(buf, sh, w)   # noqa: E731
        K.attn_bwd(*a, ab.args[6], ab.args[7], dq=view("q"), dk=view("k"), dv=view("v"), band=ab.kwargs.get("band"))
        r["dqkv_unrot"] = cpu(buf)
        cos, sin = ab.kwargs["rope"]
        K.rope_(buf, c.nh + c.nkv, c.d, cos.pre, sin.pre, c.S, inverse=True)
        _bits_equal("dqkv: attn_bwd(rope=) vs attn_bwd + rope_(inverse)", got, buf)
        r["dqkv_rot"] = got
    else:
        rc = cur.next("rope_", lambda k: k.kwargs.get("inverse", False), "dqkv")
        r["dqkv_unrot"], r["dqkv_rot"] = got, cpu(rc.arg(0).post)
    r["dqkv"] = r["dqkv_rot"]
    if c.wqn is not None:
        qb = cur.next("qk_norm_bwd", None, "dqkv")
        r["dqkv"] = cpu(qb.kwargs["dx"].post)
        for nm, role, part in (("wqn", "dwqn", qb.result[1]), ("wkn", "dwkn", qb.result[2])):
            if part is not None:
                r[role] = _norm_sink(nev, names[nm], part, start, role)
    if wo.requires_grad and wev is not None:
        r["dW_o"] = _sink_role(_wsink(wev, names["wo"], start, "dW_o"))
    xc = cur.next(("linear_dgrad_dual", "linear_dgrad"), lambda k: _is(_first_weight(k), wq), "dh1")
    r["dh1"] = _dxval(xc.result)
    for nm, p in (("q", at.q_proj.weight), ("k", at.k_proj.weight), ("v", at.v_proj.weight)):
        if p.requires_grad and wev is not None:
            r["dW_" + nm] = _sink_role(_wsink(wev, names["w" + nm], start, "dW_qkv"))
    return xc


def head_config(model, reduction="mean", ignore=IGNORE):
    fn = model.final_norm
    flash = hasattr(fn, "eps")
    return types.SimpleNamespace(eps=fn.eps if flash else fn.variance_epsilon, mode=0 if flash else 1, wf=cpu(fn.weight),
                                 wlm=cpu(model.final_proj.weight), wemb=cpu(model.embedding.weight), reduction=reduction,
                                 ignore=ignore)


def extract_ce(K, calls, at=0, gloss=None):
    """The CE roles (logits, targets, stats, row_lse, loss, inv_count; with a backward: ce_scale, dlogits)
    of the first cross-entropy forward at or after call `at`: (roles, forward call name, cursor)."""
    cur = Cursor(calls, at)
    fc = cur.next(("cross_entropy_loss_lse", "cross_entropy_loss_lse_stats"), None, "row_lse")
    r = dict(logits=cpu(fc.arg(0).pre), targets=cpu(fc.arg(1).pre))
    if fc.name.endswith("_stats"):
        r["stats"] = cpu(fc.arg(2).pre)
    r["loss"], r["row_lse"] = cpu(fc.result[0].post), cpu(fc.result[2].post)
    r["inv_count"] = cpu(fc.result[1].post) if fc.result[1] is not None else None
    if gloss is not None:
        bc = cur.next("cross_entropy_grad_lse", None, "dlogits")
        r["gloss"], r["ce_scale"], r["dlogits"] = cpu(gloss), cpu(bc.arg(3).pre), cpu(bc.result.post)
        _bits_equal("the backward's logits are the forward's", bc.arg(0).pre, fc.arg(0).pre)
        _bits_equal("the backward's row_lse is the forward's", bc.arg(2).pre, fc.result[2].post)
        r["_bwd"] = bc
    return r, fc.name, cur


def trim_vocab(r, V):
    """The padded-CE path (V off the 8-column grid): the -inf columns dropped from the recorded logits /
    dlogits, after checking that they are what the padding says."""
    if r["logits"].shape[1] != V:
        assert bool((r["logits"][:, V:] == -math.inf).all()), "logits: the padding columns must hold -inf"
        r["logits"] = r["logits"][:, :V].contiguous()
        if "dlogits" in r:
            R.check_exact("dlogits (padding columns)", r["dlogits"][:, V:], torch.zeros_like(r["dlogits"][:, V:]))
            r["dlogits"] = r["dlogits"][:, :V].contiguous()
    return r


def layer_names(model, i):
    """The names of layer i's parameters in model.named_parameters() (a Parameter shared between layers is
    listed once there, under its first name), by identity."""
    name_of = {id(p): n for n, p in model.named_parameters()}
    layer = model.decoder_layers[i]
    at, mlp = layer.attention, layer.mlp
    ps = dict(w1=layer.input_layernorm.weight, w2=layer.post_attention_layernorm.weight, wq=at.q_proj.weight,
              wk=at.k_proj.weight, wv=at.v_proj.weight, wo=at.out_proj.weight, wg=mlp.gate_proj.weight,
              wu=mlp.up_proj.weight, wd=mlp.down_proj.weight)
    if at.qk_norm:
        ps.update(wqn=at.q_norm.weight, wkn=at.k_norm.weight)
    return {k: name_of[id(p)] for k, p in ps.items()}


def grad_sinks(model):
    """{data_ptr: parameter name} of the gradient buffers (main_grad where there is one, else .grad)."""
    out = {}
    for n, p in model.named_parameters():
        g = getattr(p, "main_grad", None)
        g = p.grad if g is None else g
        if g is not None:
            out[g.data_ptr()] = n
    return out


def extract_model(K, calls, model, B, S, gloss, mask=None, reduction="mean", at=0, wgrads=True):
    """Every role of one forward + backward of a Llama (tp = 1) from the recorded calls at or after `at`:
    ([(layer constants, layer roles)], head constants, head roles, the CE forward's call name).  Besides the
    roles it asserts, by bits, that each stage received the production value of the role the model's
    data flow hands it (a layer's x is the previous layer's out, its dout the next layer's dx, ...)."""
    V = model.final_proj.weight.shape[0]
    sinks = grad_sinks(model)
    wev, nev = sink_events(calls, sinks), norm_sink_events(calls, sinks)
    cur = Cursor(calls, at)
    h = {}
    ec = cur.next("embedding_fwd", None, "x0")
    h["ids"], h["x0"] = cpu(ec.arg(0).pre), cpu(ec.result.post).reshape(B * S, -1)
    layers = []
    prev = h["x0"]
    for i, layer in enumerate(model.decoder_layers):
        c = layer_config(layer, B, S, mask)
        r = extract_layer_fwd(K, layer, cur, c)
        _bits_equal(f"layer {i}: x is the previous stage's output", r["x"], prev)
        prev = r["out"]
        layers.append((c, r))
    hc = head_config(model, reduction)
    fc = cur.next("rmsnorm_fwd", lambda k: _is(k.arg(1), model.final_norm.weight), "hf")
    h["xf"], h["hf"], h["rstdf"] = cpu(fc.arg(0).pre), cpu(fc.result[0].post), cpu(fc.result[1].post)
    _bits_equal("xf is the last layer's out", h["xf"], prev)
    lc = cur.next(("linear_ce_stats", "linear_fwd"),
                  lambda k: _is(k.arg(1), model.final_proj.weight) or _is(_first_weight(k), model.final_proj.weight), "logits")
    if lc.name == "linear_ce_stats":
        with single_pass():
            plain = K.linear_fwd(fc.result[0].post, [model.final_proj.weight])
        _bits_equal("logits: linear_ce_stats vs linear_fwd", lc.result[0].post, plain)
        lg = lc.result[0].post
    else:
        lg = lc.result.post
    ce, ce_name, ccur = extract_ce(K, calls, cur.at, gloss)
    trim_vocab(ce, V)
    _bits_equal("the CE's logits are the lm_head's", ce["logits"], lg)
    assert (ce.get("stats") is not None) == (lc.name == "linear_ce_stats"), "CE statistics without the statistics GEMM"
    if ce.get("stats") is not None:
        _bits_equal("the CE's statistics are the lm_head's", ce["stats"], lc.result[1].post)
    h.update({k: v for k, v in ce.items() if not k.startswith("_")})
    cur = ccur
    start = cur.at
    dc = cur.next("linear_dgrad", lambda k: _is(_first_weight(k), model.final_proj.weight), "dhf")
    h["dhf"] = cpu(dc.result.post)
    if wgrads:
        h["dW_lm"] = _sink_role(_wsink(wev, "final_proj.weight", start, "dW_lm"))
    nb = cur.next("rmsnorm_bwd", lambda k: _is(k.arg(2), model.final_norm.weight), "dxf")
    h["dxf"] = cpu(nb.result[0].post)
    h["dwf"] = _norm_sink(nev, "final_norm.weight", nb.result[1] if nb.kwargs.get("defer_dw") else None, start, "dwf")
    nxt = h["dxf"]
    for i in reversed(range(len(layers))):
        c, r = layers[i]
        extract_layer_bwd(K, model.decoder_layers[i], layer_names(model, i), cur, c, r, wev, nev, wgrads)
        _bits_equal(f"layer {i}: dout is the next stage's dx", r["dout"], nxt)
        nxt = r["dx"]
    eb = cur.next("embedding_bwd", None, "dW_emb")
    h["dx0"] = cpu(eb.arg(1).pre)
    _bits_equal("dx0 is layer 0's dx", h["dx0"], nxt)
    h["dW_emb"] = dict(got=cpu(eb.arg(2).post), old=cpu(eb.arg(2).pre), sink=eb.arg(3))
    return layers, hc, h, ce_name


def check_model(layers, hc, h, form, only=None):
    """check_stages over every layer and the head; returns {label: ratios}."""
    out = {}
    for i, (c, r) in enumerate(layers):
        for k, v in check_stages(r, c, layer_stages(c), form, only).items():
            out[f"L{i} {k}"] = v
    out.update(check_stages(h, hc, HEAD_FWD + HEAD_BWD, form, only))
    return out


# ============================================================================== CPU emulation
FAULTS = ("dW_gu_x_for_z", "sink_store_for_accumulate", "norm_partial_row_missing", "pair_half_missing",
          "ce_scale_without_inv_count", "ce_stats_of_other_logits", "dres_omitted", "gqa_kv_head_offset")
# fault -> (the stage that must reject it, the role its failure names)
FAULT_ROLE = {"dW_gu_x_for_z": ("dW_g/dW_u", "dW_gu"), "sink_store_for_accumulate": ("dW_d", "dW_d"),
              "norm_partial_row_missing": ("dx", "dw1"), "pair_half_missing": ("dW_o", "dW_o"),
              "ce_scale_without_inv_count": ("ce_scale", "ce_scale"), "ce_stats_of_other_logits": ("row_lse", "row_lse"),
              "dres_omitted": ("dz", "dz"), "gqa_kv_head_offset": ("o/lse", "o")}


def emu_config(B=1, S=128, H=256, I=256, nh=4, nkv=2, V=256, mode=0, seed=0):
    g = R._gen("model", B, S, H, I, V, seed)
    d = H // nh
    rn = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(BF)   # noqa: E731
    nw = lambda n: (1 + 0.1 * torch.randn(n, generator=g)).to(BF)   # noqa: E731
    ang = torch.arange(S, dtype=F64)[:, None] / 10000.0 ** (torch.arange(0, d, 2, dtype=F64) / d)[None, :]
    return types.SimpleNamespace(
        B=B, S=S, nh=nh, nkv=nkv, d=d, I=I, eps=1e-5, mode=mode, mask=None, ignore=IGNORE, reduction="mean",
        w1=nw(H), w2=nw(H), wf=nw(H), wq=rn(nh * d, H, k=H ** -0.5), wk=rn(nkv * d, H, k=H ** -0.5),
        wv=rn(nkv * d, H, k=H ** -0.5), wo=rn(H, H, k=H ** -0.5), wg=rn(I, H, k=H ** -0.5), wu=rn(I, H, k=H ** -0.5),
        wd=rn(H, I, k=I ** -0.5), wlm=rn(V, H, k=H ** -0.5), wemb=rn(V, H), cos=torch.cos(ang).repeat(1, 2).to(BF),
        sin=torch.sin(ang).repeat(1, 2).to(BF), w1_grad=True, w2_grad=True, qkv_grad=True, wqn=None, wkn=None,
        ids=torch.randint(0, V, (B, S), generator=g), targets=torch.randint(0, V, (B * S,), generator=g), gen=g)


def _old(c, shape, dtype=BF, k=0.05):
    return (torch.randn(*shape, generator=c.gen) * k).to(dtype)


def _emu_sink(c, dy, x, epi, fault=False, prev=None, drop_prev=False):
    """A weight-gradient role from the emulator: onto a random prior sink (a second micro-batch)."""
    old = _old(c, (dy.shape[1], x.shape[1]), G.sink_dtype(epi))
    a, b = dy.t(), x
    if prev is not None and not drop_prev:
        a, b = torch.cat([prev[0].t(), a], 1), torch.cat([prev[1], b], 0)
    got = G.emu_gemm(a.contiguous(), b.contiguous(), G.EPI_BF16 if fault else epi, old=old)
    out = dict(got=got, old=old, epi=epi)
    if prev is not None:
        out["prev"] = prev
    return out


def _emu_norm_bwd(c, dy, z, w, rstd, dres, sink, drop_row=False):
    """(dx, norm weight-gradient role): per-block f32 partial rows summed into the sink, as the deferred
    column sum does; drop_row leaves the last partial row out."""
    old = _old(c, (z.shape[1],), F32 if sink == R.PT_DW_ACC_F32 else BF)
    if drop_row:
        dx, _ = R.emu_norm_bwd(dy, z, w, rstd, dres, c.mode)
        _, dw = R.emu_norm_bwd(dy[:-16], z[:-16], w, rstd[:-16], None, c.mode, sink, old)
    else:
        dx, dw = R.emu_norm_bwd(dy, z, w, rstd, dres, c.mode, sink, old)
    return dx, dict(got=dw, old=old, sink=sink)


def emu_model(c, fault=None, split_dx=False):
    """(layer roles, head roles) of embedding -> one decoder layer -> final norm -> lm_head -> mean CE, forward
    and backward, as the HIP path computes them; the sinks hold prior contents (a second micro-batch)."""
    assert fault is None or fault in FAULTS, fault
    T, I = c.B * c.S, c.I
    r, h = {}, {}
    h["ids"] = c.ids
    h["x0"] = OR.emu_embedding_fwd(c.ids.reshape(-1), c.wemb, 0, c.wemb.shape[0])
    x = r["x"] = h["x0"]
    r["h1"], _, r["rstd1"] = R.emu_norm_fwd(x, None, c.w1, c.eps, c.mode)
    wqkv, wgu = torch.cat([c.wq, c.wk, c.wv]), torch.cat([c.wg, c.wu])
    r["qkv_raw"] = G.emu_gemm(r["h1"], wqkv.t().contiguous(), G.EPI_BF16)
    r["qkv"] = R.emu_rope(r["qkv_raw"], c.nh + c.nkv, c.d, c.cos, c.sin, c.S)
    q, k, v = (_heads(r["qkv"], c, n) for n in "qkv")
    sc = A.scale_of(c.d)
    kk, vv = (k.roll(1, 2), v.roll(1, 2)) if fault == "gqa_kv_head_offset" else (k, v)
    r["o"], r["lse"] = A.emu_forward(q, kk, vv, sc, True)
    r["a"] = G.emu_gemm(r["o"].reshape(T, -1), c.wo.t().contiguous(), G.EPI_BF16)
    r["h2"], r["z"], r["rstd2"] = R.emu_norm_fwd(r["a"], x, c.w2, c.eps, c.mode)
    r["gu"] = G.emu_gemm(r["h2"], wgu.t().contiguous(), G.EPI_BF16)
    gg, uu = r["gu"][:, :I], r["gu"][:, I:]
    r["hh"] = R.emu_swiglu(gg, uu, torch.zeros_like(gg))[0]
    r["out"] = G.emu_gemm(r["hh"], c.wd.t().contiguous(), G.EPI_BF16_RES, residual=r["z"])
    # head forward
    h["xf"] = r["out"]
    h["hf"], _, h["rstdf"] = R.emu_norm_fwd(h["xf"], None, c.wf, c.eps, c.mode)
    h["logits"] = G.emu_gemm(h["hf"], c.wlm.t().contiguous(), G.EPI_BF16)
    tgt = c.targets.clone()
    tgt[::19] = c.ignore
    h["targets"] = tgt
    valid = tgt != c.ignore
    lf = h["logits"].to(F32)
    if fault == "ce_stats_of_other_logits":   # the statistics of another lm_head call's logits
        lf = G.emu_gemm(h["hf"].roll(1, 0), c.wlm.t().contiguous(), G.EPI_BF16).to(F32)
    h["row_lse"] = torch.logsumexp(lf, 1)
    row_loss = torch.where(valid, h["row_lse"] - h["logits"].to(F32)[torch.arange(T), tgt.clamp_min(0)], torch.zeros(T))
    inv = torch.tensor([1.0], dtype=F32) / torch.tensor([float(valid.sum())], dtype=F32)
    h["inv_count"] = inv
    h["loss"] = (row_loss.sum() * inv[0]).to(BF)
    # head backward
    h["gloss"] = torch.tensor(0.25, dtype=BF)
    h["ce_scale"] = h["gloss"].to(F32).reshape(1) * (1.0 if fault == "ce_scale_without_inv_count" else inv)
    _, h["dlogits"] = R.emu_ce(h["logits"], tgt, h["ce_scale"].expand(T))
    if fault == "ce_stats_of_other_logits":
        p = torch.exp(h["logits"].to(F32) - h["row_lse"][:, None])
        oh = (torch.arange(lf.shape[1])[None, :] == tgt[:, None]).to(F32)
        h["dlogits"] = ((p - oh) * torch.where(valid, h["ce_scale"].expand(T), torch.zeros(T))[:, None]).to(BF)
    h["dhf"] = G.emu_gemm(h["dlogits"], c.wlm, G.EPI_BF16)
    h["dW_lm"] = _emu_sink(c, h["dlogits"], h["hf"], G.EPI_BF16_ACC)
    h["dxf"], h["dwf"] = _emu_norm_bwd(c, h["dhf"], h["xf"], c.wf, h["rstdf"], None, R.PT_DW_ACC_BF16)
    # layer backward
    dout = r["dout"] = h["dxf"]
    r["dhh"] = G.emu_gemm(dout, c.wd, G.EPI_BF16)
    _, dg, du = R.emu_swiglu(gg, uu, r["dhh"])
    r["dgu"] = torch.cat([dg, du], 1)
    r["dW_d"] = _emu_sink(c, dout, r["hh"], G.EPI_BF16_ACC, fault=fault == "sink_store_for_accumulate")
    if split_dx:
        r["dh2"] = (G.emu_gemm(r["dgu"][:, :I], wgu[:I], G.EPI_F32), G.emu_gemm(r["dgu"][:, I:], wgu[I:], G.EPI_F32))
    else:
        r["dh2"] = G.emu_gemm(r["dgu"], wgu, G.EPI_BF16)
    h2 = r["h2"]
    if fault == "dW_gu_x_for_z":   # the operand is the norm of x where the norm of z = x + a was meant
        h2 = R.emu_norm_fwd(x, None, c.w2, c.eps, c.mode)[0]
    r["dW_g"] = _emu_sink(c, r["dgu"][:, :I], h2, G.EPI_F32_ACC)
    r["dW_u"] = _emu_sink(c, r["dgu"][:, I:], h2, G.EPI_F32_ACC)
    r["dz"], r["dw2"] = _emu_norm_bwd(c, parts_bf16(r["dh2"]), r["z"], c.w2, r["rstd2"],
                                      None if fault == "dres_omitted" else dout, R.PT_DW_ACC_F32)
    r["do"] = G.emu_gemm(r["dz"], c.wo, G.EPI_BF16)
    prev = (_old(c, (T, c.wo.shape[0]), k=0.02), (torch.randn(T, c.nh * c.d, generator=c.gen)).to(BF))
    r["dW_o"] = _emu_sink(c, r["dz"], r["o"].reshape(T, -1), G.EPI_BF16_ACC, prev=prev, drop_prev=fault == "pair_half_missing")
    dq, dk, dv, _ = A.emu_backward(q, k, v, r["do"].reshape(c.B, c.S, c.nh, c.d), r["o"], r["lse"], sc, True)
    r["dqkv_unrot"] = torch.cat([t.reshape(T, -1) for t in (dq, dk, dv)], 1)
    r["dqkv_rot"] = r["dqkv"] = R.emu_rope(r["dqkv_unrot"], c.nh + c.nkv, c.d, c.cos, c.sin, c.S, inverse=True)
    r["dh1"] = G.emu_gemm(r["dqkv"], wqkv, G.EPI_BF16)
    lo = 0
    for nm, w in (("q", c.wq), ("k", c.wk), ("v", c.wv)):
        r["dW_" + nm] = _emu_sink(c, r["dqkv"][:, lo:lo + w.shape[0]], r["h1"], G.EPI_BF16_ACC)
        lo += w.shape[0]
    r["dx"], r["dw1"] = _emu_norm_bwd(c, r["dh1"], x, c.w1, r["rstd1"], r["dz"], R.PT_DW_ACC_BF16,
                                      drop_row=fault == "norm_partial_row_missing")
    h["dx0"] = r["dx"]
    old = _old(c, tuple(c.wemb.shape), BF)
    h["dW_emb"] = dict(got=OR.emu_embedding_bwd(c.ids.reshape(-1), h["dx0"], old, R.PT_DW_ACC_BF16, 0, c.wemb.shape[0]),
                       old=old, sink=R.PT_DW_ACC_BF16)
    return r, h
