"""Row-kernel conformance kit: input families, float64 references that apply each kernel's documented
roundings in the documented order, per-element bounds, checkers and fp32 emulators with injectable
faults, for csrc/rmsnorm.hip, csrc/cross_entropy.hip, csrc/swiglu.hip and csrc/rope.hip.  CPU only.

Notation: u = 2^-8 (bf16 round-to-nearest), e = 2^-24 (one f32 rounding), g(n) = n e / (1 - n e) (n
f32 roundings along one path of a sum).  A bf16 store of an f32 value with absolute error E32 is
within  B16 = u |ref| + (1 + u) E32  of the unrounded float64 target `ref` (u |ref| is floored at 2^-134,
half the spacing of bf16's denormals, wherever it stands for a bf16 rounding).  The hardware units
v_exp_f32, v_log_f32, v_rsq_f32, v_rcp_f32 are each allowed HW = 2 f32 ulps = 2^-22 of their result.
Terms of second order in e are covered by the factor SECOND = 1 + 2^-18 on every E32 (each E32 below
has fewer than 2^6 first-order terms, so their pairwise products are below 2^-18 of their sum).

Two kinds of check
    exact      expected bits computed in float64, compared with torch.equal on the bit patterns:
               z = bf16(f32(x + r)); all of RoPE (operands on a 1/64 grid: a c - b s is exact in f32
               and in f64, fmaf(a, c, -(b s)) is its single f32 rounding, which is exact, and the store
               rounds once); zero gradient rows of ignored targets; sentinel bytes.
    sequenced  (norm outputs, SwiGLU) every element within the derived bound, AND at most BIT_CAP =
               0.5 % of the elements differ in bits from the float64-sequenced expectation, each by one
               bf16 ulp of the rounding that flipped: the store's own (the element is one ulp from the
               expectation) or, where the formula rounds an intermediate to bf16 first (mode 1's
               bf16(x rstd), SwiGLU's bf16(silu(g))), that one (the element equals the expectation
               recomputed with the intermediate moved one bf16 ulp up or down -- the outer product can
               move by two ulps of the output then, which is why the condition is put on the rounding
               and not on the output).  The cap is a condition, not a measurement: a correct fp32
               evaluation stays below 1e-4 (asserted in tests/test_row_checker_cpu.py), a wrong
               rounding sequence sits near 25 %.  The norm backward's dx = rstd (p - xh dot) (+ dres) can
               be the small difference of larger terms, and its f32 error E32 then spans several ulps
               of the result: there the one ulp is replaced by FLIP(o, E32) (round_info): 0 -- the bits
               must match -- unless o is within E32 of a rounding boundary, else E32 plus one ulp.

RMSNorm forward (A = 8 ceil(cols / 512) + 6 additions on the longest path of a 64-lane row sum: the
lane's own chunks in sequence, then six butterfly levels)
    z     = bf16(f32(x + r))                                      exact
    ss    = sum z^2: products and A additions, relative g(A + 1)
    arg   = ss (1 / cols) + eps: the constant, the product, the sum: + 3 e (all terms positive)
    rstd  = rsq(arg): half the argument's relative error + HW
            E_r = (g(A + 1) + 3 e) / 2 + HW      (relative; checked per row)
    mode 0  y = bf16(z rstd w): two products:  E32 = |t| (E_r + 2 e)
    mode 1  q = z rstd: E_q = |q| (E_r + e); qb = bf16(q) flips to a neighbour only where q is within
            E_q of a rounding boundary (FLIP = that neighbour's distance, else 0); w qb is exact in f32:
            |y - w qb| <= u |w qb| + (1 + u) |w| FLIP
RMSNorm backward (rstd is an input: exact)
    p = dy w (exact in f32), xh = z rstd (e), dot = mean(p xh): xh, the product, A additions, the
    constant 1 / cols and its product:  E_dot = g(A + 4) mass / cols,  mass = sum |p xh|
    o = rstd (p - xh dot) (+ dres):
        E32 = rstd (|xh| E_dot + 2 e |xh dot| + e (|p| + |xh dot|)) + e |o| (+ e |o + dres|)
    dw[c] = sum_r dy xh (mode 1: dy bf16(xh)): xh, the product and at most rows additions in any order:
        E_dw = g(rows + 2) sum_r |dy xh|  (+ sum_r |dy| FLIP(xh) in mode 1)
    sinks: 0 B16(E_dw); PT_DW_ACC_BF16 bf16(old + db), db = bf16(dw): (u + e) |old + db| + (1 + u) FLIP(dw)
           (the f32 sum of two bf16 values, then the store);
           PT_DW_ACC_F32 f32(old + dw): E_dw + e |old + dw|

Cross-entropy (d_i = x_i - M, M the row maximum, C = ceil(V / 2048) chunk steps per thread)
    exp(x_i - M) is evaluated as v_exp(arg) with, relative to the result,
        style "sub"  __expf(x - m): the difference, log2(e) and its product: 3 e |d_i|
        style "fma"  exp2(fma(x, log2e, nl)), nl = -m log2e rounded twice (the constant, the product), the
                     constant inside the fma, the fma's own rounding: e (|x_i| + 2 X + |d_i|), X = max |x|
    plus HW; the online kernels rescale by exp(m_old - m_new), whose arguments telescope to |d_i| ("sub":
    inside the same 3 e |d_i|; "fma": one more e |d_i|, and e 3 X per chunk step, since fma(m, log2e,
    -m log2e rounded) is not 0: C 3 e X in all) with one HW per step.  A result below 2^-126 may be
    flushed: + 2^-126 each.  C = the thread's chunk steps: ceil(V / 2048), ceil(V / 8192) for the
    streaming forward (four chunks per step).
        E_S / S = sum_i p_i ARG_i + HW (C + 11) + g(11 C + 30) + V 2^-126 / S
    (11 C + 30: 8 additions and 3 rescale roundings per chunk step, 3 per level of the 6 + 4 merges)
    lse = M + ln2 v_log(S):  E_lse = E_S / S + 1.5 HW |ln S| + e |lse|;  loss = lse - x_t: + e |loss|
    p_i = exp(x_i - lse):  relative  E_lse + ARG'_i + HW  (ARG' with lse for m; E_lse = 0 when the lse
    is an input), flushed below 2^-126;  grad = (p - onehot) g:
        E32 = |g| (p E_p + 2^-126) + 3 e |(p - onehot) g| + 2^-126
    (the subtraction, g = scale inv_count, the product).  Ignored rows: loss 0 and gradient +0 by bits.
    Bad targets: NaN loss, NaN gradient row (the reference holds NaN there and the checker demands it).
    Merging (m_b, s_b) statistics (fwd_stats, vp_partial / vp_combine): the same with the s_b as terms.

SwiGLU (s = sigmoid(g) = rcp(1 + exp(-g)), E = exp(-g))
    E: log2(e) and its product, 2 e |g|, + HW;  1 + E: e;  rcp: HW:
        E_s = s (E / (1 + E) (2 e |g| + HW) + e + HW)  + 2^-126 [g < -87]
    the floor: for g < -87.34 the true sigmoid is below 2^-126, __expf(-g) is above 2^126 (and
    overflows from g < -88.72) and v_rcp's result is denormal or zero: the kernel's s is anywhere in
    [0, 2^-126], so silu carries |g| 2^-126 and dg carries |bf16(dh u)| (|g| + 1) 2^-126.
    silu = g s: E_silu = |g| E_s + e |silu|; sb = bf16(silu) flips only within E_silu of a boundary
    (FLIP; in the floor region  E_silu (1 + u) + 2 u |silu|  instead);  sb u and dh sb are exact in f32:
        h  = bf16(sb u):   u |sb u| + (1 + u) |u| FLIP         du = bf16(dh sb): the same with dh
    dg = bf16(dhu F), dhu = bf16(dh u) (exact product, one rounding: no flip), F = s (1 + g (1 - s)):
        A = 1 - s: E_A = E_s + e |A|;  B = g A: E_B = |g| E_A + e |B|;  C = 1 + B: E_C = E_B + e |C|
        E_F = |C| E_s + s E_C + e |F|;   E32 = |dhu| E_F + e |dhu F|

RoPE: o1 = bf16(f32(a c - b s')), o2 = bf16(f32(b c + a s')), s' = sin or -sin (inverse), position
row mod seq_len, table column = the pair's index in the half head; heads >= nheads untouched.

Every checker rejects non-finite values where the reference is finite (and demands NaN where it is
NaN), prints the worst |got - ref| / bound and names the worst element as row, column, 8-column chunk,
lane = chunk mod 64, register = chunk div 64.
"""
import math

import torch

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
U = 2.0 ** -8
E = 2.0 ** -24
HW = 2.0 ** -22
TINY = 2.0 ** -126
SECOND = 1 + 2.0 ** -18
BIT_CAP = 0.005
NAN16 = 0x7FC1
NAN32 = 0x7FC00001
PT_DW_ACC_BF16, PT_DW_ACC_F32 = 4, 8
IGNORE = -100
NORM_FAMILIES = ("randn", "rowscale", "tiny", "spike", "cancel")
CE_FAMILIES = ("randn3", "offset", "peaked", "flat", "neg_inf")
SWIGLU_FAMILIES = ("randn", "all_g")


def gamma(n):
    return n * E / (1 - n * E)


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (k if isinstance(k, int) else sum(ord(c) * 131 ** i for i, c in enumerate(k)))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _bf(x):
    """float64 -> f32 -> bf16 -> float64: the kernels' store of an f32 value."""
    return x.to(F32).to(BF).to(F64)


def ibits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def sentinel_cpu(shape, dtype):
    t = torch.empty(shape, dtype=dtype)
    ibits(t).fill_(NAN16 if dtype == BF else NAN32)
    return t


def _ord(t):
    """bf16 tensor -> int32, monotone in the value (both zeros 0): |difference| = distance in ulps."""
    b = ibits(t.to(BF)).to(torch.int32) & 0xFFFF
    mag = b & 0x7FFF
    return torch.where(b >= 0x8000, -mag, mag)


def _from_ord(o):
    b = torch.where(o < 0, (-o) | 0x8000, o)
    b = torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16)
    return b.view(BF)


def bf_nbr(x, step):
    """The bf16 value `step` ulps above (below) the bf16-valued float64 x, as float64."""
    return _from_ord(_ord(x.to(BF)) + step).to(F64)


def round_info(x, err):
    """(xb, flip, up, dn): xb = bf16(x); flip = how far bf16 of a value x' within err of x can land
    from xb: 0 unless x is within err of a rounding boundary; then, bf16 being monotone and within half
    an ulp of its argument, |bf16(x') - xb| <= err + half an ulp at x + half an ulp at x', which is at
    most err + max(the neighbour's distance, 2 u (|x| + err)).  up / dn: xb's bf16 neighbours."""
    xb = _bf(x)
    up, dn = bf_nbr(xb, 1), bf_nbr(xb, -1)
    near = (((xb + up) / 2 - x).abs() <= err) | (((xb + dn) / 2 - x).abs() <= err)
    step = torch.maximum((up - xb).abs(), (xb - dn).abs())
    step = torch.where(torch.isfinite(step), step, (xb - dn).abs())
    flip = torch.where(near, err + torch.maximum(step, 2 * U * (x.abs() + err)), torch.zeros_like(x))
    return xb, flip, up, dn


# ------------------------------------------------------------------------------ checkers
WORST = {}


def where(idx):
    r = int(idx[0])
    if len(idx) == 1:
        return f"row {r}"
    c = int(idx[1])
    return f"row {r} col {c} chunk {c // 8} lane {c // 8 % 64} reg {c // 8 // 64}"


def _cpu(t):
    return t.detach().to("cpu")


def check_exact(name, got, want):
    g, w = _cpu(got).contiguous(), want.contiguous()
    assert g.dtype == w.dtype and g.shape == w.shape, f"{name}: {g.dtype} {tuple(g.shape)} != {w.dtype} {tuple(w.shape)}"
    diff = ibits(g) != ibits(w)
    if bool(diff.any()):
        idx = diff.nonzero()[0]
        i = tuple(int(v) for v in idx)
        raise AssertionError(f"{name}: {int(diff.sum())} of {diff.numel()} elements differ by bits; first at "
                             f"{where(idx)}: got {float(g[i])!r} want {float(w[i])!r}")
    return 0.0


def check(name, got, ref, bound, tag=None):
    """Per element: got is NaN where ref is NaN, finite and within bound of ref elsewhere."""
    g = _cpu(got).to(F64)
    ref, bound = ref.to(F64), bound.to(F64).expand_as(ref)
    assert g.shape == ref.shape, f"{name}: shape {tuple(g.shape)} != {tuple(ref.shape)}"
    want_nan = torch.isnan(ref)
    want_inf = torch.isinf(ref)          # a target on a -inf logit: the loss is +inf, and must be
    bad = torch.where(want_nan, ~torch.isnan(g), torch.where(want_inf, g != ref, ~torch.isfinite(g)))
    if bool(bad.any()):
        idx = bad.nonzero()[0]
        raise AssertionError(f"{name}: {int(bad.sum())} values non-finite where the reference is finite (or finite "
                             f"where it is NaN), first at {where(idx)}: got {float(g[tuple(idx.tolist())])!r}")
    err = torch.where(want_nan | want_inf, torch.zeros_like(g), (g - ref).abs())
    ratio = torch.where(err > 0, err / bound, torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    WORST[(tag, name)] = max(WORST.get((tag, name), 0.0), worst)
    print(f"row-check {tag or '-'} {name} worst ratio {worst:.3f}")
    if not worst <= 1.0:
        idx = (ratio == ratio.max()).nonzero()[0]
        i = tuple(int(v) for v in idx)
        raise AssertionError(f"{name}: {int((ratio > 1).sum())} of {ratio.numel()} elements over the bound; worst at "
                             f"{where(idx)}: got {float(g[i])!r} ref {float(ref[i])!r} err {float(err[i]):.3e} "
                             f"bound {float(bound[i]):.3e} (ratio {worst:.2f})")
    return worst


def check_bits(name, got, want, alts=(), exempt=None, tag=None, cap=BIT_CAP, flip=None):
    """The sequenced condition: the share of elements whose bits differ from `want` (bf16) is at most
    cap, and each of them is one ulp from want or equals one of `alts` (the expectation with an inner
    rounding moved one ulp).  exempt: elements judged by the bound alone (SwiGLU's floor region).
    flip (float64, round_info's): instead of the one ulp, an element may be |got - want| <= flip away:
    nothing unless the f32-side error reaches a rounding boundary -- for outputs that are the small
    difference of larger terms (the norm backward's dx), whose f32 error can span several of their ulps."""
    g, w = _cpu(got), want.to(BF)
    assert g.dtype == BF and g.shape == w.shape, f"{name}: {g.dtype} {tuple(g.shape)}"
    diff = ibits(g) != ibits(w)
    if exempt is not None:
        diff &= ~exempt
    ok = (_ord(g) - _ord(w)).abs() <= 1 if flip is None else (g.to(F64) - w.to(F64)).abs() <= flip
    for a in alts:
        ok |= ibits(g) == ibits(a.to(BF))
    share = float(diff.double().mean())
    WORST[(tag, name + " bits")] = max(WORST.get((tag, name + " bits"), 0.0), share)
    print(f"row-check {tag or '-'} {name} bit-mismatch share {share:.2e}")
    far = diff & ~ok
    if bool(far.any()):
        idx = far.nonzero()[0]
        i = tuple(int(v) for v in idx)
        raise AssertionError(f"{name}: {int(far.sum())} elements are more than one rounding flip from the sequenced "
                             f"expectation; first at {where(idx)}: got {float(g[i])!r} want {float(w[i])!r}")
    assert share <= cap, f"{name}: {share:.3%} of the elements differ by bits from the sequenced expectation (cap {cap:.1%})"
    return share


def norm_rel(got, ref):
    """The suite's older global metric (tests/test_kernels_gpu.py rel_err)."""
    got, ref = _cpu(got).to(F64), ref.to(F64)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def hu(t):
    """bf16 round-to-nearest's own error at t: u |t|, and half the denormal spacing 2^-133 below 2^-126."""
    return (U * t.abs()).clamp_min(2.0 ** -134)


def b16(ref, e32):
    return hu(ref) + (1 + U) * e32


# ------------------------------------------------------------------------------ RMSNorm
def make_norm_case(family, rows, cols, seed=0):
    """bf16 CPU dict x, r (residual), w, dy, dres of one family."""
    g = _gen("norm", family, rows, cols, seed)
    x = torch.randn(rows, cols, generator=g, dtype=F64)
    w = 1 + 0.25 * torch.randn(cols, generator=g, dtype=F64)
    dy = torch.randn(rows, cols, generator=g, dtype=F64)
    rr = torch.arange(rows)
    if family == "rowscale":
        x = x * torch.pow(2.0, (rr % 23 - 11).to(F64))[:, None]
    elif family == "tiny":
        x = x * 2.0 ** -20
    elif family == "spike":
        nch = cols // 8
        x = x * 2.0 ** -10
        col = torch.where(rr % 2 == 0, cols - 1 - rr % 8, min(63, nch - 1) * 8 + rr % 8)
        x[rr, col] = 64.0
    elif family == "cancel":
        h = cols // 2
        x = torch.cat([x[:, :h], x[:, :h]], 1)
        w = torch.cat([w[:h], w[:h]])
        d = dy[:, :h].to(BF).to(F64)
        dy = torch.cat([d, -bf_nbr(d, 1)], 1)      # the pair sums to one bf16 ulp of dy, times w xh
    elif family != "randn":
        raise KeyError(family)
    res = x * 0.5 + torch.randn(rows, cols, generator=g, dtype=F64) * x.abs().mean(1, keepdim=True)
    dres = torch.randn(rows, cols, generator=g, dtype=F64)
    x16 = x.to(BF)
    if family == "cancel":
        res = torch.zeros_like(x)
    return dict(x=x16, r=res.to(BF), w=w.to(BF), dy=dy.to(BF), dres=dres.to(BF))


def _adds(cols):
    return 8 * math.ceil(cols / 512) + 6


def ref_norm_fwd(x, r, w, eps, mode):
    """Float64-sequenced forward.  dict: z (bf16, exact; None without residual), rstd, rstd_bound,
    y_ref (unrounded target), y_want (bf16), y_bound, y_alts."""
    cols = x.shape[1]
    z = (x.to(F64) + r.to(F64)).to(F32).to(BF) if r is not None else None
    zz = (z if r is not None else x).to(F64)
    w6 = w.to(F64)[None, :]
    eps32 = float(torch.tensor(eps, dtype=F32))
    rstd = 1.0 / torch.sqrt((zz * zz).sum(1) / cols + eps32)
    e_r = ((gamma(_adds(cols) + 1) + 3 * E) / 2 + HW) * SECOND
    out = dict(z=z, rstd=rstd, rstd_bound=rstd * e_r)
    rs = rstd[:, None]
    if mode == 0:
        t = zz * rs * w6
        out.update(y_ref=t, y_want=_bf(t).to(BF), y_bound=b16(t, t.abs() * (e_r + 2 * E) * SECOND), y_alts=())
    else:
        q = zz * rs
        qb, flip, up, dn = round_info(q, q.abs() * (e_r + E) * SECOND)
        t = w6 * qb
        out.update(y_ref=t, y_want=_bf(t).to(BF), y_bound=hu(t) + (1 + U) * w6.abs() * flip,
                   y_alts=(_bf(w6 * up).to(BF), _bf(w6 * dn).to(BF)))
    return out


def ref_norm_bwd(dy, z, w, rstd, dres, mode):
    """Float64-sequenced backward from the f32 rstd the forward saved.  dict: dx_ref, dx_want, dx_bound,
    dw (float64 column sums), dw_err."""
    rows, cols = z.shape
    A = _adds(cols)
    zz, d, w6, rs = z.to(F64), dy.to(F64), w.to(F64)[None, :], rstd.to(F64)[:, None]
    p, xh = d * w6, zz * rs
    dot = (p * xh).sum(1, keepdim=True) / cols
    mass = (p * xh).abs().sum(1, keepdim=True)
    e_dot = gamma(A + 4) * mass / cols
    inner = p - xh * dot
    o = rs * inner
    e32 = rs * (xh.abs() * e_dot + 2 * E * (xh * dot).abs() + E * (p.abs() + (xh * dot).abs())) + E * o.abs()
    if dres is not None:
        o = o + dres.to(F64)
        e32 = e32 + E * o.abs()
    e32 = e32 * SECOND
    if mode == 0:
        gterm, e_dw = d * xh, gamma(rows + 2) * (d * xh).abs().sum(0)
    else:
        xb, flip, _, _ = round_info(xh, xh.abs() * E * SECOND)
        gterm = d * xb
        e_dw = gamma(rows + 2) * gterm.abs().sum(0) + (d.abs() * flip).sum(0)
    return dict(dx_ref=o, dx_want=_bf(o).to(BF), dx_bound=b16(o, e32), dx_flip=round_info(o, e32)[1], dw=gterm.sum(0),
                dw_err=e_dw * SECOND, dot=dot, mass=mass)


def dw_target_bound(dw, e_dw, sink, old=None):
    """(target, bound) of a dweight sink: 0 bf16 store, PT_DW_ACC_BF16 (sequenced: the target holds the
    inner bf16(dw), the bound its FLIP), PT_DW_ACC_F32."""
    if sink == 0:
        return dw, b16(dw, e_dw)
    if sink == PT_DW_ACC_BF16:
        db, flip, _, _ = round_info(dw, e_dw)
        t = old.to(F64) + db
        return t, hu(t) + E * t.abs() + (1 + U) * flip
    t = old.to(F64) + dw
    return t, e_dw + E * t.abs()


def _rne(x):
    return x.to(BF).to(F32)


NORM_FWD_FAULTS = ("no_eps", "wrong_mode", "neighbour_rstd", "ss_drops_last_chunk")
NORM_BWD_FAULTS = ("dot_without_w", "dres_dropped", "dw_skips_last_row", "dw_partial_bf16", "acc_bf16_single_rounding")


def emu_norm_fwd(x, r, w, eps, mode, fault=None):
    """(y bf16, z bf16 or None, rstd f32) as the kernels compute them, in fp32 torch."""
    cols = x.shape[1]
    z = _rne(x.to(F32) + r.to(F32)) if r is not None else x.to(F32)
    sq = z * z
    if fault == "ss_drops_last_chunk":
        sq = sq[:, :cols - 8]
    rstd = torch.rsqrt(sq.sum(1) * torch.tensor(1.0 / cols, dtype=F32) + (0.0 if fault == "no_eps" else eps))
    rs = rstd.roll(-1) if fault == "neighbour_rstd" else rstd
    wf = w.to(F32)[None, :]
    if (mode == 0) != (fault == "wrong_mode"):
        y = z * rs[:, None] * wf
    else:
        y = wf * _rne(z * rs[:, None])
    return y.to(BF), (z.to(BF) if r is not None else None), rstd


def emu_norm_bwd(dy, z, w, rstd, dres, mode, sink=0, old=None, fault=None, block_rows=16):
    """(dx bf16, dweight in the sink's dtype): per-block f32 partial sums of block_rows rows, then their sum."""
    rows, cols = z.shape
    d, zz, wf, rs = dy.to(F32), z.to(F32), w.to(F32)[None, :], rstd.to(F32)[:, None]
    xh = zz * rs
    dot = ((d * xh) if fault == "dot_without_w" else (d * wf * xh)).sum(1, keepdim=True) * torch.tensor(1.0 / cols, dtype=F32)
    o = rs * (d * wf - xh * dot)
    if dres is not None and fault != "dres_dropped":
        o = o + dres.to(F32)
    gterm = d * (xh if mode == 0 else _rne(xh))
    if fault == "dw_skips_last_row":
        gterm = gterm[:rows - 1]
    parts = [gterm[i:i + block_rows].sum(0) for i in range(0, gterm.shape[0], block_rows)]
    if fault == "dw_partial_bf16":
        parts = [_rne(p) for p in parts]
    dw = torch.stack(parts).sum(0)
    if sink == PT_DW_ACC_F32:
        out = old.to(F32) + dw
    elif sink == PT_DW_ACC_BF16:
        out = (old.to(F32) + (dw if fault == "acc_bf16_single_rounding" else _rne(dw))).to(BF)
    else:
        out = dw.to(BF)
    return o.to(BF), out


# ------------------------------------------------------------------------------ cross-entropy
TARGETS = ("0", "7", "8", "V-1", "ignore")
BAD_TARGETS = (-1, "V", 2 ** 40)


def make_ce_case(family, rows, V, seed=0):
    """bf16 CPU logits [rows, V] of one family."""
    g = _gen("ce", family, rows, V, seed)
    x = torch.randn(rows, V, generator=g, dtype=F64)
    rr = torch.arange(rows)
    if family == "randn3":
        x = x * 3
    elif family == "offset":
        x = x + (40.0 * (rr % 7 - 3)).to(F64)[:, None]
    elif family == "peaked":
        x[rr, peak_col(rr, V)] = x.max() + 60.0
    elif family == "flat":
        x = torch.full_like(x, 1.5)
    elif family == "neg_inf":
        x = x * 3
        x[torch.rand(rows, V, generator=g) < 0.05] = -math.inf
        nch = V // 8
        for r in range(rows):   # whole aligned chunks: chunk 0, a later thread's first chunk, the last
            for ch in {0, min(r + 1, nch - 1), min(255, nch - 1), nch - 1} - ({nch - 1} if r % 2 else set()):
                x[r, ch * 8:ch * 8 + 8] = -math.inf
            if not bool(torch.isfinite(x[r]).any()):
                x[r, V - 1] = 0.5
        x[rr, V - 1 - rr % 5] = x[rr, V - 1 - rr % 5].clamp_min(-1.0)   # a finite logit in every row
    else:
        raise KeyError(family)
    return x.to(BF)


def peak_col(rr, V):
    return (rr * 8 + 7) % V


def make_targets(rows, V, x=None, ignore=IGNORE):
    """int64 targets cycling 0, 7, 8, V-1, ignore_index, a chunk edge and the row's own peak column."""
    base = [0, 7 % V, 8 % V, V - 1, ignore, (V // 2 // 8) * 8 % V, (V // 2 // 8 * 8 - 1) % V]
    t = torch.tensor([base[r % len(base)] for r in range(rows)], dtype=torch.int64)
    return t


def _arg_err(xv, m, d, style, steps=0):
    if style == "sub":
        return 3 * E * d.abs()
    xmax = torch.where(torch.isfinite(xv), xv.abs(), torch.zeros_like(xv)).amax(1, keepdim=True)
    X = torch.maximum(xmax, torch.where(torch.isfinite(m), m.abs(), torch.zeros_like(m)))
    return E * (xv.abs() + 2 * X + (2 if steps else 1) * d.abs() + 3 * steps * X)


def _zero_nan(t):
    return torch.where(torch.isfinite(t), t, torch.zeros_like(t))


def ref_ce_fwd(x, tgt, ignore=IGNORE, style="sub", vocab=None, steps=None):
    """dict lse, lse_bound, loss, loss_bound (float64 [rows]; NaN for a bad target, loss 0 for ignored)."""
    rows, V = x.shape
    vocab = vocab or V
    xv = x.to(F64)
    M = xv.amax(1, keepdim=True)
    d = xv - M
    ex = torch.exp(d)
    S = ex.sum(1, keepdim=True)
    C = steps or math.ceil(V / 2048)
    arg = _zero_nan(ex / S * _arg_err(xv, M, d, style, C)).sum(1, keepdim=True)
    e_s = arg + HW * (C + 11) + gamma(11 * C + 30) + V * TINY / S
    lse = (M + torch.log(S))
    e_lse = ((e_s + 1.5 * HW * torch.log(S).abs() + E * lse.abs()) * SECOND).squeeze(1)
    lse = lse.squeeze(1)
    valid = tgt != ignore
    bad = valid & ((tgt < 0) | (tgt >= vocab))
    xt = xv[torch.arange(rows), tgt.clamp(0, V - 1)]
    loss = torch.where(valid, lse - xt, torch.zeros_like(lse))
    e_loss = torch.where(valid, e_lse + E * loss.abs(), torch.zeros_like(lse))
    nan = torch.full_like(lse, math.nan)
    return dict(lse=torch.where(bad, nan, lse), lse_bound=e_lse, loss=torch.where(bad, nan, loss), loss_bound=e_loss,
                lse_clean=lse, bad=bad, valid=valid)


def ref_ce_bwd(x, tgt, lse, lse_err, gscale, ignore=IGNORE, style="sub", vocab_lo=0):
    """(grad_ref float64 [rows, V], bound): (exp(x - lse) - onehot) g per row; lse float64 [rows] (NaN rows give NaN
    rows), lse_err its absolute error (0 when the kernel reads it), gscale float64 [rows] (ignored rows: any)."""
    rows, V = x.shape
    xv, L = x.to(F64), lse.to(F64)[:, None]
    valid = (tgt != ignore)[:, None]
    g = torch.where(valid, gscale.to(F64)[:, None].expand(rows, 1), torch.zeros(rows, 1, dtype=F64))
    d = xv - L
    p = torch.exp(d)
    onehot = (torch.arange(V)[None, :] == (tgt - vocab_lo)[:, None]).to(F64)
    e_p = _zero_nan(lse_err.to(F64)[:, None] + _arg_err(xv, L, d, style)) + HW
    ref = (p - onehot) * g
    e32 = (g.abs() * (p * e_p + TINY) + 3 * E * ref.abs()) * SECOND + TINY
    return ref, b16(ref, e32)


def merge_stats(m, s, steps=None):
    """(lse, its absolute error bound) of statistics m, s [..., n] merged along the last axis (float64);
    steps: the merges on the longest path (default: every 8th tile in sequence, then 8 groups)."""
    M = m.amax(-1, keepdim=True)
    term = torch.where(torch.isfinite(m), s * torch.exp(m - M), torch.zeros_like(s))
    S = term.sum(-1, keepdim=True)
    n = m.shape[-1]
    steps = steps or math.ceil(n / 8) + 8
    arg = _zero_nan(term / S * 3 * E * (m - M).abs()).sum(-1, keepdim=True)
    e_s = arg + HW * steps + gamma(3 * steps) + n * TINY / S
    lse = M + torch.log(S)
    e_lse = (e_s + 1.5 * HW * torch.log(S).abs() + E * lse.abs()) * SECOND
    return lse.squeeze(-1), e_lse.squeeze(-1)


CE_FAULTS = ("onehot_off_by_one", "lse_skips_last_chunk", "ignored_row_nonzero", "row_scale_uses_row0", "p_in_bf16",
             "neg_inf_chunk_nan")


def emu_ce(x, tgt, gscale, ignore=IGNORE, fault=None):
    """(loss f32 [rows], grad bf16 [rows, V]) in fp32 torch; gscale f32 [rows]."""
    rows, V = x.shape
    xf = x.to(F32)
    xs = xf[:, :V - 8] if fault == "lse_skips_last_chunk" else xf
    m = xs.amax(1, keepdim=True)
    lse = m + torch.log(torch.exp(xs - m).sum(1, keepdim=True))
    if fault == "neg_inf_chunk_nan":   # a thread's first chunk (chunks 0 .. 255) all -inf: exp(-inf - -inf)
        first = xf[:, :min(V, 2048)].reshape(rows, -1, 8)
        lse = torch.where((first == -math.inf).all(2).any(1, keepdim=True), torch.full_like(lse, math.nan), lse)
    valid = tgt != ignore
    bad = valid & ((tgt < 0) | (tgt >= V))
    lse = torch.where(bad[:, None], torch.full_like(lse, math.nan), lse)
    xt = xf[torch.arange(rows), tgt.clamp(0, V - 1)]
    loss = torch.where(valid, lse.squeeze(1) - xt, torch.zeros(rows))
    gs = gscale.to(F32)
    if fault == "row_scale_uses_row0":
        gs = gs[:1].expand(rows)
    g = torch.where(valid, gs, torch.zeros(rows) if fault != "ignored_row_nonzero" else gs * 2.0 ** -9)[:, None]
    p = torch.exp(xf - lse)
    if fault == "p_in_bf16":
        p = _rne(p)
    t = tgt + 1 if fault == "onehot_off_by_one" else tgt
    onehot = (torch.arange(V)[None, :] == t[:, None]).to(F32)
    return loss, ((p - onehot) * g).to(BF)


# ------------------------------------------------------------------------------ SwiGLU
def all_g():
    """Every finite bf16 bit pattern (65 280 values) padded with zeros to [256, 256]."""
    b = torch.arange(65536, dtype=torch.int32)
    b = b[(b & 0x7F80) != 0x7F80]
    b = torch.cat([b, torch.zeros(65536 - b.numel(), dtype=torch.int32)])
    return torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16).view(BF).reshape(256, 256)


ALL_G_VALUES = (1.0, -0.75, 0.0234375)     # u; |u|, |dh| <= 1: no product overflows f32
ALL_G_DH = (0.80078125, -0.66796875, 0.59765625)   # 205, -171, 153 / 256: dh u needs its rounding in two blocks


def make_swiglu_case(family, rows=None, cols=None, seed=0):
    """bf16 CPU (g, u, dh).  all_g: [768, 256], the 256 x 256 pattern block against three u / dh values."""
    if family == "all_g":
        g = all_g().repeat(3, 1)
        u = torch.tensor(ALL_G_VALUES, dtype=F64).repeat_interleave(256)[:, None].expand(768, 256)
        dh = torch.tensor(ALL_G_DH, dtype=F64).repeat_interleave(256)[:, None].expand(768, 256)
        return g, u.to(BF).contiguous(), dh.to(BF).contiguous()
    gen = _gen("swiglu", family, rows, cols, seed)
    return tuple((torch.randn(rows, cols, generator=gen, dtype=F64) * s).to(BF) for s in (2.0, 1.0, 1.0))


def _sig(g6):
    return 1.0 / (1.0 + torch.exp(-g6))


def _swiglu_terms(g):
    g6 = g.to(F64)
    ex = torch.exp(-g6)
    s = _sig(g6)
    floor = g6 < -87.0
    frac = torch.where(torch.isinf(ex), torch.ones_like(ex), ex / (1 + ex))
    e_s = s * (frac * (2 * E * g6.abs() + HW) + E + HW) + torch.where(floor, TINY, 0.0)
    silu = g6 * s
    e_silu = (g6.abs() * e_s + E * silu.abs()) * SECOND
    sb, flip, up, dn = round_info(silu, e_silu)
    flip = torch.where(floor, e_silu * (1 + U) + 2 * U * silu.abs(), flip)
    return g6, s, e_s, silu, sb, flip, up, dn, floor


def ref_swiglu_fwd(g, u):
    """dict h_ref, h_want, h_bound, h_alts, floor (the g < -87 region, judged by the bound alone)."""
    g6, s, e_s, silu, sb, flip, up, dn, floor = _swiglu_terms(g)
    u6 = u.to(F64)
    t = sb * u6
    return dict(h_ref=t, h_want=_bf(t).to(BF), h_bound=hu(t) + (1 + U) * u6.abs() * flip,
                h_alts=(_bf(up * u6).to(BF), _bf(dn * u6).to(BF)), floor=floor)


def ref_swiglu_bwd(dh, g, u):
    g6, s, e_s, silu, sb, flip, up, dn, floor = _swiglu_terms(g)
    d6, u6 = dh.to(F64), u.to(F64)
    tu = d6 * sb
    dhu = _bf(d6 * u6)
    A = 1 - s
    eA = e_s + E * A.abs()
    B = g6 * A
    eB = g6.abs() * eA + E * B.abs()
    C = 1 + B
    eC = eB + E * C.abs()
    F = s * C
    eF = C.abs() * e_s + s * eC + E * F.abs()
    tg = dhu * F
    e32 = (dhu.abs() * eF + E * tg.abs()) * SECOND
    return dict(du_ref=tu, du_want=_bf(tu).to(BF), du_bound=hu(tu) + (1 + U) * d6.abs() * flip,
                du_alts=(_bf(up * d6).to(BF), _bf(dn * d6).to(BF)),
                dg_ref=tg, dg_want=_bf(tg).to(BF), dg_bound=b16(tg, e32), floor=floor)


SWIGLU_FAULTS = ("silu_unrounded", "dhu_unrounded", "sigmoid_negated")


def emu_swiglu(g, u, dh, fault=None):
    """(h, dg, du) bf16 in fp32 torch."""
    a, b, d = g.to(F32), u.to(F32), dh.to(F32)
    s = 1.0 / (1.0 + torch.exp(a if fault == "sigmoid_negated" else -a))
    silu = a * s
    sb = silu if fault == "silu_unrounded" else _rne(silu)
    dhu = d * b if fault == "dhu_unrounded" else _rne(d * b)
    return (sb * b).to(BF), (dhu * (s * (1.0 + a * (1.0 - s)))).to(BF), (d * sb).to(BF)


# ------------------------------------------------------------------------------ RoPE
def grid64(shape, gen):
    """Random multiples of 1/64 in [-1, 1] (bf16, exact)."""
    return (torch.randint(-64, 65, shape, generator=gen).to(F64) / 64).to(BF)


def make_rope_case(rows, width, seq_len, head_dim, seed=0):
    """(x [rows, width], cos, sin [seq_len, head_dim]) bf16 on the 1/64 grid: the tables' two halves differ."""
    g = _gen("rope", rows, width, seq_len, head_dim, seed)
    return grid64((rows, width), g), grid64((seq_len, head_dim), g), grid64((seq_len, head_dim), g)


ROPE_FAULTS = ("pos_div_not_mod", "halves_swapped", "inverse_sign", "table_second_half")


def _rope(x, nheads, head_dim, cos, sin, seq_len, inverse, dtype, fault=None):
    rows = x.shape[0]
    half = head_dim // 2
    rr = torch.arange(rows)
    pos = (rr // seq_len).clamp_max(seq_len - 1) if fault == "pos_div_not_mod" else rr % seq_len
    lo = half if fault == "table_second_half" else 0
    c = cos.to(dtype)[pos, lo:lo + half][:, None, :]
    s = sin.to(dtype)[pos, lo:lo + half][:, None, :]
    if bool(inverse) != (fault == "inverse_sign"):
        s = -s
    out = x.clone()
    v = x[:, :nheads * head_dim].to(dtype).reshape(rows, nheads, head_dim)
    a, b = v[..., :half], v[..., half:]
    if fault == "halves_swapped":
        a, b = b, a
    o = torch.cat([a * c - b * s, b * c + a * s], -1)
    out[:, :nheads * head_dim] = o.to(F32).to(BF).reshape(rows, nheads * head_dim)
    return out


def ref_rope(x, nheads, head_dim, cos, sin, seq_len, inverse=False):
    """The whole row block after pt_rope, bit-exact (float64 arithmetic, exact for the 1/64 grid and for its
    once-rotated bf16 values: 8 + 7 significant bits per product, sums of two below 2^24 ulps apart)."""
    return _rope(x, nheads, head_dim, cos, sin, seq_len, inverse, F64)


def emu_rope(x, nheads, head_dim, cos, sin, seq_len, inverse=False, fault=None):
    return _rope(x, nheads, head_dim, cos, sin, seq_len, inverse, F32, fault)
