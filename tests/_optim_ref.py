"""Optimizer and embedding conformance kit: launch geometry, input families, references, per-element
bounds, checkers and emulators with injectable faults for csrc/adamw.hip and csrc/embedding.hip.  CPU
only.  Notation and helpers are tests/_row_ref.py's: u = 2^-8, e = 2^-24, g(n) = n e / (1 - n e),
B16 = u |ref| + (1 + u) E32, FLIP (round_info), SECOND, BIT_CAP.  T = 2^-149 is added once per f32
product or quotient, which may land among f32's denormals (bf16 and f32 share their exponent range, so
the `tiny` family's bf16 denormals are f32 denormals).  sqrtf and the divisions are the correctly
rounded forms in every AdamW kernel (the gfx950 code of csrc/adamw.hip at -O3: v_sqrt_f32 behind the
2^32 input scaling with two fused correction steps, and v_div_scale / v_rcp / four fused steps /
v_div_fmas / v_div_fixup), so each counts one e like an addition: no HW allowance anywhere.

Geometry (multi_grid, grid_for, runs): the list kernels cut the virtual concatenation of 8-element
chunks into `blocks` runs of `per_block` chunks; a thread of the 256 takes chunk from + tid, + 256, ...
of each tensor segment in its run.  bf16 step: prologue (one or two chunks ahead), steady state from
the third trip of one segment (>= 769 full chunks), drain, the ragged tail.  Master step: one ahead,
steady state from the second trip (>= 513).  Norm: the four-way loop from 769 chunks of a segment.

bf16 state, one step (adam_elem, bf = true), r() = bf16 rounding, every input a bf16 value:
    p1 = r(p decay)                         E32 = e |p decay| + T
    m1 = r(m + w1 (g - m))                  E32 = e (|w1| |g - m| + |w1 (g - m)| + |m1|) + 2 T
                                            (difference, product, sum; the fused form has one fewer)
    v1 = r(v beta2)                         E32 = e |v beta2| + T
    v2 = r(v1 + c2 (g g))                   E32 = e (2 |c2 g g| + |v2|) + 2 T
    d1 = r(sqrt(v2))   d2 = r(d1 / bc2s)   d3 = r(d2 + eps)     E32 = e |.| (+ T for the quotient)
    p2 = r(p1 + step (m1 / d3))             E32 = e (2 |step m1 / d3| + |p2|) + 2 T (1 + |step|)
  all times SECOND.  An f32 intermediate at or above 2^128 is inf in the reference as in the kernel.
  Sequenced check (check_bf16_step): the outputs (p2, m1, v2) are NaN / inf exactly where the
  expectation is; at most BIT_CAP of the elements differ from it in bits; each of those is explained
  by ONE rounding k that moved: x_k is within E32_k of a rounding boundary (round_info's FLIP > 0) and
  all three outputs equal the expectation recomputed with r_k moved one bf16 ulp up or down -- or only
  p differs and |p - want| <= FLIP(p2) (the `cancel` family: p2 is the small difference of larger
  terms and E32 spans several of its ulps); or m (v) is within FLIP(m1) (FLIP(v2)) of its expectation
  -- m + w1 (g - m) cancels where g is near -9 m -- and the other outputs equal the expectation
  recomputed from the m (v) the kernel stored.  Every element is within
      hu(x_o) + (1 + u) (E32_o + P_o)     of x_o, the argument of its output's last rounding,
  P_o = the largest move of x_o under the upstream roundings that are near a boundary (0 for all but
  about 1e-4 of the elements: a rounding that did not flip forgets its argument's f32 error).

f32 state (adamw_scalar_kernel<float>, contraction left to the compiler; check_f32_step), float64
reference, absolute bounds, first order times SECOND:
    E_p1 = e |p1| + T       E_m = e (|w1| |g - m| + |w1 (g - m)| + |m1|) + 2 T
    E_v  = e |v beta2| + T + e (2 |c2 g g| + |v2|) + 2 T
    E_d1 = min(E_v / sqrt(v2), sqrt(E_v)) + e d1     (|sqrt(a + x) - sqrt(a)| <= both)
    E_d3 = E_d1 / bc2s + e d2 + T + e d3
    E_q  = (E_m + |q| E_d3) / (d3 - E_d3) + e |q| + T,  q = m1 / d3
    E_p  = E_p1 + |step| E_q + e |step q| + T + e |p2|
Master path (adam_elem_master; check_master_step): contraction is off and the three fused operations
are spelled out, so master_expect computes the expected BITS: torch float32 products, sums and quotients
on the CPU are IEEE, sqrtf is the float64 root rounded to f32 (_sqrt32; torch's float32 sqrt is not
IEEE); fmaf(a, b, c) = the float64 a b + c (the product is exact in float64)
rounded to f32 -- a double rounding on about 2^-29 of the arguments.  Demanded: E_p, E_m, E_v above on
every element, equal bits except on at most BIT_CAP of the elements, each of those one f32 ulp away,
and param == bf16(master) by bits.
Clip: coef = min(1, max_norm / (sqrt(sq) + 1e-6)) in IEEE f32 (clip_coef) from the sq the kernel
produced; the clipped gradient bf16(f32(g coef)), or f32(g coef) for f32 state and master weights, is
an exact function of the inputs (clip_grad) and the step is then checked as an unclipped one.
Norm (sq_adds): all terms >= 0, bf16 squares exact, fmaf rounds once per term, so the relative error
is g(adds), adds = the additions on the longest path: an accumulator takes ceil(k / 4) chunks of a
segment of k chunks per thread (four-way loop, then the tail into accumulators 0, 1, 2), over the run
at most ceil(ceil(per_block / 256) / 4) + 2 per tensor, 8 additions each; the ragged elements (thread 0,
accumulator 3); 2 for the four accumulators, 6 for the wave butterfly, 3 for the four waves; the final
kernel: ceil(blocks / 256) + 6 + 3, the weight product 1; 2 spare.
Embedding: exact.  emu_embedding_bwd is the documented order in torch float32 (sequential sum over an
id's tokens in ascending position, one bf16 rounding, then the sink).

Worst |got - ref| / bound (1 = the bound) and largest bit-mismatch share (cap 5e-3) on an MI355X, measured
2026-10-20 on top of commit 73cf1f0 (tests/test_optim_conformance_gpu.py prints every figure with -rA and
the whole table in test_zz_worst_ratio_table):

    check                                   small            mid              cap
    bf16 list step (+ clip)      ratio      0.996            1.000 (tiny)     0.996
                                 bits       0                9.7e-05 (cancel) 5.0e-05 (cancel)
      chained steps              ratio / bits                0.996 / 0
    master list step (+ clip)    ratio      0.998            1.000            1.000
                                 bits       0                0                0
    single tensor bf16 / f32     ratio 1.000 (tiny) / 0.997         bits 4.9e-04 (cancel, n 2051) / -
    master single                ratio 0.984                        bits 0
    norm, list forms             ratio      5.1e-03          -                7.3e-03
    norm, single tensor          ratio 4.5e-02 (f32, n 20); 3.5e-02 at n 10 000 136
    `exact` family, scale, descriptor cache, guards, embedding: bit for bit.

The bf16 figures sit at 0.996 by construction (round-to-nearest's own error reaches u |ref| at the low end
of a binade; 1.000 is an exact tie of the store's rounding); the master path's expected bits were met on
every element of every case, and its 1.000 is the f32 bound reached by two roundings that both fall near
half an ulp among 13 M elements.  The norm uses under a twentieth of its bound.  No kernel failed a check.
"""
import math

import numpy as np
import torch

from tests import _row_ref as R
from tests._row_ref import BF, BIT_CAP, E, F32, F64, NAN16, NAN32, SECOND, U, _bf, b16, bf_nbr, gamma, hu, ibits, round_info

T149 = 2.0 ** -149
INF = math.inf
PT_DW_ACC_BF16, PT_DW_ACC_F32 = R.PT_DW_ACC_BF16, R.PT_DW_ACC_F32
STEP_CAP, NORM_CAP, STREAM_CAP = 1024, 2048, 2048
FAMILIES = ("randn", "fresh", "tiny", "overflow", "nan_grad", "cancel", "exact")
COEF_ONE = ("exact", "cancel")   # built against the unscaled gradient: their clipped runs use a max_norm above the norm
WORST = {}


# ------------------------------------------------------------------------------ geometry
def chunk_starts(lengths):
    cs = [0]
    for n in lengths:
        cs.append(cs[-1] + (n + 7) // 8)
    return cs


def multi_grid(total_chunks, cap=STEP_CAP):
    """(blocks, per_block) of csrc/adamw.hip's multi_grid."""
    want = (total_chunks + 511) // 512
    blocks = 1 if want < 1 else min(want, cap)
    return blocks, (total_chunks + blocks - 1) // blocks


def grid_for(work, cap=STREAM_CAP):
    """Workgroups of the single-tensor kernels (256 threads, grid-strided)."""
    return min(cap, max(1, (work + 255) // 256))


def runs(lengths, cap=STEP_CAP, grid=None):
    """Per workgroup the list of (tensor, from, to) chunk ranges it walks -- the kernels' binary search
    and forward walk."""
    cs = chunk_starts(lengths)
    nt, total = len(lengths), cs[-1]
    blocks, per_block = grid or multi_grid(total, cap)
    out = []
    for b in range(blocks):
        lo, hi = b * per_block, min(b * per_block + per_block, total)
        segs = []
        if lo < hi:
            a, z = 0, nt - 1
            while a < z:
                mid = (a + z + 1) >> 1
                if cs[mid] <= lo:
                    a = mid
                else:
                    z = mid - 1
            t = a
            while t < nt and cs[t] < hi:
                segs.append((t, max(lo, cs[t]) - cs[t], min(hi, cs[t + 1]) - cs[t]))
                t += 1
        out.append(segs)
    return out


def geometry(lengths, cap=STEP_CAP):
    """dict blocks, per_block, seg_full (the most full chunks of one tensor inside one run), run_tensors
    (the most non-empty tensors in one run), ragged (the most ragged elements in one run), mid_start
    (some run starts inside a tensor at a chunk that is no multiple of 256)."""
    blocks, per_block = multi_grid(chunk_starts(lengths)[-1], cap)
    seg_full = run_tensors = ragged = 0
    mid = False
    for segs in runs(lengths, cap):
        run_tensors = max(run_tensors, sum(1 for _, frm, to in segs if frm < to))
        rg = 0
        for i, (t, frm, to) in enumerate(segs):
            full = lengths[t] >> 3
            seg_full = max(seg_full, min(to, full) - frm)
            rg += lengths[t] & 7 if to > full else 0
            mid |= i == 0 and frm % 256 != 0
        ragged = max(ragged, rg)
    return dict(blocks=blocks, per_block=per_block, seg_full=seg_full, run_tensors=run_tensors, ragged=ragged,
                mid_start=mid)


def sq_adds(per_block, run_tensors, ragged, blocks):
    """f32 additions on the longest path from a squared gradient to pt_grad_sq_multi's result."""
    acc = 8 * (-(-(-(-per_block // 256)) // 4) + 2 * run_tensors) + ragged
    return acc + 2 + 6 + 3 + -(-blocks // 256) + 6 + 3 + 1 + 2


def sq_adds_single(n):
    """The same for pt_grad_sq (grid-strided, four accumulators)."""
    wg = grid_for(n)
    per_thread = -(-n // (wg * 256))
    return -(-per_thread // 4) + 1 + 2 + 6 + 3 + -(-wg // 256) + 6 + 3 + 1 + 2


# ------------------------------------------------------------------------------ scalars
class S:
    """The seven scalars as the kernels see them (f32 values held as Python floats)."""
    NAMES = ("decay", "w1", "beta2", "c2", "bc2_sqrt", "eps", "step_size")

    def __init__(self, **kw):
        for k in self.NAMES:
            setattr(self, k, float(np.float32(kw[k])))

    def kw(self):
        return {k: getattr(self, k) for k in self.NAMES}


def scalars(t=3, lr=3e-4, wd=0.01, beta1=0.9, beta2=0.999, eps=1e-8):
    return S(decay=1 - lr * wd, w1=1 - beta1, beta2=beta2, c2=1 - beta2, bc2_sqrt=math.sqrt(1 - beta2 ** t), eps=eps,
             step_size=-lr / (1 - beta1 ** t))


EXACT_S = S(decay=1.0, w1=0.5, beta2=0.5, c2=0.5, bc2_sqrt=1.0, eps=0.0, step_size=-1.0)


def clip_coef(sq, max_norm):
    """clip_coef of csrc/adamw.hip in IEEE f32; None when sq is inf or NaN (the step is skipped)."""
    with np.errstate(all="ignore"):
        sq = np.float32(sq)
        if not sq <= np.float32(3.402823466e+38):
            return None
        return float(min(np.float32(1.0), np.float32(max_norm) / (np.sqrt(sq) + np.float32(1e-6))))


def clip_grad(g, coef, bf):
    """The clipped gradient: one f32 product (exact in float64: 24 + 24 bits), rounded to bf16 if bf."""
    x = (g.to(F64) * coef).to(F32)
    return x.to(BF) if bf else x


# ------------------------------------------------------------------------------ buffers
def _pat(dtype):
    return NAN16 if dtype == BF else NAN32


class ListBuf:
    """The tensors of one field of a list, carved from ONE sentinel-filled allocation: every tensor
    starts on a 16-byte boundary (+ `skew` elements) and is followed by at least 16 sentinel bytes."""

    def __init__(self, lengths, dtype, device="cpu", skew=0):
        per16 = 8 if dtype == BF else 4
        self.lengths, self.dtype, self.off = list(lengths), dtype, []
        cur = per16
        for n in lengths:
            self.off.append(cur + skew)
            cur = -(-(cur + skew + n + per16) // per16) * per16
        self.flat = torch.empty(cur, dtype=dtype, device=device)
        ibits(self.flat).fill_(_pat(dtype))

    def views(self):
        return [self.flat[o:o + n] for o, n in zip(self.off, self.lengths)]

    def fill(self, tensors):
        for v, t in zip(self.views(), tensors):
            v.copy_(t.reshape(-1))
        return self

    def cat(self):
        return torch.cat([v.detach().cpu() for v in self.views()]) if self.lengths else self.flat[:0].cpu()

    def gaps_intact(self):
        ib = ibits(self.flat.detach().cpu()).clone()
        for o, n in zip(self.off, self.lengths):
            ib[o:o + n] = _pat(self.dtype)
        return bool((ib == _pat(self.dtype)).all())

    def clone(self):
        c = ListBuf.__new__(ListBuf)
        c.lengths, c.dtype, c.off, c.flat = self.lengths, self.dtype, self.off, self.flat.clone()
        return c

    def to(self, device):
        c = self.clone()
        c.flat = self.flat.to(device)
        return c


def same_bits(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(ibits(a), ibits(b))


# ------------------------------------------------------------------------------ families
def _ordinal(t):
    if t.dtype == BF:
        return R._ord(t).to(torch.int64)
    b = ibits(t).to(torch.int64)
    return torch.where(b < 0, -(b & 0x7FFFFFFF), b)


def nbr(t, k):
    """The value k ulps of t's own dtype (bf16 or f32) above t."""
    if t.dtype == BF:
        return R._from_ord((R._ord(t) + k).to(torch.int32))
    o = _ordinal(t) + k
    b = torch.where(o < 0, (-o) | 0x80000000, o)
    return torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32).view(F32)


def make_state(family, n, seed=0, sc=None, dtype=BF, gdtype=None):
    """(p, g, m, v) of one family as 1-D CPU tensors: p, m, v in dtype, g in gdtype (default dtype).
    sc: the step's scalars (the `cancel` family is built against them; `exact` goes with EXACT_S)."""
    gdtype = gdtype or dtype
    gen = R._gen("optim", family, n, seed)
    rn = lambda: torch.randn(n, generator=gen, dtype=F64)   # noqa: E731
    p, g, m, v = rn(), rn() * 0.1, rn() * 0.01, rn().abs() * 1e-4
    if family == "fresh":
        m, v = torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
        g[torch.rand(n, generator=gen) < 0.1] = 0.0
    elif family == "tiny":
        ex = lambda lo, hi: torch.pow(2.0, -torch.randint(lo, hi + 1, (n,), generator=gen).to(F64))   # noqa: E731
        g, m, v = rn() * ex(0, 133), rn() * ex(0, 133), rn().abs() * ex(0, 133)
    elif family == "overflow":
        g = rn() * torch.pow(10.0, torch.rand(n, generator=gen, dtype=F64) * 20)
    elif family == "nan_grad":
        if n:
            for c in sorted({0, (n // 8) // 2, max(n // 8 - 1, 0), n // 8}):   # first, middle, last full, ragged
                i = min(c * 8 + (c * 5 + 3) % 8, n - 1)
                g[i] = math.nan
    elif family == "cancel":
        m = m.to(dtype)
        g = nbr(m, torch.randint(-3, 4, (n,), generator=gen)).to(F64)
        m = m.to(F64)
    elif family == "exact":
        s = torch.randint(0, 2, (n,), generator=gen).to(F64) * 2 - 1
        a = torch.randint(-8, 9, (n,), generator=gen).to(F64)
        g = m = s * torch.pow(2.0, a)
        v = torch.pow(4.0, a)
        p = (torch.arange(n) % 251 - 125).to(F64)
    elif family != "randn":
        raise KeyError(family)
    p, g, m, v = p.to(dtype), g.to(gdtype), m.to(dtype), v.to(dtype)
    if family == "cancel" and n:
        rnd = (lambda k, x: _bf(x)) if dtype == BF else (lambda k, x: x.to(F32).to(F64))
        zero = torch.zeros(n, dtype=F64)
        _, m1, _, rec = sequence(zero, g.to(F64), m.to(F64), v.to(F64), sc, rnd)
        d3 = rnd("d3", rec["d3"][0])
        k = torch.randint(6, 13, (n,), generator=gen) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)
        p = nbr((-sc.step_size * m1 / d3 / sc.decay).to(dtype), k)   # p2 is 6 to 12 ulps of p: five bits cancel
    return p, g, m, v


def make_list(family, lengths, seed=0, sc=None, dtype=BF, gdtype=None):
    """make_state over the concatenation, split into the list's tensors: four lists of 1-D tensors."""
    flat = make_state(family, sum(lengths), seed, sc, dtype, gdtype)
    return [list(torch.split(t, list(lengths))) for t in flat]


# ------------------------------------------------------------------------------ the sequence
ROUNDS = ("p1", "m1", "v1", "v2", "d1", "d2", "d3", "p2")
LAST = dict(p="p2", m="m1", v="v2")


def _ovf(x):
    """An f32 intermediate whose magnitude reaches f32's overflow threshold is inf (NaN stays)."""
    return torch.where(x.abs() >= 2.0 ** 128 * (1 - 2.0 ** -25), torch.sign(x) * INF, x)


def sequence(p, g, m, v, s, rnd):
    """The eight lines of adam_elem on float64 tensors; rnd(k, x) is rounding k.  Returns (p2, m1, v2,
    rec) with rec[k] = (x_k, E32_k): the argument of rounding k and its f32 error bound."""
    rec = {}

    def r(k, x, e):
        rec[k] = (x, e * SECOND)
        return rnd(k, x)
    x = p * s.decay
    p1 = r("p1", x, E * x.abs() + T149)
    a = _ovf(g - m)
    b = _ovf(s.w1 * a)
    x = m + b
    m1 = r("m1", x, E * (abs(s.w1) * a.abs() + b.abs() + x.abs()) + 2 * T149)
    x = v * s.beta2
    v1 = r("v1", x, E * x.abs() + T149)
    c = _ovf(s.c2 * _ovf(g * g))
    x = v1 + c
    v2 = r("v2", x, E * (2 * c.abs() + x.abs()) + 2 * T149)
    x = torch.sqrt(v2)
    d1 = r("d1", x, E * x.abs())
    x = d1 / s.bc2_sqrt
    d2 = r("d2", x, E * x.abs() + T149)
    x = d2 + s.eps
    d3 = r("d3", x, E * x.abs())
    t = _ovf(s.step_size * _ovf(m1 / d3))
    x = p1 + t
    p2 = r("p2", x, E * (2 * t.abs() + x.abs()) + 2 * T149 * (1 + abs(s.step_size)))
    return p2, m1, v2, rec


def _r16(k, x):
    return _bf(x)


def _class_bad(g, w):
    """Elements whose class is wrong: NaN where the expectation is NaN, the same inf where it is inf,
    finite elsewhere."""
    return torch.where(torch.isnan(w), ~torch.isnan(g), torch.where(torch.isinf(w), g != w, ~torch.isfinite(g)))


def _differs(g, w):
    """bit difference, any NaN equal to any NaN"""
    return (ibits(g) != ibits(w)) & ~(torch.isnan(g) & torch.isnan(w))


def _ratio(err, bound, finite):
    z = torch.zeros_like(err)
    return torch.where(finite & (err > 0), err / bound, z)


def _report(tag, name, worst, share=None):
    WORST[(tag, name)] = max(WORST.get((tag, name), 0.0), worst)
    msg = f"optim-check {tag or '-'} {name} worst ratio {worst:.3f}"
    if share is not None:
        WORST[(tag, name + " bits")] = max(WORST.get((tag, name + " bits"), 0.0), share)
        msg += f" bit-mismatch share {share:.2e}"
    print(msg)


def check_bf16_step(name, got, inp, s, tag=None, cap=BIT_CAP):
    """The sequenced check of one bf16 step.  got = (p, m, v) after, inp = (p, g, m, v) before (g already
    clipped), any shapes.  Returns (worst ratio, bit-mismatch share)."""
    gp, gm, gv = (t.detach().cpu().reshape(-1) for t in got)
    p, g, m, v = (t.detach().cpu().reshape(-1).to(F64) for t in inp)
    assert gp.dtype == gm.dtype == gv.dtype == BF and gp.numel() == p.numel()
    if p.numel() == 0:
        return 0.0, 0.0
    out = sequence(p, g, m, v, s, _r16)
    w, rec = dict(zip("pmv", out[:3])), out[3]
    got16 = dict(p=gp, m=gm, v=gv)
    got64 = {o: t.to(F64) for o, t in got16.items()}
    D = torch.zeros(p.numel(), dtype=torch.bool)
    ratio = {}
    for o in "pmv":
        bad = _class_bad(got64[o], w[o])
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            raise AssertionError(f"{name} {o}: {int(bad.sum())} elements of the wrong class (NaN / inf / finite), first at "
                                 f"{i} (chunk {i // 8}): got {float(got64[o][i])!r} want {float(w[o][i])!r}")
        D |= _differs(got16[o], w[o].to(BF))
        x, e = rec[LAST[o]]
        fin = torch.isfinite(x) & torch.isfinite(w[o])
        ratio[o] = _ratio((got64[o] - x).abs(), b16(x, e), fin)
    share = float(D.double().mean())
    idx = D.nonzero().reshape(-1)
    if idx.numel():
        sub = [t[idx] for t in (p, g, m, v)]
        gs = {o: got16[o][idx] for o in "pmv"}
        recs = {k: (x[idx], e[idx]) for k, (x, e) in rec.items()}
        flips = {}
        for k in ROUNDS:
            x, e = recs[k]
            fin = torch.isfinite(x)
            f = round_info(torch.where(fin, x, torch.zeros_like(x)), torch.where(fin, e, torch.zeros_like(e)))[1]
            flips[k] = torch.where(fin, f, torch.zeros_like(f))
        ws = {o: w[o][idx] for o in "pmv"}
        same = {o: ~_differs(gs[o], ws[o].to(BF)) for o in "pmv"}
        explained = same["m"] & same["v"] & ((gs["p"].to(F64) - ws["p"]).abs() <= flips["p2"])
        prop = {o: torch.zeros(idx.numel(), dtype=F64) for o in "pmv"}
        for o in "mv":   # m1 / v2 itself landed within its FLIP (m + w1 (g - m) can cancel): the rest follows from it
            k = LAST[o]
            alt = sequence(*sub, s, lambda kk, x: torch.where(torch.isfinite(x), gs[o].to(F64), _bf(x)) if kk == k else _bf(x))
            ok = (gs[o].to(F64) - ws[o]).abs() <= flips[k]
            within = ok.clone()
            for o2, a in zip("pmv", alt[:3]):
                ok &= ~_differs(gs[o2], a.to(BF))
                if o2 != o:
                    mv = (alt[3][LAST[o2]][0] - recs[LAST[o2]][0]).abs()
                    prop[o2] = torch.maximum(prop[o2], torch.where(within & torch.isfinite(mv), mv, torch.zeros_like(mv)))
            explained |= ok
        for k in ROUNDS:
            for step in (1, -1):
                alt = sequence(*sub, s, lambda kk, x: bf_nbr(_bf(x), step) if kk == k else _bf(x))
                near = flips[k] > 0
                ok = near.clone()
                for o, a in zip("pmv", alt[:3]):
                    ok &= ~_differs(gs[o], a.to(BF))
                    if LAST[o] != k:
                        mv = (alt[3][LAST[o]][0] - recs[LAST[o]][0]).abs()
                        prop[o] = torch.maximum(prop[o], torch.where(near & torch.isfinite(mv), mv, torch.zeros_like(mv)))
                explained |= ok
        for o in "pmv":
            x, e = recs[LAST[o]]
            fin = torch.isfinite(x) & torch.isfinite(ws[o])
            ratio[o][idx] = _ratio((gs[o].to(F64) - x).abs(), hu(x) + (1 + U) * (e + prop[o]), fin)
        if not bool(explained.all()):
            j = int((~explained).nonzero()[0])
            i = int(idx[j])
            raise AssertionError(
                f"{name}: {int((~explained).sum())} of {p.numel()} elements differ from the sequenced expectation and no "
                f"single flipped rounding explains them; first at {i} (chunk {i // 8}, element {i % 8}): got p m v "
                f"{[float(gs[o][j]) for o in 'pmv']} want {[float(ws[o][j]) for o in 'pmv']}")
    worst = 0.0
    for o in "pmv":
        wo = float(ratio[o].max())
        worst = max(worst, wo)
        if not wo <= 1.0:
            i = int(ratio[o].argmax())
            raise AssertionError(f"{name} {o}: {int((ratio[o] > 1).sum())} elements over the bound; worst at {i} (chunk "
                                 f"{i // 8}): got {float(got64[o][i])!r} ref {float(rec[LAST[o]][0][i])!r} ratio {wo:.2f}")
    _report(tag, name, worst, share)
    assert share <= cap, f"{name}: {share:.3%} of the elements differ by bits from the sequenced expectation (cap {cap:.1%})"
    return worst, share


def ref_f32(p, g, m, v, s):
    """Float64 reference of one f32-state step and its absolute bounds: dict p, m, v -> (ref, bound)."""
    ident = lambda k, x: x   # noqa: E731
    p2, m1, v2, rec = sequence(p, g, m, v, s, ident)
    e = {k: rec[k][1] for k in ROUNDS}
    e_v = e["v1"] + e["v2"]
    sq = torch.sqrt(v2)
    e_d1 = torch.where(sq > 0, torch.minimum(e_v / sq.clamp_min(1e-300), torch.sqrt(e_v)), torch.sqrt(e_v)) + e["d1"]
    e_d3 = e_d1 / abs(s.bc2_sqrt) + e["d2"] + e["d3"]
    d3 = rec["d3"][0]
    q = m1 / d3
    e_q = (e["m1"] + q.abs() * e_d3) / (d3 - e_d3).clamp_min(1e-300) + E * q.abs() + T149
    e_p = e["p1"] + (abs(s.step_size) * e_q) * SECOND + e["p2"]
    return dict(p=(p2, e_p), m=(m1, e["m1"]), v=(v2, e_v))


def _check_bound(name, got, refs, tag):
    worst = 0.0
    for o in "pmv":
        g = got[o].detach().cpu().reshape(-1).to(F64)
        ref, bound = refs[o]
        bad = _class_bad(g, ref)
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            raise AssertionError(f"{name} {o}: {int(bad.sum())} elements of the wrong class, first at {i}: got "
                                 f"{float(g[i])!r} want {float(ref[i])!r}")
        fin = torch.isfinite(ref) & torch.isfinite(bound)
        ratio = _ratio((g - ref).abs(), bound, fin)
        wo = float(ratio.max()) if ratio.numel() else 0.0
        worst = max(worst, wo)
        if not wo <= 1.0:
            i = int(ratio.argmax())
            raise AssertionError(f"{name} {o}: {int((ratio > 1).sum())} elements over the bound; worst at {i}: got "
                                 f"{float(g[i])!r} ref {float(ref[i])!r} bound {float(bound[i]):.3e} ratio {wo:.2f}")
    return worst


def check_f32_step(name, got, inp, s, tag=None):
    """got = (p, m, v) f32 after, inp = (p, g, m, v) f32 before (g already clipped): the derived bound."""
    if got[0].numel() == 0:
        return 0.0
    refs = ref_f32(*(t.detach().cpu().reshape(-1).to(F64) for t in inp), s)
    worst = _check_bound(name, dict(zip("pmv", got)), refs, tag)
    _report(tag, name, worst)
    return worst


def _sqrt32(x):
    """sqrtf, correctly rounded: the float64 root rounded to f32 (53 >= 2 x 24 + 2 bits: the double rounding is
    innocuous).  torch's float32 sqrt on the CPU is a vector routine that is one ulp off on 0.6 % of its arguments."""
    return torch.sqrt(x.to(F64)).to(F32)


def _fma32(a, b, c):
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def master_expect(w, g, m, v, s):
    """adam_elem_master's bits: (w, m, v) f32 from f32 tensors (g: float(grad), clipped or not)."""
    sc = {k: torch.tensor(getattr(s, k), dtype=F32) for k in S.NAMES}
    p = w * sc["decay"]
    m1 = _fma32(sc["w1"], g - m, m)
    v1 = v * sc["beta2"]
    v2 = _fma32(sc["c2"], g * g, v1)
    d = _sqrt32(v2)
    d = d / sc["bc2_sqrt"]
    d = d + sc["eps"]
    return _fma32(sc["step_size"], m1 / d, p), m1, v2


def check_master_step(name, got, inp, s, tag=None, cap=BIT_CAP, bound=True):
    """got = (master f32, param bf16, m f32, v f32) after, inp = (master, g f32, m, v) before.  bound=False (the
    `exact` family, whose expected bits are the exact result): no float64 pass."""
    gw, gp, gm, gv = (t.detach().cpu().reshape(-1) for t in got)
    w, g, m, v = (t.detach().cpu().reshape(-1) for t in inp)
    assert gw.dtype == gm.dtype == gv.dtype == F32 and gp.dtype == BF and g.dtype == F32
    if w.numel() == 0:
        return 0.0, 0.0
    assert not bool(_differs(gp, gw.to(BF)).any()), f"{name}: the published parameter is not bf16(master)"
    worst = 0.0
    if bound:
        worst = _check_bound(name, dict(p=gw, m=gm, v=gv), ref_f32(*(t.to(F64) for t in (w, g, m, v)), s), tag)
    D = torch.zeros(w.numel(), dtype=torch.bool)
    for o, gt, want in zip("pmv", (gw, gm, gv), master_expect(w, g, m, v, s)):
        d = _differs(gt, want)
        far = d & ((_ordinal(gt) - _ordinal(want)).abs() > 1)
        if bool(far.any()):
            i = int(far.nonzero()[0])
            raise AssertionError(f"{name} {o}: {int(far.sum())} elements more than one f32 ulp from the expected bits; first "
                                 f"at {i} (chunk {i // 8}): got {float(gt[i])!r} want {float(want[i])!r}")
        D |= d
    share = float(D.double().mean())
    _report(tag, name, worst, share)
    assert share <= cap, f"{name}: {share:.3%} of the elements differ by bits (cap {cap:.1%})"
    return worst, share


# ------------------------------------------------------------------------------ the list kernel's walk, emulated
STEP_FAULTS = ("drop_rounding", "eps_before_div", "v_swapped", "step_on_m", "stale_pipeline", "tail_one_too_far",
               "tail_skipped", "neighbour_moments", "coef_after_rounding")


def emu_elem(p, g, m, v, s, bf=True, fault=None):
    """adam_elem in torch float32, one rounding per operation (no contraction).  Faults: drop_rounding
    (v beta2 is not rounded), eps_before_div, v_swapped (the two v updates), step_on_m (step applied
    to m, and rounded, before the division)."""
    sc = {k: torch.tensor(getattr(s, k), dtype=F32) for k in S.NAMES}
    r = (lambda x: x.to(BF).to(F32)) if bf else (lambda x: x)
    p, g, m, v = (t.to(F32) for t in (p, g, m, v))
    p = r(p * sc["decay"])
    m = r(m + sc["w1"] * (g - m))
    if fault == "v_swapped":
        v = r(v + sc["c2"] * (g * g))
        v = r(v * sc["beta2"])
    else:
        v = v * sc["beta2"]
        v = v if fault == "drop_rounding" else r(v)
        v = r(v + sc["c2"] * (g * g))
    d = r(_sqrt32(v))
    if fault == "eps_before_div":
        d = r(r(d + sc["eps"]) / sc["bc2_sqrt"])
    else:
        d = r(d / sc["bc2_sqrt"])
        d = r(d + sc["eps"])
    if fault == "step_on_m":
        p = r(p + r(sc["step_size"] * m) / d)
    else:
        p = r(p + sc["step_size"] * (m / d))
    return p, m, v


def emu_list_step(P, G, M, V, s, coef=None, grid=None, fault=None):
    """adamw_multi_bf16_kernel's walk over four bf16 ListBufs, in place on P, M, V: workgroup runs, the
    binary search, full chunks thread by thread (the register rotation only matters to the
    stale_pipeline fault: a chunk is computed from the loads of the chunk 256 further on, where the
    thread has one), the ragged tail.  For the checker's self-test; not a reference."""
    lengths = P.lengths
    for segs in runs(lengths, grid=grid):
        for i, (t, frm, to) in enumerate(segs):
            n = lengths[t]
            full = n >> 3
            end = min(to, full)
            tm = t - 1 if (fault == "neighbour_moments" and i > 0) else t
            jobs = []
            if end > frm:
                c = torch.arange(frm, end)
                src = torch.where(c + 256 < end, c + 256, c) if fault == "stale_pipeline" else c
                e8 = torch.arange(8)
                jobs.append(((src[:, None] * 8 + e8).reshape(-1), (c[:, None] * 8 + e8).reshape(-1)))
            if to > full and fault != "tail_skipped":
                el = torch.arange(full * 8, n + (1 if fault == "tail_one_too_far" else 0))
                jobs.append((el, el))
            for src, dst in jobs:
                p, g = P.flat[P.off[t] + src], G.flat[G.off[t] + src]
                m, v = M.flat[M.off[tm] + src], V.flat[V.off[tm] + src]
                if coef is not None:
                    g = g.to(F32) * torch.tensor(coef, dtype=F32)
                    g = g if fault == "coef_after_rounding" else g.to(BF)
                p, m, v = emu_elem(p, g, m, v, s, True, fault)
                P.flat[P.off[t] + dst] = p.to(BF)
                M.flat[M.off[t] + dst] = m.to(BF)
                V.flat[V.off[t] + dst] = v.to(BF)


def check_exact_step(name, got, inp, s, tag=None):
    """The `exact` family: (p, m, v) equal the float32 evaluation -- which is exact -- by bits."""
    want = emu_elem(*(t.detach().cpu().reshape(-1) for t in inp), s, got[0].dtype == BF)
    for o, gt, w in zip("pmv", got, want):
        R.check_exact(f"{name} {o}", gt.detach().cpu().reshape(-1), w.to(gt.dtype))
    _report(tag, name, 0.0, 0.0)
    return 0.0, 0.0


def check_list_bf16(name, after, before, s, coef=None, tag=None):
    """One bf16 list step: after = (P, M, V) ListBufs, before = (P, G, M, V) ListBufs as they were (G also
    as it is now: the caller passes the buffer the kernel saw).  Gaps and gradients by bits, then the
    sequenced check over the concatenation."""
    P0, G0, M0, V0 = before
    for nm, b in zip("pmv", after):
        assert b.gaps_intact(), f"{name}: the kernel wrote outside the tensors of {nm}"
    g = G0.cat()
    if coef is not None:
        g = clip_grad(g, coef, True)
    return check_bf16_step(name, [b.cat() for b in after], (P0.cat(), g, M0.cat(), V0.cat()), s, tag)


# ------------------------------------------------------------------------------ embedding
EMB_FAULTS = ("descending", "f32_sink_second_rounding", "segment_end_late", "columns_stop_at_512")


def emu_embedding_fwd(ids, weight, lo, hi):
    """out[t] = weight[ids[t] - lo], zero rows outside [lo, hi)."""
    ids = ids.reshape(-1)
    inside = (ids >= lo) & (ids < hi)
    out = weight[(ids - lo).clamp(0, max(weight.shape[0] - 1, 0))].clone() if weight.shape[0] else \
        torch.zeros(ids.numel(), weight.shape[1], dtype=weight.dtype)
    out[~inside] = 0
    return out


def emu_embedding_bwd(ids, dy, dw, sink, lo, hi, padding_idx=None, fault=None):
    """The new dweight (dw's dtype and shape): per touched row an f32 sum over its tokens in ascending
    position, one bf16 rounding, then the sink.  Untouched rows keep their bits."""
    ids = ids.reshape(-1)
    T, H = ids.numel(), dy.shape[1]
    out = dw.clone()
    skip = (ids < lo) | (ids >= hi)
    if padding_idx is not None:
        skip |= ids == padding_idx
    keys = torch.where(skip, torch.full_like(ids, -1), ids)
    sk, perm = torch.sort(keys, stable=True)
    if T == 0 or bool(skip.all()):
        return out
    start = torch.ones(T, dtype=torch.bool)
    start[1:] = sk[1:] != sk[:-1]
    seg = torch.cumsum(start, 0) - 1
    first = start.nonzero().reshape(-1)
    count = torch.diff(torch.cat([first, torch.tensor([T])]))
    rank = torch.arange(T) - first[seg]
    if fault == "descending":
        rank = count[seg] - 1 - rank
    if fault == "segment_end_late":   # the entry after a segment joins it
        late = first[1:]
        sk, perm, rank = torch.cat([sk, sk[late - 1]]), torch.cat([perm, perm[late]]), torch.cat([rank, count[seg[late - 1]]])
    cols = min(H, 512) if fault == "columns_stop_at_512" else H
    live = sk >= 0
    rows_all = (sk - lo)
    acc = torch.zeros(dw.shape[0], cols, dtype=F32)
    for k in range(int(rank[live].max()) + 1):
        sel = live & (rank == k)
        acc[rows_all[sel]] += dy[perm[sel], :cols].to(F32)
    touched = torch.unique(rows_all[live])
    a = acc[touched].to(BF).to(F32)
    if sink == PT_DW_ACC_F32:
        new = out[touched, :cols] + a
        if fault == "f32_sink_second_rounding":
            new = new.to(BF).to(F32)
    elif sink == PT_DW_ACC_BF16:
        new = (out[touched, :cols].to(F32) + a).to(BF)
    else:
        new = a.to(BF)
    out[touched, :cols] = new
    return out
