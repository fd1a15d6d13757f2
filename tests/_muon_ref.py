"""Muon conformance kit: float64 references of every stage of optim.Muon's step (csrc/muon.hip and
kernels.muon_newton_schulz) with the bf16 roundings where the device has them, per-element bounds
derived from the operation count, and a Python emulator of the step with injectable faults
(tests/test_muon_checker_cpu.py shows the checker rejects each and accepts the clean emulator).

Every stage is checked on the inputs the device actually used (its own stored intermediates), so
an error is charged to the stage that made it and nothing is amplified by the iteration.

Elementwise stages: INTERVALS.  The exact value v of a stage computed in f32 lies within `slack`
(below: half an f32 ulp per operation, on the magnitudes it acts on) of the float64 value r; the
stored value is RNE(v) and rounding is monotone, so stored in [RNE(r - slack), RNE(r + slack)] --
half an ulp of the storage dtype plus the f32 slack, nothing tuned.  With h = 2^-24:

    lerp(s, e, w)      torch's two forms: w < 0.5: fma(w, e - s, s); else fma(-(e - s), 1 - w, e)
                       (1 - w is exact for w in [0.5, 1]): slack = h (min(w, 1 - w) |e - s| + |r|)
    clip g * coef      one product: h |r|; coef itself is a given f32 (computed here as the device does)
    u                  bf16(lerp(g', buf, mu)) of the STORED buf: an interval [u_lo, u_hi] of bf16 values
    sq = sum u^2       u in [u_lo, u_hi] gives [sum min u^2, sum max u^2]; the f32 sum of N >= 0 terms
                       over a chain of `adds` additions widens it by adds h (relative)
    X0 = bf16(u / d)   d = max(sqrt(sq), eps) from the STORED sq: sqrt and division, 2 h relative
    P' = bf16(a I + b A + c S)   f32(b) f32(c) f32(a), a product, an fma, an add:
                       slack = 4 h (|a| on the diagonal + |b A| + |c S|)
    apply              p1 = bf16(p decay): slack h |r| (+ h for f32(decay)); p = bf16(fma(-lr_adj, O, p1)),
                       lr_adj = f32(lr) f32(ratio): 3 h relative on lr_adj, h |r| for the fma
GEMM stages (A, S, X): tests/_gemm_ref.target_and_bound on the stored operands.
"""
import math

import torch

from tests import _gemm_ref as G

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
H = 2.0 ** -24
GRID = 64
BLOCK_CHUNKS = 2048   # csrc/muon.hip kBlockChunks: a block is 2048 chunks of 8 elements
NS_COEFFS = (3.4445, -4.7750, 2.0315)
FAULTS = ("lerp_branch", "norm_unrounded", "eps_added", "diag_missing", "a_whole_row", "s_bf16", "untransposed_gram",
          "decay_after", "lr_unadjusted", "tail_dropped")


def up(n):
    return -(-int(n) // GRID) * GRID


def bf(x):
    """float64 -> bf16 round-to-nearest-even -> float64"""
    return x.to(F32).to(BF).to(F64)


def rnd(x, dtype):
    return bf(x) if dtype == BF else x.to(F32).to(F64)


def f32(v):
    """a Python float as the f32 the entry points receive"""
    return float(torch.tensor(float(v), dtype=F32))


def lr_ratio(adjust_lr_fn, shape):
    R, C = shape
    if adjust_lr_fn is None or adjust_lr_fn == "original":
        return math.sqrt(max(1, R / C))
    assert adjust_lr_fn == "match_rms_adamw"
    return 0.2 * math.sqrt(max(R, C))


# ------------------------------------------------------------------------------ intervals
def interval(r, slack, dtype):
    """[RNE(r - slack), RNE(r + slack)] in the storage dtype (float64 tensors)."""
    return rnd(r - slack, dtype), rnd(r + slack, dtype)


def check_interval(name, got, lo, hi):
    """lo <= got <= hi per element, got finite; names the worst element."""
    g = got.detach().to("cpu").to(F64)
    assert g.shape == lo.shape, f"{name}: shape {tuple(g.shape)} != {tuple(lo.shape)}"
    if not bool(torch.isfinite(g).all()):
        raise AssertionError(f"{name}: {int((~torch.isfinite(g)).sum())} non-finite values")
    out = torch.maximum(lo - g, g - hi).clamp_min(0)
    bad = int((out > 0).sum())
    width = float((hi - lo).abs().max())
    print(f"muon-check {name}: {bad} of {g.numel()} outside, widest interval {width:.3e}")
    if bad:
        i = tuple(int(v) for v in (out == out.max()).nonzero()[0])
        raise AssertionError(f"{name}: {bad} of {g.numel()} elements outside their interval; worst at {i}: got "
                             f"{float(g[i])!r} not in [{float(lo[i])!r}, {float(hi[i])!r}]")


def lerp_ref(s, e, w):
    """(float64 value, f32 slack) of torch's lerp with the f32 weight w"""
    r = s + w * (e - s)
    return r, H * (min(abs(w), abs(1 - w)) * (e - s).abs() + r.abs())


def clip_coef32(global_sq, max_norm):
    """min(1, max_norm / (sqrt(sq) + 1e-6)) in f32, as every clip consumer computes it"""
    sq = torch.tensor(float(global_sq), dtype=F32)
    return float(torch.minimum(torch.tensor(1.0, dtype=F32), torch.tensor(float(max_norm), dtype=F32) /
                               (torch.sqrt(sq) + torch.tensor(1e-6, dtype=F32))))


def clipped(g, coef):
    """g' = r(g * coef) in the gradient's dtype, exactly (one IEEE f32 product)."""
    if coef is None:
        return g.to(F64)
    x = g.to(F32) * torch.tensor(coef, dtype=F32)
    return (x.to(g.dtype) if g.dtype == BF else x).to(F64)


def sq_adds(n):
    """The longest chain of f32 additions from a term to a tensor's squared norm (csrc/muon.hip): a
    thread's up to 8 chunks x 8 fused adds, the wave butterfly (6), four waves (3); the final kernel:
    ceil(blocks / 256) per thread, 6, 3."""
    blocks = -(-(-(-n // 8)) // BLOCK_CHUNKS)
    return 64 + 6 + 3 + -(-blocks // 256) + 6 + 3


# ------------------------------------------------------------------------------ the stage checks
class Case:
    """One matrix's step.  p, g, buf: CPU tensors in their storage dtypes ([R, C]); hyper-parameters as
    optim.Muon's; coef: the f32 clip coefficient or None."""

    def __init__(self, p, g, buf, lr=0.02, weight_decay=0.1, momentum=0.95, nesterov=True, ns_coefficients=NS_COEFFS,
                 eps=1e-7, ns_steps=5, adjust_lr_fn=None, coef=None):
        self.p, self.g, self.buf = p, g, buf
        self.lr, self.wd, self.mu, self.nesterov = lr, weight_decay, momentum, nesterov
        self.coeffs, self.eps, self.ns_steps, self.adjust, self.coef = ns_coefficients, eps, ns_steps, adjust_lr_fn, coef
        self.R, self.C = p.shape
        # the scheduler sees the padded images: the Gram matrix is X^T X where up(R) > up(C), X X^T
        # otherwise (equal padded sides included: its side is the same either way)
        self.tall = up(self.R) > up(self.C)


def check_momentum(c, buf_new, tag=""):
    """the stored momentum buffer"""
    gq = clipped(c.g, c.coef)
    r, slack = lerp_ref(c.buf.to(F64), gq, f32(1 - c.mu))
    check_interval(f"{tag}buf", buf_new, *interval(r, slack, c.g.dtype))


def u_interval(c, buf_new):
    """[u_lo, u_hi]: the bf16 update of every element, from the STORED new buffer"""
    gq = clipped(c.g, c.coef)
    b = buf_new.detach().to("cpu").to(F64)
    if not c.nesterov:
        return bf(b), bf(b)
    r, slack = lerp_ref(gq, b, f32(c.mu))
    return interval(r, slack, BF)


def check_sq(c, buf_new, sq, tag=""):
    """the tensor's squared norm: float64 sums over the interval of u, widened by the f32 additions"""
    lo, hi = u_interval(c, buf_new)
    mn = torch.where((lo <= 0) & (hi >= 0), torch.zeros_like(lo), torch.minimum(lo * lo, hi * hi))
    mx = torch.maximum(lo * lo, hi * hi)
    e = sq_adds(c.g.numel()) * H
    s_lo, s_hi = float(mn.sum()) * (1 - e), float(mx.sum()) * (1 + e)
    got = float(sq)
    print(f"muon-check {tag}sq: got {got:.9e} in [{s_lo:.9e}, {s_hi:.9e}] (adds {sq_adds(c.g.numel())})")
    assert math.isfinite(got) and s_lo <= got <= s_hi, f"{tag}sq: {got!r} not in [{s_lo!r}, {s_hi!r}]"


def check_x0(c, buf_new, sq, x0, tag=""):
    """X0 in the padded image: the real block per element, the padding zero"""
    lo, hi = u_interval(c, buf_new)
    d = max(math.sqrt(float(sq)), f32(c.eps))
    qlo, qhi = lo / d, hi / d
    xl = bf(qlo - 2 * H * qlo.abs())
    xh = bf(qhi + 2 * H * qhi.abs())
    x = x0.detach().to("cpu")
    assert tuple(x.shape) == (up(c.R), up(c.C)), f"{tag}X0: image {tuple(x.shape)}"
    check_interval(f"{tag}X0", x[:c.R, :c.C], xl, xh)
    check_padding(f"{tag}X0", x, c.R, c.C)


def check_padding(name, x, R, C):
    x = x.detach().to("cpu").to(F64)
    pad = x.clone()
    pad[:R, :C] = 0
    assert float(pad.abs().max()) == 0.0 and bool(torch.isfinite(x).all()), f"{name}: the padding is not zero"


def check_poly(c, A, S, P, tag=""):
    a, b, cc = (f32(v) for v in c.coeffs)
    A6, S6 = A.detach().to("cpu").to(F64), S.detach().to("cpu").to(F64)
    m = A6.shape[0]
    eye = torch.eye(m, dtype=F64)
    r = a * eye + b * A6 + cc * S6
    slack = 4 * H * (abs(a) * eye + (b * A6).abs() + (cc * S6).abs())
    check_interval(f"{tag}P", P, *interval(r, slack, BF))


def check_iteration(c, X_in, st, tag=""):
    """A, S, P', X of one iteration from the stored operands.  X_in / st[...]: padded images."""
    Rp, Cp = up(c.R), up(c.C)
    m = min(Rp, Cp)
    X = X_in.detach().to("cpu")
    A, S, P, Xn = (st[k].detach().to("cpu") for k in "ASPX")
    assert tuple(A.shape) == (m, m) == tuple(S.shape) == tuple(P.shape), f"{tag}: Gram side {tuple(A.shape)} != {m}"
    assert A.dtype == BF and S.dtype == F32 and P.dtype == BF and Xn.dtype == BF and tuple(Xn.shape) == (Rp, Cp)
    xa, xb = (X.t(), X) if c.tall else (X, X.t())   # A = X^T X | X X^T
    acc, Sabs = G.ref_product(xa, xb)
    G.check(f"{tag}A", A, *G.target_and_bound(acc, Sabs, xa.shape[1], G.EPI_BF16), tag="muon")
    acc, Sabs = G.ref_product(A, A)
    G.check(f"{tag}S", S, *G.target_and_bound(acc, Sabs, m, G.EPI_F32), tag="muon")
    check_poly(c, A, S, P, tag)
    acc, Sabs = G.ref_product(X, P) if c.tall else G.ref_product(P, X)
    G.check(f"{tag}X", Xn, *G.target_and_bound(acc, Sabs, m, G.EPI_BF16), tag="muon")
    # zero rows / columns of X stay zero; the padding of P' holds a on the diagonal only
    check_padding(f"{tag}X", Xn, c.R, c.C)
    k = c.C if c.tall else c.R   # the Gram matrix's real block
    check_padding(f"{tag}A", A, k, k)
    check_padding(f"{tag}S", S, k, k)
    Pp = P.to(F64).clone()
    Pp[:k, :k] = 0
    want = torch.zeros(m, m, dtype=F64)
    idx = torch.arange(k, m)
    want[idx, idx] = float(bf(torch.tensor(f32(c.coeffs[0]), dtype=F64)))
    assert torch.equal(Pp, want), f"{tag}P: the padding is not a on the diagonal"


def check_apply(c, p_new, O, tag=""):
    """the parameter after the decayed, scaled apply, from the STORED O (padded image)"""
    o = O.detach().to("cpu").to(F64)[:c.R, :c.C]
    decay = f32(1 - c.lr * c.wd)
    r1 = c.p.to(F64) * decay
    lo1, hi1 = interval(r1, H * r1.abs(), BF)
    la = f32(c.lr) * f32(lr_ratio(c.adjust, (c.R, c.C)))
    step = la * o
    ds = 3 * H * step.abs()
    rl, rh = lo1 - step, hi1 - step
    lo = bf(rl - ds - H * rl.abs())
    hi = bf(rh + ds + H * rh.abs())
    check_interval(f"{tag}p", p_new, lo, hi)


def check_step(c, out, tag=""):
    """Every stage of one matrix's step.  out: buf, sq, X0, iters [{A, S, P, X}], p (device or CPU)."""
    check_momentum(c, out["buf"], tag)
    check_sq(c, out["buf"], out["sq"], tag)
    check_x0(c, out["buf"], out["sq"], out["X0"], tag)
    X = out["X0"]
    assert len(out["iters"]) == c.ns_steps
    for k, st in enumerate(out["iters"]):
        check_iteration(c, X, st, f"{tag}it{k} ")
        X = st["X"]
    check_apply(c, out["p"], X, tag)


# ------------------------------------------------------------------------------ end to end
def ns_f64(u, coeffs=NS_COEFFS, ns_steps=5, eps=1e-7):
    """The float64 iteration with no roundings (O64)."""
    a, b, c = coeffs
    X = u.to(F64)
    t = X.shape[0] > X.shape[1]
    if t:
        X = X.t()
    X = X / X.norm().clamp_min(eps)
    for _ in range(ns_steps):
        A = X @ X.t()
        X = a * X + (b * A + c * (A @ A)) @ X
    return X.t() if t else X


def ns_torch_bf16(u, coeffs=NS_COEFFS, ns_steps=5, eps=1e-7):
    """torch.optim._muon._zeropower_via_newtonschulz in bf16 on the CPU."""
    from torch.optim._muon import _zeropower_via_newtonschulz
    return _zeropower_via_newtonschulz(u.clone(), tuple(coeffs), ns_steps, eps).to(F64)


def fro_rel(got, ref):
    got, ref = got.detach().to("cpu").to(F64), ref.to(F64)
    return float((got - ref).norm() / ref.norm())


def make_grad(kind, R, C, seed=0):
    """'gauss': N(0, 1) * 0.02; 'colscaled': the same with column j scaled by 2^((j mod 9) - 4)."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * R + C)
    x = torch.randn(R, C, generator=g) * 0.02
    if kind == "colscaled":
        x = x * torch.pow(2.0, (torch.arange(C) % 9 - 4).float())[None, :]
    return x.to(BF)


def cancel_case(R, C, seed=0):
    """The adversarial family for lerp's two forms (f32 storage, momentum 0.25 so that buf.lerp_ takes
    the w >= 0.5 form): buf = -3 g (1 + 1e-3 noise), so 0.25 buf + 0.75 g nearly cancels and the result is
    of the order of the noise; the right form's slack is h 0.25 |g - buf|, the wrong form errs by up to
    h 0.75 |g - buf|."""
    gen = torch.Generator().manual_seed(104729 * seed + R * 131 + C)
    g = (torch.randn(R, C, generator=gen) * 0.05).to(BF).to(F32)
    buf = (-3.0 * g.to(F64) * (1 + 1e-3 * torch.rand(R, C, generator=gen, dtype=F64))).to(F32)
    return g, buf


# ------------------------------------------------------------------------------ emulator
def _lerp32(s, e, w, wrong=False):
    """torch's lerp on f32 tensors with the device's fused multiply-adds (a product of two f32 values is
    exact in float64, so float64 and one rounding to f32 is the fma); wrong: the other form"""
    small = (abs(w) < 0.5) != wrong
    d = (e - s).to(F64)
    if small:
        return (w * d + s.to(F64)).to(F32)
    return (e.to(F64) - d * f32(1 - w)).to(F32)


def emu_step(c, fault=None):
    """The step as the device computes it, in f32 torch on the CPU; returns check_step's `out`."""
    assert fault is None or fault in FAULTS
    bfd = c.g.dtype == BF
    g = clipped(c.g, c.coef).to(F32)
    buf = _lerp32(c.buf.to(F32), g, f32(1 - c.mu), wrong=fault == "lerp_branch")
    buf = buf.to(c.g.dtype)
    if fault == "tail_dropped" and c.g.numel() % 8:
        flat, old = buf.reshape(-1), c.buf.reshape(-1)
        flat[c.g.numel() // 8 * 8:] = old[c.g.numel() // 8 * 8:]
    b32 = buf.to(F32)
    u_raw = _lerp32(g, b32, f32(c.mu)) if c.nesterov else b32
    u = u_raw.to(BF).to(F32)
    sq = ((u_raw if fault == "norm_unrounded" else u).to(F64) ** 2).sum().to(F32)
    eps = torch.tensor(c.eps, dtype=F32)
    d = sq.sqrt() + eps if fault == "eps_added" else torch.maximum(sq.sqrt(), eps)
    Rp, Cp = up(c.R), up(c.C)
    X = torch.zeros(Rp, Cp, dtype=BF)
    X[:c.R, :c.C] = (u / d).to(BF)
    out = {"buf": buf, "sq": sq, "X0": X.clone(), "iters": []}
    a, b, cc = (torch.tensor(v, dtype=F32) for v in c.coeffs)
    gram_tall = c.tall and fault != "untransposed_gram"
    for _ in range(c.ns_steps):
        Xf = X.to(F32)
        A = (Xf.t() @ Xf if gram_tall else Xf @ Xf.t()).to(BF)
        S = A.to(F32) @ A.to(F32)
        m = A.shape[0]
        Sp = S.to(BF).to(F32) if fault == "s_bf16" else S
        P = b * A.to(F32) + cc * Sp
        if fault == "a_whole_row":
            P[3] += a
        if fault != "diag_missing":
            P = P + a * torch.eye(m, dtype=F32)
        P = P.to(BF)
        X = (Xf @ P.to(F32) if gram_tall else P.to(F32) @ Xf).to(BF)
        out["iters"].append({"A": A, "S": S, "P": P, "X": X.clone()})
    o = X.to(F32)[:c.R, :c.C]
    decay = torch.tensor(1 - c.lr * c.wd, dtype=F32)
    ratio = 1.0 if fault == "lr_unadjusted" else lr_ratio(c.adjust, (c.R, c.C))
    la = torch.tensor(c.lr, dtype=F32) * torch.tensor(ratio, dtype=F32)
    p = c.p.to(F32)
    if fault == "decay_after":
        p = ((p.to(F64) - la.to(F64) * o.to(F64)).to(F32).to(BF).to(F32) * decay).to(BF)
    else:   # (the fma through float64, as in _lerp32)
        p = ((p * decay).to(BF).to(F64) - la.to(F64) * o.to(F64)).to(F32).to(BF)
    out["p"] = p
    return out
