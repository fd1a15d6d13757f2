"""Mixture-of-experts routing conformance kit: a CPU reference in integers and float64 for every
kernel of csrc/moe.hip, the logit families of the tests, and per-element checkers.

Definitions (kernels.moe_route / moe_plan / moe_dispatch / moe_combine / moe_combine_bwd /
moe_route_bwd), T tokens, E experts, k choices, C rows per expert:
    p        = softmax over the E STORED bf16 logits, float64 here
    idx      = the k largest stored values, ties to the lower expert, best first      (integers)
    gate     = p[idx], divided by their sum under norm_topk_prob
    counts_e = the number of items (t, j) with idx = e, before dropping               (integers)
    aux      = E sum_e (counts_e / (T k)) (mean_t p[t, e])
    item i = t k + j;  pos(i) = the number of items before i with the same expert
    slot[i]  = idx C + pos where pos < C, else -1;  src[slot] = i, -1 for empty rows  (integers)
    xe[r]    = x[src[r] // k], zeros for empty rows                                   (bits)
    y[t]     = residual[t] + sum_j gate[t, j] ye[slot[t, j]] over the kept items
    dye[r]   = gate[src[r]] dy[src[r] // k], zeros for empty rows
    dgate[i] = <dy[t], ye[slot[i]]>, 0 for dropped items
    dlogits  = d/dlogits of sum(gate dgate) + d_aux aux with idx and counts held fixed

Logit families (`make_logits`): "randn" Gaussian; "equal" every value the same, so every selection is
a tie; "dominant" one expert far above the rest for every token, which overflows its capacity at
capacity_factor 1; "pm60" values near +-60, where exp overflows without the max subtraction.

Relative error (`rel_err`): |got - ref| / max(|ref|, 2^-100).  f32 holds no relative precision below
its normal range (2^-126), so a value down there is judged absolutely, at 2^-126 / 2^-100 = 2^-26.
"""

import torch

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
I32 = torch.int32
REL_FLOOR = 2.0 ** -100
LOGIT_FAMILIES = ("randn", "equal", "dominant", "pm60")
TOKENS = (1, 63, 192, 1000)
EXPERTS = ((1, 1), (8, 2), (60, 4), (128, 8))
HIDDEN = (64, 128)
PLAN_BLOCK = 1024   # items per workgroup of pt_moe_plan (pt_moe_plan_block()): T k straddles it below


def route_cases():
    """(family, T, E, k) of the route / plan conformance tests: the grid, plus T k one below, at and
    above the plan kernels' block (k = 1: 1023, 1024, 1025 items; k = 2: 1022, 1024, 1026)."""
    out = [(f, T, E, k) for f in LOGIT_FAMILIES for T in TOKENS for E, k in EXPERTS]
    out += [(f, PLAN_BLOCK + d, 1, 1) for f in ("randn",) for d in (-1, 0, 1)]
    out += [(f, PLAN_BLOCK // 2 + d, 8, 2) for f in ("randn", "dominant") for d in (-1, 0, 1)]
    out += [("dominant", PLAN_BLOCK + 1, 60, 4)]
    return out

# torch's own f32 CPU softmax + renormalisation + aux formula against float64, the largest rel_err over
# every (family, T, E, k, norm) case of tests/test_moe_conformance_gpu.py (`route_cases`): measured
# 7.19e-7 (probs 7.19e-7 at "dominant" T 1025 E 60, gate 4.71e-7, aux 2.17e-7;
# tests/test_moe_checker_cpu.py re-measures it and holds it under this figure).  The kernels are allowed 4 times
# that, and never less than 2^-22: exponentials and summation orders differ legitimately, a wrong
# formula is orders of magnitude away.
TORCH_F32_REL = 7.2e-7
F32_TOL = max(4 * TORCH_F32_REL, 2.0 ** -22)


def _seed(*key):
    """A seed that does not depend on Python's hash randomisation."""
    s = 0
    for ch in "|".join(str(k) for k in key):
        s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


def gen(*key):
    g = torch.Generator()
    g.manual_seed(_seed(*key))
    return g


def make_logits(family, T, E, seed=0):
    """bf16 [T, E] CPU logits of one family."""
    g = gen("logits", family, T, E, seed)
    if family == "randn":
        x = torch.randn(T, E, generator=g)
    elif family == "equal":
        x = torch.full((T, E), 0.75)
    elif family == "dominant":
        x = torch.randn(T, E, generator=g)
        x[:, (seed + 3) % E] += 12.0
    elif family == "pm60":
        sign = torch.randint(0, 2, (T, E), generator=g).float() * 2 - 1
        x = sign * 60.0 + torch.randn(T, E, generator=g)
    else:
        raise KeyError(family)
    return x.to(BF)


# ------------------------------------------------------------------------------------- reference
def ref_select(logits, k):
    """idx int32 [T, k]: the k largest stored values, ties to the lower index (a stable sort)."""
    v = logits.to(F32)   # exact
    order = torch.sort(v, dim=1, descending=True, stable=True).indices
    return order[:, :k].to(I32).contiguous()


def ref_route(logits, k, norm=True, idx=None, dtype=F64):
    """(idx, gate, probs, counts, aux) in `dtype` arithmetic (float64: the reference; float32:
    torch's own f32 evaluation, whose error sizes the kernels' tolerance)."""
    T, E = logits.shape
    if idx is None:
        idx = ref_select(logits, k)
    p = torch.softmax(logits.to(dtype), dim=1)
    sel = p.gather(1, idx.long())
    gate = sel / sel.sum(dim=1, keepdim=True) if norm else sel
    counts = torch.bincount(idx.reshape(-1).long(), minlength=E).to(I32)
    f = counts.to(dtype) / (T * k)
    aux = E * (f * p.mean(dim=0)).sum()
    return idx, gate, p, counts, aux.reshape(1)


def ref_plan(idx, E, C):
    """(slot int32 [T, k], src int32 [E C]) by the definition, in integers."""
    T, k = idx.shape
    flat = idx.reshape(-1).long()
    onehot = flat[:, None] == torch.arange(E)[None, :]
    pos = (onehot.cumsum(0) - 1)[torch.arange(flat.numel()), flat]
    keep = pos < C
    slot = torch.where(keep, flat * C + pos, torch.full_like(pos, -1))
    src = torch.full((E * C,), -1, dtype=torch.long)
    src[slot[keep]] = torch.arange(flat.numel())[keep]
    return slot.reshape(T, k).to(I32), src.to(I32)


def ref_dispatch(x, src, k):
    out = torch.zeros(src.numel(), x.shape[1], dtype=x.dtype)
    kept = src >= 0
    out[kept] = x[(src[kept] // k).long()]
    return out


def ref_combine(ye, slot, gate=None, residual=None):
    """float64 [T, H] (unrounded)."""
    T, k = slot.shape
    y = residual.to(F64).clone() if residual is not None else torch.zeros(T, ye.shape[1], dtype=F64)
    for j in range(k):
        s = slot[:, j].long()
        kept = s >= 0
        w = gate[:, j].to(F64) if gate is not None else torch.ones(T, dtype=F64)
        y[kept] += w[kept, None] * ye[s[kept]].to(F64)
    return y


def ref_combine_bwd(dy, ye, slot, src, gate):
    """(dye float64 [R, H], dgate float64 [T, k], sum_h |dy ye| per item: the dot products' scale)."""
    T, k = slot.shape
    R, H = ye.shape
    dye = torch.zeros(R, H, dtype=F64)
    kept = src >= 0
    items = src[kept].long()
    dye[kept] = gate.reshape(-1).to(F64)[items, None] * dy.to(F64)[items // k]
    dgate = torch.zeros(T * k, dtype=F64)
    mag = torch.zeros(T * k, dtype=F64)
    s = slot.reshape(-1).long()
    on = s >= 0
    tok = torch.arange(T * k)[on] // k
    prod = dy.to(F64)[tok] * ye.to(F64)[s[on]]
    dgate[on] = prod.sum(1)
    mag[on] = prod.abs().sum(1)
    return dye, dgate.reshape(T, k), mag.reshape(T, k)


def ref_route_bwd(logits, idx, dgate, d_aux, norm=True):
    """float64 autograd through the reference router with idx (and so counts) held fixed."""
    T, E = logits.shape
    k = idx.shape[1]
    lg = logits.to(F64).clone().requires_grad_(True)
    p = torch.softmax(lg, dim=1)
    sel = p.gather(1, idx.long())
    gate = sel / sel.sum(dim=1, keepdim=True) if norm else sel
    f = torch.bincount(idx.reshape(-1).long(), minlength=E).to(F64) / (T * k)
    aux = E * (f * p.mean(dim=0)).sum()
    ((gate * dgate.to(F64)).sum() + float(d_aux) * aux).backward()
    return lg.grad, p.detach()


def route_bwd_allowance(p, idx, dgate, d_aux, norm=True, tol=None):
    """The f32 tolerance of the forward, propagated to dlogits (float64 [T, E], added to the one bf16
    ulp of the store).  The kernel reads probs that carry a relative error tol, re-forms gate = p / s
    from them (2 tol), the dot product sum_i dgate_i gate_i and the division by s (tol each): to
    first order every dp[t, e] is off by at most 4 tol m[t, e], with m the sum of the MAGNITUDES that
    meet in it,
        m[t, idx_j] = (|dgate_j| + sum_i |dgate_i| gate_i) / s   (norm)   |   |dgate_j|
        m[t, e]    += |d_aux| E f_e / T,
    and dlogit = p (dp - sum_e' p dp) adds the error of p itself (tol) and of the inner sum: at most
        8 tol p[t, e] (m[t, e] + sum_e' p[t, e'] m[t, e']).
    The f32 roundings of the kernel's own arithmetic (2^-24 each) are far inside the factor 8."""
    tol = F32_TOL if tol is None else tol
    T, E = p.shape
    k = idx.shape[1]
    p = p.to(F64)
    sel = p.gather(1, idx.long())
    g = dgate.to(F64).abs()
    if norm:
        s = sel.sum(1, keepdim=True)
        msel = (g + (g * sel / s).sum(1, keepdim=True)) / s
    else:
        msel = g
    f = torch.bincount(idx.reshape(-1).long(), minlength=E).to(F64) / (T * k)
    m = (abs(float(d_aux)) * E * f / T)[None, :].expand(T, E).clone()
    m.scatter_add_(1, idx.long(), msel)
    return 8 * tol * p * (m + (p * m).sum(1, keepdim=True))


# -------------------------------------------------------------------------------------- checkers
def _cpu(t):
    return t.detach().to("cpu")


def rel_err(got, ref):
    g, r = _cpu(got).to(F64), ref.to(F64)
    assert g.shape == r.shape, f"shape {tuple(g.shape)} != {tuple(r.shape)}"
    assert bool(torch.isfinite(g).all()), "non-finite values"
    return float(((g - r).abs() / r.abs().clamp_min(REL_FLOOR)).max()) if g.numel() else 0.0


def check_exact(name, got, want):
    """Equal in dtype, shape and every element (integers; bf16 bit copies)."""
    g, w = _cpu(got).contiguous(), want.contiguous()
    assert g.dtype == w.dtype and g.shape == w.shape, f"{name}: {g.dtype} {tuple(g.shape)} != {w.dtype} {tuple(w.shape)}"
    a = g.view(torch.int16) if g.dtype == BF else g
    b = w.view(torch.int16) if w.dtype == BF else w
    diff = a != b
    if bool(diff.any()):
        i = tuple(int(v) for v in diff.nonzero()[0])
        raise AssertionError(f"{name}: {int(diff.sum())} of {diff.numel()} elements differ; first at {i}: "
                             f"got {g[i].item()!r} want {w[i].item()!r}")


def check_rel(name, got, ref, tol=F32_TOL):
    """rel_err(got, ref) <= tol; prints the figure first."""
    assert _cpu(got).dtype == F32, f"{name}: dtype {got.dtype}"
    e = rel_err(got, ref)
    print(f"moe-check {name} rel err {e:.3e} (tol {tol:.3e})")
    assert e <= tol, f"{name}: relative error {e:.3e} over {tol:.3e}"
    return e


def bf16_ulp(ref):
    """The spacing of bf16 at |ref| (float64): 2^(floor(log2 |ref|) - 7), the subnormal spacing below 2^-126."""
    a = ref.to(F64).abs().clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 7)


def check_bound(name, got, ref, bound):
    """Per element: finite and |got - ref| <= bound.  Prints and returns the worst ratio."""
    g = _cpu(got).to(F64)
    ref, bound = ref.to(F64), bound.to(F64)
    assert g.shape == ref.shape, f"{name}: shape {tuple(g.shape)} != {tuple(ref.shape)}"
    assert bool(torch.isfinite(g).all()), f"{name}: non-finite values"
    err = (g - ref).abs()
    ratio = torch.where(err > 0, err / bound, torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"moe-check {name} worst ratio {worst:.3f}")
    if not worst <= 1.0:
        i = tuple(int(v) for v in (ratio == ratio.max()).nonzero()[0])
        raise AssertionError(f"{name}: {int((ratio > 1).sum())} of {ratio.numel()} elements over the bound; worst at {i}: "
                             f"got {float(g[i])!r} ref {float(ref[i])!r} err {float(err[i]):.3e} bound {float(bound[i]):.3e}")
    return worst


def check_bf16(name, got, ref, extra=None, zero=None):
    """A bf16 output against its float64 value: |got - ref| <= 1 bf16 ulp of ref (+ extra, a
    per-element float64 allowance); the elements under the mask `zero` must be exactly zero."""
    assert _cpu(got).dtype == BF, f"{name}: dtype {got.dtype}"
    bound = bf16_ulp(ref) if extra is None else bf16_ulp(ref) + extra.to(F64)
    if zero is not None:
        z = _cpu(got)[zero]
        assert bool((z.view(torch.int16) == 0).all()) if z.numel() else True, f"{name}: a dropped / empty element is not +0"
    return check_bound(name, got, ref, bound)


def check_dgate(name, got, ref, mag, H, dropped):
    """|got - ref| <= H 2^-23 sum_h |dy ye| (the f32 dot-product bound); dropped items exactly 0."""
    g = _cpu(got)
    assert g.dtype == F32, f"{name}: dtype {g.dtype}"
    assert bool((g[dropped] == 0).all()), f"{name}: a dropped item's dgate is not 0"
    return check_bound(name, got, ref, H * 2.0 ** -23 * mag)


def coherent_rows(src, k, T, H, seed, empty=1.0e4):
    """(residual [T, H], ye [R, H], sign [T, H]) bf16 test data for the combine checks: magnitudes in
    [0.5, 2), and every term that meets in one output element (t, h) -- the residual and the expert
    rows of token t -- carries the same sign s[t, h].  A sum of same-signed terms has no cancellation,
    so the f32 accumulation error (at most 9 roundings of 2^-24 relative) is far inside one bf16 ulp of
    the result and the 1-ulp bound holds by construction.  Empty rows hold `empty`: reading one shows."""
    g = gen("coherent", T, H, src.numel(), seed)
    sign = (torch.randint(0, 2, (T, H), generator=g).float() * 2 - 1)
    res = (sign * (0.5 + 1.5 * torch.rand(T, H, generator=g))).to(BF)
    R = src.numel()
    ye = torch.full((R, H), empty)
    kept = src >= 0
    tok = (src[kept] // k).long()
    ye[kept] = sign[tok] * (0.5 + 1.5 * torch.rand(int(kept.sum()), H, generator=g))
    return res, ye.to(BF), sign
