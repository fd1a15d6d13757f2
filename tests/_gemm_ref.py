"""GEMM conformance kit: exact and adversarial input families, a float64 reference with the epilogues'
semantics, a per-element checker and an fp32 emulator of the kernels' arithmetic (csrc/gemm.hip).

The logical problem everywhere: C[M, N] = A[M, K] . B[K, N] on bf16 CPU tensors a [M, K], b [K, N];
`operands` lays them out for a (a_kcontig, b_kcontig) pair and `padded` gives any 2-D tensor a leading
dimension of width + 8 whose gap (and guard rows) hold a NaN sentinel.

Input families (`make_case`, deterministic)
    ints         uniform integers in [-15, 15].  Every product and every partial sum is an integer below
                 2^24 for K <= 8192 (8192 * 225 < 2^21), so f32 accumulation is exact in every order and
                 on every MFMA: the expected output is the float64 result rounded once to the sink's
                 type, compared BIT FOR BIT.  Sums reach several hundred at K = 64: bf16 rounding and
                 its ties (odd integers in [256, 512)) are exercised.
    ints_scaled  ints with row m of A scaled by 2^((m mod 17) - 8) and column n of B by
                 2^((n mod 13) - 6): still exact, still bit for bit, output magnitudes 2^28 apart.
    randn        the baseline: A ~ N(0, 1), B ~ N(0, 1) / sqrt(K).  Per-element bound.
    cancel       sum_k |a||b| >> |C|: a > 0; b in [1, 2) on a 1/8 grid for k < K/2 and b[K/2 + k] =
                 -(b[k] + s 2^-7), s a non-zero integer in [-3, 3] (exact in bf16), a[K/2 + k] = a[k].
                 The partial sum at every K-tile up to K/2 is of the order of sum |a||b|, the result
                 -2^-7 sum_k a s: any rounding of a partial to bf16 is far outside the bound.
    poison       `poison(a, b, ...)`: a randn case with one NaN in A or in B (dependency footprint).
The accumulating / residual epilogues' initial values (`make_old`) are, for the exact families,
integers on the output's own scale, so that old + bf16(acc) is exact in f32 as well.

Epilogues (`expected` bit-exact on the exact families, `target_and_bound` for the others), acc the
exact product:
    EPI_BF16 bf16(acc) | EPI_BF16_ACC bf16(old + bf16(acc)) | EPI_F32 f32(acc) |
    EPI_F32_ACC f32(old + acc) | EPI_BF16_RES bf16(R + bf16(acc))
pt_gemm_splitk_reduce's modes 0-4 and pt_gemm_splitk_sum apply the same expressions to the summed
partials.

Per-element bound (derived, no slack factor): products of two bf16 values are exact in f32; a sum
of K of them in any order has at most K roundings of at most one f32 ulp each (the MFMA's internal
alignment of its products is not documented: one ulp, not half), so
    E32 = K 2^-23 sum_k |a||b|
and with u = 2^-8 (bf16 round-to-nearest):
    bf16 store      B16 = u |ref| + (1 + u) E32
    f32 store       2^-24 |ref| + E32
    EPI_BF16_ACC    B16 + u (|old + ref| + B16)          one more bf16 rounding of old + bf16(acc)
    EPI_BF16_RES    the same with R for old
    EPI_F32_ACC     2^-24 |ref| + E32 + 2^-24 |old + ref|
Every check rejects non-finite values, prints its worst |got - ref| / bound and names the worst
element with its tile and 16x16-fragment coordinates.

Emulator (`emu_gemm`): fp32 torch, 32 products per step into an f32 accumulator, then the epilogue.
`fault=` injects the bugs the checker must reject (tests/test_gemm_checker_cpu.py).
"""
import torch

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
U = 2.0 ** -8
EPI_BF16, EPI_BF16_ACC, EPI_F32, EPI_F32_ACC, EPI_BF16_RES = 0, 1, 2, 3, 4
EPILOGUES = (EPI_BF16, EPI_BF16_ACC, EPI_F32, EPI_F32_ACC, EPI_BF16_RES)
FAMILIES = ("ints", "ints_scaled", "randn", "cancel")
EXACT = ("ints", "ints_scaled")
NAN16 = 0x7FC1          # a bf16 NaN with a payload
NAN32 = 0x7FC00001      # an f32 NaN with a payload


def sink_dtype(epilogue):
    return F32 if epilogue in (EPI_F32, EPI_F32_ACC) else BF


# ------------------------------------------------------------------------------ input families
def _gen(family, M, N, K, seed):
    return torch.Generator().manual_seed(100003 * seed + 7919 * FAMILIES.index(family) + 31 * M + 17 * N + K)


def _scales(M, N):
    """ints_scaled's row and column powers of two (float64 [M, 1], [1, N])."""
    rs = torch.pow(2.0, (torch.arange(M) % 17 - 8).to(F64))[:, None]
    cs = torch.pow(2.0, (torch.arange(N) % 13 - 6).to(F64))[None, :]
    return rs, cs


def make_case(family, M, N, K, seed=0):
    """bf16 CPU (a [M, K], b [K, N]) of one family."""
    g = _gen(family, M, N, K, seed)
    if family in EXACT:
        a = torch.randint(-15, 16, (M, K), generator=g).to(F64)
        b = torch.randint(-15, 16, (K, N), generator=g).to(F64)
        if family == "ints_scaled":
            rs, cs = _scales(M, N)
            a, b = a * rs, b * cs
    elif family == "randn":
        a = torch.randn(M, K, generator=g)
        b = torch.randn(K, N, generator=g) / K ** 0.5
    elif family == "cancel":
        assert K % 2 == 0
        h = K // 2
        a1 = (torch.randn(M, h, generator=g).abs() + 0.5).to(BF).to(F64)
        b1 = torch.randint(8, 16, (h, N), generator=g).to(F64) / 8.0
        s = torch.randint(1, 4, (h, N), generator=g).to(F64) * (torch.randint(0, 2, (h, N), generator=g) * 2 - 1)
        a = torch.cat([a1, a1], 1)
        b = torch.cat([b1, -(b1 + s * 2.0 ** -7)], 0)
    else:
        raise KeyError(family)
    a16, b16 = a.to(BF), b.to(BF)
    if family != "randn":
        assert torch.equal(a16.to(F64), a.to(F64)) and torch.equal(b16.to(F64), b.to(F64)), "exact in bf16"
    return a16, b16


def make_old(family, M, N, dtype, seed=1):
    """The initial value of an accumulating sink / the residual [M, N]: for the exact families integers
    (|.| <= 1000, representable in bf16: multiples of 8) on the output's scale; else N(0, 1)."""
    g = _gen(family, M, N, 5, seed)
    if family in EXACT:
        o = (torch.randint(-125, 126, (M, N), generator=g) * 8).to(F64)
        if family == "ints_scaled":
            rs, cs = _scales(M, N)
            o = o * rs * cs
        out = o.to(dtype)
        assert torch.equal(out.to(F64), o)
        return out
    return torch.randn(M, N, generator=g).to(dtype)


def poison(a, b, which, i, j):
    """A copy of (a, b) with one NaN at a[i, j] (which = 'a': row i of C depends on it) or at b[i, j]
    ('b': column j of C)."""
    a, b = a.clone(), b.clone()
    (a if which == "a" else b)[i, j] = float("nan")
    return a, b


# ------------------------------------------------------------------------------ layouts, sentinels
def operands(a, b, a_kcontig, b_kcontig):
    """The stored operands: A [M, K] (a_kcontig) else [K, M]; B [N, K] (b_kcontig) else [K, N]."""
    return (a if a_kcontig else a.t()).contiguous(), (b.t() if b_kcontig else b).contiguous()


def _ibits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def sentinel_cpu(shape, dtype):
    t = torch.empty(shape, dtype=dtype)
    _ibits(t).fill_(NAN16 if dtype == BF else NAN32)
    return t


def padded(t, gap=8, guard=1):
    """(full, region): `full` [guard + rows + guard, width + gap] holds the NaN sentinel everywhere but
    full[region] == t; the operand is full[region], its leading dimension width + gap."""
    rows, w = t.shape
    full = sentinel_cpu((rows + 2 * guard, w + gap), t.dtype)
    region = (slice(guard, guard + rows), slice(0, w))
    full[region] = t
    return full, region


# ------------------------------------------------------------------------------ float64 reference
def ref_product(a, b):
    """(acc, S): the exact product and sum_k |a||b| in float64."""
    a6, b6 = a.to(F64), b.to(F64)
    return a6 @ b6, a6.abs() @ b6.abs()


def _bf(x):
    """float64 -> bf16 round-to-nearest-even -> float64 (through f32: exact for the exact families,
    whose values are f32 numbers; a 2^-24 relative effect elsewhere, where nothing is compared by bits)."""
    return x.to(F32).to(BF).to(F64)


def expected(acc, epilogue, old=None, residual=None):
    """The sink's contents for the exact product acc, each rounding where the epilogue has one, in the
    sink's dtype: what an exact-family output must equal bit for bit."""
    if epilogue == EPI_BF16:
        return acc.to(F32).to(BF)
    if epilogue == EPI_BF16_ACC:
        return (old.to(F64) + _bf(acc)).to(F32).to(BF)
    if epilogue == EPI_F32:
        return acc.to(F32)
    if epilogue == EPI_F32_ACC:
        return (old.to(F64) + acc).to(F32)
    if epilogue == EPI_BF16_RES:
        return (residual.to(F64) + _bf(acc)).to(F32).to(BF)
    raise KeyError(epilogue)


def target_and_bound(acc, S, K, epilogue, old=None, residual=None):
    """(unrounded float64 target, per-element bound) of an epilogue; see the module docstring."""
    e32 = K * 2.0 ** -23 * S
    b16 = U * acc.abs() + (1 + U) * e32
    if epilogue == EPI_BF16:
        return acc, b16
    if epilogue == EPI_F32:
        return acc, 2.0 ** -24 * acc.abs() + e32
    if epilogue == EPI_F32_ACC:
        t = old.to(F64) + acc
        return t, 2.0 ** -24 * acc.abs() + e32 + 2.0 ** -24 * t.abs()
    base = (old if epilogue == EPI_BF16_ACC else residual).to(F64)
    t = base + acc
    return t, b16 + U * (t.abs() + b16)


# ------------------------------------------------------------------------------ checker
WORST = {}   # (tag, name) -> worst ratio to the bound seen in this process


def where(idx, tile=None):
    """'row r col c [tile (i, j) fragment (fi, fj)]' of an output element, for a (bm, bn) tile."""
    r, c = int(idx[0]), int(idx[1])
    s = f"row {r} col {c}"
    if tile:
        bm, bn = tile
        s += f" tile ({r // bm}, {c // bn}) fragment ({r % bm // 16}, {c % bn // 16})"
    return s


def _cpu(t):
    return t.detach().to("cpu")


def check_exact(name, got, want, tile=None):
    """got == want bit for bit (dtype included); names the first differing element."""
    g, w = _cpu(got).contiguous(), want.contiguous()
    assert g.dtype == w.dtype and g.shape == w.shape, f"{name}: {g.dtype} {tuple(g.shape)} != {w.dtype} {tuple(w.shape)}"
    diff = _ibits(g) != _ibits(w)
    if bool(diff.any()):
        idx = diff.nonzero()[0]
        i = tuple(int(v) for v in idx)
        raise AssertionError(f"{name}: {int(diff.sum())} of {diff.numel()} elements differ by bits; first at "
                             f"{where(idx, tile)}: got {float(g[i])!r} want {float(w[i])!r}")
    return 0.0


def check(name, got, ref, bound, tag=None, tile=None):
    """Per element: got finite and |got - ref| <= bound.  Returns and prints the worst ratio (0 / 0
    counts as 0); raises AssertionError naming the worst element otherwise."""
    g = _cpu(got).to(F64)
    ref, bound = ref.to(F64), bound.to(F64)
    assert g.shape == ref.shape, f"{name}: shape {tuple(g.shape)} != {tuple(ref.shape)}"
    finite = torch.isfinite(g)
    if not bool(finite.all()):
        raise AssertionError(f"{name}: {int((~finite).sum())} non-finite values, first at "
                             f"{where((~finite).nonzero()[0], tile)}")
    err = (g - ref).abs()
    ratio = torch.where(err > 0, err / bound, torch.zeros_like(err))
    worst = float(ratio.max())
    key = (tag, name)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"gemm-check {tag or '-'} {name} worst ratio {worst:.3f}")
    if not worst <= 1.0:
        idx = (ratio == ratio.max()).nonzero()[0]
        i = tuple(int(v) for v in idx)
        raise AssertionError(f"{name}: {int((ratio > 1).sum())} of {ratio.numel()} elements over the bound; worst at "
                             f"{where(idx, tile)}: got {float(g[i])!r} ref {float(ref[i])!r} err {float(err[i]):.3e} "
                             f"bound {float(bound[i]):.3e} (ratio {worst:.2f})")
    return worst


def check_case(family, got, a, b, epilogue, old=None, residual=None, tag=None, tile=None, name=None, prod=None):
    """The family's check of one output: bit-exact for the exact families, else the bound.  prod: a
    cached ref_product(a, b)."""
    acc, S = prod if prod is not None else ref_product(a, b)
    name = name or f"e{epilogue}"
    if family in EXACT:
        g = _cpu(got)
        assert bool(torch.isfinite(g.float()).all()), \
            f"{name}: non-finite, first at {where((~torch.isfinite(g.float())).nonzero()[0], tile)}"
        return check_exact(name, g, expected(acc, epilogue, old, residual), tile)
    assert _cpu(got).dtype == sink_dtype(epilogue), f"{name}: dtype {got.dtype}"
    t, bound = target_and_bound(acc, S, a.shape[1], epilogue, old, residual)
    return check(name, got, t, bound, tag or family, tile)


def norm_rel(got, ref):
    """The suite's older global metric: Frobenius-norm ratio."""
    got, ref = _cpu(got).to(F64), ref.to(F64)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------ fp32 emulator
FAULTS = ("trunc_store", "half_away", "bf16_ktile", "bf16_half", "drop_k32", "dup_k32", "transposed_frag",
          "swapped_tiles", "acc_twice", "res_wrong_row", "skip_tile")
FRAG = (1, 2)    # the 16x16 fragment (row, column index) the fragment-local faults hit
FAULT_ROW = 21   # the row acc_twice hits; res_wrong_row hits the 16-row group holding it


def _rne(x):
    return x.to(BF).to(F32)


def _trunc(x):
    return (x.contiguous().view(torch.int32) & -65536).view(F32)


def _half_away(x):
    """f32 -> bf16 rounding ties away from zero (magnitude + half an ulp, truncated)."""
    return ((x.contiguous().view(torch.int32) + 0x8000) & -65536).view(F32)


def emu_gemm(a, b, epilogue, old=None, residual=None, fault=None, tile=(64, 64)):
    """The sink's contents as the kernels compute them (bf16 or f32 tensor)."""
    M, K = a.shape
    N = b.shape[1]
    af, bf = a.to(F32), b.to(F32)
    r0, c0 = 16 * FRAG[0], 16 * FRAG[1]
    acc = torch.zeros(M, N, dtype=F32)
    steps = list(range(0, K, 32))
    for k0 in steps:
        p = af[:, k0:k0 + 32] @ bf[k0:k0 + 32]
        if fault == "drop_k32" and k0 == steps[-1]:
            p[r0:r0 + 16, c0:c0 + 16] = 0
        if fault == "dup_k32" and k0 == steps[len(steps) // 2]:
            p[r0:r0 + 16, c0:c0 + 16] *= 2
        acc = acc + p
        done = k0 + 32
        if (fault == "bf16_ktile" and done % 64 == 0) or (fault == "bf16_half" and done == K // 2):
            acc = _rne(acc)
    if fault == "transposed_frag":
        acc[r0:r0 + 16, c0:c0 + 16] = acc[r0:r0 + 16, c0:c0 + 16].t().clone()
    if fault == "swapped_tiles":
        bm, bn = tile
        t0 = acc[:bm, :bn].clone()
        acc[:bm, :bn] = acc[M - bm:, N - bn:]
        acc[M - bm:, N - bn:] = t0
    rnd = {"trunc_store": _trunc, "half_away": _half_away}.get(fault, _rne)
    if epilogue == EPI_BF16:
        out = rnd(acc)
    elif epilogue == EPI_F32:
        out = acc
    elif epilogue == EPI_F32_ACC:
        out = old.to(F32) + acc
    elif epilogue == EPI_BF16_ACC:
        o = old.to(F32)
        if fault == "acc_twice":
            o = o.clone()
            o[FAULT_ROW] *= 2
        out = rnd(o + rnd(acc))
    elif epilogue == EPI_BF16_RES:
        r = residual.to(F32)
        if fault == "res_wrong_row":
            g0 = FAULT_ROW // 16 * 16
            r = r.clone()
            r[g0:g0 + 16] = residual.to(F32)[g0 + 1:g0 + 17]
        out = rnd(r + rnd(acc))
    else:
        raise KeyError(epilogue)
    out = out.to(sink_dtype(epilogue))
    if fault == "skip_tile":
        bm, bn = tile
        out[M - bm:, :bn] = sentinel_cpu((bm, bn), out.dtype)
    return out
