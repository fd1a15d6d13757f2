"""GEMM kernels (csrc/gemm.hip, through picotron_amd.kernels and the C ABI) against a float64 reference,
per element, on exact and adversarial inputs.  Families, reference, epilogue semantics, bounds and
their derivation: tests/_gemm_ref.py (self-tested without a GPU in tests/test_gemm_checker_cpu.py).

On `ints` / `ints_scaled` every f32 sum is exact in any order, so every tile, layout, epilogue,
split-K, K-halves, paired and dual launch must equal the float64 result rounded once -- bit for bit,
and therefore each other.  `randn` and `cancel` are held to the derived per-element bound.  Every
output (and every split-K workspace the tests own) starts as a NaN-payload sentinel or as known data:
a tile that is never written cannot pass.

Shapes: for tile (bm, bn) M = 2 bm, N = 3 bn (both tile indices non-zero and unequal); K = 64 ... 448
covers 1-5 and 7 K-tiles (the 2-, 3- and 4-buffer rings' prologues and tails, tiles 14 / 15's half
split), plus one K = 2048 run per tile.

What is built (mirrors kTiles / epi_layouts of gemm.hip, pinned by tests/test_gemm_host_cpu.py): the
plain sinks 0-3 on every layout of tiles 2, 3 and on every layout but (A M-contiguous, B K-contiguous)
of tiles 12-15; EPI_BF16_RES on the forward layout (A and B K-contiguous) only: 86 combinations, the
other 34 answer PT_EUNSUPPORTED (test_unbuilt_combinations_are_refused).  The fused epilogues 5-8 (SwiGLU
forward and backward, RoPE, CE statistics) and the launch forms that exist only for them are held to the
same kind of reference in tests/test_gemm_epilogue_conformance_gpu.py.

Worst observed |got - ref| / bound (1 = the bound) per family and tile over the dispatch-table test
(sections a, b), and per form for section f, on an MI355X (each check prints its figure: run with
-rA; test_zz_worst_ratio_table prints this table).  The exact families have no ratio: they passed
bit for bit.

    family  tile  EPI_BF16  BF16_ACC  F32    F32_ACC  BF16_RES (and in place)
    randn   2     0.987     0.969     0.009  0.013    0.969
    randn   3     0.989     0.979     0.008  0.013    0.979
    randn   12    0.990     0.985     0.013  0.015    0.985
    randn   13    0.987     0.972     0.013  0.015    0.972
    randn   14    0.987     0.972     0.011  0.012    0.972
    randn   15    0.987     0.969     0.008  0.012    0.969
    cancel  2     0.578     0.874     0.001  0.001    0.874
    cancel  3     0.552     0.872     0.001  0.001    0.872
    cancel  12    0.675     0.891     0.002  0.002    0.891
    cancel  13    0.639     0.902     0.002  0.002    0.902
    cancel  14    0.639     0.902     0.001  0.001    0.902
    cancel  15    0.578     0.874     0.001  0.001    0.874

    form (section f; worst over its outputs)        randn   cancel
    ksplit 1-8 slices + reduce, bf16 sinks          0.950   0.233
    ksplit 1-8 slices + reduce, f32 sinks           0.001   0.001
    fwd-halves / fwd-halves-res                     0.849   0.074
    dgrad-halves                                    0.849   0.032
    paired, bf16 sinks / f32 sink                   0.930   0.329  /  0.002  0.000
    dual dX / dW (f32 or bf16 sinks)                0.896   0.066  /  0.926  0.212

No shipped kernel exceeded a bound and every exact case passed by bits.  The bf16 sinks on randn sit
at 0.97-0.99 by construction: round-to-nearest's own error reaches u |ref| exactly at the low end of
a binade, and the bound has no slack factor; the f32 sinks show how little of E32 (K roundings of one
ulp) the hardware's accumulation uses.  The file's 208 cases run in about 5 s on an MI355X.
"""
import ctypes
import functools

import pytest
import torch

from picotron_amd import switches
from tests import _gemm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32

TILES = {2: (128, 128), 3: (64, 64), 12: (256, 256), 13: (256, 128), 14: (256, 128), 15: (128, 128)}
SIMPLE = (2, 3)
LAYOUTS = ((1, 1), (1, 0), (0, 0), (0, 1))       # (a_kcontig, b_kcontig): forward, dX, dW, the unused one
KS = (64, 128, 192, 256, 320, 448)
K_LONG = 2048


def built(tile, ak, bk, epi):
    """kTiles / epi_layouts of gemm.hip."""
    return (tile in SIMPLE or (ak, bk) != (0, 1)) and (epi != R.EPI_BF16_RES or (ak, bk) == (1, 1))


TILE_LAYOUTS = [(t, ak, bk) for t in TILES for ak, bk in LAYOUTS if built(t, ak, bk, R.EPI_BF16)]
TL_IDS = [f"t{t}-a{'k' if ak else 'm'}-b{'k' if bk else 'n'}" for t, ak, bk in TILE_LAYOUTS]


def K_():
    from picotron_amd import kernels
    return kernels


def C_():
    from picotron_amd import _C
    return _C


def shape_of(tile):
    bm, bn = TILES[tile]
    return 2 * bm, 3 * bn


@functools.lru_cache(maxsize=48)
def case(family, M, N, K, seed=0):
    """(a, b, (acc, S)) of one family and shape: the float64 reference is computed once and shared."""
    a, b = R.make_case(family, M, N, K, seed)
    return a, b, R.ref_product(a, b)


@functools.lru_cache(maxsize=48)
def old_of(family, M, N, dtype):
    return R.make_old(family, M, N, dtype)


# ------------------------------------------------------------------------------ buffers
def ibits(t):
    """The bits of a bf16 / f32 tensor as an integer CPU tensor."""
    return t.detach().contiguous().view(torch.int16 if t.dtype == BF else torch.int32).cpu()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(ibits(a), ibits(b))


def sentinel(shape, dtype):
    """A device tensor whose every element is a NaN with a payload."""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.int16 if dtype == BF else torch.int32).fill_(R.NAN16 if dtype == BF else R.NAN32)
    return t


def guards_intact(buf, region):
    """Every element of `buf` outside buf[region] still holds the sentinel's bits."""
    ib = buf.view(torch.int16 if buf.dtype == BF else torch.int32).clone()
    pat = R.NAN16 if buf.dtype == BF else R.NAN32
    ib[region] = pat
    return bool((ib == pat).all())


class Buf:
    """A 2-D device operand: `v` the logical view handed to the kernel, `full` its allocation.  pad:
    leading dimension width + gap with the sentinel in the gap and in one guard row before and after."""

    def __init__(self, t, pad=False, gap=8):
        if pad:
            full, self.region = R.padded(t, gap=gap)
        else:
            full, self.region = t, (slice(None), slice(None))
        self.full = full.to(DEV, copy=True)      # never the cached CPU tensor itself
        self.v = self.full[self.region]
        self.ld = self.v.stride(0)
        assert self.ld % 8 == 0 and self.v.data_ptr() % 16 == 0

    def intact(self):
        return guards_intact(self.full, self.region)


def out_buf(M, N, epi, old=None, pad=False, gap=8):
    """The sink of an epilogue: the sentinel for the storing ones, `old` for the accumulating ones."""
    dt = R.sink_dtype(epi)
    init = old if epi in (R.EPI_BF16_ACC, R.EPI_F32_ACC) else R.sentinel_cpu((M, N), dt)
    assert init.dtype == dt
    return Buf(init, pad, gap)


def launch(tile, ak, bk, epi, A, B, C, M, N, K, res=None):
    """One pt_gemm through kernels._gemm: unsegmented operands A, B, C (Buf), residual res (Buf)."""
    K_()._gemm(A.v, A.ld, ak, [B.v], [B.ld], [0, N], bk, 0, [C.v], [C.ld], [0, M], M, N, K, epi, tile,
               residual=None if res is None else res.v, ldr=0 if res is None else res.ld)
    torch.cuda.synchronize()


def run_plain(family, tile, ak, bk, epi, K, pad=False, alias=False, ab=None):
    """One (tile, layout, epilogue) launch at the tile's default shape; returns (got view, C Buf, args
    for R.check_case).  ab: other logical operands of the same shape (poison)."""
    M, N = shape_of(tile)
    a, b, prod = case(family, M, N, K)
    if ab is not None:
        a, b = ab
    A_st, B_st = R.operands(a, b, ak, bk)
    A, B = Buf(A_st, pad), Buf(B_st, pad)
    old = old_of(family, M, N, R.sink_dtype(epi)) if epi in (R.EPI_BF16_ACC, R.EPI_F32_ACC, R.EPI_BF16_RES) else None
    if alias:                       # EPI_BF16_RES in place: R is C
        C = Buf(old, pad)
        res = C
    else:
        C = out_buf(M, N, epi, old, pad)
        res = Buf(old, pad) if epi == R.EPI_BF16_RES else None
    launch(tile, ak, bk, epi, A, B, C, M, N, K, res)
    return C.v, C, dict(a=a, b=b, epilogue=epi, old=old, residual=old, prod=prod, tile=TILES[tile])


# ------------------------------------------------------------------------------ a. the dispatch table
@pytest.mark.parametrize("tile,ak,bk", TILE_LAYOUTS, ids=TL_IDS)
def test_dispatch_table_exact(tile, ak, bk):
    """Every built (tile, layout, epilogue) on `ints` at every K of KS and K_LONG, `ints_scaled` at a
    subset: bit-identical to the float64 result rounded once."""
    for epi in R.EPILOGUES:
        if not built(tile, ak, bk, epi):
            continue
        for K in KS + (K_LONG,):
            for family in ("ints", "ints_scaled") if K in (64, 192, 448, K_LONG) else ("ints",):
                got, _, ref = run_plain(family, tile, ak, bk, epi, K)
                R.check_case(family, got, name=f"{family} t{tile} a{ak} b{bk} e{epi} K{K}", **ref)


def test_unbuilt_combinations_are_refused():
    """The combinations kTiles / epi_layouts do not build answer PT_EUNSUPPORTED and write nothing."""
    from picotron_amd._C import HipKernelError
    unbuilt = [(t, 0, 1, e) for t in (12, 13, 14, 15) for e in R.EPILOGUES] + \
              [(t, ak, bk, R.EPI_BF16_RES) for t in (2, 3) for ak, bk in ((1, 0), (0, 0), (0, 1))] + \
              [(t, ak, bk, R.EPI_BF16_RES) for t in (12, 13, 14, 15) for ak, bk in ((1, 0), (0, 0))]
    every = [(t, ak, bk, e) for t in TILES for ak, bk in LAYOUTS for e in R.EPILOGUES]
    assert sorted(unbuilt) == sorted(c for c in every if not built(*c)) and len(every) - len(unbuilt) == 86
    for tile, ak, bk, epi in unbuilt:
        M, N = shape_of(tile)
        a, b, _ = case("ints", M, N, 64)
        A_st, B_st = R.operands(a, b, ak, bk)
        C = Buf(R.sentinel_cpu((M, N), R.sink_dtype(epi)), pad=True)
        res = Buf(old_of("ints", M, N, BF)) if epi == R.EPI_BF16_RES else None
        with pytest.raises(HipKernelError, match="UNSUPPORTED"):
            launch(tile, ak, bk, epi, Buf(A_st), Buf(B_st), C, M, N, 64, res)
        assert guards_intact(C.full, (slice(0, 0), slice(0, 0))), (tile, ak, bk, epi)


@pytest.mark.parametrize("tile", list(TILES))
@pytest.mark.parametrize("family", ["randn", "cancel"])
def test_dispatch_table_bound(family, tile):
    """The same matrix on the inexact families at K = 64, 320, 2048 with the per-element bound."""
    for ak, bk in LAYOUTS:
        for epi in R.EPILOGUES:
            if not built(tile, ak, bk, epi):
                continue
            for K in (64, 320, K_LONG):
                got, _, ref = run_plain(family, tile, ak, bk, epi, K)
                R.check_case(family, got, tag=f"{family}/t{tile}", name=f"e{epi}", **ref)


# ------------------------------------------------------------------------------ b. leading dimensions, guards
@pytest.mark.parametrize("tile,ak,bk", TILE_LAYOUTS, ids=TL_IDS)
def test_leading_dimensions_and_guards(tile, ak, bk):
    """A, B, C and R with ld = width + 8, the sentinel in every gap and in a guard row before and
    after each buffer: the output is bit-exact (so finite: no gap of A, B or R entered a product) and
    C's gaps and guards are intact by bits."""
    for epi in (R.EPI_BF16, R.EPI_BF16_ACC, R.EPI_F32_ACC, R.EPI_BF16_RES):
        if not built(tile, ak, bk, epi):
            continue
        for K in (64, 192, 320):
            got, C, ref = run_plain("ints", tile, ak, bk, epi, K, pad=True)
            assert C.ld == got.shape[1] + 8
            R.check_case("ints", got, name=f"padded t{tile} a{ak} b{bk} e{epi} K{K}", **ref)
            assert C.intact(), f"t{tile} a{ak} b{bk} e{epi} K{K}: a gap or guard row of C was written"


@pytest.mark.parametrize("tile", list(TILES))
def test_residual_in_place_equals_separate(tile):
    """EPI_BF16_RES with R aliasing C gives the bits of R separate (and of the reference)."""
    for K in (64, 320):
        for pad in (False, True):
            sep, _, ref = run_plain("ints", tile, 1, 1, R.EPI_BF16_RES, K, pad=pad)
            inp, C, _ = run_plain("ints", tile, 1, 1, R.EPI_BF16_RES, K, pad=pad, alias=True)
            R.check_case("ints", inp, name=f"in-place t{tile} K{K}", **ref)
            assert same_bits(sep, inp) and C.intact()
        got, _, ref = run_plain("randn", tile, 1, 1, R.EPI_BF16_RES, K, alias=True)
        R.check_case("randn", got, tag=f"randn/t{tile}", name="e4-in-place", **ref)


# ------------------------------------------------------------------------------ c. segments
def _split(t, sizes, dim, gaps):
    """t cut along dim into pieces of `sizes`, each its own padded allocation (Buf) with its own gap."""
    out, lo = [], 0
    for n, gap in zip(sizes, gaps):
        out.append(Buf(t.narrow(dim, lo, n).contiguous(), pad=True, gap=gap))
        lo += n
    return out


@pytest.mark.parametrize("tile", list(TILES))
def test_b_segments_along_n(tile):
    """The forward's stacked weights (and the N-contiguous form): B in 4 unequal N-segments on the
    tile's smallest boundaries, each its own allocation and leading dimension."""
    K_mod = K_()
    bm, bn = TILES[tile]
    sizes = [bn, 2 * bn, bn, bn]
    M, N = 2 * bm, sum(sizes)
    for ak, bk in ((1, 1), (0, 0)):
        for K in (64, 192):
            a, b, prod = case("ints", M, N, K)
            A_st, B_st = R.operands(a, b, ak, bk)
            A = Buf(A_st, pad=True)
            Bs = _split(B_st, sizes, 0 if bk else 1, (8, 16, 24, 8))
            for epi in (R.EPI_BF16, R.EPI_F32_ACC):
                old = old_of("ints", M, N, R.sink_dtype(epi))
                C = out_buf(M, N, epi, old, pad=True)
                K_mod._gemm(A.v, A.ld, ak, [s.v for s in Bs], [s.ld for s in Bs], K_mod._bounds(sizes), bk, 0, [C.v],
                            [C.ld], [0, M], M, N, K, epi, tile)
                torch.cuda.synchronize()
                R.check_case("ints", C.v, a, b, epi, old=old, prod=prod, tile=TILES[tile],
                             name=f"N-segments t{tile} a{ak} b{bk} e{epi} K{K}")
                assert C.intact()


@pytest.mark.parametrize("tile", list(TILES))
def test_b_segments_along_k(tile):
    """The dX's stacked weights: B in 4 unequal K-segments on 64-element boundaries, each its own
    allocation; one leading dimension over the segments (args_fit)."""
    K_mod = K_()
    M, N = shape_of(tile)
    sizes = [64, 128, 64, 192]
    K = sum(sizes)
    a, b, prod = case("ints", M, N, K)
    for ak, bk in ((1, 0), (1, 1), (0, 0)):
        A_st, B_st = R.operands(a, b, ak, bk)
        A = Buf(A_st, pad=True)
        # [N, k_i] pieces (B K-contiguous): gaps chosen so that k_i + gap is one leading dimension
        Bs = _split(B_st, sizes, 1 if bk else 0, (336, 272, 336, 208) if bk else (8, 8, 8, 8))
        assert len({s.ld for s in Bs}) == 1
        for epi in (R.EPI_BF16, R.EPI_BF16_ACC):
            old = old_of("ints", M, N, BF)
            C = out_buf(M, N, epi, old, pad=True)
            K_mod._gemm(A.v, A.ld, ak, [s.v for s in Bs], [s.ld for s in Bs], K_mod._bounds(sizes), bk, 1, [C.v], [C.ld],
                        [0, M], M, N, K, epi, tile)
            torch.cuda.synchronize()
            R.check_case("ints", C.v, a, b, epi, old=old, prod=prod, tile=TILES[tile],
                         name=f"K-segments t{tile} a{ak} b{bk} e{epi}")
            assert C.intact()


@pytest.mark.parametrize("tile", list(TILES))
def test_k_segments_with_their_own_ld_are_refused(tile):
    """Every kernel steps a tile's B image with one leading dimension, so K-segments whose leading
    dimensions differ are refused before the launch -- on the simple tiles too, which used to accept
    them and read the later segments at the first one's stride (outside the segment)."""
    from picotron_amd._C import HipKernelError
    K_mod = K_()
    M, N = shape_of(tile)
    a, b, _ = case("ints", M, N, 128)
    A_st, B_st = R.operands(a, b, 1, 0)
    A = Buf(A_st)
    Bs = _split(B_st, [64, 64], 0, (8, 16))
    C = Buf(R.sentinel_cpu((M, N), BF), pad=True)
    with pytest.raises(HipKernelError, match="UNSUPPORTED"):
        K_mod._gemm(A.v, A.ld, 1, [s.v for s in Bs], [s.ld for s in Bs], [0, 64, 128], 0, 1, [C.v], [C.ld], [0, M],
                    M, N, 128, R.EPI_BF16, tile)
    torch.cuda.synchronize()
    assert guards_intact(C.full, (slice(0, 0), slice(0, 0)))


@pytest.mark.parametrize("tile", list(TILES))
def test_c_segments_along_m(tile):
    """The weight gradient's stacked outputs: C in 4 unequal row segments on the tile's smallest
    boundaries, each its own allocation and leading dimension, guards intact."""
    K_mod = K_()
    bm, bn = TILES[tile]
    sizes = [bm, 2 * bm, bm, bm]
    M, N = sum(sizes), 3 * bn
    for ak, bk in ((0, 0), (1, 1)):
        for K in (64, 192):
            a, b, prod = case("ints", M, N, K)
            A_st, B_st = R.operands(a, b, ak, bk)
            A, B = Buf(A_st, pad=True), Buf(B_st, pad=True)
            for epi in (R.EPI_BF16, R.EPI_BF16_ACC, R.EPI_F32, R.EPI_F32_ACC):
                dt = R.sink_dtype(epi)
                old = old_of("ints", M, N, dt)
                init = old if epi in (R.EPI_BF16_ACC, R.EPI_F32_ACC) else R.sentinel_cpu((M, N), dt)
                Cs = _split(init, sizes, 0, (8, 24, 16, 8))
                K_mod._gemm(A.v, A.ld, ak, [B.v], [B.ld], [0, N], bk, 0, [c.v for c in Cs], [c.ld for c in Cs],
                            K_mod._bounds(sizes), M, N, K, epi, tile)
                torch.cuda.synchronize()
                got = torch.cat([c.v for c in Cs])
                R.check_case("ints", got, a, b, epi, old=old, prod=prod, tile=TILES[tile],
                             name=f"C-segments t{tile} a{ak} b{bk} e{epi} K{K}")
                assert all(c.intact() for c in Cs)


# ------------------------------------------------------------------------------ d. tile order
def _problem(A, B, C, M, N, K, bdim=0):
    return K_()._problem(A.v if isinstance(A, Buf) else A, A.ld if isinstance(A, Buf) else A.stride(0), [B.v], [B.ld],
                         [0, K if bdim else N], bdim, [C.v if isinstance(C, Buf) else C],
                         [C.ld if isinstance(C, Buf) else C.stride(0)], [0, M], M, N, K)


def _grouped(probs, ak, bk, epi, tile):
    C = C_()
    arr = (C.GemmProblem * len(probs))(*probs)
    rc = C.lib().pt_gemm_grouped(arr, len(probs), ak, bk, epi, tile, C.stream_ptr(torch.device(DEV, torch.cuda.current_device())))
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows", [7, 13])
@pytest.mark.parametrize("tile", [12, 13])
def test_tile_order_with_group_remainders(tile, rows):
    """7 and 13 tile rows (groups of 6 leave remainders of 1) by 3 tile columns: 21 / 39 tiles, not a
    multiple of 8, so the XCD remap takes its remainder branch.  Sentinel-filled output: a skipped or
    doubly assigned tile cannot pass."""
    bm, bn = TILES[tile]
    M, N, K = rows * bm, 3 * bn, 64
    for ak, bk in ((1, 1), (0, 0)):
        a, b, prod = case("ints", M, N, K)
        A_st, B_st = R.operands(a, b, ak, bk)
        C = out_buf(M, N, R.EPI_BF16, pad=True)
        launch(tile, ak, bk, R.EPI_BF16, Buf(A_st), Buf(B_st), C, M, N, K)
        R.check_case("ints", C.v, a, b, R.EPI_BF16, prod=prod, tile=TILES[tile], name=f"order t{tile} rows{rows} a{ak}")
        assert C.intact()


GROUP_SHAPES = {  # tile -> 4 problems (M, N) in tiles, different shapes, 16 tiles + remainders
    12: [(1, 3), (7, 1), (2, 2), (3, 1)], 13: [(1, 3), (7, 1), (2, 2), (3, 1)], 15: [(2, 5), (7, 1), (1, 1), (3, 2)],
    3: [(1, 3), (7, 2), (2, 2), (5, 1)]}


@pytest.mark.parametrize("ksplit", [1, 2])
@pytest.mark.parametrize("tile", list(GROUP_SHAPES))
def test_grouped_launch_of_four_problems(tile, ksplit):
    """pt_gemm_grouped with 4 problems of different shapes, unsplit (EPI_BF16) and as 2 K-slices
    (f32 partials in a sentinel-filled workspace + pt_gemm_splitk_reduce): bit-exact on `ints`."""
    C = C_()
    bm, bn = TILES[tile]
    K = 192 if ksplit == 1 else 384
    for ak, bk in ((0, 0), (1, 1)):
        probs, checks = [], []
        for i, (tm, tn) in enumerate(GROUP_SHAPES[tile]):
            M, N = tm * bm, tn * bn
            a, b, prod = case("ints", M, N, K, seed=i)
            A_st, B_st = R.operands(a, b, ak, bk)
            A, B = Buf(A_st, pad=True), Buf(B_st, pad=True)
            out = out_buf(M, N, R.EPI_BF16, pad=True)
            if ksplit == 1:
                pr = _problem(A, B, out, M, N, K)
                ws = None
            else:
                ws = sentinel((ksplit * M * N + 64,), F32)
                pr = _problem(A, B, ws[32:32 + ksplit * M * N].view(ksplit * M, N), M, N, K)
                pr.ksplit, pr.kpart_stride = ksplit, M * N
            probs.append(pr)
            checks.append((A, B, out, ws, pr, a, b, prod, M, N))
        _grouped(probs, ak, bk, R.EPI_BF16 if ksplit == 1 else R.EPI_F32, tile)
        for i, (A, B, out, ws, pr, a, b, prod, M, N) in enumerate(checks):
            if ws is not None:
                parts = ws[32:32 + ksplit * M * N]
                assert bool(torch.isfinite(parts).all()), "a slice's partial tile was not written"
                assert guards_intact(ws, slice(32, 32 + ksplit * M * N))
                K_()._splitk_reduce(pr, ([out.v], [0, M], R.EPI_BF16, None, 0), C.stream_ptr(out.v.device))
                torch.cuda.synchronize()
            R.check_case("ints", out.v, a, b, R.EPI_BF16, prod=prod, tile=TILES[tile],
                         name=f"grouped t{tile} ks{ksplit} a{ak} problem {i}")
            assert out.intact()


# ------------------------------------------------------------------------------ e. dependency footprint
@pytest.mark.parametrize("tile,ak,bk", TILE_LAYOUTS, ids=TL_IDS)
def test_dependency_footprint(tile, ak, bk):
    """One NaN at (m0, k0) of A makes exactly row m0 of C NaN, one at (k0, n0) of B exactly column
    n0; every other element keeps the bits of the run without it.  m0, n0 in the second tile's last
    fragment, k0 in the last k-substep: ordinary data through a valid call."""
    bm, bn = TILES[tile]
    M, N = shape_of(tile)
    K = 128
    m0, n0, k0 = 2 * bm - 3, 2 * bn - 5, K - 2
    a, b, _ = case("randn", M, N, K)
    for epi in (R.EPI_BF16, R.EPI_F32_ACC) if tile == 12 else (R.EPI_BF16,):
        clean, _, _ = run_plain("randn", tile, ak, bk, epi, K)
        assert bool(torch.isfinite(clean.float()).all())
        for which, (i, j) in (("a", (m0, k0)), ("b", (k0, n0))):
            got, _, _ = run_plain("randn", tile, ak, bk, epi, K, ab=R.poison(a, b, which, i, j))
            nan = torch.isnan(got.float()).cpu()
            want = torch.zeros(M, N, dtype=torch.bool)
            if which == "a":
                want[m0] = True
            else:
                want[:, n0] = True
            assert torch.equal(nan, want), f"t{tile} a{ak} b{bk} e{epi}: NaN in {which} reached " \
                f"{int((nan & ~want).sum())} foreign elements, missed {int((want & ~nan).sum())}; first foreign " \
                f"{R.where((nan & ~want).nonzero()[0], TILES[tile]) if bool((nan & ~want).any()) else '-'}"
            keep = ~want
            assert torch.equal(ibits(got)[keep], ibits(clean)[keep])


# ------------------------------------------------------------------------------ f. forms that change the summation order
class Out:
    """One output of a form with what its check needs."""

    def __init__(self, name, got, a, b, epi, prod, old=None, tile=None):
        self.name, self.got, self.a, self.b, self.epi, self.prod, self.old, self.tile = name, got, a, b, epi, prod, old, tile


def _check_outs(family, outs, tag):
    for o in outs:
        R.check_case(family, o.got, o.a, o.b, o.epi, old=o.old, residual=o.old, prod=o.prod, tile=o.tile,
                     tag=f"{family}/{tag}", name=o.name)


def form_ksplit(family, tile, s, ak, bk, seg=None):
    """pt_gemm_grouped with ksplit = s into a sentinel-filled workspace, then pt_gemm_splitk_reduce
    through every sink mode 0-4, modes 1 and 3 into two row segments with their own ld.  seg: B in two
    segments along "k" (the slice boundary at 256 falls inside the second: the few-tile dX over stacked
    weights, kernels.linear_dgrad) or along "n" (the few-tile forward over stacked weights)."""
    C = C_()
    bm, bn = TILES[tile]
    M, N, K = 2 * bm, 3 * bn, 512
    a, b, prod = case(family, M, N, K)
    A_st, B_st = R.operands(a, b, ak, bk)
    A = Buf(A_st)
    n = s * M * N
    ws = sentinel((n + 64,), F32)
    part = ws[32:32 + n].view(s * M, N)
    if seg is None:
        B = Buf(B_st)
        pr = _problem(A, B, part, M, N, K)
    else:
        sizes = [192, 320] if seg == "k" else [bn, 2 * bn]
        cut_rows = (seg == "k") != bool(bk)       # the stored B is cut along its rows / its columns
        B = _split(B_st, sizes, 0 if cut_rows else 1, (8, 8) if cut_rows else (136, 8) if seg == "k" else (8, 16))
        assert seg == "n" or len({p.ld for p in B}) == 1
        pr = K_()._problem(A.v, A.ld, [p.v for p in B], [p.ld for p in B], K_()._bounds(sizes), int(seg == "k"), [part],
                           [N], [0, M], M, N, K)
    pr.ksplit, pr.kpart_stride = s, M * N
    _grouped([pr], ak, bk, R.EPI_F32, tile)
    assert bool(torch.isfinite(ws[32:32 + n]).all()) and guards_intact(ws, slice(32, 32 + n))
    outs = []
    for mode in R.EPILOGUES:
        dt = R.sink_dtype(mode)
        old = old_of(family, M, N, dt) if mode in (1, 3, 4) else None
        init = old if mode in (1, 3) else R.sentinel_cpu((M, N), dt)
        sizes = [bm, M - bm] if mode in (1, 3) else [M]
        segs = _split(init, sizes, 0, (8, 16))
        res = Buf(old, pad=True) if mode == 4 else None
        K_()._splitk_reduce(pr, ([c.v for c in segs], K_()._bounds(sizes), mode, None if res is None else res.v,
                                 0 if res is None else res.ld), C.stream_ptr(A.v.device))
        torch.cuda.synchronize()
        assert all(c.intact() for c in segs)
        outs.append(Out(f"ks{s}-mode{mode}", torch.cat([c.v for c in segs]), a, b, mode, prod, old, TILES[tile]))
    return outs


def form_fwd_halves(family, residual):
    """kernels._linear_fwd_splitk: two K halves on 256x256 tiles + the sum pass (with the residual)."""
    Km = K_()
    T, N, K = 512, 512, 1024
    a, b, prod = case(family, T, N, K)
    x, w = Buf(a), Buf(b.t().contiguous())
    old = old_of(family, T, N, BF) if residual else None
    y = sentinel((T, N), BF)
    with switches.override(splitk2_min=256):
        h = Km._splitk_halves(T, N, K)
        assert h == 512
        Km._linear_fwd_splitk(x.v, [w.v[:256], w.v[256:]], h, y, None if old is None else old.to(DEV))
    torch.cuda.synchronize()
    return [Out("fwd-halves" + ("-res" if residual else ""), y, a, b, R.EPI_BF16_RES if residual else R.EPI_BF16, prod,
                old, (256, 256))]


def form_dgrad_halves(family):
    """kernels._linear_dgrad_splitk: the halves cut through the second of two stacked weights."""
    Km = K_()
    T, Kin, N = 512, 512, 1024
    a, b, prod = case(family, T, Kin, N)          # dX [T, Kin] = dY [T, N] . W [N, Kin]
    dy, w = Buf(a), Buf(b)
    dx = sentinel((T, Kin), BF)
    with switches.override(splitk2_min=256):
        h = Km._dx_splits(T, Kin, N, [w.v[:384], w.v[384:]], [384, 640], None)
        assert h == 512
        Km._linear_dgrad_splitk(dy.v, [w.v[:384], w.v[384:]], h, dx)
    torch.cuda.synchronize()
    return [Out("dgrad-halves", dx, a, b, R.EPI_BF16, prod, None, (256, 256))]


def form_paired(family, epi):
    """The paired weight gradient (KPair: A2 and two K-segments) into two row segments."""
    Km = K_()
    T, Nw, Kin = 192, 512, 512
    a, b, prod = case(family, Nw, Kin, 2 * T)      # dW [Nw, Kin] = [dY_a; dY_b]^T [X_a; X_b]
    dys = [Buf(a[:, i * T:(i + 1) * T].t().contiguous(), pad=True) for i in range(2)]
    xs = [Buf(b[i * T:(i + 1) * T].contiguous(), pad=True) for i in range(2)]
    dt = R.sink_dtype(epi)
    old = old_of(family, Nw, Kin, dt) if epi != R.EPI_BF16 else None
    init = old if old is not None else R.sentinel_cpu((Nw, Kin), dt)
    segs = _split(init, [256, 256], 0, (8, 16))
    job = (Km.KPair(dys[0].v, dys[1].v), Km.KPair(xs[0].v, xs[1].v), [c.v for c in segs])
    assert Km.wgrad_form([job], epi) == (12, 1)
    _grouped([Km._wgrad_problem(*job)], 0, 0, epi, 12)     # the launch linear_wgrad_grouped makes, refusals not hidden
    assert all(c.intact() for c in segs)
    return [Out(f"paired-e{epi}", torch.cat([c.v for c in segs]), a, b, epi, prod, old, (256, 256))]


def form_dual(family, order, ksplit, wepi=R.EPI_F32_ACC):
    """pt_gemm_dual: the plain dX epilogue beside a weight-gradient group, unsplit or as K-slices."""
    C = C_()
    T, N, Kin = 512, 512, 1024
    a0, b0, prod0 = case(family, T, Kin, N)            # dX [T, Kin] = dY [T, N] . W [N, Kin]
    a1, b1, prod1 = case(family, N, Kin, T, seed=1)    # dW [N, Kin] = dY^T [N, T] . X [T, Kin]
    dy, w = Buf(a0, pad=True), Buf(b0, pad=True)
    dyt, x = Buf(a1.t().contiguous(), pad=True), Buf(b1, pad=True)
    dx = out_buf(T, Kin, R.EPI_BF16, pad=True)
    p0 = _problem(dy, w, dx, T, Kin, N, bdim=1)
    old = old_of(family, N, Kin, R.sink_dtype(wepi))
    dw = out_buf(N, Kin, wepi, old, pad=True)
    if ksplit > 1:
        n = ksplit * N * Kin
        ws = sentinel((n + 64,), F32)
        p1 = _problem(dyt, x, ws[32:32 + n].view(ksplit * N, Kin), N, Kin, T)
        p1.ksplit, p1.kpart_stride = ksplit, N * Kin
    else:
        p1 = _problem(dyt, x, dw, N, Kin, T)
    g0, g1 = (C.GemmProblem * 1)(p0), (C.GemmProblem * 1)(p1)
    stream = C.stream_ptr(dx.v.device)
    rc = C.lib().pt_gemm_dual(g0, 1, 1, 0, R.EPI_BF16, g1, 1, 0, 0, R.EPI_F32 if ksplit > 1 else wepi, order, stream)
    assert rc == 0, rc
    if ksplit > 1:
        torch.cuda.synchronize()
        assert bool(torch.isfinite(ws[32:32 + n]).all()) and guards_intact(ws, slice(32, 32 + n))
        K_()._splitk_reduce(p1, ([dw.v], [0, N], wepi, None, 0), stream)
    torch.cuda.synchronize()
    assert dx.intact() and dw.intact()
    return [Out(f"dual-o{order}-ks{ksplit}-dx", dx.v, a0, b0, R.EPI_BF16, prod0, None, (256, 256)),
            Out(f"dual-o{order}-ks{ksplit}-dw", dw.v, a1, b1, wepi, prod1, old, (256, 256))]


FORMS = {}
for _t, _s, _l in ((12, 2, (1, 1)), (12, 4, (0, 0)), (12, 8, (1, 0)), (15, 1, (1, 1)), (15, 2, (1, 1)), (15, 2, (0, 0)),
                   (15, 4, (1, 0)), (3, 8, (1, 1)), (13, 2, (1, 0)), (14, 2, (1, 1)), (2, 4, (0, 0))):
    FORMS[f"ksplit-t{_t}-s{_s}-a{_l[0]}b{_l[1]}"] = functools.partial(form_ksplit, tile=_t, s=_s, ak=_l[0], bk=_l[1])
for _t, _s, _l, _g in ((15, 2, (1, 0), "k"), (15, 2, (1, 1), "n"), (12, 2, (1, 0), "k"), (3, 4, (1, 1), "k"), (13, 2, (0, 0), "n")):
    FORMS[f"ksplit-t{_t}-s{_s}-a{_l[0]}b{_l[1]}-{_g}seg"] = functools.partial(form_ksplit, tile=_t, s=_s, ak=_l[0],
                                                                             bk=_l[1], seg=_g)
FORMS["fwd-halves"] = functools.partial(form_fwd_halves, residual=False)
FORMS["fwd-halves-res"] = functools.partial(form_fwd_halves, residual=True)
FORMS["dgrad-halves"] = form_dgrad_halves
for _e in (R.EPI_BF16, R.EPI_BF16_ACC, R.EPI_F32_ACC):
    FORMS[f"paired-e{_e}"] = functools.partial(form_paired, epi=_e)
for _o in (0, 1, 2):
    for _ks in (1, 2):
        FORMS[f"dual-o{_o}-ks{_ks}"] = functools.partial(form_dual, order=_o, ksplit=_ks)
FORMS["dual-o2-ks1-bf16acc"] = functools.partial(form_dual, order=2, ksplit=1, wepi=R.EPI_BF16_ACC)
FORMS["dual-o2-ks2-bf16"] = functools.partial(form_dual, order=2, ksplit=2, wepi=R.EPI_BF16)


@pytest.mark.parametrize("form", list(FORMS))
def test_forms_exact(form):
    """Each form on `ints` (the K-sliced ones on `ints_scaled` too): bit-exact against float64, hence
    equal to every other form and to the single-pass kernels of section a."""
    _check_outs("ints", FORMS[form]("ints"), form)
    if form.startswith("ksplit") or form.startswith("paired"):
        _check_outs("ints_scaled", FORMS[form]("ints_scaled"), form)


@pytest.mark.parametrize("form", list(FORMS))
def test_forms_bound_on_cancel(form):
    _check_outs("cancel", FORMS[form]("cancel"), form.split("-")[0])


# ------------------------------------------------------------------------------ g. the padded path
@pytest.mark.parametrize("T,K,ns", [(100, 72, [40, 24]), (96, 128, [128])])
def test_padded_path_exact(T, K, ns):
    """kernels._linear_*_padded on `ints` off the 64-grid, every sink: bit-exact against float64 on
    the unpadded operands, the caller's out guards intact."""
    Km = K_()
    N = sum(ns)
    a, b, prod = case("ints", T, N, K)                      # Y [T, N] = x [T, K] . W^T
    x = Buf(a, pad=True)
    wt = b.t().contiguous()                                   # [N, K]
    ws = [t.to(DEV) for t in wt.split(ns)]
    for residual in (False, True):
        old = old_of("ints", T, N, BF) if residual else None
        y = out_buf(T, N, R.EPI_BF16, pad=True)
        Km._linear_fwd_padded(x.v, ws, y.v, None if old is None else Buf(old, pad=True).v)
        torch.cuda.synchronize()
        R.check_case("ints", y.v, a, b, R.EPI_BF16_RES if residual else R.EPI_BF16, residual=old, prod=prod,
                     name=f"fwd-padded res{residual}")
        assert y.intact()
    y0 = Km._linear_fwd_padded(x.v, ws, None, None)
    R.check_case("ints", y0, a, b, R.EPI_BF16, prod=prod, name="fwd-padded new")
    # dX [T, K] = dY [T, N] . W [N, K]
    ad, bd, prodd = case("ints", T, K, N, seed=1)
    dy = Buf(ad, pad=True)
    wd = [t.contiguous().to(DEV) for t in bd.split(ns)]
    for acc in (False, True):
        epi = R.EPI_BF16_ACC if acc else R.EPI_BF16
        old = old_of("ints", T, K, BF)
        dx = out_buf(T, K, epi, old, pad=True)
        Km._linear_dgrad_padded(dy.v, wd, dx.v, acc)
        torch.cuda.synchronize()
        R.check_case("ints", dx.v, ad, bd, epi, old=old, prod=prodd, name=f"dgrad-padded acc{acc}")
        assert dx.intact()
    # dW_i [n_i, K] = dY_i^T [n_i, T] . X [T, K]
    aw, bw, prodw = case("ints", N, K, T, seed=2)
    dyw, xw = Buf(aw.t().contiguous(), pad=True), Buf(bw, pad=True)
    for epi in (R.EPI_BF16, R.EPI_BF16_ACC, R.EPI_F32, R.EPI_F32_ACC):
        dt = R.sink_dtype(epi)
        old = old_of("ints", N, K, dt)
        init = old if epi in (R.EPI_BF16_ACC, R.EPI_F32_ACC) else R.sentinel_cpu((N, K), dt)
        outs = _split(init, ns, 0, (8, 16))
        Km._linear_wgrad_padded(dyw.v, xw.v, [o.v for o in outs], epi)
        torch.cuda.synchronize()
        R.check_case("ints", torch.cat([o.v for o in outs]), aw, bw, epi, old=old, prod=prodw, name=f"wgrad-padded e{epi}")
        assert all(o.intact() for o in outs)


# ------------------------------------------------------------------------------ h. run to run
@pytest.mark.parametrize("form", list(FORMS))
def test_forms_run_to_run(form):
    """The header promises a fixed summation order: each form launched twice on `randn` gives the
    same bits (and stays inside the bound)."""
    first = FORMS[form]("randn")
    second = FORMS[form]("randn")
    _check_outs("randn", first, form.split("-")[0])
    for x, y in zip(first, second):
        assert same_bits(x.got, y.got), x.name


def test_zz_worst_ratio_table():
    """Prints the worst ratio to the bound per (family / tile or form) seen by the checks of this
    process -- the module docstring's table.  Recorded, not asserted beyond the bound itself."""
    rows = {}
    for (tag, name), w in sorted(R.WORST.items(), key=lambda kv: (str(kv[0][0]), kv[0][1])):
        rows.setdefault(tag, []).append(f"{name} {w:.3f}")
    for tag, cells in rows.items():
        print(f"worst-table {tag}: " + "  ".join(cells))
    assert all(w <= 1.0 for w in R.WORST.values())
