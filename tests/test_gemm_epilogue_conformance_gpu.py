"""The GEMM's fused epilogues (csrc/gemm.hip: EPI_SWIGLU_FWD 5, EPI_SWIGLU_BWD 6, EPI_ROPE 7, EPI_CE_STATS 8,
and the launch forms that exist only for them) through the C ABI against a float64 reference, per element,
on exact inputs.  Families, constructions, expectations, the sumexp bound and its derivation:
tests/_gemm_epi_ref.py (self-tested without a GPU in tests/test_gemm_epi_checker_cpu.py, which also says
which of these checks rejects which injected fault).  tests/test_gemm_conformance_gpu.py holds the plain
epilogues 0-4; its buffers, sentinels and problem builders are reused here.

On `ints` / `ints_unit` every f32 accumulator is exact in any summation order, so bf16(acc) -- what each of
these epilogues stages before applying its function -- is known by bits: g|u, the RoPE output, the logits
and the statistics' maxima are compared BIT FOR BIT, h / dg / du as the row suite compares the stand-alone
SwiGLU kernels (derived bound + the sequenced bit condition under R.BIT_CAP), sumexp within its derived
bound.  Every output and workspace starts as the NaN sentinel, every 2-D operand and output has a leading
dimension of width + 8 with guard rows, and gaps and guards are asserted intact after every launch.

Sections (the smallest shapes that reach every tile index and wave)
    a  SwiGLU forward    pt_gemm epilogue 5, tile -1 and 12
    b  SwiGLU backward   pt_gemm epilogue 6; group 0 of pt_gemm_dual (orders 0-2) beside a weight
                         gradient; 2 K-slices + pt_gemm_splitk_reduce mode 6 -- each against the
                         reference, and on ints_unit against each other's bits
    c  RoPE              pt_gemm_rope, tiles 12, 13, 14, auto with the mixed 256x256 / 256x128 launch on and
                         off; rot_cols on a wave-tile edge inside a block tile, 0 and N; seq_len below
                         the wave tile's rows.  Tile 12 does not tile N = 384: PT_EUNSUPPORTED is
                         asserted in its place, the sentinel intact.
    d  CE statistics     pt_gemm_ce_stats block 256 (tile 12) and 128 (tile 13), then
                         pt_cross_entropy_fwd_stats on the GPU's own statistics against R.ref_ce_fwd of
                         the expected logits within R.merge_stats' bound
    e  run to run        each route twice: the same bits
    f  the ratio table

Worst observed |got - ref| / bound (1 = the bound) per section and family on an MI355X, and the worst share
of elements whose bits differ from the float64-sequenced expectation (the cap is R.BIT_CAP = 5e-3); each
check prints its figure (run with -rA), test_zz_epilogue_ratio_table prints this table.  g|u, the RoPE
outputs, the logits and the statistics' maxima have no ratio: they passed bit for bit.

    section / family        h      h bits     dg     dg bits    du     du bits
    fwd / ints_unit         0.988  1.7e-3
    fwd / all_g             1.000  5.1e-6
    bwd pt_gemm / ints_unit                   0.996  2.7e-5     0.988  6.1e-5
    bwd pt_gemm / all_g                       0.996  0          1.000  1.5e-5
    bwd ksplit  / ints_unit, all_g            the bits of pt_gemm's (asserted), so its figures
    bwd dual    / ints_unit                   0.996  2.7e-5     0.988  7.3e-5

    CE family               sumexp   row_lse   row_loss
    ints_unit               0.266    0.402     0.412
    offset                  0.308    0.903     0.794
    offset_low              0.143    0.752     0.679
    flat                    0.173    0.265     0.237

No shipped kernel exceeded a bound or missed a bit.  h, dg and du sit at the bound by construction, as the
bf16 sinks of the sibling module do: where no inner rounding can flip, the bound is round-to-nearest's own
u |ref|, reached at the low end of a binade.  row_lse on `offset` is the closest of the derived ones: the
row's logits sit near 80, and merge_stats' bound is one f32 rounding of the lse plus the merge's terms.
The file's 94 cases run in about 3 s on an MI355X.
"""
import ctypes

import pytest
import torch

from picotron_amd import switches
from tests import _gemm_epi_ref as X
from tests import _gemm_ref as G
from tests import _row_ref as R
from tests.test_gemm_conformance_gpu import Buf, C_, K_, _grouped, _problem, case, guards_intact, old_of, same_bits, sentinel

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
UNSUPPORTED = -3


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return C_().stream_ptr(torch.device(DEV, torch.cuda.current_device()))


def out2d(rows, width, dtype=BF):
    """A sentinel-filled output [rows, width] with ld = width + 8 and guard rows."""
    return Buf(G.sentinel_cpu((rows, width), dtype), pad=True)


def flat_out(n, dtype=F32):
    """(full, view): a flat sentinel buffer of n elements between two 32-element guards."""
    full = sentinel((n + 64,), dtype)
    return full, full[32:32 + n]


def all_intact(*bufs):
    return all(b.intact() for b in bufs)


# ------------------------------------------------------------------------------ a. SwiGLU forward
FWD_CASES = [("ints_unit",) + s for s in X.SWIGLU_FWD_SHAPES] + [("all_g",) + X.ALL_G_SHAPE]


def route_fwd(family, M, I, K, tile):
    """pt_gemm epilogue 5: returns (h, g|u)."""
    a, b, _, _ = X.fwd_case(family, M, I, K)
    A = Buf(a, pad=True)
    Wg, Wu = (Buf(w.t().contiguous(), pad=True) for w in (b[:, :I], b[:, I:]))
    H, GU = out2d(M, I), out2d(M, 2 * I)
    assert H.ld == I + 8 and GU.ld == 2 * I + 8 and A.ld == K + 8
    K_()._gemm(A.v, A.ld, 1, [Wg.v, Wu.v], [Wg.ld, Wu.ld], [0, I, 2 * I], 1, 0, [H.v, GU.v], [H.ld, GU.ld], [0, M, M],
               M, 2 * I, K, X.EPI_SWIGLU_FWD, tile)
    torch.cuda.synchronize()
    assert all_intact(A, Wg, Wu, H, GU), f"fwd {family} {M}x{I}x{K} t{tile}: a gap or guard row was written"
    return H.v, GU.v


@pytest.mark.parametrize("tile", [-1, 12])
@pytest.mark.parametrize("family,M,I,K", FWD_CASES)
def test_swiglu_forward(family, M, I, K, tile):
    h, gu = route_fwd(family, M, I, K, tile)
    X.check_swiglu_fwd(f"fwd {family} {M}x{I}x{K} t{tile}", h, gu, X.fwd_case(family, M, I, K)[3], tag=f"epi fwd/{family}")


# ------------------------------------------------------------------------------ b. SwiGLU backward
BWD_CASES = [("ints_unit",) + s for s in X.SWIGLU_BWD_SHAPES] + [("all_g",) + X.ALL_G_SHAPE]


def _bwd_operands(family, M, I, H):
    a, b, gu, _, _ = X.bwd_case(family, M, I, H)
    A, W, RES, DGU = Buf(a, pad=True), Buf(b, pad=True), Buf(gu, pad=True), out2d(M, 2 * I)
    assert RES.ld == 2 * I + 8 and DGU.ld == 2 * I + 8 and A.ld == H + 8 and W.ld == I + 8
    return A, W, RES, DGU


def route_bwd_gemm(family, M, I, H, tile=-1):
    """pt_gemm epilogue 6: returns dg|du."""
    A, W, RES, DGU = _bwd_operands(family, M, I, H)
    K_()._gemm(A.v, A.ld, 1, [W.v], [W.ld], [0, I], 0, 0, [DGU.v], [DGU.ld], [0, M], M, I, H, X.EPI_SWIGLU_BWD, tile,
               residual=RES.v, ldr=RES.ld)
    torch.cuda.synchronize()
    assert all_intact(A, W, RES, DGU), f"bwd {family} {M}x{I}x{H} t{tile}: a gap or guard row was written"
    return DGU.v


def route_bwd_ksplit(family, M, I, H, s=2):
    """s K-slices of dh as f32 partials in a sentinel workspace, then pt_gemm_splitk_reduce mode 6."""
    A, W, RES, DGU = _bwd_operands(family, M, I, H)
    n = s * M * I
    ws, part = flat_out(n)
    pr = _problem(A, W, part.view(s * M, I), M, I, H)
    pr.ksplit, pr.kpart_stride = s, M * I
    _grouped([pr], 1, 0, G.EPI_F32, 12)
    assert bool(torch.isfinite(part).all()) and guards_intact(ws, slice(32, 32 + n))
    K_()._splitk_reduce(pr, ([DGU.v], [0, M], X.EPI_SWIGLU_BWD, RES.v, RES.ld), stream())
    torch.cuda.synchronize()
    assert all_intact(A, W, RES, DGU) and guards_intact(ws, slice(32, 32 + n))
    return DGU.v


def route_bwd_dual(order, family="ints_unit"):
    """pt_gemm_dual: epilogue 6 as group 0 beside a weight-gradient group (EPI_F32_ACC on G's `ints`).
    Returns (dg|du, dW, what G.check_case needs for dW)."""
    C = C_()
    M, I, H = X.SWIGLU_DUAL_SHAPE
    A, W, RES, DGU = _bwd_operands(family, M, I, H)
    p0 = _problem(A, W, DGU, M, I, H)
    p0.residual, p0.ldr = RES.v.data_ptr(), RES.ld
    a1, b1, prod1 = case("ints", H, I, M, seed=1)          # dW [H, I] = dY^T [H, T] . X [T, I]
    DYT, XX = Buf(a1.t().contiguous(), pad=True), Buf(b1, pad=True)
    old = old_of("ints", H, I, F32)
    DW = Buf(old, pad=True)
    p1 = _problem(DYT, XX, DW, H, I, M)
    g0, g1 = (C.GemmProblem * 1)(p0), (C.GemmProblem * 1)(p1)
    rc = C.lib().pt_gemm_dual(g0, 1, 1, 0, X.EPI_SWIGLU_BWD, g1, 1, 0, 0, G.EPI_F32_ACC, order, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert all_intact(A, W, RES, DGU, DYT, XX, DW), f"dual order {order}: a gap or guard row was written"
    return DGU.v, DW.v, dict(a=a1, b=b1, epilogue=G.EPI_F32_ACC, old=old, prod=prod1, tile=(256, 256))


@pytest.mark.parametrize("tile", [-1, 12])
@pytest.mark.parametrize("family,M,I,H", BWD_CASES)
def test_swiglu_backward_gemm(family, M, I, H, tile):
    dgu = route_bwd_gemm(family, M, I, H, tile)
    X.check_swiglu_bwd(f"bwd {family} {M}x{I}x{H} t{tile}", dgu, X.bwd_case(family, M, I, H)[4], tag=f"epi bwd-gemm/{family}")


@pytest.mark.parametrize("family,M,I,H", BWD_CASES[1:])
def test_swiglu_backward_ksplit_reduce(family, M, I, H):
    dgu = route_bwd_ksplit(family, M, I, H)
    X.check_swiglu_bwd(f"bwd-ksplit {family} {M}x{I}x{H}", dgu, X.bwd_case(family, M, I, H)[4], tag=f"epi bwd-ksplit/{family}")
    assert same_bits(dgu, route_bwd_gemm(family, M, I, H)), "the reduce pass and the fused epilogue differ by bits"


@pytest.mark.parametrize("order", [0, 1, 2])
def test_swiglu_backward_dual(order):
    M, I, H = X.SWIGLU_DUAL_SHAPE
    dgu, dw, wref = route_bwd_dual(order)
    X.check_swiglu_bwd(f"bwd-dual o{order}", dgu, X.bwd_case("ints_unit", M, I, H)[4], tag="epi bwd-dual/ints_unit")
    G.check_case("ints", dw, name=f"dual o{order} dW", **wref)
    assert same_bits(dgu, route_bwd_gemm("ints_unit", M, I, H)), "the dual launch and pt_gemm differ by bits"
    assert same_bits(dgu, route_bwd_ksplit("ints_unit", M, I, H)), "the dual launch and the reduce pass differ by bits"


# ------------------------------------------------------------------------------ c. RoPE
ROPE_MODES = {"t12": (12, None), "t13": (13, None), "t14": (14, None), "auto-mix1": (-1, 1), "auto-mix0": (-1, 0)}
TILE_BN = {12: 256, 13: 128, 14: 128}


def mix_launch_taken(M, N, rot_cols, bounds):
    """launch_mix_rope's conditions (csrc/gemm.hip), restated: the rotated columns in 256x256 tiles, the
    rest in 256x128 ones, both tile shapes fitting the problem and each part dividing over the 8 XCDs."""
    if not 0 < rot_cols < N or rot_cols % 256 or (N - rot_cols) % 128:
        return False
    if M % 256 or N % 256 or any(b % 256 for b in bounds):
        return False
    t0, t1 = M // 256 * (rot_cols // 256), M // 256 * ((N - rot_cols) // 128)
    return t0 % 8 == 0 and t1 % 8 == 0 and t0 <= 256


def rope_built(tile, N, bounds):
    """args_fit for the forced tile: N and every q | k | v boundary on the tile's column grid."""
    return tile < 0 or (N % TILE_BN[tile] == 0 and all(b % TILE_BN[tile] == 0 for b in bounds))


def route_rope(family, M, N, K, rot, seq, tile, mix=None):
    """pt_gemm_rope with B as the three segments q | k | v, tables with stride 72.  Returns (rc, C Buf)."""
    a, b, cos, sin, _, _ = X.rope_case(family, M, N, K, rot, seq)
    sizes = [N // 3] * 3
    bounds = K_()._bounds(sizes)
    A, COS, SIN, C = Buf(a, pad=True), Buf(cos, pad=True), Buf(sin, pad=True), out2d(M, N)
    Bs = [Buf(b[:, lo:lo + n].t().contiguous(), pad=True, gap=gap) for lo, n, gap in zip(bounds, sizes, (8, 16, 24))]
    assert COS.ld == SIN.ld == 72
    Cm = C_()

    def go():
        return Cm.lib().pt_gemm_rope(ptr(A.v), A.ld, Cm.ptrarr([s.v.data_ptr() for s in Bs]), Cm.i64arr([s.ld for s in Bs]),
                                     Cm.i64arr(bounds), 3, ptr(C.v), C.ld, M, N, K, ptr(COS.v), ptr(SIN.v), COS.ld, seq,
                                     rot, X.HEAD, tile, stream())
    if mix is None:
        rc = go()
    else:
        with switches.override(gemm_mix=mix):
            rc = go()
    torch.cuda.synchronize()
    assert all_intact(A, COS, SIN, C, *Bs), f"rope {M}x{N} r{rot} s{seq} t{tile}: a gap or guard row was written"
    return rc, C


@pytest.mark.parametrize("K", X.ROPE_KS)
@pytest.mark.parametrize("mode", list(ROPE_MODES))
@pytest.mark.parametrize("M,N,rot,seq", X.ROPE_SHAPES)
def test_rope(M, N, rot, seq, mode, K):
    tile, mix = ROPE_MODES[mode]
    bounds = K_()._bounds([N // 3] * 3)
    # the mixed launch is the form auto takes at exactly one of these shapes, and only while it is switched on
    assert mix_launch_taken(M, N, rot, bounds) == ((M, N) == (1024, 768))
    for family in X.FAMILIES:
        rc, C = route_rope(family, M, N, K, rot, seq, tile, mix)
        if not rope_built(tile, N, bounds):
            assert rc == UNSUPPORTED, rc
            assert guards_intact(C.full, (slice(0, 0), slice(0, 0))), "a refused launch wrote its output"
            continue
        assert rc == 0, rc
        X.check_rope(f"rope {family} {M}x{N}x{K} r{rot} s{seq} {mode}", C.v, X.rope_case(family, M, N, K, rot, seq)[5])


# ------------------------------------------------------------------------------ d. CE statistics
def route_ce(family, M, N, K, block):
    """pt_gemm_ce_stats, then pt_cross_entropy_fwd_stats on its statistics.  Returns (logits, the flat
    statistics, row_loss, row_lse, targets)."""
    a, b, _, _, _ = X.ce_case(family, M, N, K, block)
    Kp = a.shape[1]
    A, W, C = Buf(a, pad=True), Buf(b.t().contiguous(), pad=True), out2d(M, N)
    nblk = N // block
    sfull, stats = flat_out(nblk * M * 2)
    Cm = C_()
    rc = Cm.lib().pt_gemm_ce_stats(ptr(A.v), A.ld, ptr(W.v), W.ld, ptr(C.v), C.ld, ptr(stats), block, M, N, Kp, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert all_intact(A, W, C) and guards_intact(sfull, slice(32, 32 + stats.numel())), \
        f"ce {family} {M}x{N}x{K} b{block}: a gap or guard was written"
    tgt = R.make_targets(M, N)
    lfull, loss = flat_out(M)
    efull, lse = flat_out(M)
    td = tgt.to(DEV)
    rc = Cm.lib().pt_cross_entropy_fwd_stats(ptr(C.v), C.ld, ptr(td), ptr(stats), nblk, ptr(loss), ptr(lse), M, N, R.IGNORE,
                                             None, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guards_intact(lfull, slice(32, 32 + M)) and guards_intact(efull, slice(32, 32 + M)) and C.intact()
    assert guards_intact(sfull, slice(32, 32 + stats.numel()))
    return C.v, stats, loss, lse, tgt


@pytest.mark.parametrize("family", X.CE_FAMILIES)
@pytest.mark.parametrize("M,N,block", X.CE_SHAPES)
def test_ce_statistics(M, N, block, family):
    for K in X.CE_KS:
        logits, stats, loss, lse, tgt = route_ce(family, M, N, K, block)
        _, _, _, x, exp = X.ce_case(family, M, N, K, block)
        name, tag = f"ce {family} {M}x{N}x{K} b{block}", f"epi ce/{family}"
        G.check_exact(f"{name} logits", logits, x)
        X.check_stats(name, stats, exp, tag=tag)
        ref = R.ref_ce_fwd(x, tgt)
        _, lerr = R.merge_stats(exp["max"].t().to(F64), exp["sumexp"].t())
        R.check("row_lse", lse, ref["lse_clean"], lerr, tag)
        R.check("row_loss", loss, ref["loss"], torch.where(ref["valid"], lerr + R.E * ref["loss"].abs(), torch.zeros_like(lerr)), tag)


# ------------------------------------------------------------------------------ e. run to run
ROUTES = {
    "fwd-auto": lambda: route_fwd("ints_unit", 512, 384, 192, -1),
    "fwd-t12": lambda: route_fwd("ints_unit", 512, 384, 192, 12),
    "bwd-gemm": lambda: (route_bwd_gemm("ints_unit", 512, 512, 128),),
    "bwd-ksplit": lambda: (route_bwd_ksplit("ints_unit", 512, 512, 128),),
    "bwd-dual-o0": lambda: route_bwd_dual(0)[:2],
    "bwd-dual-o1": lambda: route_bwd_dual(1)[:2],
    "bwd-dual-o2": lambda: route_bwd_dual(2)[:2],
    "rope-t12": lambda: (route_rope("ints_unit", 1024, 768, 192, 512, 256, 12)[1].v,),
    "rope-t13": lambda: (route_rope("ints_unit", 512, 384, 192, 192, 64, 13)[1].v,),
    "rope-t14": lambda: (route_rope("ints_unit", 512, 384, 192, 192, 64, 14)[1].v,),
    "rope-mix": lambda: (route_rope("ints_unit", 1024, 768, 192, 512, 256, -1, 1)[1].v,),
    "rope-auto": lambda: (route_rope("ints_unit", 1024, 768, 192, 512, 256, -1, 0)[1].v,),
    "ce-b256": lambda: route_ce("ints_unit", 512, 512, 128, 256)[:4],
    "ce-b128": lambda: route_ce("ints_unit", 256, 384, 128, 128)[:4],
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_routes_run_to_run(route):
    """Each route of a-d launched twice on one ints_unit case gives the same bits."""
    first, second = ROUTES[route](), ROUTES[route]()
    assert len(first) == len(second) and all(same_bits(x, y) for x, y in zip(first, second)), route


# ------------------------------------------------------------------------------ f. the ratio table
def test_zz_epilogue_ratio_table():
    """Prints the worst |got - ref| / bound (and the worst share of bit differences from the sequenced
    expectation) per section and family seen by this process -- the module docstring's table."""
    rows = {}
    for (tag, name), w in sorted(R.WORST.items(), key=lambda kv: (str(kv[0][0]), kv[0][1])):
        if str(tag).startswith("epi "):
            rows.setdefault(tag, []).append((name, w))
    for tag, cells in rows.items():
        print(f"worst-table {tag}: " + "  ".join(f"{n} {w:.2e}" if n.endswith(" bits") else f"{n} {w:.3f}" for n, w in cells))
    assert all(w <= 1.0 for cells in rows.values() for _, w in cells)
