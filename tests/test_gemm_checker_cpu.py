"""The GEMM conformance kit (tests/_gemm_ref.py) tested on itself, without a GPU.

  * the clean fp32 emulator passes every check for every family and every plain epilogue at
    K = 64, 256, 2048, bit for bit on `ints` and `ints_scaled`;
  * every injected fault is rejected on at least one family;
  * the families' own claims hold in float64.

Each fault, the families whose check rejects it (at 128 x 192 x 256, 64 x 64 tiles, through the
epilogue the fault lives in: every one unless named), and what the suite's older metric -- one
Frobenius-norm ratio < 1e-2 on `randn` -- makes of it at 512 x 512 x 256, and for the faults confined
to one 16 x 16 fragment at 4096 x 2048 as well (the 512 x 512 slice holding the fragment, the clean
error and the reference norm scaled to the other 31 slices).  FAULT_TABLE, asserted by
test_injected_fault_is_rejected, which prints the metric's values:

    fault            rejected on                          old metric 512x512x256   at 4096x2048
    trunc_store      ints, ints_scaled, randn             missed (0.0033)
    half_away        ints, ints_scaled                    missed (0.0017 = clean)
    bf16_ktile       every family                         missed (0.0026)
    bf16_half        every family                         missed (0.0020)
    drop_k32         every family                         caught (0.0104)          missed (0.0025)
    dup_k32          every family                         caught (0.0109)          missed (0.0025)
    transposed_frag  every family                         caught (0.045)           missed (0.0082)
    swapped_tiles    every family                         caught (0.25)
    acc_twice        every family (EPI_BF16_ACC)          caught (0.034, one row of 512)
    res_wrong_row    every family (EPI_BF16_RES)          caught (0.18)
    skip_tile        every family (non-finite)            caught (NaN)

half_away differs from round-to-nearest-even only on exact ties, which random data never produces:
only the exact families see it (every odd sum in [256, 512) of `ints` is a tie).  trunc_store's error
(up to 2 u |ref|) leaves the bf16 bound on most of randn's elements but stays inside cancel's, whose
bound is dominated by E32.
"""
import math

import pytest
import torch

from tests import _gemm_ref as R


@pytest.fixture(autouse=True)
def _leave_the_worst_table_alone():
    """The injected faults' ratios must not reach the table tests/test_gemm_conformance_gpu.py prints
    (and bounds) from R.WORST when both files run in one process."""
    saved = dict(R.WORST)
    yield
    R.WORST.clear()
    R.WORST.update(saved)


ALL = R.FAMILIES
# fault -> (families that must reject it, the epilogue the old metric is evaluated through,
#           caught by rel_err < 1e-2 on randn at 512 x 512 x 256, caught at 4096 x 2048 (fragment-local faults))
FAULT_TABLE = {
    "trunc_store": (("ints", "ints_scaled", "randn"), R.EPI_BF16, False, None),
    "half_away": (("ints", "ints_scaled"), R.EPI_BF16, False, None),
    "bf16_ktile": (ALL, R.EPI_BF16, False, None),
    "bf16_half": (ALL, R.EPI_BF16, False, None),
    "drop_k32": (ALL, R.EPI_BF16, True, False),
    "dup_k32": (ALL, R.EPI_BF16, True, False),
    "transposed_frag": (ALL, R.EPI_BF16, True, False),
    "swapped_tiles": (ALL, R.EPI_BF16, True, None),
    "acc_twice": (ALL, R.EPI_BF16_ACC, True, None),
    "res_wrong_row": (ALL, R.EPI_BF16_RES, True, None),
    "skip_tile": (ALL, R.EPI_BF16, True, None),
}
TILE = (64, 64)


def _case(family, M, N, K):
    a, b = R.make_case(family, M, N, K)
    return a, b, R.ref_product(a, b)


def _passes(family, epilogue, fault, a, b, prod):
    """True when the (faulty) emulator's output passes the family's check."""
    M, N = a.shape[0], b.shape[1]
    old = R.make_old(family, M, N, R.sink_dtype(epilogue))
    got = R.emu_gemm(a, b, epilogue, old=old, residual=old, fault=fault, tile=TILE)
    try:
        R.check_case(family, got, a, b, epilogue, old=old, residual=old, prod=prod, tile=TILE)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("K", [64, 256, 2048])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_clean_emulator_passes_every_check(family, K):
    M, N = 128, 192
    a, b, prod = _case(family, M, N, K)
    for e in R.EPILOGUES:
        old = R.make_old(family, M, N, R.sink_dtype(e))
        got = R.emu_gemm(a, b, e, old=old, residual=old)
        R.check_case(family, got, a, b, e, old=old, residual=old, prod=prod, tile=TILE)   # bit-exact on EXACT
        t, _ = R.target_and_bound(*prod, K, e, old, old)
        assert R.norm_rel(got, t) < 1e-2


@pytest.mark.parametrize("fault", R.FAULTS)
def test_injected_fault_is_rejected(fault):
    assert set(FAULT_TABLE) == set(R.FAULTS)
    families, epi, old_catches, old_catches_big = FAULT_TABLE[fault]
    epis = R.EPILOGUES if fault not in ("acc_twice", "res_wrong_row") else (epi,)
    for family in R.FAMILIES:
        a, b, prod = _case(family, 128, 192, 256)
        for e in epis:
            assert _passes(family, e, None, a, b, prod), f"the clean emulator must pass on {family} e{e}"
        rejected = any(not _passes(family, e, fault, a, b, prod) for e in epis)
        assert rejected == (family in families), f"{fault} on {family}: rejected {rejected}"
    # the older global metric on the benign family
    M = N = 512
    a, b, (acc, _) = _case("randn", M, N, 256)
    old = R.make_old("randn", M, N, R.sink_dtype(epi))
    ref = acc if epi == R.EPI_BF16 else old.double() + acc
    got = R.emu_gemm(a, b, epi, old=old, residual=old, fault=fault, tile=TILE)
    rel = R.norm_rel(got, ref)
    print(f"fault {fault}: old metric on randn 512x512x256 {rel:.4g}")
    assert (rel < 1e-2) == (not old_catches)          # NaN compares False: caught
    if old_catches_big is not None:
        # 4096 x 2048: 32 slices of 512 x 512, 31 of them clean (the clean emulator's error and the
        # reference's norm on this slice stand for theirs), one holding the faulty fragment
        clean = R.emu_gemm(a, b, epi, old=old, residual=old, tile=TILE)
        e_clean = float((clean.double() - ref).pow(2).sum())
        e_fault = float((got.double() - ref).pow(2).sum())
        rel_big = math.sqrt((31 * e_clean + e_fault) / (32 * float(ref.pow(2).sum())))
        print(f"fault {fault}: old metric extrapolated to 4096x2048 {rel_big:.4g}")
        assert (rel_big < 1e-2) == (not old_catches_big)


def test_old_metric_misses_the_rounding_and_single_fragment_faults():
    """What the issue set out to show: truncation, half-away, a bf16 partial and every single-fragment
    fault pass rel_err < 1e-2 (the fragment faults at the layer's 4096 x 2048)."""
    for f in ("trunc_store", "half_away", "bf16_ktile", "bf16_half"):
        assert FAULT_TABLE[f][2] is False
    for f in ("drop_k32", "dup_k32", "transposed_frag"):
        assert FAULT_TABLE[f][3] is False
    assert all(len(v[0]) >= 1 for v in FAULT_TABLE.values())


def test_checker_rejects_non_finite_and_reports_the_element():
    ref = torch.ones(40, 70, dtype=torch.float64)
    got = ref.clone()
    got[33, 69] = float("nan")
    with pytest.raises(AssertionError, match=r"non-finite.*row 33 col 69 tile \(1, 1\) fragment \(0, 0\)"):
        R.check("x", got, ref, torch.ones_like(ref), tile=(32, 64))
    got[33, 69] = 3.0
    with pytest.raises(AssertionError, match=r"worst at row 33 col 69 tile \(1, 1\)"):
        R.check("x", got, ref, torch.ones_like(ref), tile=(32, 64))
    with pytest.raises(AssertionError):      # any error against a zero bound
        R.check("x", ref + 1e-9, ref, torch.zeros_like(ref))
    assert R.check("x", ref, ref, torch.zeros_like(ref)) == 0.0
    w = torch.ones(40, 70, dtype=R.BF)
    g = w.clone()
    g[17, 5] = 1.0078125       # one bf16 ulp
    with pytest.raises(AssertionError, match=r"1 of 2800 elements differ by bits; first at row 17 col 5 tile \(0, 0\) "
                                             r"fragment \(1, 0\)"):
        R.check_exact("x", g, w, tile=(32, 64))
    with pytest.raises(AssertionError):      # the dtype is part of the result
        R.check_exact("x", w.float(), w)
    neg0 = torch.zeros(2, 2, dtype=R.BF)
    with pytest.raises(AssertionError):      # -0 and +0 differ by bits
        R.check_exact("x", -neg0, neg0)


def test_padded_and_operands():
    a, b = R.make_case("ints", 64, 128, 64)
    A, B = R.operands(a, b, False, True)
    assert A.shape == (64, 64) and B.shape == (128, 64) and torch.equal(A, a.t()) and torch.equal(B.t(), b)
    full, region = R.padded(B)
    assert full.shape == (130, 72) and full.stride(0) % 8 == 0 and torch.equal(full[region], B)
    gap = full.clone()
    gap[region] = float("nan")
    assert bool(torch.isnan(gap.float()).all())
    assert int(full.view(torch.int16)[0, 0]) == R.NAN16
    f32, _ = R.padded(torch.zeros(4, 8))
    assert int(f32.view(torch.int32)[0, 0]) == R.NAN32


def test_ints_partial_sums_stay_below_2_24():
    a, b = R.make_case("ints", 64, 64, 8192)
    _, S = R.ref_product(a, b)         # sum |a||b| bounds every partial sum in every order
    assert float(S.max()) < 2 ** 24 and 8192 * 225 < 2 ** 24
    a, b = R.make_case("ints_scaled", 64, 64, 2048)
    rs, cs = R._scales(64, 64)
    _, S = R.ref_product(a, b)
    assert float((S / (rs * cs)).max()) < 2 ** 24          # integers on the element's own scale
    # and the emulator, any order, is therefore exact
    assert torch.equal(R.emu_gemm(a, b, R.EPI_F32).double(), R.ref_product(a, b)[0])


def test_ints_k64_exercises_bf16_rounding_and_ties():
    a, b = R.make_case("ints", 128, 192, 64)       # the pinned (default) seed
    acc, _ = R.ref_product(a, b)
    mag = acc.abs()
    assert float((mag > 256).double().mean()) >= 0.10
    ties = (mag >= 256) & (mag < 512) & (mag % 2 == 1)     # odd integers where bf16's spacing is 2
    assert int(ties.sum()) >= 1
    down = R._rne(acc.float()[ties]).double().abs() < mag[ties]
    assert bool(down.any()) and bool((~down).any())        # ties to even go both ways


def test_cancel_cancels():
    for K in (64, 320, 2048):
        a, b = R.make_case("cancel", 128, 192, K)
        acc, S = R.ref_product(a, b)
        assert float((S / acc.abs()).median()) >= 2 ** 8
        assert float((acc != 0).double().mean()) > 0.99
        h = K // 2
        half, _ = R.ref_product(a[:, :h], b[:h])
        assert float((half / S).min()) > 0.4                # the partial at K/2 is of the order of sum |a||b|


def test_poison_places_one_nan():
    a, b = R.make_case("randn", 64, 64, 64)
    pa, pb = R.poison(a, b, "a", 3, 5)
    assert int(torch.isnan(pa.float()).sum()) == 1 and bool(torch.isnan(pa[3, 5])) and torch.equal(pb, b)
    pa, pb = R.poison(a, b, "b", 7, 9)
    assert int(torch.isnan(pb.float()).sum()) == 1 and bool(torch.isnan(pb[7, 9])) and torch.equal(pa, a)
