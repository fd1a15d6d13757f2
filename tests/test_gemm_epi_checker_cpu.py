"""The fused-epilogue conformance kit (tests/_gemm_epi_ref.py) tested on itself, without a GPU.

  * the clean fp32 emulators pass every check that tests/test_gemm_epilogue_conformance_gpu.py applies,
    on the same inputs and shapes; where the check is sequenced (SwiGLU) their share of bit differences
    from the float64-sequenced expectation is below 1e-4, far under R.BIT_CAP: the reference alone
    stays within the cap;
  * every construction asserts its own exactness, and the figures the kit's docstring quotes hold;
  * every injected fault is rejected.  REJECTED_BY (asserted: exactly these cases of the GPU module
    reject the fault, K = 64; `*` = every case of the section that the fault can touch):

    fault                      rejected by
    f_on_unrounded_acc         SwiGLU forward: h beyond one rounding flip, ints_unit (all_g's accumulators
                               are bf16 numbers already: it passes there); backward: dg / du, ints_unit
                               (all_g: dh = 205 / 256 ... is a bf16 number); RoPE: bits, every rotated case
    up_from_gate_columns       forward: g|u by bits *; backward: du / dg bound *
    gu_ld_as_width             backward *: the gap's sentinel reaches dg|du (non-finite)
    rope_pos_tile_local        bits where seq_len exceeds the 128-row wave tile (seq_len 512, 256)
    rope_partner_16            bits, every case with rot_cols > 0
    rope_ignores_rot_cols      bits, every case with rot_cols < N
    rope_boundary_block_tile   bits, rot_cols = 192 only (the wave-tile edge inside a block tile)
    stats_of_unrounded         max by bits (ints_unit, offset, offset_low) or sumexp (flat): *
    stats_row_major            max by bits wherever there is more than one block
    stats_drops_a_wave         sumexp: ints_unit, flat, offset_low; missed on `offset` where the dropped
                               quarter weighs e^-80 -- unless it is the raised one (block 128)
    stats_max_of_first_wave    max by bits: * but flat (every wave's maximum is equal there)
"""
import pytest
import torch

from tests import _gemm_epi_ref as X
from tests import _gemm_ref as G
from tests import _row_ref as R

F32, F64 = torch.float32, torch.float64


@pytest.fixture(autouse=True)
def _leave_the_worst_tables_alone():
    """The injected faults' ratios must not reach the tables the GPU modules print from R.WORST / G.WORST."""
    saved = dict(R.WORST), dict(G.WORST)
    yield
    for d, s in zip((R.WORST, G.WORST), saved):
        d.clear()
        d.update(s)


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------ one function per section and case
FWD = {f"fwd-{M}x{I}x{K}": ("ints_unit", M, I, K) for M, I, K in X.SWIGLU_FWD_SHAPES}
FWD["fwd-all_g"] = ("all_g",) + X.ALL_G_SHAPE
BWD = {f"bwd-{M}x{I}x{H}": ("ints_unit", M, I, H) for M, I, H in X.SWIGLU_BWD_SHAPES + (X.SWIGLU_DUAL_SHAPE,)}
BWD["bwd-all_g"] = ("all_g",) + X.ALL_G_SHAPE
ROPE = {f"rope-{M}x{N}-r{rot}-s{seq}-{fam}": (fam, M, N, 64, rot, seq) for M, N, rot, seq in X.ROPE_SHAPES
        for fam in X.FAMILIES}
CE = {f"ce-{M}x{N}-b{blk}-{fam}": (fam, M, N, 64, blk) for M, N, blk in X.CE_SHAPES for fam in X.CE_FAMILIES}


def run_fwd(key, fault=None):
    _, _, acc32, exp = X.fwd_case(*FWD[key])
    h, gu = X.emu_swiglu_fwd(acc32, fault)
    return X.check_swiglu_fwd(key, h, gu, exp)


def run_bwd(key, fault=None):
    _, _, gu, acc32, exp = X.bwd_case(*BWD[key])
    full, region = G.padded(gu)
    return X.check_swiglu_bwd(key, X.emu_swiglu_bwd(acc32, full, region, fault), exp)


def run_rope(key, fault=None):
    fam, M, N, K, rot, seq = ROPE[key]
    _, _, cos, sin, acc32, want = X.rope_case(fam, M, N, K, rot, seq)
    return X.check_rope(key, X.emu_rope(acc32, cos, sin, seq, rot, fault), want)


def run_ce(key, fault=None):
    fam, M, N, K, blk = CE[key]
    _, _, acc32, x, exp = X.ce_case(fam, M, N, K, blk)
    logits, stats = X.emu_ce_stats(acc32, blk, fault)
    G.check_exact(f"{key} logits", logits, x)
    return X.check_stats(key, stats, exp)


SECTIONS = ((FWD, run_fwd, ("f_on_unrounded_acc", "up_from_gate_columns")),
            (BWD, run_bwd, X.SWIGLU_EPI_FAULTS),
            (ROPE, run_rope, ("f_on_unrounded_acc",) + X.ROPE_EPI_FAULTS),
            (CE, run_ce, X.STATS_FAULTS))


def rejecting(fault):
    """The cases (of every section the fault applies to) whose check rejects the fault."""
    return {k for cases, run, faults in SECTIONS if fault in faults for k in cases if _rejected(lambda: run(k, fault))}


def _keys(cases, pred=lambda *c: True):
    return {k for k, c in cases.items() if pred(*c)}


REJECTED_BY = {
    "f_on_unrounded_acc": _keys(FWD, lambda fam, *_: fam != "all_g") | _keys(BWD, lambda fam, *_: fam != "all_g")
                          | _keys(ROPE, lambda fam, M, N, K, rot, seq: rot > 0),
    "up_from_gate_columns": _keys(FWD) | _keys(BWD),
    "gu_ld_as_width": _keys(BWD),
    "rope_pos_tile_local": _keys(ROPE, lambda fam, M, N, K, rot, seq: rot > 0 and seq > 128),
    "rope_partner_16": _keys(ROPE, lambda fam, M, N, K, rot, seq: rot > 0),
    "rope_ignores_rot_cols": _keys(ROPE, lambda fam, M, N, K, rot, seq: rot < N),
    "rope_boundary_block_tile": _keys(ROPE, lambda fam, M, N, K, rot, seq: rot % 128 != 0),
    "stats_of_unrounded": _keys(CE),
    "stats_row_major": _keys(CE, lambda fam, M, N, K, blk: N > blk),
    "stats_drops_a_wave": _keys(CE, lambda fam, M, N, K, blk: fam != "offset" or blk == 128),
    "stats_max_of_first_wave": _keys(CE, lambda fam, M, N, K, blk: fam != "flat"),
}


# ------------------------------------------------------------------------------ the clean emulators
@pytest.mark.parametrize("key", list(FWD))
def test_clean_swiglu_forward_passes(key):
    assert run_fwd(key) < 1e-4


@pytest.mark.parametrize("key", list(BWD))
def test_clean_swiglu_backward_passes(key):
    assert run_bwd(key) < 1e-4


@pytest.mark.parametrize("K", X.ROPE_KS)
def test_clean_rope_is_exact(K):
    for fam, M, N, _, rot, seq in ROPE.values():
        _, _, cos, sin, acc32, want = X.rope_case(fam, M, N, K, rot, seq)
        X.check_rope(f"rope {fam} {M}x{N} K{K}", X.emu_rope(acc32, cos, sin, seq, rot), want)


@pytest.mark.parametrize("K", X.CE_KS)
def test_clean_ce_statistics_pass(K):
    for fam, M, N, _, blk in CE.values():
        _, _, acc32, x, exp = X.ce_case(fam, M, N, K, blk)
        logits, stats = X.emu_ce_stats(acc32, blk)
        G.check_exact("logits", logits, x)
        assert X.check_stats(f"ce {fam} {M}x{N} K{K}", stats, exp) <= 1.0


# ------------------------------------------------------------------------------ the faults
@pytest.mark.parametrize("fault", X.FAULTS)
def test_fault_is_rejected(fault):
    assert set(REJECTED_BY) == set(X.FAULTS) == {f for _, _, faults in SECTIONS for f in faults}
    got = rejecting(fault)
    assert got, f"{fault}: no case rejects it"
    assert got == REJECTED_BY[fault], f"{fault}: also {sorted(got - REJECTED_BY[fault])}, not {sorted(REJECTED_BY[fault] - got)}"


# ------------------------------------------------------------------------------ the constructions and the quoted figures
def test_ints_unit_is_exact_and_unsaturated():
    a, b = X.make_case("ints_unit", 256, 256, 64)
    acc = X.product(a, b)
    g = X.bf(acc).to(F64).abs()
    med, below8 = float(g.median()), float((g < 8).double().mean())
    ties = float((X.bf(acc).to(F64) != acc).double().mean())       # not bf16 numbers: they round
    half = (acc - X.bf(acc).to(F64)).abs() == (R.bf_nbr(X.bf(acc).to(F64), 1) - X.bf(acc).to(F64)).abs() / 2
    print(f"ints_unit K 64: median |bf16(acc)| {med:.2f}, below 8 {below8:.3f}, rounded {ties:.3f}, ties {float(half.double().mean()):.3f}")
    assert 3.0 < med < 4.0 and 0.85 < below8 < 0.93
    assert ties > 0.4 and float(half.double().mean()) > 0.2      # the bf16 rounding, and its ties, are exercised
    for K in (64, 192, 512):
        for fam in X.FAMILIES:
            aa, bb = X.make_case(fam, 128, 128, K)
            x = X.bf(X.product(aa, bb))
            cos, sin = X.rope_tables(64)
            X.assert_rope_exact(x, cos, sin, 64, 128)


def test_all_g_constructions():
    a, b = X.make_all_g_fwd()          # asserts the gate patterns and the per-block u itself
    gu = X.bf(X.product(a, b))
    pats = set((R.ibits(gu[:256, :256]).to(torch.int32) & 0xFFFF).flatten().tolist())
    normal = {p for p in range(65536) if (p & 0x7F80) not in (0, 0x7F80)}
    assert normal <= pats and pats - normal == {0}
    for blk, val in enumerate(R.ALL_G_VALUES):
        assert bool((gu[256 * blk:256 * (blk + 1), 256:].to(F64) == val).all())
    dy, w, res = X.make_all_g_bwd()    # asserts dh by bits
    assert res.shape == (768, 512)


def test_ce_constructions():
    for M, N, blk in X.CE_SHAPES:
        _, _, _, x, exp = X.ce_case("flat", M, N, 64, blk)
        v = x.to(F64).reshape(M, N // blk, blk)
        assert bool((v == v[..., :1]).all())
        assert bool((exp["sumexp"] == float(blk)).all()), "flat: sumexp == block exactly"
        _, _, _, x, _ = X.ce_case("offset", M, N, 64, blk)
        mw = x.to(F64).reshape(M, N // blk, blk // 64, 64).amax(3)
        top = mw.argmax(2)
        want = 1 + torch.arange(N // blk) % (blk // 64 - 1)
        assert bool((top == want[None, :]).all()) and bool((top != 0).all())
        rest = torch.where(torch.arange(blk // 64)[None, None, :] == top[..., None], -1e9, mw).amax(2)
        assert bool((mw.amax(2) - rest > 40).all())                 # e^-40 and below beside the raised quarter
        _, _, _, x, _ = X.ce_case("offset_low", M, N, 64, blk)
        assert bool((x.to(F64) < -60).all())


def test_checks_name_what_is_wrong():
    """A statistic left as the sentinel, and a logit one ulp off, are each rejected by name."""
    key = "ce-256x256-b256-ints_unit"
    fam, M, N, K, blk = CE[key]
    _, _, acc32, x, exp = X.ce_case(fam, M, N, K, blk)
    _, stats = X.emu_ce_stats(acc32, blk)
    bad = stats.clone()
    bad.view(torch.int32)[2 * 77 + 1] = R.NAN32
    with pytest.raises(AssertionError, match="not written"):
        X.check_stats(key, bad, exp)
    bad = stats.clone()
    bad[2 * 77 + 1] *= 1 + 2.0 ** -12
    with pytest.raises(AssertionError, match="over the bound"):
        X.check_stats(key, bad, exp)
