"""tests/_sr_ref.py tested on itself, without a GPU: Philox4x32-10's known answers, the layout of the bits,
sr_bf16's probabilities and special values, the checker against the emulator's injected faults, and what
stochastic rounding is for -- a drift the plain bf16 step loses and the rounded one keeps in expectation."""
import math

import numpy as np
import pytest
import torch

from tests import _optim_ref as O
from tests import _sr_ref as SR

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SEED = 0x123456789ABCDEF0


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


@pytest.mark.parametrize("ctr, key, out", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
    ((5, 0, 3, 9), (0x9ABCDEF0, 0x12345678), "e8561bc6 a4b5d744 d06a8905 b7bcc794")])
def test_philox_known_answers(ctr, key, out):
    assert _hex(SR.philox4x32_10(ctr, key)) == out


def test_layout_of_the_bits():
    """seed 0x123456789abcdef0, stream 2, which 1, step 3: elements 40..47 are chunk 5, counter (5, 0, 3, 9)."""
    r = SR.sr_bits(SEED, 2, 3, SR.EXP_AVG, 48)
    assert [f"{int(x):04x}" for x in r[40:48]] == ["1bc6", "e856", "d744", "a4b5", "8905", "d06a", "c794", "b7bc"]
    # a pure function of the element index: a shorter tensor sees the same leading bits, ragged or not
    assert np.array_equal(SR.sr_bits(SEED, 2, 3, SR.EXP_AVG, 43), r[:43])
    # chunk indices above 2^32 reach the counter's second word
    hi = SR._bits(SEED, 2, 3, 1, [(1 << 32) + 5], 8)
    w = SR.philox4x32_10((5, 1, 3, 9), (SEED & SR.MASK, SEED >> 32))
    assert int(hi[0]) == int(w[0]) & 0xFFFF and int(hi[7]) == int(w[3]) >> 16
    # every coordinate matters
    for other in (SR.sr_bits(SEED + 1, 2, 3, 1, 48), SR.sr_bits(SEED ^ (1 << 40), 2, 3, 1, 48), SR.sr_bits(SEED, 3, 3, 1, 48),
                  SR.sr_bits(SEED, 2, 4, 1, 48), SR.sr_bits(SEED, 2, 3, 2, 48)):
        assert not np.array_equal(other, r)


def _f32_of_bits(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.int32).copy()).view(F32)


@pytest.mark.parametrize("low16", [0, 1, 0x7FFF, 0x8000, 0xFFFF])
@pytest.mark.parametrize("high", [0x3F80, 0xBF80, 0x0001, 0x7F00])
def test_rounds_up_for_exactly_low16_draws(low16, high):
    """over all 65536 r the magnitude goes up low16 times (either sign, a denormal, a large value)"""
    u = (high << 16) | low16
    x = _f32_of_bits(np.full(65536, u, dtype=np.uint32))
    out = SR.ibits(SR.sr_round(x, np.arange(65536))).numpy().astype(np.int64) & 0xFFFF
    assert int((out == high + 1).sum()) == low16 and int((out == high).sum()) == 65536 - low16


def test_special_values():
    every = np.arange(65536)

    def rounded(u):
        return SR.sr_round(_f32_of_bits(np.full(65536, u, dtype=np.uint32)), every)
    for u, want in ((0x7F800000, 0x7F80), (0xFF800000, 0xFF80), (0x00000000, 0x0000), (0x80000000, 0x8000)):
        assert bool(((SR.ibits(rounded(u)).numpy().astype(np.int64) & 0xFFFF) == want).all()), hex(u)
    for u in (0x7F800001, 0xFFFFFFFF, 0x7FC00000, 0xFFC00001):   # the integer path would give inf or zero for the first two
        assert bool(torch.isnan(rounded(u)).all()), hex(u)
    with_fault = SR.sr_round(_f32_of_bits(np.full(65536, 0x7F800001, dtype=np.uint32)), every, "nan_integer")
    assert int(torch.isinf(with_fault).sum()) == 65535   # all but r = 0xffff
    # an f32 denormal below bf16's smallest: up to 2^-133 with probability low16 / 65536, else +0
    out = SR.ibits(rounded(0x00004000)).numpy().astype(np.int64) & 0xFFFF
    assert int((out == 1).sum()) == 0x4000 and int((out == 0).sum()) == 65536 - 0x4000
    # the largest finite f32 sits in the last bf16 ulp below inf: it may become inf, and does for low16 draws
    out = SR.ibits(rounded(0x7F7FFFFF)).numpy().astype(np.int64) & 0xFFFF
    assert int((out == 0x7F80).sum()) == 0xFFFF and int((out == 0x7F7F).sum()) == 1
    # a bf16 value never changes
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0)).to(BF)
    assert O.same_bits(SR.sr_round(x.to(F32), SR.sr_bits(1, 0, 1, 0, 4096)), x)


# ------------------------------------------------------------------------------ the checker
L_TEST = [0, 17, 8, 1001, 5, 2048, 0, 9]
STREAMS = [3, 0, 7, 1, 12, 5, 2, 9]


def _state(family, gdt, seed=0):
    s = O.EXACT_S if family == "exact" else O.scalars(3)
    data = O.make_list(family, L_TEST, seed, s, BF, gdt)
    return [O.ListBuf(L_TEST, ts[0].dtype).fill(ts) for ts in data], s


@pytest.mark.parametrize("gdt", [BF, F32], ids=["gbf16", "gf32"])
@pytest.mark.parametrize("coef", [None, 0.3])
def test_checker_accepts_the_clean_emulator(gdt, coef):
    for family in ("randn", "fresh", "tiny", "overflow", "nan_grad"):
        bufs, s = _state(family, gdt)
        before = [b.clone() for b in bufs]
        SR.emu_sr_list_step(*bufs, STREAMS, s, SEED, 3, coef)
        assert O.same_bits(bufs[1].flat, before[1].flat)
        SR.check_sr_list(f"emu {family}", (bufs[0], bufs[2], bufs[3]), before, STREAMS, s, SEED, 3, coef)


def test_exact_family_is_the_plain_cast():
    """every f32 result is a bf16 value: stochastic rounding changes nothing"""
    bufs, s = _state("exact", BF)
    before = [b.clone() for b in bufs]
    SR.emu_sr_list_step(*bufs, STREAMS, s, SEED, 3)
    want = O.emu_elem(*(b.cat() for b in before), s, True)
    for got, w in zip((bufs[0], bufs[2], bufs[3]), want):
        assert O.same_bits(got.cat(), w.to(BF))


@pytest.mark.parametrize("fault", [f for f in SR.FAULTS if f != "nan_integer"])
def test_checker_rejects_step_faults(fault):
    bufs, s = _state("randn", BF)
    before = [b.clone() for b in bufs]
    coef = 0.3 if fault == "clip_rounded" else None
    SR.emu_sr_list_step(*bufs, STREAMS, s, SEED, 3, coef, fault)
    with pytest.raises(AssertionError):
        SR.check_sr_list(fault, (bufs[0], bufs[2], bufs[3]), before, STREAMS, s, SEED, 3, coef)


def test_checker_rejects_a_write_into_a_gap_and_a_wrong_class():
    bufs, s = _state("randn", BF)
    before = [b.clone() for b in bufs]
    SR.emu_sr_list_step(*bufs, STREAMS, s, SEED, 3)
    keep = bufs[2].flat.clone()
    bufs[2].flat[bufs[2].off[1] + 17] = 0.0   # one element past tensor 1
    with pytest.raises(AssertionError, match="outside"):
        SR.check_sr_list("gap", (bufs[0], bufs[2], bufs[3]), before, STREAMS, s, SEED, 3)
    bufs[2].flat.copy_(keep)
    bufs[0].views()[3][5] = math.nan
    with pytest.raises(AssertionError, match="class"):
        SR.check_sr_list("class", (bufs[0], bufs[2], bufs[3]), before, STREAMS, s, SEED, 3)


def test_cast_checker_rejects_nan_through_the_integer_path():
    x = _f32_of_bits(np.array([0x3F800001, 0x7F800001, 0xFFFFFFFF, 0x7F800000, 0x80000000], dtype=np.uint32))
    r = np.array([0xFFFF, 0x0001, 0x0001, 0x1234, 0xFFFF])
    SR.check_sr_cast("clean", SR.sr_round(x, r), x, r)
    with pytest.raises(AssertionError):
        SR.check_sr_cast("nan_integer", SR.sr_round(x, r, "nan_integer"), x, r)
    with pytest.raises(AssertionError):
        SR.check_sr_cast("nearest", SR.sr_round(x, r, "nearest"), x, r)


# ------------------------------------------------------------------------------ what it is for
def test_drift_survives_in_expectation():
    """4096 weights at 1, a constant gradient, lr = 2^-12, no decay, 256 steps.  Every update is 1/16 of the
    bf16 ulp below 1 (2^-8): the plain bf16 step rounds each one away and p stays 1; the f32 master moves by
    256 lr; the stochastically rounded weights' mean follows the master.

    sigma, from the per-step Bernoulli variance: a weight on the 2^-8 grid takes a decrement d_t (the
    master's own: the rounded moments are unbiased and move d_t by parts in 2^8 of itself), is stored one ulp
    lower with probability q_t = d_t / ulp and where it was otherwise: variance ulp^2 q_t (1 - q_t) per step,
    independent over steps and over elements (every element has its own 16 bits).  The mean of n elements
    after the steps has variance sum_t ulp^2 q_t (1 - q_t) / n."""
    n, steps, lr, ulp = 4096, 256, 2.0 ** -12, 2.0 ** -8
    g = torch.full((n,), 0.25, dtype=BF)
    plain = [torch.ones(n, dtype=BF), torch.zeros(n, dtype=BF), torch.zeros(n, dtype=BF)]
    master = [torch.ones(n, dtype=F32), torch.zeros(n, dtype=F32), torch.zeros(n, dtype=F32)]
    sr = [t.clone() for t in plain]
    var = 0.0
    for t in range(1, steps + 1):
        s = O.scalars(t=t, lr=lr, wd=0.0)
        plain = [x.to(BF) for x in O.emu_elem(plain[0], g, plain[1], plain[2], s, bf=True)]
        new = O.master_expect(master[0], g.to(F32), master[1], master[2], s)
        q = float(master[0][0] - new[0][0]) / ulp
        assert 0.0 < q < 0.5
        var += ulp * ulp * q * (1.0 - q) / n
        master = list(new)
        sr = list(SR.expect_step(sr[0], g, sr[1], sr[2], s, SR_SEED, 4, t)[0])
    assert bool((plain[0] == 1.0).all()), "round to nearest was expected to lose every update"
    moved = 1.0 - float(master[0][0])
    assert abs(moved - steps * lr) < 0.01 * steps * lr
    mean, sigma = float(sr[0].to(F64).mean()), math.sqrt(var)
    print(f"master {float(master[0][0]):.6f} sr mean {mean:.6f} sigma {sigma:.2e} deviation {abs(mean - float(master[0][0])) / sigma:.2f} sigma")
    assert abs(mean - float(master[0][0])) <= 6.0 * sigma
    assert sr[1].dtype == sr[2].dtype == BF


SR_SEED = 20261021
