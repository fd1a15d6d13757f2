"""The optimizer / embedding conformance kit (tests/_optim_ref.py) tested on itself, without a GPU.

  * the geometry helper reproduces the (257, 512) that tests/test_grad_clip_gpu.py and
    tests/test_master_weights_gpu.py assert for their six shapes, at both caps;
  * the faithful float32 emulator of the list kernel's walk passes the sequenced check on every
    family, clipped and unclipped, with a bit-mismatch share below 1e-3 (the cap is 5e-3);
  * every injected fault is rejected on at least one family (FAULT_TABLE, asserted);
  * the `exact` family's expectation is exact: float64 and float32 evaluation agree with p - s, m, v;
  * the f32-state bound and the master path's expected bits accept a faithful float32 evaluation and
    reject a wrong one;
  * the embedding emulator's four faults change the bits of a case built to show them.
"""
import math

import pytest
import torch

from tests import _optim_ref as O
from tests import _row_ref as R

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
MID = [2048, 1001, 512 * 2048, 37, 105, 8]
# 984 chunks walked as 3 runs of 330: run 1 starts 199 chunks into the 4099-element tensor and holds 314 of
# its chunks (58 threads make a second trip), then three more tensors; empty tensors inside and at the end
LENS = [1001, 37, 0, 4099, 105, 8, 2600, 0]
GRID = (3, 330)
SC = O.scalars(t=3)

# fault -> the families that must reject it
FAULT_TABLE = {
    "drop_rounding": ("randn",),
    "eps_before_div": ("tiny",),
    "v_swapped": ("exact",),
    "step_on_m": ("cancel",),
    "stale_pipeline": ("exact", "randn"),
    "tail_one_too_far": ("exact", "randn"),
    "tail_skipped": ("exact", "randn"),
    "neighbour_moments": ("exact", "randn"),
    "coef_after_rounding": ("randn",),
}


@pytest.fixture(autouse=True)
def _leave_the_worst_table_alone():
    saved = dict(O.WORST)
    yield
    O.WORST.clear()
    O.WORST.update(saved)


def _bufs(family, sc, lengths=LENS, seed=0):
    return [O.ListBuf(lengths, BF).fill(ts) for ts in O.make_list(family, lengths, seed, sc)]


def _run(family, clip, fault=None):
    sc = O.EXACT_S if family == "exact" else SC
    P, G, M, V = _bufs(family, sc)
    before = [b.clone() for b in (P, G, M, V)]
    coef = None
    if clip:
        sq = float(G.cat().double().pow(2).sum())
        coef = O.clip_coef(sq, (4 if family in O.COEF_ONE else 0.3) * math.sqrt(sq))
        if coef is None:
            return None
    O.emu_list_step(P, G, M, V, sc, coef, GRID, fault)
    assert O.same_bits(G.flat, before[1].flat)
    return O.check_list_bf16(f"{family}{' clip' if clip else ''}", (P, M, V), before, sc, coef)


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_geometry_helper():
    chunks = O.chunk_starts(MID)[-1]
    assert chunks == 131474
    assert O.multi_grid(chunks, O.STEP_CAP) == (257, 512) and O.multi_grid(chunks, O.NORM_CAP) == (257, 512)
    geo = O.geometry(MID)
    assert (geo["blocks"], geo["per_block"]) == (257, 512) and geo["seg_full"] == 512
    assert O.multi_grid(0) == (1, 0) and O.multi_grid(1) == (1, 1) and O.multi_grid(513) == (2, 257)
    assert O.multi_grid(1024 * 512 + 1) == (1024, 513) and O.multi_grid(1024 * 512 + 1, 2048) == (1025, 512)
    assert O.grid_for(0) == 1 and O.grid_for(257) == 2 and O.grid_for(10 ** 7) == 2048
    # the runs tile the chunks exactly once, in order, and skip the empty tensors
    seen = []
    for segs in O.runs(LENS, grid=GRID):
        for t, frm, to in segs:
            assert frm < to or LENS[t] == 0
            seen += [(t, c) for c in range(frm, to)]
    assert seen == [(t, c) for t, n in enumerate(LENS) for c in range((n + 7) // 8)]
    assert O.runs(LENS, grid=GRID)[1][0] == (3, 199, 513) and len(O.runs(LENS, grid=GRID)[1]) == 4
    # the norm bound at the six shapes is inside the suite's older inline derivation
    old = 8 * (2 + 6) + 7 * 6 + 2 + 6 + 3 + 2 + 6 + 3 + 1 + 2
    assert O.sq_adds(512, geo["run_tensors"], geo["ragged"], 257) <= old


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("family", O.FAMILIES)
def test_clean_emulator_passes(family, clip):
    res = _run(family, clip)
    if res is None:
        assert family in ("overflow", "nan_grad")   # sq is inf / NaN: a clipped step is skipped
        return
    worst, share = res
    assert worst <= 1.0 and share < 1e-3, (worst, share)


@pytest.mark.parametrize("fault", O.STEP_FAULTS)
def test_fault_rejected(fault):
    clip = fault == "coef_after_rounding"
    for family in FAULT_TABLE[fault]:
        assert _rejected(lambda: _run(family, clip, fault)), f"{fault} was not rejected on {family}"


def test_exact_family_is_exact():
    n = 5000
    p, g, m, v = O.make_state("exact", n, 1)
    s = (g.to(F64).sign())
    for rnd in (lambda k, x: x, lambda k, x: R._bf(x), lambda k, x: x.to(F32).to(F64)):
        p2, m1, v2, _ = O.sequence(p.to(F64), g.to(F64), m.to(F64), v.to(F64), O.EXACT_S, rnd)
        assert torch.equal(p2, p.to(F64) - s) and torch.equal(m1, m.to(F64)) and torch.equal(v2, v.to(F64))
    ep, em, ev = O.emu_elem(p, g, m, v, O.EXACT_S)
    assert torch.equal(ep.to(F64), p.to(F64) - s) and torch.equal(em.to(BF), m) and torch.equal(ev.to(BF), v)
    w2, m2, v2 = O.master_expect(p.to(F32), g.to(F32), m.to(F32), v.to(F32), O.EXACT_S)
    assert torch.equal(w2.to(F64), p.to(F64) - s) and torch.equal(m2, m.to(F32)) and torch.equal(v2, v.to(F32))
    assert int(p.to(F64).abs().max()) <= 125 and len(set(p.tolist())) == 251


@pytest.mark.parametrize("family", O.FAMILIES)
def test_f32_state_and_master(family):
    sc = O.EXACT_S if family == "exact" else SC
    n = 4099
    p, g, m, v = O.make_state(family, n, 2, sc, F32)
    ep, em, ev = O.emu_elem(p, g, m, v, sc, bf=False)
    assert O.check_f32_step(family, (ep, em, ev), (p, g, m, v), sc) <= 1.0
    want = O.master_expect(p, g, m, v, sc)
    worst, share = O.check_master_step(family, (want[0], want[0].to(BF), want[1], want[2]), (p, g, m, v), sc)
    assert share == 0.0 and worst <= 1.0
    if family in ("randn", "cancel"):
        bad = O.emu_elem(p, g, m, v, sc, bf=False, fault="eps_before_div")
        assert _rejected(lambda: O.check_f32_step(family, bad, (p, g, m, v), sc))
        # the uncontracted evaluation is inside the bound, but its bits differ on too many elements
        assert _rejected(lambda: O.check_master_step(family, (ep, ep.to(BF), em, ev), (p, g, m, v), sc))
        assert _rejected(lambda: O.check_master_step(family, (want[0], O.nbr(want[0].to(BF), 1), want[1], want[2]),
                                                     (p, g, m, v), sc))


def test_clip_coefficient():
    assert O.clip_coef(math.inf, 1.0) is None and O.clip_coef(math.nan, 1.0) is None
    assert O.clip_coef(4.0, 8.0) == 1.0 and O.clip_coef(0.0, 1.0) == 1.0
    c = O.clip_coef(16.0, 1.0)
    assert c == float(torch.tensor(1.0) / (torch.tensor(16.0).sqrt() + torch.tensor(1e-6)))
    g = torch.tensor([0.1, -3.0, 1e-30], dtype=BF)
    assert torch.equal(O.clip_grad(g, c, True), (g.float() * torch.tensor(c)).to(BF))


# ------------------------------------------------------------------------------ embedding
def _emb_case(H=520, T=300, V=40, lo=8):
    gen = R._gen("emb", H, T, V)
    ids = torch.randint(lo - 2, lo + V + 2, (T,), generator=gen)
    dy = (torch.randn(T, H, generator=gen) * torch.pow(2.0, torch.randint(-12, 13, (T, 1), generator=gen))).to(BF)
    return ids, dy, lo, lo + V


@pytest.mark.parametrize("sink", [0, O.PT_DW_ACC_BF16, O.PT_DW_ACC_F32])
def test_embedding_emulator_against_float64(sink):
    """The documented order is within the f32 sum's error of a float64 sum; untouched rows keep their bits."""
    ids, dy, lo, hi = _emb_case()
    ids[ids == lo + 5] = lo + 6      # row 5 is touched by no token
    old = torch.randn(hi - lo, dy.shape[1], generator=R._gen("old", sink)).to(F32 if sink == O.PT_DW_ACC_F32 else BF)
    new = O.emu_embedding_bwd(ids, dy, old, sink, lo, hi, padding_idx=lo + 3)
    assert O.same_bits(new[5], old[5]) and O.same_bits(new[3], old[3])
    ref = torch.zeros(hi - lo, dy.shape[1], dtype=F64)
    for t in range(ids.numel()):
        if lo <= ids[t] < hi and ids[t] != lo + 3:
            ref[ids[t] - lo] += dy[t].to(F64)
    cnt = torch.bincount((ids - lo).clamp(0, hi - lo - 1), minlength=hi - lo).max().item()
    mass = torch.zeros_like(ref).index_add_(0, (ids - lo).clamp(0, hi - lo - 1), dy.to(F64).abs())
    touched = [r for r in range(hi - lo) if r not in (3, 5) and bool((ids == lo + r).any())]
    base = old.to(F64) if sink else torch.zeros_like(ref)
    tgt = base + ref
    bound = R.gamma(cnt) * mass + R.hu(ref) + (R.hu(tgt) if sink == O.PT_DW_ACC_BF16 else R.E * tgt.abs())
    assert bool(((new.to(F64) - tgt).abs() <= bound * 1.01)[touched].all())


@pytest.mark.parametrize("fault", O.EMB_FAULTS)
def test_embedding_fault_rejected(fault):
    ids, dy, lo, hi = _emb_case(H=1032 if fault == "columns_stop_at_512" else 264)
    if fault == "descending":   # X, -X, small in ascending position: (X - X) + s is s, (s - X) + X is not
        ids[:3] = lo + 1
        ids[3:][ids[3:] == lo + 1] = lo + 2
        dy[0] = (dy[0].float() * 2.0 ** 20).to(BF)
        dy[1] = -dy[0]
    sink = O.PT_DW_ACC_F32 if fault == "f32_sink_second_rounding" else 0
    old = torch.randn(hi - lo, dy.shape[1], generator=R._gen("old", 1)).to(F32 if sink else BF)
    good = O.emu_embedding_bwd(ids, dy, old, sink, lo, hi)
    bad = O.emu_embedding_bwd(ids, dy, old, sink, lo, hi, fault=fault)
    assert _rejected(lambda: R.check_exact("dw", bad, good))
    R.check_exact("dw", O.emu_embedding_bwd(ids, dy, old, sink, lo, hi), good)


def test_embedding_forward_emulator():
    ids, _, lo, hi = _emb_case()
    w = torch.randn(hi - lo, 264, generator=R._gen("w")).to(BF)
    out = O.emu_embedding_fwd(ids, w, lo, hi)
    for t in range(ids.numel()):
        want = w[ids[t] - lo] if lo <= ids[t] < hi else torch.zeros(264, dtype=BF)
        assert O.same_bits(out[t], want)
