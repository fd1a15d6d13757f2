"""The row-kernel conformance kit (tests/_row_ref.py) tested on itself, without a GPU.

  * the faithful fp32 emulators pass every check on every family; where the check is sequenced (norm
    forward, SwiGLU) their bit-mismatch share stays below 1e-4, fifty times under the 0.5 % cap;
  * every injected fault is rejected by the checker on at least one family;
  * what the suite's older assertion -- the matching rel_err limit of tests/test_kernels_gpu.py on the
    benign family -- makes of each fault.  FAULT_TABLE (asserted; the test prints the metric):

    fault                      rejected by                       old metric (limit)
    no_eps                     rstd, tiny                        missed  (y 5e-3)
    wrong_mode                 bits, every family                missed  (y 5e-3)
    neighbour_rstd             y, rowscale (and randn)           caught at cols 8192 (1.03e-2 > y's 5e-3); its
                                                                 backward twin is missed (dx 1e-2 at 16384:
                                                                 test_neighbour_rstd_backward_twin_...)
    ss_drops_last_chunk        rstd, spike                       missed  (y 5e-3)
    dot_without_w              dx                                missed  (dx 1e-2: 0.8e-2 with w = 1 + randn / 4)
    dres_dropped               dx                                caught  (dx 1e-2)
    dw_skips_last_row          dw                                caught  (dw 1e-2)
    dw_partial_bf16            dw, cancel (the mass bound)       missed  (dw 1e-2)
    acc_bf16_single_rounding   dw (PT_DW_ACC_BF16)               missed  (dw 1e-2)
    onehot_off_by_one          grad                              caught  (grad 1e-2)
    lse_skips_last_chunk       loss and grad, flat and randn3    missed  (grad 1e-2: 0.4e-2 at V 2048)
    ignored_row_nonzero        zero rows by bits                 missed  (grad 1e-2)
    row_scale_uses_row0        grad (scale_stride 1)             missed: the old test has one scale for all rows
    p_in_bf16                  grad                              missed  (grad 1e-2)
    neg_inf_chunk_nan          neg_inf (non-finite)              missed: randn has no -inf
    silu_unrounded             bits                              missed  (1e-2)
    dhu_unrounded              bits                              missed  (1e-2)
    sigmoid_negated            bound                             caught  (1e-2)
    pos_div_not_mod            bits                              caught on random tables
    halves_swapped             bits                              caught
    inverse_sign               bits                              caught
    table_second_half          bits                              missed on the real cos/sin table (halves equal)
"""
import math

import pytest
import torch

from tests import _row_ref as R

EPS = 1e-5


@pytest.fixture(autouse=True)
def _leave_the_worst_table_alone():
    """The injected faults' ratios must not reach the table tests/test_row_conformance_gpu.py prints
    (and bounds) from R.WORST when both files run in one process."""
    saved = dict(R.WORST)
    yield
    R.WORST.clear()
    R.WORST.update(saved)


ROWS, COLS = 48, 1032          # two registers per lane, a lone chunk in the second


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------ norm
def _norm_fwd_check(c, mode, res, fault=None):
    r = c["r"] if res else None
    y, z, rstd = R.emu_norm_fwd(c["x"], r, c["w"], EPS, mode, fault)
    ref = R.ref_norm_fwd(c["x"], r, c["w"], EPS, mode)
    if res:
        R.check_exact("z", z, ref["z"])
    R.check("rstd", rstd, ref["rstd"], ref["rstd_bound"])
    R.check("y", y, ref["y_ref"], ref["y_bound"])
    return R.check_bits("y", y, ref["y_want"], ref["y_alts"])


def _norm_bwd_check(c, mode, sink, fault=None):
    z = c["x"]
    rstd = R.emu_norm_fwd(z, None, c["w"], EPS, mode)[2]
    old = None if sink == 0 else torch.randn(z.shape[1], generator=R._gen("old", sink)).to(R.BF if sink == 4 else R.F32)
    dx, dw = R.emu_norm_bwd(c["dy"], z, c["w"], rstd, c["dres"], mode, sink, old, fault)
    ref = R.ref_norm_bwd(c["dy"], z, c["w"], rstd, c["dres"], mode)
    R.check("dx", dx, ref["dx_ref"], ref["dx_bound"])
    R.check_bits("dx", dx, ref["dx_want"], flip=ref["dx_flip"])
    t, b = R.dw_target_bound(ref["dw"], ref["dw_err"], sink, old)
    R.check("dw", dw, t, b)


@pytest.mark.parametrize("family", R.NORM_FAMILIES)
def test_faithful_norm_emulator_passes(family):
    c = R.make_norm_case(family, ROWS, COLS)
    for mode in (0, 1):
        for res in (False, True):
            assert _norm_fwd_check(c, mode, res) < 1e-4
        for sink in (0, R.PT_DW_ACC_BF16, R.PT_DW_ACC_F32):
            _norm_bwd_check(c, mode, sink)


def _old_norm_y(fault, cols=8192, rows=16):
    c = R.make_norm_case("randn", rows, cols)
    y = R.emu_norm_fwd(c["x"], None, c["w"], EPS, 0, fault)[0]
    return R.norm_rel(y, R.ref_norm_fwd(c["x"], None, c["w"], EPS, 0)["y_ref"])


def _old_norm_bwd(fault, what, sink=0):
    c = R.make_norm_case("randn", 64, 512)
    rstd = R.emu_norm_fwd(c["x"], None, c["w"], EPS, 0)[2]
    old = None if sink == 0 else torch.zeros(512, dtype=R.BF) + 3
    dx, dw = R.emu_norm_bwd(c["dy"], c["x"], c["w"], rstd, c["dres"], 0, sink, old, fault)
    ref = R.ref_norm_bwd(c["dy"], c["x"], c["w"], rstd, c["dres"], 0)
    if what == "dx":
        return R.norm_rel(dx, ref["dx_ref"])
    return R.norm_rel(dw, R.dw_target_bound(ref["dw"], ref["dw_err"], sink, old)[0])


# fault -> (families that must reject it, the old assertion's (metric, limit), caught by it)
NORM_TABLE = {
    "no_eps": (("tiny",), (lambda f: _old_norm_y(f), 5e-3), False),
    "wrong_mode": (R.NORM_FAMILIES, (lambda f: _old_norm_y(f), 5e-3), False),
    "neighbour_rstd": (("randn", "rowscale"), (lambda f: _old_norm_y(f), 5e-3), True),
    "ss_drops_last_chunk": (("spike",), (lambda f: _old_norm_y(f), 5e-3), False),
    "dot_without_w": (("randn",), (lambda f: _old_norm_bwd(f, "dx"), 1e-2), False),
    "dres_dropped": (("randn",), (lambda f: _old_norm_bwd(f, "dx"), 1e-2), True),
    "dw_skips_last_row": (("randn",), (lambda f: _old_norm_bwd(f, "dw"), 1e-2), True),
    "dw_partial_bf16": (("cancel",), (lambda f: _old_norm_bwd(f, "dw"), 1e-2), False),
    "acc_bf16_single_rounding": (("randn",), (lambda f: _old_norm_bwd(f, "dw", R.PT_DW_ACC_BF16), 1e-2), False),
}


@pytest.mark.parametrize("fault", R.NORM_FWD_FAULTS + R.NORM_BWD_FAULTS)
def test_norm_fault_is_rejected(fault):
    assert set(NORM_TABLE) == set(R.NORM_FWD_FAULTS + R.NORM_BWD_FAULTS)
    must, (metric, limit), caught = NORM_TABLE[fault]
    for family in must:
        c = R.make_norm_case(family, ROWS, COLS)
        if fault in R.NORM_FWD_FAULTS:
            assert any(_rejected(lambda: _norm_fwd_check(c, m, False, fault)) for m in (0, 1)), (fault, family)
        else:
            sinks = (R.PT_DW_ACC_BF16,) if fault == "acc_bf16_single_rounding" else (0,)
            assert any(_rejected(lambda: _norm_bwd_check(c, m, s, fault)) for m in (0, 1) for s in sinks), (fault, family)
    rel = metric(fault)
    print(f"fault {fault}: old metric {rel:.4g} (limit {limit})")
    assert (rel < limit) == (not caught)


def test_neighbour_rstd_backward_twin_is_missed_by_the_old_limit():
    """The backward reading a neighbouring row's rstd at cols 16384: dx moves by |rstd' / rstd - 1| ~
    1 / sqrt(cols) = 0.8 % in norm, under the 1e-2 limit; per element it is far outside the bound."""
    c = R.make_norm_case("randn", 8, 16384)
    rstd = R.emu_norm_fwd(c["x"], None, c["w"], EPS, 0)[2]
    dx, _ = R.emu_norm_bwd(c["dy"], c["x"], c["w"], rstd.roll(-1), None, 0)
    ref = R.ref_norm_bwd(c["dy"], c["x"], c["w"], rstd, None, 0)
    assert R.norm_rel(dx, ref["dx_ref"]) < 1e-2
    assert _rejected(lambda: R.check("dx", dx, ref["dx_ref"], ref["dx_bound"]))


def test_cancel_family_cancels_and_spike_sits_where_it_says():
    c = R.make_norm_case("cancel", ROWS, COLS)
    rstd = R.emu_norm_fwd(c["x"], None, c["w"], EPS, 0)[2]
    ref = R.ref_norm_bwd(c["dy"], c["x"], c["w"], rstd, None, 0)
    assert float((ref["mass"] / COLS / ref["dot"].abs()).median()) > 2 ** 6
    s = R.make_norm_case("spike", 4, COLS)["x"].double()
    assert int(s[0].abs().argmax()) // 8 == COLS // 8 - 1 and int(s[1].abs().argmax()) // 8 % 64 == 63
    rs = R.make_norm_case("rowscale", 23, 64)["x"].double().pow(2).mean(1)
    assert len({round(math.log2(float(v))) for v in rs}) >= 20


# ------------------------------------------------------------------------------ cross-entropy
V = 4104       # three chunk steps of a thread: 513 chunks


def _ce_check(family, fault=None, per_row_scale=True, style="sub", rows=14):
    x = R.make_ce_case(family, rows, V)
    tgt = R.make_targets(rows, V)
    if family == "peaked":   # the target on the peak in even rows, off it in odd ones
        rr = torch.arange(rows)
        tgt = torch.where((rr % 2 == 0) & (tgt != R.IGNORE), R.peak_col(rr, V), tgt)
    gs = (0.25 * (1 + torch.arange(rows) % 3)).to(R.F32) if per_row_scale else torch.full((rows,), 0.125)
    loss, grad = R.emu_ce(x, tgt, gs, fault=fault)
    f = R.ref_ce_fwd(x, tgt, style=style)
    R.check("loss", loss, f["loss"], f["loss_bound"])
    ref, bound = R.ref_ce_bwd(x, tgt, f["lse"], f["lse_bound"], gs.double(), style=style)
    R.check("grad", grad, ref, bound)
    ign = tgt == R.IGNORE
    R.check_exact("ignored rows", grad[ign], torch.zeros_like(grad[ign]))
    return x, tgt, grad, ref


@pytest.mark.parametrize("family", R.CE_FAMILIES)
def test_faithful_ce_emulator_passes(family):
    for style in ("sub", "fma"):
        _ce_check(family, style=style)


def test_ce_reference_bad_targets_and_neg_inf():
    x = R.make_ce_case("neg_inf", 8, V)
    ch = x.double().reshape(8, -1, 8)
    assert bool((ch[:, 0] == -math.inf).all()) and bool((ch[:, :256] == -math.inf).all(2).any(1).all())
    assert bool(torch.isfinite(x.double()).any(1).all())
    tgt = torch.tensor([-1, V, 2 ** 40, V - 1 - 3, R.IGNORE, V - 1, V - 2, V - 3])   # finite logits (r mod 5)
    f = R.ref_ce_fwd(x, tgt)
    assert f["bad"].tolist() == [True] * 3 + [False] * 5
    assert bool(torch.isnan(f["loss"][:3]).all()) and bool(torch.isfinite(f["loss"][3:]).all()) and float(f["loss"][4]) == 0
    loss, grad = R.emu_ce(x, tgt, torch.ones(8))
    R.check("loss", loss, f["loss"], f["loss_bound"])
    ref, bound = R.ref_ce_bwd(x, tgt, f["lse"], f["lse_bound"], torch.ones(8, dtype=R.F64))
    R.check("grad", grad, ref, bound)
    assert bool(torch.isnan(ref[:3]).all()) and bool(torch.isfinite(ref[3:]).all())
    finite = grad.clone()
    finite[0] = 0
    assert _rejected(lambda: R.check("grad", finite, ref, bound))      # a bad target's row must be NaN


def _old_ce(fault):
    x = R.make_ce_case("randn3", 16, 2048)
    tgt = torch.randint(0, 2048, (16,), generator=R._gen("oldce"))
    tgt[3] = R.IGNORE
    gs = torch.full((16,), 1.0 / 15)
    grad = R.emu_ce(x, tgt, gs, fault=fault)[1]
    f = R.ref_ce_fwd(x, tgt)
    return R.norm_rel(grad, R.ref_ce_bwd(x, tgt, f["lse"], f["lse_bound"], gs.double())[0])


# fault -> (families that must reject it, caught by rel_err(grad) < 1e-2 on randn with one scale)
CE_TABLE = {
    "onehot_off_by_one": (R.CE_FAMILIES, True),
    "lse_skips_last_chunk": (("flat", "randn3"), False),
    "ignored_row_nonzero": (R.CE_FAMILIES, False),
    "row_scale_uses_row0": (R.CE_FAMILIES, False),   # the old test has one scale for every row
    "p_in_bf16": (("randn3", "offset", "peaked", "neg_inf"), False),   # flat: bf16(1 / V) then one rounding stays inside
    "neg_inf_chunk_nan": (("neg_inf",), False),
}


@pytest.mark.parametrize("fault", R.CE_FAULTS)
def test_ce_fault_is_rejected(fault):
    assert set(CE_TABLE) == set(R.CE_FAULTS)
    must, caught = CE_TABLE[fault]
    for family in must:
        assert _rejected(lambda: _ce_check(family, fault)), (fault, family)
    rel = _old_ce(fault)
    print(f"fault {fault}: old metric {rel:.4g}")
    assert (rel < 1e-2) == (not caught)


def test_merge_stats_equals_the_whole_row():
    x = R.make_ce_case("neg_inf", 6, 2048)
    xv = x.double().reshape(6, 8, 256)
    m = xv.amax(2)
    s = torch.where(torch.isfinite(m), torch.exp(xv - torch.where(torch.isfinite(m), m, 0.0)[..., None]).sum(2), 0.0)
    lse, err = R.merge_stats(m, s)
    want = R.ref_ce_fwd(x, torch.zeros(6, dtype=torch.int64))["lse_clean"]
    assert float((lse - want).abs().max()) < 1e-12 and float(err.max()) < 1e-4


# ------------------------------------------------------------------------------ SwiGLU
def _swiglu_check(family, fault=None):
    g, u, dh = R.make_swiglu_case(family, 40, 264)
    h, dg, du = R.emu_swiglu(g, u, dh, fault)
    f, b = R.ref_swiglu_fwd(g, u), R.ref_swiglu_bwd(dh, g, u)
    R.check("h", h, f["h_ref"], f["h_bound"])
    R.check("du", du, b["du_ref"], b["du_bound"])
    R.check("dg", dg, b["dg_ref"], b["dg_bound"])
    return max(R.check_bits("h", h, f["h_want"], f["h_alts"], f["floor"]),
               R.check_bits("du", du, b["du_want"], b["du_alts"], b["floor"]),
               R.check_bits("dg", dg, b["dg_want"], (), b["floor"]))


@pytest.mark.parametrize("family", R.SWIGLU_FAMILIES)
def test_faithful_swiglu_emulator_passes(family):
    assert _swiglu_check(family) < 1e-4


def _old_swiglu(fault):
    g, u, dh = R.make_swiglu_case("randn", 64, 512)
    h, dg, du = R.emu_swiglu(g, u, dh, fault)
    f, b = R.ref_swiglu_fwd(g, u), R.ref_swiglu_bwd(dh, g, u)
    return max(R.norm_rel(h, f["h_ref"]), R.norm_rel(dg, b["dg_ref"]), R.norm_rel(du, b["du_ref"]))


SWIGLU_TABLE = {"silu_unrounded": False, "dhu_unrounded": False, "sigmoid_negated": True}


@pytest.mark.parametrize("fault", R.SWIGLU_FAULTS)
def test_swiglu_fault_is_rejected(fault):
    for family in R.SWIGLU_FAMILIES:
        assert _rejected(lambda: _swiglu_check(family, fault)), (fault, family)
    rel = _old_swiglu(fault)
    print(f"fault {fault}: old metric {rel:.4g}")
    assert (rel < 1e-2) == (not SWIGLU_TABLE[fault])


def test_all_g_holds_every_finite_pattern_once():
    g = R.all_g()
    bits = R.ibits(g).flatten().to(torch.int32) & 0xFFFF
    assert bool(torch.isfinite(g.float()).all()) and len(set(bits.tolist())) == 65280
    assert float(g.float().min()) < -3e38 and float(g.float().max()) > 3e38


def test_swiglu_floor_region_needs_its_floor():
    """g in (-96, -87.3): the true silu is a normal or denormal bf16 number, the kernel's is 0."""
    g = torch.tensor([[-88.0, -89.0, -90.0, -92.0, -87.5, -100.0, -1e4, -3e38]], dtype=R.BF)
    u = torch.ones_like(g)
    f = R.ref_swiglu_fwd(g, u)
    assert bool(f["floor"].all()) and float(f["h_ref"][0, 0]) < -2.0 ** -126
    R.check("h", torch.zeros_like(g), f["h_ref"], f["h_bound"])
    assert float(f["h_bound"][0, 0]) < 2 * 89 * 2.0 ** -126


# ------------------------------------------------------------------------------ RoPE
def _rope_check(fault=None, inverse=False, head_dim=64):
    x, cos, sin = R.make_rope_case(72, 3 * head_dim + 8, 24, head_dim)
    got = R.emu_rope(x, 2, head_dim, cos, sin, 24, inverse, fault)
    R.check_exact("rope", got, R.ref_rope(x, 2, head_dim, cos, sin, 24, inverse))
    return x, cos, sin, got


@pytest.mark.parametrize("head_dim", [16, 64, 128])
def test_faithful_rope_emulator_is_exact(head_dim):
    for inverse in (False, True):
        x, cos, sin, y = _rope_check(None, inverse, head_dim)
        back = R.emu_rope(y, 2, head_dim, cos, sin, 24, not inverse)
        R.check_exact("round trip", back, R.ref_rope(y, 2, head_dim, cos, sin, 24, not inverse))
        assert torch.equal(y[:, 2 * head_dim:], x[:, 2 * head_dim:])


def _old_rope(fault):
    """The old test: the real cos/sin table (both halves equal), bound 2 * 2^-7 * global max."""
    S, d = 24, 64
    inv = 1.0 / 10000 ** (torch.arange(0, d, 2).double() / d)
    ang = torch.arange(S).double()[:, None] * inv[None, :]
    cos, sin = torch.cat([ang.cos()] * 2, 1).to(R.BF), torch.cat([ang.sin()] * 2, 1).to(R.BF)
    x = torch.randn(72, 2 * d, generator=R._gen("oldrope")).to(R.BF)
    got, ref = R.emu_rope(x, 2, d, cos, sin, S, fault=fault), R.ref_rope(x, 2, d, cos, sin, S)
    return float((got.double() - ref.double()).abs().max()) <= 2 * 2.0 ** -7 * float(ref.double().abs().max())


ROPE_TABLE = {"pos_div_not_mod": True, "halves_swapped": True, "inverse_sign": True, "table_second_half": False}


@pytest.mark.parametrize("fault", R.ROPE_FAULTS)
def test_rope_fault_is_rejected(fault):
    assert _rejected(lambda: _rope_check(fault)), fault
    assert _old_rope(fault) == (not ROPE_TABLE[fault])


# ------------------------------------------------------------------------------ the whole table
# fault -> caught by the suite's older assertion (each entry asserted by the test of its fault above)
FAULT_TABLE = {**{f: v[2] for f, v in NORM_TABLE.items()}, **{f: v[1] for f, v in CE_TABLE.items()}, **SWIGLU_TABLE,
               **ROPE_TABLE}


def test_old_limits_miss_what_the_kit_was_built_to_see():
    assert set(FAULT_TABLE) == set(R.NORM_FWD_FAULTS + R.NORM_BWD_FAULTS + R.CE_FAULTS + R.SWIGLU_FAULTS + R.ROPE_FAULTS)
    for f in ("wrong_mode", "no_eps", "ss_drops_last_chunk", "dw_partial_bf16", "acc_bf16_single_rounding",
              "silu_unrounded", "dhu_unrounded", "table_second_half", "p_in_bf16", "ignored_row_nonzero",
              "lse_skips_last_chunk", "row_scale_uses_row0", "neg_inf_chunk_nan"):
        assert FAULT_TABLE[f] is False, f
    # a neighbouring row's rstd: 1.03e-2 at cols 8192, over y's 5e-3 limit but under the backward's 1e-2
    # at 16384 (test_neighbour_rstd_backward_twin_is_missed_by_the_old_limit)
    assert FAULT_TABLE["neighbour_rstd"] is True


# ------------------------------------------------------------------------------ the checker itself
def test_checker_names_the_element_and_rejects_non_finite():
    ref = torch.ones(4, 1040, dtype=R.F64)
    got = ref.clone()
    got[2, 1033] = float("inf")
    with pytest.raises(AssertionError, match=r"non-finite.*row 2 col 1033 chunk 129 lane 1 reg 2"):
        R.check("x", got, ref, torch.ones_like(ref))
    got[2, 1033] = 3.0
    with pytest.raises(AssertionError, match=r"worst at row 2 col 1033 chunk 129 lane 1 reg 2"):
        R.check("x", got, ref, torch.ones_like(ref))
    nan_ref = ref.clone()
    nan_ref[1] = float("nan")
    with pytest.raises(AssertionError):
        R.check("x", ref, nan_ref, torch.ones_like(ref))          # finite where NaN is documented
    w = torch.ones(4, 16, dtype=R.BF)
    g = w.clone()
    g[3, 9] = 1.0078125
    assert R.check_bits("x", g, w, cap=1.0) == 1 / 64
    g[3, 9] = 1.015625                                            # two ulps
    with pytest.raises(AssertionError, match=r"row 3 col 9 chunk 1 lane 1 reg 0"):
        R.check_bits("x", g, w, cap=1.0)
    g = w.clone()
    g[:, :4] = 1.0078125                                          # 25 %: one ulp each, over the cap
    with pytest.raises(AssertionError, match="cap"):
        R.check_bits("x", g, w)
    with pytest.raises(AssertionError):
        R.check_exact("x", -torch.zeros(2, 2, dtype=R.BF), torch.zeros(2, 2, dtype=R.BF))
    assert int(R.ibits(R.sentinel_cpu((2,), R.BF))[0]) == R.NAN16 and int(R.ibits(R.sentinel_cpu((2,), R.F32))[0]) == R.NAN32
