"""The MoE conformance kit checks itself (CPU): every checker of tests/_moe_ref.py accepts the
reference rounded to the kernels' output types and rejects a planted error of the kind a wrong
kernel would make; the tolerance constant is re-measured.  (Like its sibling checker self-tests, this
file exercises tests/_moe_ref.py only, so it passes with or without the feature; the kernels meet these
checkers in tests/test_moe_conformance_gpu.py.)"""
import pytest
import torch

from tests import _moe_ref as R

BF, F32, F64, I32 = R.BF, R.F32, R.F64, R.I32


def _case(family="randn", T=192, E=8, k=2, norm=True, C=64, H=64):
    lg = R.make_logits(family, T, E)
    idx, gate, probs, counts, aux = R.ref_route(lg, k, norm)
    slot, src = R.ref_plan(idx, E, C)
    return lg, idx, gate, probs, counts, aux, slot, src


def test_torch_f32_error_is_under_the_recorded_figure():
    """TORCH_F32_REL is what torch's own f32 evaluation loses against float64 on the tests' inputs."""
    worst = 0.0
    for family, T, E, k in R.route_cases():
        for norm in (True, False):
            lg = R.make_logits(family, T, E)
            idx, g64, p64, _, a64 = R.ref_route(lg, k, norm)
            _, g32, p32, _, a32 = R.ref_route(lg, k, norm, idx=idx, dtype=F32)
            worst = max(worst, R.rel_err(p32, p64), R.rel_err(g32, g64), R.rel_err(a32, a64))
    print(f"torch f32 routing error against float64: {worst:.3e}")
    assert 0.5 * R.TORCH_F32_REL <= worst <= R.TORCH_F32_REL   # the recorded figure is the measured one
    assert R.F32_TOL == max(4 * R.TORCH_F32_REL, 2.0 ** -22)


def test_route_cases_cover_the_issue():
    cases = R.route_cases()
    for f in R.LOGIT_FAMILIES:
        for T in (1, 63, 192, 1000):
            for Ek in ((1, 1), (8, 2), (60, 4), (128, 8)):
                assert (f, T) + Ek in cases
    items = {T * k for _, T, _, k in cases}
    assert {R.PLAN_BLOCK - 1, R.PLAN_BLOCK, R.PLAN_BLOCK + 1} <= items


@pytest.mark.parametrize("family", R.LOGIT_FAMILIES)
def test_selection_is_exact_and_ties_go_low(family):
    lg, idx, *_ = _case(family)
    R.check_exact("idx", idx.clone(), idx)
    v = lg.float()
    picked = v.gather(1, idx.long())
    assert bool((picked[:, :-1] >= picked[:, 1:]).all())   # best first
    if family == "equal":
        assert bool((idx == torch.arange(idx.shape[1], dtype=I32)).all())   # all ties: experts 0 .. k-1
        wrong = idx.flip(1).contiguous()   # ties to the higher index / worst first
        with pytest.raises(AssertionError):
            R.check_exact("idx", wrong, idx)
    bad = idx.clone()
    bad[5, 0] = (bad[5, 0] + 1) % lg.shape[1]
    with pytest.raises(AssertionError):
        R.check_exact("idx", bad, idx)


def test_plan_by_brute_force_and_planted_errors():
    _, idx, _, _, counts, _, slot, src = _case("dominant", C=64)
    # the definition, item by item
    E, C = 8, 64
    seen = [0] * E
    for i, e in enumerate(idx.reshape(-1).tolist()):
        want = e * C + seen[e] if seen[e] < C else -1
        assert int(slot.reshape(-1)[i]) == want
        if want >= 0:
            assert int(src[want]) == i
        seen[e] += 1
    assert seen == counts.tolist() and max(seen) > C   # the dominant expert overflows: drops
    assert int((src < 0).sum()) == E * C - int((slot >= 0).sum())
    R.check_exact("slot", slot.clone(), slot)
    for name, ref, bad in (("slot", slot, torch.where(slot >= 0, slot + 1, slot)),
                           ("slot", slot, slot.clamp_min(0)),
                           ("src", src, src.clamp_min(0)),
                           ("src", src, src.roll(1))):
        with pytest.raises(AssertionError):
            R.check_exact(name, bad.contiguous(), ref)
    with pytest.raises(AssertionError):
        R.check_exact("slot", slot.long(), slot)   # dtype


def test_rel_checker_accepts_f32_and_rejects_wrong_formulas():
    lg, idx, gate, probs, counts, aux, *_ = _case("randn", norm=True)
    R.check_rel("probs", probs.to(F32), probs)
    R.check_rel("gate", gate.to(F32), gate)
    R.check_rel("aux", aux.to(F32), aux)
    _, raw, *_ = R.ref_route(lg, 2, norm=False)
    with pytest.raises(AssertionError):
        R.check_rel("gate", raw.to(F32), gate)            # renormalisation forgotten
    with pytest.raises(AssertionError):
        R.check_rel("aux", (aux * 2).to(F32), aux)        # HF Mixtral's k times the Switch value
    with pytest.raises(AssertionError):
        R.check_rel("probs", probs.to(BF).to(F32), probs)  # probabilities kept in bf16
    with pytest.raises(AssertionError):
        R.check_rel("probs", probs, probs)                # dtype: float64 is not the kernel's output
    hot = (R.make_logits("pm60", 63, 8).float() * 1.5).to(BF)   # +-90: exp overflows f32 past 88.7
    naive = torch.exp(hot.float()) / torch.exp(hot.float()).sum(1, keepdim=True)   # no max subtraction
    with pytest.raises(AssertionError):
        R.check_rel("probs", naive, R.ref_route(hot, 2)[2])


def test_bf16_checker_one_ulp():
    _, idx, gate, _, _, _, slot, src = _case("dominant", C=64)
    res, ye, _ = R.coherent_rows(src, 2, 192, 64, seed=1)
    ref = R.ref_combine(ye, slot, gate.to(F32), res)
    good = ref.to(F32).to(BF)
    R.check_bf16("y", good, ref)
    ulp = R.bf16_ulp(ref)
    R.check_bf16("y", (ref + 0.45 * ulp).to(F32).to(BF), ref)   # either neighbour of ref
    two = (good.to(F64) + 2 * R.bf16_ulp(good.to(F64))).to(F32).to(BF)
    with pytest.raises(AssertionError):
        R.check_bf16("y", two, ref)
    with pytest.raises(AssertionError):
        R.check_bf16("y", R.ref_combine(ye, slot, None, res).to(F32).to(BF), ref)   # the gate forgotten
    with pytest.raises(AssertionError):
        R.check_bf16("y", R.ref_combine(ye, slot.clamp_min(0), gate.to(F32), res).to(F32).to(BF), ref)   # drops kept
    # empty rows and dropped items must be exactly zero
    dy = torch.randn(192, 64, generator=R.gen("dy")).to(BF)
    dye, dgate, mag = R.ref_combine_bwd(dy, ye, slot, src, gate.to(F32))
    empty = (src < 0)[:, None].expand_as(dye)
    R.check_bf16("dye", dye.to(F32).to(BF), dye, zero=empty)
    dirty = dye.to(F32).to(BF)
    dirty[(src < 0).nonzero()[0, 0], 3] = 2.0 ** -130
    with pytest.raises(AssertionError):
        R.check_bf16("dye", dirty, dye, zero=empty)
    R.check_dgate("dgate", dgate.to(F32), dgate, mag, 64, slot < 0)
    with pytest.raises(AssertionError):
        R.check_dgate("dgate", (dgate + 2 * 64 * 2.0 ** -23 * mag).to(F32), dgate, mag, 64, slot < 0)
    leak = dgate.to(F32)
    leak[(slot < 0).nonzero()[0, 0], (slot < 0).nonzero()[0, 1]] = 1e-30
    with pytest.raises(AssertionError):
        R.check_dgate("dgate", leak, dgate, mag, 64, slot < 0)


def test_bf16_ulp_values():
    x = torch.tensor([1.0, 1.5, 2.0, -3.0, 2.0 ** -126, 0.0, 2.0 ** -140], dtype=F64)
    want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133, 2.0 ** -133], dtype=F64)
    assert torch.equal(R.bf16_ulp(x), want)


@pytest.mark.parametrize("norm", [True, False])
def test_route_bwd_reference_matches_finite_differences_and_rejects_errors(norm):
    lg = R.make_logits("randn", 7, 8)
    idx = R.ref_select(lg, 2)
    dgate = torch.randn(7, 2, generator=R.gen("dg"), dtype=F64)
    d_aux = 0.37
    grad, p = R.ref_route_bwd(lg, idx, dgate, d_aux, norm)

    def loss(l64):
        pp = torch.softmax(l64, 1)
        sel = pp.gather(1, idx.long())
        g = sel / sel.sum(1, keepdim=True) if norm else sel
        f = torch.bincount(idx.reshape(-1).long(), minlength=8).to(F64) / 14
        return float((g * dgate).sum() + d_aux * 8 * (f * pp.mean(0)).sum())

    base = lg.to(F64)
    for (t, e) in ((0, 0), (3, 5), (6, 7)):
        hi, lo = base.clone(), base.clone()
        hi[t, e] += 1e-6
        lo[t, e] -= 1e-6
        assert abs((loss(hi) - loss(lo)) / 2e-6 - float(grad[t, e])) < 1e-7
    assert float(grad.sum(1).abs().max()) < 1e-12   # a softmax gradient sums to zero over the experts
    R.check_bf16("dlogits", grad.to(F32).to(BF), grad)
    no_aux, _ = R.ref_route_bwd(lg, idx, dgate, 0.0, norm)
    with pytest.raises(AssertionError):
        R.check_bf16("dlogits", no_aux.to(F32).to(BF), grad)
    other, _ = R.ref_route_bwd(lg, idx, dgate, d_aux, not norm)
    with pytest.raises(AssertionError):
        R.check_bf16("dlogits", other.to(F32).to(BF), grad)


def test_dispatch_reference_is_a_bit_copy():
    _, _, _, _, _, _, slot, src = _case("dominant", C=64)
    x = torch.randn(192, 64, generator=R.gen("x")).to(BF)
    x[0, 0] = float("nan")
    x[1, 1] = -0.0
    xe = R.ref_dispatch(x, src, 2)
    R.check_exact("xe", xe.clone(), xe)
    kept = (src >= 0).nonzero().flatten()
    assert torch.equal(xe[kept].view(torch.int16), x[(src[kept] // 2).long()].view(torch.int16))
    assert bool((xe[src < 0].view(torch.int16) == 0).all())
    bad = xe.clone()
    bad[(src < 0).nonzero()[0, 0], 0] = -0.0   # an empty row must be +0 bits
    with pytest.raises(AssertionError):
        R.check_exact("xe", bad, xe)
