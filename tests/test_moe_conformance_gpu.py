"""The MoE routing kernels on the GPU (csrc/moe.hip), each on the chain's own inputs, against
tests/_moe_ref.py: selection, counts and the slot plan exactly; probabilities, gates and the aux loss
within four times torch's own f32 error; dispatch by bits; combine and its backwards within one bf16
ulp of the float64 value; the dot products within the f32 bound; dlogits against float64 autograd.

Shapes: H in {64, 128}, T in {1, 63, 192, 1000}, (E, k) in {(1, 1), (8, 2), (60, 4), (128, 8)}, and
T k of 1023 / 1024 / 1025 (k = 1) and 1022 / 1024 / 1026 (k = 2) around the 1024 items one workgroup
of pt_moe_plan ranks.  capacity_factor 1.0 on the "dominant" family (one expert chosen by every
token: drops), 1.25 elsewhere."""
import functools

import pytest
import torch

from tests import _moe_ref as R

DEV = "cuda"
pytestmark = pytest.mark.gpu
BF, F32, F64, I32 = R.BF, R.F32, R.F64, R.I32


def _cf(family):
    return 1.0 if family == "dominant" else 1.25


@functools.lru_cache(maxsize=None)
def _ref(family, T, E, k, norm, cf=None):
    """The CPU reference of one routing case, computed once: (logits, idx, gate, probs, counts, aux, C, slot, src)."""
    from picotron_amd import kernels as K
    lg = R.make_logits(family, T, E)
    idx, gate, probs, counts, aux = R.ref_route(lg, k, norm)
    C = K.moe_capacity(T, E, k, _cf(family) if cf is None else cf)
    slot, src = R.ref_plan(idx, E, C)
    return lg, idx, gate, probs, counts, aux, C, slot, src


def _route_checked(family, T, E, k, norm=True, logits_dev=None, cf=None):
    """moe_route + moe_plan on the device, every output checked; returns the device tensors."""
    from picotron_amd import kernels as K
    lg, idx, gate, probs, counts, aux, C, slot, src = _ref(family, T, E, k, norm, cf)
    out = K.moe_route(lg.to(DEV) if logits_dev is None else logits_dev, k, norm)
    tag = f"{family} T{T} E{E} k{k} norm{int(norm)}"
    R.check_exact(f"idx {tag}", out[0], idx)
    R.check_exact(f"counts {tag}", out[3], counts)
    R.check_rel(f"probs {tag}", out[2], probs)
    R.check_rel(f"gate {tag}", out[1], gate)
    R.check_rel(f"aux {tag}", out[4], aux)
    plan = K.moe_plan(out[0], E, C)
    R.check_exact(f"slot {tag}", plan[0], slot)
    R.check_exact(f"src {tag}", plan[1], src)
    return out, plan, C


@pytest.mark.parametrize("family,T,E,k", R.route_cases())
def test_route_and_plan(family, T, E, k):
    _route_checked(family, T, E, k, norm=True)
    _route_checked(family, T, E, k, norm=False)
    if family == "dominant" and T >= 192 and E > 1:
        assert int((_ref(family, T, E, k, True)[7] < 0).sum()) > 0   # this case does drop


def test_plan_block_is_what_the_cases_straddle():
    from picotron_amd import _C
    assert _C.load_library().pt_moe_plan_block() == R.PLAN_BLOCK


def test_route_on_a_strided_view_and_twice():
    from picotron_amd import kernels as K
    family, T, E, k = "randn", 192, 60, 4
    lg = _ref(family, T, E, k, True)[0]
    wide = torch.full((T, 64), 99.0, dtype=BF, device=DEV)   # columns past E must not be read
    wide[:, :E] = lg.to(DEV)
    a, plan_a, C = _route_checked(family, T, E, k, logits_dev=wide[:, :E])
    b = K.moe_route(wide[:, :E], k, True)
    plan_b = K.moe_plan(b[0], E, C)
    for x, y in zip(a + plan_a, b + plan_b):
        assert torch.equal(x, y)   # two runs, the same bits


@pytest.mark.parametrize("H", R.HIDDEN)
@pytest.mark.parametrize("E,k", R.EXPERTS)
@pytest.mark.parametrize("T", R.TOKENS)
@pytest.mark.parametrize("family", ["randn", "dominant"])
def test_row_kernels(family, T, E, k, H):
    _row_kernels(family, T, E, k, H)


def test_row_kernels_wide_rows_past_one_grid():
    """H = 1024 and R H / 8 = 9216 * 128 > 2^20 threads: the dispatch kernel's grid-stride loop takes a second
    trip (its grid is capped at 4096 workgroups of 256) and a wave of combine_bwd walks its row in two
    trips (H / 8 = 128 chunks over 64 lanes).  Dropless (capacity_factor = E / k), so every row kernel
    moves T k = 2200 full rows."""
    from picotron_amd import kernels as K
    T, E, k, H = 1100, 8, 2, 1024
    assert K.moe_capacity(T, E, k, 4.0) * E * (H // 8) > 4096 * 256
    _row_kernels("randn", T, E, k, H, cf=4.0)


def _row_kernels(family, T, E, k, H, cf=None):
    """dispatch, combine (gated with residual; unweighted = the dispatch backward) and combine_bwd on
    the slots and gates the device's own route / plan produced (checked exact / in tolerance first).
    The combine inputs are sign-coherent (R.coherent_rows): no cancellation, so one bf16 ulp of the
    float64 value bounds the f32 accumulation by construction."""
    from picotron_amd import kernels as K
    (idx_d, gate_d, _, _, _), (slot_d, src_d), C = _route_checked(family, T, E, k, cf=cf)
    slot, src, gate = slot_d.cpu(), src_d.cpu(), gate_d.cpu()
    tag = f"{family} T{T} E{E} k{k} H{H}"
    g = R.gen("rows", family, T, E, k, H)
    x = torch.randn(T, H, generator=g).to(BF)
    x[0, 0] = float("nan")          # a bit copy carries NaN payloads and signed zeros
    x[T - 1, H - 1] = -0.0
    xe = K.moe_dispatch(x.to(DEV), src_d, k)
    R.check_exact(f"xe {tag}", xe, R.ref_dispatch(x, src, k))

    res, ye, _ = R.coherent_rows(src, k, T, H, seed=E)
    y = K.moe_combine(ye.to(DEV), slot_d, gate_d, res.to(DEV))
    R.check_bf16(f"combine {tag}", y, R.ref_combine(ye, slot, gate, res))
    all_dropped = (slot < 0).all(1)
    if bool(all_dropped.any()):   # the residual alone carries such a token, bit for bit
        R.check_exact(f"combine dropped rows {tag}", y.cpu()[all_dropped], res[all_dropped])
    dx = K.moe_combine(ye.to(DEV), slot_d)
    R.check_bf16(f"dx {tag}", dx, R.ref_combine(ye, slot), zero=all_dropped[:, None].expand(T, H))

    dy = torch.randn(T, H, generator=g).to(BF)
    dye, dgate = K.moe_combine_bwd(dy.to(DEV), ye.to(DEV), slot_d, src_d, gate_d)
    dye_ref, dgate_ref, mag = R.ref_combine_bwd(dy, ye, slot, src, gate)
    R.check_bf16(f"dye {tag}", dye, dye_ref, zero=(src < 0)[:, None].expand_as(dye_ref))
    R.check_dgate(f"dgate {tag}", dgate, dgate_ref, mag, H, slot < 0)


@pytest.mark.parametrize("norm,d_aux", [(True, 0.0), (True, 0.37), (False, 0.0), (False, -1.5)])
@pytest.mark.parametrize("family,T,E,k", [c for c in R.route_cases() if c[0] in ("randn", "dominant") and c[1] in (1, 63, 1000)]
                         + [("equal", 192, 8, 2), ("pm60", 192, 60, 4)])
def test_route_bwd(family, T, E, k, norm, d_aux):
    """dlogits against float64 autograd through the reference router with the kernel's own idx fixed
    (proven exact first): one bf16 ulp plus the forward's f32 tolerance, propagated
    (R.route_bwd_allowance)."""
    from picotron_amd import kernels as K
    (idx_d, gate_d, probs_d, counts_d, _), _, _ = _route_checked(family, T, E, k, norm)
    lg = _ref(family, T, E, k, norm)[0]
    dgate = torch.randn(T, k, generator=R.gen("dgate", family, T, E, k)).to(F32)
    da = torch.tensor([d_aux], dtype=F32, device=DEV) if d_aux != 0.0 else None
    dl = K.moe_route_bwd(dgate.to(DEV), probs_d, idx_d, counts_d, da, norm)
    ref, p = R.ref_route_bwd(lg, idx_d.cpu(), dgate, d_aux, norm)
    R.check_bf16(f"dlogits {family} T{T} E{E} k{k} norm{int(norm)} aux{d_aux}", dl, ref,
                 extra=R.route_bwd_allowance(p, idx_d.cpu(), dgate, d_aux, norm))
    if d_aux != 0.0:   # a zero device scalar is the same as none
        z = K.moe_route_bwd(dgate.to(DEV), probs_d, idx_d, counts_d, torch.zeros(1, dtype=F32, device=DEV), norm)
        assert torch.equal(z, K.moe_route_bwd(dgate.to(DEV), probs_d, idx_d, counts_d, None, norm))


def test_route_bwd_zeroes_padded_columns():
    """The ABI's dlogits [T, ldl]: columns E .. ldl are written as zeros."""
    import ctypes
    from picotron_amd import _C, kernels as K
    T, E, k, ldl = 63, 60, 4, 64
    (idx_d, _, probs_d, counts_d, _), _, _ = _route_checked("randn", T, E, k)
    dgate = torch.randn(T, k, generator=R.gen("pad")).to(DEV)
    out = torch.full((T, ldl), 7.0, dtype=BF, device=DEV)
    rc = _C.lib().pt_moe_route_bwd(dgate.data_ptr(), probs_d.data_ptr(), idx_d.data_ptr(), counts_d.data_ptr(), None, 1,
                                   out.data_ptr(), ldl, T, E, k, _C.stream_ptr(out.device))
    assert rc == 0
    assert torch.equal(out[:, :E], K.moe_route_bwd(dgate, probs_d, idx_d, counts_d))
    assert bool((out[:, E:].view(torch.int16) == 0).all())
