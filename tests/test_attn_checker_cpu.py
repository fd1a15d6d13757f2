"""The attention conformance checker (tests/_attn_ref.py) tested on itself, without a GPU.

  * the fp32 emulator of the kernels' numerics passes every check for every input family;
  * every injected fault is rejected on at least one adversarial family;
  * the closed forms of `zeroq` and `headcode` hold in the float64 reference.

Each fault, the families whose check rejects it, and whether the suite's older metric (Frobenius-norm
ratio < 1e-2 for the output on `randn`, max |lse error| < 1e-2) would have caught it on `randn`
(FAULT_TABLE, asserted by test_injected_fault_is_rejected):

    fault        rejected on                                              old metric on randn
    mask_lt      every family (row 0 sees no key: non-finite)             caught (NaN)
    mask_le1     every family                                             caught (0.35)
    no_alpha_o   peaked, ramp                                             missed (0.002)
    no_alpha_l   peaked, ramp                                             missed (0.002)
    m_init0      offset- (l underflows to 0: non-finite)                  missed (0.002)
    kv_mod       every family                                             caught (1.03)
    p_trunc      randn, peaked (f32 accumulator), headcode (exactness)    missed (0.003)
    bad_row      every family but headcode (its rows are equal)           caught (0.044, one of 1024 rows)
    bad_elem     randn, peaked, headcode                                  missed (0.002)
    lse_off      every family                                             missed (1e-3 < 1e-2)

P truncated instead of rounded stays inside the bf16-output bound by construction (its error is at
most 2 u A, the bound 1.5 u (A + |ref|)); it is the f32 accumulator's bound 1.5 u A and headcode's
exact output that reject it.  The battery applied to a family here (_forward_passes) is the one the
GPU tests apply: out, lse, the merge mode's f32 addend, and headcode's exact output.
"""
import math

import pytest
import torch

from tests import _attn_ref as R

SHAPES = [  # Sq, Sk, D, causal
    (256, 256, 64, True),
    (256, 256, 128, False),
    (128, 384, 64, False),
]
B, H, HKV = 1, 4, 2

# fault -> (families on which the checker must reject it, caught by the old norm metric on randn)
FAULT_TABLE = {
    "mask_lt": (R.FAMILIES, True),
    "mask_le1": (R.FAMILIES, True),
    "no_alpha_o": (("peaked", "ramp"), False),
    "no_alpha_l": (("peaked", "ramp"), False),
    "m_init0": (("offset-",), False),
    "kv_mod": (R.FAMILIES, True),
    "p_trunc": (("randn", "peaked", "headcode"), False),
    "bad_row": (("randn", "peaked", "offset+", "offset-", "ramp", "zeroq"), True),
    "bad_elem": (("randn", "peaked", "headcode"), False),
    "lse_off": (R.FAMILIES, False),
}


def _mask(Sq, Sk, causal):
    return R.causal_mask(Sq, Sk) if causal else None


def _forward_passes(family, fault, Sq=256, Sk=256, D=64, causal=True):
    """True when the (faulty) emulator's forward passes the checker on this family."""
    q, k, v, _ = R.make_case(family, B, Sq, Sk, H, HKV, D)
    scale = R.scale_of(D)
    ref = R.ref_forward(q, k, v, scale, _mask(Sq, Sk, causal))
    o, lse = R.emu_forward(q, k, v, scale, causal, fault=fault)
    acc, _ = R.emu_forward(q, k, v, scale, causal, fault=fault, f32_out=True)   # the merge mode's addend
    try:
        R.check_out(o, ref, family)
        R.check_lse(lse, ref.lse, family)
        R.check_acc(acc, ref, family)
        if family == "headcode":
            assert torch.equal(o.double(), ref.o.round()), "headcode: the output is exact in bf16"
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("Sq,Sk,D,causal", SHAPES)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_emulator_passes_the_checker(family, Sq, Sk, D, causal):
    q, k, v, do = R.make_case(family, B, Sq, Sk, H, HKV, D)
    scale = R.scale_of(D)
    mask = _mask(Sq, Sk, causal)
    ref = R.ref_forward(q, k, v, scale, mask)
    o, lse = R.emu_forward(q, k, v, scale, causal)
    R.check_out(o, ref, family)
    R.check_lse(lse, ref.lse, family)
    assert R.norm_rel(o, ref.o) < 1e-2
    dq, dk, dv, delta = R.emu_backward(q, k, v, do, o, lse, scale, causal)
    bwd = R.ref_backward(q, k, v, do, lse, scale, mask, o=o)
    R.check_delta(delta, bwd, family)
    R.check_grads(dq, dk, dv, bwd, family)
    # f32 accumulation onto non-zero gradients
    init = {n: torch.full_like(getattr(bwd, n), 0.25, dtype=torch.float32) for n in ("dq", "dk", "dv")}
    gq, gk, gv, _ = R.emu_backward(q, k, v, do, o, lse, scale, causal, f32=True)
    R.check_grads_f32(init["dq"] + gq, init["dk"] + gk, init["dv"] + gv, bwd, init, family)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_injected_fault_is_rejected(fault):
    families, old_catches = FAULT_TABLE[fault]
    for family in families:
        assert _forward_passes(family, None), f"the clean emulator must pass on {family}"
        assert not _forward_passes(family, fault), f"{fault} not rejected on {family}"
    # the older global metric on the benign family
    q, k, v, _ = R.make_case("randn", B, 256, 256, H, HKV, 64)
    ref = R.ref_forward(q, k, v, R.scale_of(64), R.causal_mask(256, 256))
    o, lse = R.emu_forward(q, k, v, R.scale_of(64), True, fault=fault)
    rel = R.norm_rel(o, ref.o)
    lse_err = float((lse.double() - ref.lse).abs().max())
    old_passes = rel < 1e-2 and lse_err < 1e-2      # NaN compares False: caught
    print(f"fault {fault}: old metric on randn rel {rel:.4g} lse {lse_err:.4g}")
    assert old_passes == (not old_catches)


def test_checker_rejects_non_finite_and_reports_the_element():
    ref = torch.ones(2, 3, dtype=torch.float64)
    got = ref.clone()
    got[1, 2] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        R.check("x", got, ref, torch.ones_like(ref))
    got[1, 2] = 3.0
    with pytest.raises(AssertionError, match=r"worst at \(1, 2\)"):
        R.check("x", got, ref, torch.ones_like(ref))
    with pytest.raises(AssertionError):      # any error against a zero bound
        R.check("x", ref + 1e-9, ref, torch.zeros_like(ref))
    assert R.check("x", ref, ref, torch.zeros_like(ref)) == 0.0


def test_zeroq_closed_form_in_the_reference():
    S, D = 256, 64
    q, k, v, _ = R.make_case("zeroq", B, S, S, H, HKV, D)
    ref = R.ref_forward(q, k, v, R.scale_of(D), R.causal_mask(S, S))
    n = torch.arange(1, S + 1, dtype=torch.float64)
    assert torch.allclose(ref.lse, torch.log(n).expand(B, H, S), rtol=0, atol=1e-13)
    mean = v.double().cumsum(1) / n[None, :, None, None]                    # [B, S, HKV, D]
    assert torch.allclose(ref.o, mean.repeat_interleave(H // HKV, 2), rtol=0, atol=1e-13)
    full = R.ref_forward(q, k, v, R.scale_of(D))
    assert torch.allclose(full.lse, torch.full_like(full.lse, math.log(S)), rtol=0, atol=1e-13)


def test_headcode_closed_form_in_the_reference():
    S, D = 256, 64
    q, k, v, _ = R.make_case("headcode", B, S, S, H, HKV, D)
    ref = R.ref_forward(q, k, v, R.scale_of(D), R.causal_mask(S, S))
    code = (torch.arange(H) // (H // HKV) + 1).double()[None, None, :, None].expand(B, S, H, D)
    assert torch.allclose(ref.o, code, rtol=0, atol=1e-13)
    assert torch.equal(ref.o.to(torch.bfloat16).double(), code)


def test_merge_case_blocks_lie_100_nats_apart():
    for family in ("peaked", "offset+", "offset-"):
        q, blocks, _ = R.make_merge_case(family, 1, 128, 2, 1, 64)
        lses = [R.ref_forward(q, kb, vb, R.scale_of(64), R.causal_mask(128, 128) if i == 0 else None).lse
                for i, (kb, vb) in enumerate(blocks)]
        assert float((lses[1] - lses[0]).min()) > 100 and float((lses[0] - lses[2]).min()) > 100
        s_max = max(float(R._scores(q, kb, R.scale_of(64), None).abs().max()) for kb, _ in blocks)
        assert s_max < 330
