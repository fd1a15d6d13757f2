"""Self-test of the z-loss checker (tests/_ce_z_ref.py) on the CPU: the faithful fp32 emulation of the _z
kernels passes the derived bounds on every input family, for every z the GPU tests use and at their shapes,
and each fault a z-loss implementation can plausibly have is rejected there -- a GPU test whose inputs
cannot tell these apart would show nothing."""
import pytest
import torch

from tests import _ce_z_ref as Z
from tests import _row_ref as R

V_SHAPES = (8, 2040, 8200, 49160, 65544)     # tests/test_ce_z_conformance_gpu.py's fused widths
GS = (0.25 * (1 + torch.arange(Z.CE_ROWS) % 3)).to(R.F32)


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _check(family, V, z, fault=None, style="sub", fused=True):
    """The emulation against the bounds: fused (the LSE carries its error into the gradient) or the
    streaming pair (the backward reads the stored f32 LSE)."""
    x, tgt = Z.ce_case(family, V)
    loss, rz, lse, grad = Z.emu_ce_z(x, tgt, GS, z, fault=fault)
    f = R.ref_ce_fwd(x, tgt, style=style)
    zf = Z.ref_z_fwd_from(f, z)
    R.check("row_z", rz, zf["row_z"], zf["row_z_bound"])
    R.check("loss", loss, zf["loss"], zf["loss_bound"])
    if fused:
        ref, bound = Z.ref_z_bwd(x, tgt, f["lse"], f["lse_bound"], GS.double(), z, style=style)
    else:
        ref, bound = Z.ref_z_bwd(x, tgt, lse.double(), torch.zeros(Z.CE_ROWS, dtype=R.F64), GS.double(), z, style=style)
    R.check("grad", grad, ref, bound)
    ign = tgt == R.IGNORE
    R.check_exact("ignored rows", grad[ign], torch.zeros_like(grad[ign]))
    R.check_exact("ignored row_z", rz[ign], torch.zeros_like(rz[ign]))


@pytest.mark.parametrize("V", V_SHAPES)
@pytest.mark.parametrize("family", R.CE_FAMILIES)
def test_faithful_z_emulator_passes(family, V):
    for z in Z.Z_VALUES:
        for fused in (True, False):
            _check(family, V, z, style="sub" if fused else "fma", fused=fused)


def test_z_zero_is_the_plain_reference():
    """At z = 0 the z references and bounds are _row_ref's own, and the emulation is emu_ce's by bits."""
    for family in R.CE_FAMILIES:
        x, tgt = Z.ce_case(family, 2040)
        f = R.ref_ce_fwd(x, tgt)
        zf = Z.ref_z_fwd_from(f, 0.0)
        assert torch.equal(zf["row_z"], torch.zeros(Z.CE_ROWS, dtype=R.F64)) and not bool(zf["row_z_bound"].any())
        assert torch.equal(torch.nan_to_num(zf["loss"], 7.0), torch.nan_to_num(f["loss"], 7.0))
        assert torch.equal(zf["loss_bound"], R._zero_nan(f["loss_bound"]))
        ref, bound = R.ref_ce_bwd(x, tgt, f["lse"], f["lse_bound"], GS.double())
        zref, zbound = Z.ref_z_bwd(x, tgt, f["lse"], f["lse_bound"], GS.double(), 0.0)
        assert torch.equal(ref, zref) and torch.equal(bound, zbound)
        loss, grad = R.emu_ce(x, tgt, GS)
        zloss, rz, _, zgrad = Z.emu_ce_z(x, tgt, GS, 0.0)
        R.check_exact("loss", zloss, loss)
        R.check_exact("grad", zgrad, grad)


def test_z_coefficient_is_the_f32_value():
    """1e-4 is not an f32 value: the reference uses what the kernel receives, not the Python double."""
    assert Z.z32(1e-4) != 1e-4 and Z.z32(0.25) == 0.25
    x, tgt = Z.ce_case("flat", 8)
    f = R.ref_ce_fwd(x, tgt)
    zf = Z.ref_z_fwd_from(f, 1e-4)
    v = f["valid"]
    assert torch.equal(zf["row_z"][v], (Z.z32(1e-4) * f["lse"] * f["lse"])[v])
    assert not torch.equal(zf["row_z"][v], (1e-4 * f["lse"] * f["lse"])[v])


# the peaked family's LSE is its peak logit, a bf16 value already: rounding it changes nothing there
NOT_SEEN_BY = {"lse_bf16_before_square": ("peaked",)}


@pytest.mark.parametrize("V", V_SHAPES)
@pytest.mark.parametrize("fault", Z.Z_FAULTS)
def test_z_fault_is_rejected(fault, V):
    """Every fault is rejected at every width the GPU tests use, at z = 2^-2, on every family that can show it,
    against the fused bounds and against the streaming pair's."""
    for family in R.CE_FAMILIES:
        for fused in (True, False):
            rej = _rejected(lambda: _check(family, V, 0.25, fault, style="sub" if fused else "fma", fused=fused))
            assert rej == (family not in NOT_SEEN_BY.get(fault, ())), (fault, family, V, fused)


def test_only_the_large_z_tests_the_gradient_by_much():
    """Why 2^-2 is among the values: at z = 1e-4 and an LSE near 13 the factor is 1 + 2.6e-3, and a backward
    without it misses the bound by less than 3x on randn3 (one bf16 ulp decides); at 2^-2 by more than 100x."""
    def worst(z):
        x, tgt = Z.ce_case("randn3", 8200)
        f = R.ref_ce_fwd(x, tgt)
        grad = Z.emu_ce_z(x, tgt, GS, z, fault="grad_without_z")[3]
        ref, bound = Z.ref_z_bwd(x, tgt, f["lse"], f["lse_bound"], GS.double(), z)
        return float(((grad.double() - ref).abs() / bound).max())
    assert worst(1e-4) < 3 and worst(0.25) > 100
