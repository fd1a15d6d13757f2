"""Float64 reference, per-element bounds and an fp32 emulator with injectable faults for the auxiliary
z-loss of csrc/cross_entropy.hip (the _z entry points).  Builds on tests/_row_ref.py (its notation:
u = 2^-8, e = 2^-24, HW, TINY = 2^-126, SECOND).  CPU only.

With z the coefficient AS THE KERNEL RECEIVES IT (its f32 value, z32), L the float64 LSE of the bf16
logits and e_L the bound on the kernel's f32 LSE (ref_ce_fwd's lse_bound, merge_stats' for the forms
fed by statistics):

    row_z  = z (lse lse)      two f32 multiplies of lse = L + d, |d| <= e_L:
             E_z = z (2 |L| e_L + e_L^2) + 2 e z (|L| + e_L)^2 + 2 TINY
             (the square's and the product's roundings; either may be flushed below 2^-126)
    loss   = (lse - x_t) + row_z   one more addition:
             E_loss = loss_bound + E_z + e |loss|
    c      = 1 + 2 z lse      (2 z is exact; a product and a sum, or one fma: at most two roundings)
             E_c = 2 z e_c + e (|2 z L| + |c|),  e_c = e_L in the fused form, 0 where the backward reads
             the forward's stored f32 LSE (then L is that f32 value)
    grad   = (p c - onehot) g, p = exp(x - lse) with ref_ce_bwd's relative error E_p:
             E32 = |g| (p |c| E_p + p E_c + e p |c| + TINY (1 + |c|)) + 3 e |(p c - onehot) g| + TINY
             (ref_ce_bwd's bound with c's error and the rounding of p c added), then b16.
    Ignored rows: row_z 0, loss 0, gradient +0 by bits (c is taken as 1 there).  Bad targets: NaN.
    z = 0: every bound above reduces to _row_ref's own (E_z = 0 is asserted as exact zeros).
"""
import math

import torch

from tests import _row_ref as R

F32, F64, BF = R.F32, R.F64, R.BF
Z_VALUES = (0.25, 1e-4, 0.0)


CE_ROWS = 8


def ce_case(family, V, rows=CE_ROWS):
    """(logits bf16 [rows, V], targets): make_targets' cycle (columns 0, 7, 8, V - 1, the ignored row, the chunk
    edges); in the peaked family the target sits on the peak in even rows."""
    x = R.make_ce_case(family, rows, V)
    tgt = R.make_targets(rows, V)
    if family == "peaked":
        rr = torch.arange(rows)
        tgt = torch.where((rr % 2 == 0) & (tgt != R.IGNORE), R.peak_col(rr, V), tgt)
    return x, tgt


def z32(z):
    """The coefficient as the kernels receive it: the f32 nearest to the Python float, as a float."""
    return float(torch.tensor(z, dtype=F32))


def ref_z_fwd(z, lse, e_lse, valid, loss, loss_bound):
    """dict row_z, row_z_bound, loss, loss_bound (float64 [rows]) from the float64 LSE (NaN on bad rows), its
    bound, the valid mask and the plain loss / bound (ref_ce_fwd's, or the statistics tests' own)."""
    z = z32(z)
    L = lse.to(F64)
    e_L = e_lse.to(F64)
    zero = torch.zeros_like(L)
    rz = torch.where(valid, z * L * L, zero)
    if z:
        e_z = (z * (2 * L.abs() * e_L + e_L * e_L) + 2 * R.E * z * (L.abs() + e_L) ** 2) * R.SECOND + 2 * R.TINY
        e_z = R._zero_nan(torch.where(valid, e_z, zero))       # a bad target's row is NaN: no bound
    else:
        e_z = zero
    tot = loss.to(F64) + rz
    e_loss = R._zero_nan(torch.where(valid, loss_bound.to(F64) + e_z + (R.E * tot.abs() if z else 0.0), zero))
    return dict(row_z=rz, row_z_bound=e_z, loss=tot, loss_bound=e_loss)


def ref_z_fwd_from(f, z):
    """ref_z_fwd from ref_ce_fwd's dict."""
    return ref_z_fwd(z, f["lse"], f["lse_bound"], f["valid"], f["loss"], f["loss_bound"])


def ref_z_bwd(x, tgt, lse, lse_err, gscale, z, ignore=R.IGNORE, style="sub", vocab_lo=0):
    """(grad_ref float64 [rows, V], bound): (exp(x - lse) (1 + 2 z lse) - onehot) g; the arguments of
    R.ref_ce_bwd and the coefficient."""
    z = z32(z)
    rows, V = x.shape
    xv, L = x.to(F64), lse.to(F64)[:, None]
    e_L = lse_err.to(F64)[:, None]
    valid = (tgt != ignore)[:, None]
    g = torch.where(valid, gscale.to(F64)[:, None].expand(rows, 1), torch.zeros(rows, 1, dtype=F64))
    d = xv - L
    p = torch.exp(d)
    onehot = (torch.arange(V)[None, :] == (tgt - vocab_lo)[:, None]).to(F64)
    e_p = R._zero_nan(e_L + R._arg_err(xv, L, d, style)) + R.HW
    c = torch.where(valid, 1 + 2 * z * L, torch.ones_like(L))
    e_c = torch.where(valid, 2 * z * R._zero_nan(e_L) + R.E * ((2 * z * L).abs() + c.abs()), torch.zeros_like(L)) if z \
        else torch.zeros_like(L)
    e_c = R._zero_nan(e_c)
    ca = R._zero_nan(c.abs())
    ref = (p * c - onehot) * g
    extra = R.E * p * ca if z else 0.0
    e32 = (g.abs() * (p * ca * e_p + p * e_c + extra + R.TINY * (1 + (ca if z else 0.0))) + 3 * R.E * ref.abs()) * R.SECOND + R.TINY
    return ref, R.b16(ref, e32)


Z_FAULTS = ("grad_without_z", "factor_missing_2", "factor_on_onehot", "z_not_in_row_z", "ignored_row_z_nonzero",
            "ignored_row_grad_nonzero", "lse_bf16_before_square", "row_z_linear")


def emu_ce_z(x, tgt, gscale, z, ignore=R.IGNORE, fault=None):
    """(loss f32 [rows], row_z f32 [rows], lse f32 [rows], grad bf16 [rows, V]) in fp32 torch, as the _z
    kernels compute them; gscale f32 [rows]."""
    rows, V = x.shape
    zf = torch.tensor(z, dtype=F32)
    xf = x.to(F32)
    m = xf.amax(1, keepdim=True)
    lse = (m + torch.log(torch.exp(xf - m).sum(1, keepdim=True))).squeeze(1)
    valid = tgt != ignore
    bad = valid & ((tgt < 0) | (tgt >= V))
    lse = torch.where(bad, torch.full_like(lse, math.nan), lse)
    xt = xf[torch.arange(rows), tgt.clamp(0, V - 1)]
    zon = float(zf) > 0
    ls = R._rne(lse) if fault == "lse_bf16_before_square" else lse
    rz_all = (zf * ls if fault == "row_z_linear" else zf * (ls * ls)) if zon else torch.zeros(rows)
    rz = torch.where(valid, rz_all, torch.zeros(rows))
    loss = torch.where(valid, lse - xt, torch.zeros(rows))
    if zon:
        loss = torch.where(valid, loss + rz, loss)
    if fault == "z_not_in_row_z":
        rz = torch.zeros(rows)
    if fault == "ignored_row_z_nonzero":
        rz = rz_all
    gs = gscale.to(F32)
    g = torch.where(valid, gs, gs * 2.0 ** -9 if fault == "ignored_row_grad_nonzero" else torch.zeros(rows))[:, None]
    two = 1.0 if fault == "factor_missing_2" else 2.0
    c = torch.where(valid, 1 + (two * zf) * lse, torch.ones(rows))[:, None] if zon and fault != "grad_without_z" \
        else torch.ones(rows, 1)
    p = torch.exp(xf - lse[:, None])
    onehot = (torch.arange(V)[None, :] == tgt[:, None]).to(F32)
    grad = (p - onehot) * c * g if fault == "factor_on_onehot" else (p * c - onehot) * g
    return loss, rz, lse, grad.to(BF)
