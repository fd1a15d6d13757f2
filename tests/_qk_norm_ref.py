"""Conformance kit of csrc/qk_norm.hip (per-head QK-norm fused with RoPE), built on tests/_row_ref.py:
its notation (u, e, g(n), HW, SECOND, B16, FLIP), input families, checkers and its derivation of the
RMSNorm bounds are used as they are; only what differs for d-wide head rows is stated here.  CPU only.

The head rows.  The first nq + nk heads of every token row are `rows * heads` independent RMSNorm rows
of d = head_dim columns; q heads take the weight wq, k heads wk.  The references work on those
[rows * heads, d] matrices (split_heads / join_heads move between the two layouts).

The addition count.  The kernel's sum of squares (and the backward's sum of p xh) is NOT the 64-lane
row sum _row_ref._adds describes: a lane owns 16 of the head's columns -- chunk c of the first half,
then chunk c of the second half -- and adds their 16 products in sequence (15 additions: the first
lands on 0), and the d / 16 lanes of the head then combine in log2(d / 16) butterfly levels
(__shfl_xor 1, 2 and, at d = 128, 4).  The longest path has

        A(d) = 15 + log2(d / 16)  additions:   17 at d = 64,  18 at d = 128

(_row_ref._adds(64) = 14 would be too few).  With that A the bounds are _row_ref's, term for term:

    forward    E_r = (g(A + 1) + 3 e) / 2 + HW         (1 / d is a power of two: its e is not used)
               mode 0  y = bf16(x rstd w):      E32 = |t| (E_r + 2 e)
               mode 1  y = bf16(w bf16(x rstd)): |y - w qb| <= u |w qb| + (1 + u) |w| FLIP(q, |q| (E_r + e))
    backward   E_dot = g(A + 4) mass / d,  mass = sum |p xh|
               dx:  E32 = rstd (|xh| E_dot + 2 e |xh dot| + e (|p| + |xh dot|)) + e |o|
               dw[c] = the sum over the rows * heads head rows of one weight: E_dw = g(n + 2) sum |dy xh|
               (+ sum |dy| FLIP(xh) in mode 1), n = rows * heads terms in any order -- a thread's own
               units in sequence, the workgroup's threads through LDS, pt_rmsnorm_colsum_batch.

The rotation.  The kernel rounds y to bf16 and then rotates it exactly as csrc/rope.hip does, so the
fused output is checked by bits against pt_rope applied to the kernel's own norm-only output (and
rstd by bits between the two runs); no bound is involved.

The bit-mismatch cap BIT_CAP applies to CAPPED = randn, rowscale, tiny, cancel.  `spike` (one 64.0 in
a row of 2^-10-sized values) is judged by the per-element bound only: at 64 columns, mode 0, a correct
fp32 evaluation differs from the float64-sequenced expectation in 0.9 % - 1.3 % of the y elements and
2 - 3e-3 of dx (the spike's square sits on an f32 rounding boundary of the sum, and every other
element of the row follows rstd), which would trip the cap on correct code; it stays inside the bounds.

emu_qk_fwd / emu_qk_bwd evaluate the kernel's formulas in fp32 in the kernel's own summation order,
on the q|k|v layout, with injectable faults (FWD_FAULTS, BWD_FAULTS).
"""
import math

import torch

from tests import _row_ref as R

BF, F32, F64 = R.BF, R.F32, R.F64
CAPPED = ("randn", "rowscale", "tiny", "cancel")
FAMILIES = R.NORM_FAMILIES
FWD_FAULTS = ("k_uses_q_weight", "neighbour_rstd", "ss_drops_last_chunk", "rope_before_rounding", "v_touched")
BWD_FAULTS = ("dw_skips_last_head", "dot_without_w", "k_uses_q_weight", "neighbour_rstd")


def adds(d):
    """Additions on the longest path of the kernel's d-column sums: 15 in the lane, log2(d / 16) levels."""
    return 15 + int(math.log2(d // 16))


# ------------------------------------------------------------------------------ layouts and cases
def split_heads(t, nq, nk, d):
    """[rows, >= (nq + nk) d] -> (q head rows [rows * nq, d], k head rows [rows * nk, d]), contiguous."""
    rows = t.shape[0]
    return (t[:, :nq * d].reshape(rows * nq, d).contiguous(),
            t[:, nq * d:(nq + nk) * d].reshape(rows * nk, d).contiguous())


def join_heads(q, k, rows, nq, nk, d):
    return torch.cat([q.reshape(rows, nq * d), k.reshape(rows, nk * d)], 1)


def make_qk_case(family, rows, nq, nk, d, seed=0):
    """One family as q|k|v rows: dict x, dy [rows, (nq + 2 nk) d] bf16 whose v columns hold the NaN
    sentinel, wq, wk [d], and the head-row matrices xq, xk, dyq, dyk the references take."""
    cq = R.make_norm_case(family, rows * nq, d, seed)
    ck = R.make_norm_case(family, rows * nk, d, seed + 1)
    v = R.sentinel_cpu((rows, nk * d), BF)
    x = torch.cat([join_heads(cq["x"], ck["x"], rows, nq, nk, d), v], 1)
    dy = torch.cat([join_heads(cq["dy"], ck["dy"], rows, nq, nk, d), v], 1)
    return dict(x=x, dy=dy, wq=cq["w"], wk=ck["w"], xq=cq["x"], xk=ck["x"], dyq=cq["dy"], dyk=ck["dy"],
                rows=rows, nq=nq, nk=nk, d=d, family=family)


def make_tables(seq_len, d, seed=0):
    """bf16 cos / sin [seq_len, d] of real angles, the two halves equal (get_cos_sin's layout)."""
    g = R._gen("qk tables", seq_len, d, seed)
    ang = torch.rand(seq_len, d // 2, generator=g, dtype=F64) * 2 * math.pi
    return torch.cos(ang).repeat(1, 2).to(BF), torch.sin(ang).repeat(1, 2).to(BF)


# ------------------------------------------------------------------------------ float64 references
def ref_fwd(x, w, eps, mode):
    """Float64-sequenced norm of head rows x [n, d] with weight w [d].  dict: rstd, rstd_bound, y_ref
    (unrounded target), y_want (bf16), y_bound, y_alts -- _row_ref.ref_norm_fwd with A = adds(d)."""
    d = x.shape[1]
    xx, w6 = x.to(F64), w.to(F64)[None, :]
    eps32 = float(torch.tensor(eps, dtype=F32))
    rstd = 1.0 / torch.sqrt((xx * xx).sum(1) / d + eps32)
    e_r = ((R.gamma(adds(d) + 1) + 3 * R.E) / 2 + R.HW) * R.SECOND
    out = dict(rstd=rstd, rstd_bound=rstd * e_r)
    rs = rstd[:, None]
    if mode == 0:
        t = xx * rs * w6
        out.update(y_ref=t, y_want=R._bf(t).to(BF), y_bound=R.b16(t, t.abs() * (e_r + 2 * R.E) * R.SECOND), y_alts=())
    else:
        q = xx * rs
        qb, flip, up, dn = R.round_info(q, q.abs() * (e_r + R.E) * R.SECOND)
        t = w6 * qb
        out.update(y_ref=t, y_want=R._bf(t).to(BF), y_bound=R.hu(t) + (1 + R.U) * w6.abs() * flip,
                   y_alts=(R._bf(w6 * up).to(BF), R._bf(w6 * dn).to(BF)))
    return out


def ref_bwd(dy, x, w, rstd, mode):
    """Float64-sequenced backward of head rows from the f32 rstd the forward saved.  dict: dx_ref, dx_want,
    dx_bound, dx_flip, dw (float64 column sums over the n head rows), dw_err -- _row_ref.ref_norm_bwd
    with A = adds(d) and no dres."""
    n, d = x.shape
    A = adds(d)
    xx, g, w6, rs = x.to(F64), dy.to(F64), w.to(F64)[None, :], rstd.to(F64)[:, None]
    p, xh = g * w6, xx * rs
    dot = (p * xh).sum(1, keepdim=True) / d
    mass = (p * xh).abs().sum(1, keepdim=True)
    e_dot = R.gamma(A + 4) * mass / d
    o = rs * (p - xh * dot)
    e32 = (rs * (xh.abs() * e_dot + 2 * R.E * (xh * dot).abs() + R.E * (p.abs() + (xh * dot).abs())) + R.E * o.abs()) * R.SECOND
    if mode == 0:
        gterm, e_dw = g * xh, R.gamma(n + 2) * (g * xh).abs().sum(0)
    else:
        xb, flip, _, _ = R.round_info(xh, xh.abs() * R.E * R.SECOND)
        gterm = g * xb
        e_dw = R.gamma(n + 2) * gterm.abs().sum(0) + (g.abs() * flip).sum(0)
    return dict(dx_ref=o, dx_want=R._bf(o).to(BF), dx_bound=R.b16(o, e32), dx_flip=R.round_info(o, e32)[1],
                dw=gterm.sum(0), dw_err=e_dw * R.SECOND)


def ref_case_fwd(c, eps, mode):
    """(q reference, k reference) of a make_qk_case dict."""
    return ref_fwd(c["xq"], c["wq"], eps, mode), ref_fwd(c["xk"], c["wk"], eps, mode)


def rstd_heads(rstd, rows, nq, nk):
    """rstd [rows, nq + nk] -> (q head rows' [rows * nq], k head rows' [rows * nk])."""
    return rstd[:, :nq].reshape(rows * nq), rstd[:, nq:nq + nk].reshape(rows * nk)


# ------------------------------------------------------------------------------ checks on the q|k|v layout
def check_forward(c, y, rstd, eps, mode, tag, bits=None):
    """y [rows, >= (nq + nk) d] bf16 (the norm-only output) and rstd [rows, nq + nk] f32 of case c against
    the reference: per-element bounds on every family, the bit condition on the capped ones."""
    rows, nq, nk, d = c["rows"], c["nq"], c["nk"], c["d"]
    bits = c["family"] in CAPPED if bits is None else bits
    yq, yk = split_heads(R._cpu(y), nq, nk, d)
    rq, rk = rstd_heads(R._cpu(rstd), rows, nq, nk)
    for nm, yy, rr, ref in zip("qk", (yq, yk), (rq, rk), ref_case_fwd(c, eps, mode)):
        R.check(f"{nm} rstd", rr, ref["rstd"], ref["rstd_bound"], tag)
        R.check(f"{nm} y mode {mode}", yy, ref["y_ref"], ref["y_bound"], tag)
        if bits:
            R.check_bits(f"{nm} y mode {mode}", yy, ref["y_want"], ref["y_alts"], tag=tag)


def check_backward(c, dx, rstd, mode, tag, bits=None):
    """dx [rows, >= (nq + nk) d] bf16 against the reference from the f32 rstd [rows, nq + nk] the forward
    saved.  Returns the (q, k) reference dicts (dw, dw_err for the sinks)."""
    rows, nq, nk, d = c["rows"], c["nq"], c["nk"], c["d"]
    bits = c["family"] in CAPPED if bits is None else bits
    dq, dk = split_heads(R._cpu(dx), nq, nk, d)
    rq, rk = rstd_heads(R._cpu(rstd), rows, nq, nk)
    refs = (ref_bwd(c["dyq"], c["xq"], c["wq"], rq, mode), ref_bwd(c["dyk"], c["xk"], c["wk"], rk, mode))
    for nm, dd, ref in zip("qk", (dq, dk), refs):
        R.check(f"{nm} dx mode {mode}", dd, ref["dx_ref"], ref["dx_bound"], tag)
        if bits:
            R.check_bits(f"{nm} dx mode {mode}", dd, ref["dx_want"], tag=tag, flip=ref["dx_flip"])
    return refs


def check_untouched(name, buf, width):
    """Every bf16 element of buf [rows, stride] from column `width` on still holds the NaN sentinel's bits."""
    tail = R.ibits(R._cpu(buf))[:, width:]
    assert bool((tail == R.NAN16).all()), f"{name}: bytes beyond the q|k heads were written"


# ------------------------------------------------------------------------------ fp32 emulator
def _lane_sum(t, d):
    """The kernel's sum over a head row's d columns of t [n, d] f32: each of the d / 16 lanes adds chunk c
    of the first half then chunk c of the second half in sequence, then the butterfly over the lanes."""
    n, cph = t.shape[0], d // 16
    lanes = torch.cat([t[:, :d // 2].reshape(n, cph, 8), t[:, d // 2:].reshape(n, cph, 8)], 2)   # [n, cph, 16]
    s = torch.zeros(n, cph, dtype=F32)
    for j in range(16):
        s = s + lanes[:, :, j]
    o = 1
    while o < cph:
        s = s + s[:, torch.arange(cph) ^ o]
        o <<= 1
    return s[:, 0]


def _weights(wq, wk, rows, nq, nk, fault):
    wk_ = wq if fault == "k_uses_q_weight" else wk
    return torch.cat([wq.to(F32).expand(nq, -1), wk_.to(F32).expand(nk, -1)], 0)[None].expand(rows, -1, -1)


def emu_qk_fwd(x, nq, nk, d, wq, wk, eps, mode, cos=None, sin=None, seq_len=None, fault=None):
    """(y bf16 [rows, stride] with every column past the q|k heads as in x, rstd f32 [rows, nq + nk]) as the
    kernel computes them, in fp32 torch.  cos / sin: the fused form (the bf16 y rotated as csrc/rope.hip)."""
    rows, nh = x.shape[0], nq + nk
    xh = x[:, :nh * d].to(F32).reshape(rows * nh, d)
    sq = xh * xh
    if fault == "ss_drops_last_chunk":
        sq = torch.cat([sq[:, :d - 8], torch.zeros(rows * nh, 8)], 1)
    rstd = torch.rsqrt(_lane_sum(sq, d) * torch.tensor(1.0 / d, dtype=F32) + eps).reshape(rows, nh)
    rs = (rstd.roll(-1, 1) if fault == "neighbour_rstd" else rstd)[:, :, None]
    w = _weights(wq, wk, rows, nq, nk, fault)
    xv = xh.reshape(rows, nh, d)
    y = xv * rs * w if mode == 0 else w * R._rne(xv * rs)
    out = x.clone()
    if cos is not None:
        half = d // 2
        pos = torch.arange(rows) % seq_len
        c, s = cos.to(F32)[pos, :half][:, None, :], sin.to(F32)[pos, :half][:, None, :]
        yb = y if fault == "rope_before_rounding" else R._rne(y)
        a, b = yb[..., :half], yb[..., half:]
        y = torch.cat([a * c - b * s, b * c + a * s], -1)
    out[:, :nh * d] = y.to(BF).reshape(rows, nh * d)
    if fault == "v_touched":
        out[:, nh * d:nh * d + 8] = 0
    return out, rstd


def emu_qk_bwd(dy, x, nq, nk, d, wq, wk, rstd, mode, fault=None, units_per_block=64):
    """(dx bf16 [rows, stride], later columns as in dy; dwq, dwk f32 [d]) in fp32 torch: per-block partial
    sums of units_per_block head rows in sequence, then their sum."""
    rows, nh = x.shape[0], nq + nk
    g = dy[:, :nh * d].to(F32).reshape(rows, nh, d)
    xv = x[:, :nh * d].to(F32).reshape(rows, nh, d)
    w = _weights(wq, wk, rows, nq, nk, fault)
    rs = (rstd.roll(-1, 1) if fault == "neighbour_rstd" else rstd).to(F32)[:, :, None]
    xh = xv * rs
    dterm = g * xh if fault == "dot_without_w" else g * w * xh
    dot = (_lane_sum(dterm.reshape(rows * nh, d), d) * torch.tensor(1.0 / d, dtype=F32)).reshape(rows, nh, 1)
    o = rs * (g * w - xh * dot)
    out = dy.clone()
    out[:, :nh * d] = o.to(BF).reshape(rows, nh * d)
    gterm = g * (xh if mode == 0 else R._rne(xh))
    dws = []
    for lo, hi in ((0, nq), (nq, nh)):
        if fault == "dw_skips_last_head":
            hi -= 1
        t = gterm[:, lo:hi].reshape(-1, d)
        parts = [t[i:i + units_per_block].sum(0) for i in range(0, t.shape[0], units_per_block)] or [torch.zeros(d)]
        dws.append(torch.stack(parts).sum(0))
    return out, dws[0], dws[1]


# ------------------------------------------------------------------------------ torch autograd reference
def rotate(y, cos, sin, seq_len):
    """RoPE of head rows y [rows, heads, d] (any float dtype), position = row % seq_len."""
    half = y.shape[-1] // 2
    pos = torch.arange(y.shape[0]) % seq_len
    c, s = cos.to(y.dtype)[pos, :half][:, None, :], sin.to(y.dtype)[pos, :half][:, None, :]
    a, b = y[..., :half], y[..., half:]
    return torch.cat([a * c - b * s, b * c + a * s], -1)


def autograd_qk(c, eps, mode, cos, sin, seq_len, dtype=F32):
    """Per-head RMSNorm + RoPE in plain torch with autograd, fed the output gradient rotate(dy) so that the
    gradient reaching the norm output is dy up to the tables' rounding (cos^2 + sin^2 = 1 to their
    precision).  mode 1's inner bf16 rounding is a straight-through identity, as in the kernel's formula.
    Returns (dx [rows, (nq + nk) d], dwq [d], dwk [d]) in `dtype`."""
    rows, nq, nk, d = c["rows"], c["nq"], c["nk"], c["d"]
    nh = nq + nk
    x = c["x"][:, :nh * d].to(dtype).reshape(rows, nh, d).requires_grad_(True)
    wq, wk = c["wq"].to(dtype).requires_grad_(True), c["wk"].to(dtype).requires_grad_(True)
    w = torch.cat([wq.expand(nq, -1), wk.expand(nk, -1)], 0)[None]
    xh = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    if mode == 1:
        xh = xh + (xh.detach().to(BF).to(dtype) - xh.detach())
    out = rotate(xh * w, cos, sin, seq_len)
    gout = rotate(c["dy"][:, :nh * d].to(dtype).reshape(rows, nh, d), cos, sin, seq_len)
    out.backward(gout)
    return x.grad.reshape(rows, nh * d), wq.grad, wk.grad
