"""Conformance kit for the GEMM's fused epilogues (csrc/gemm.hip: EPI_SWIGLU_FWD 5, EPI_SWIGLU_BWD 6,
EPI_ROPE 7, EPI_CE_STATS 8): tests/_gemm_ref.py's exact accumulators (G) composed with tests/_row_ref.py's
references, bounds and checkers (R).  CPU only; self-tested in tests/test_gemm_epi_checker_cpu.py.

The method: on an exact family every f32 accumulator is the float64 product, in any summation order and
on any MFMA, so bf16(acc) -- what every one of these epilogues stages before it applies its function --
is known bit for bit, and the row kit's float64 reference is evaluated on those exact bf16 inputs.  A
mistake in code that the fused epilogue and the stand-alone row kernel share cannot hide here.

Families (`make_case`, A [M, K], B [K, N] logical, as in G)
    ints       G's: integers in [-15, 15].  Sums of several hundred: used for RoPE, where magnitude does
               not matter.
    ints_unit  ints with A scaled by 2^-7: every accumulator is a multiple of 2^-7 below 2^17, exact in
               f32 in any order, and bf16(acc) lands where sigmoid, exp and the bf16 roundings are not
               saturated: at K = 64 the median |bf16(acc)| is 3.4 and 89 % of the values are below 8;
               46 % of the accumulators are not bf16 numbers and 22 % are bf16 ties.  For K <= 192
               (SwiGLU forward, CE); the SwiGLU backward's accumulator is dh, which nothing
               saturates, at any K.
Constructions (every one asserts its own exactness)
    all_g      forward: K = 256, A holds a 1 at k = m mod 256 and B_gate = R.all_g() with the bf16
               subnormal patterns replaced by zero (what the MFMA does with subnormal operands is not
               stated anywhere in the project; the stand-alone kernel's suite covers those patterns),
               so the gate accumulator of each 256-row block is every normal bf16 pattern (-0 arrives
               as +0).  Row 255 of R.all_g() is its zero padding, so column 255 of A is free: it holds
               R.ALL_G_VALUES per 256-row block against B_up = a 1 in row 255, which makes u that
               constant.  backward: dh = R.ALL_G_DH per block as a rank-1 product (column 0 of dY times
               a row of ones), g|u = R.make_swiglu_case("all_g") passed as the residual.
    offset     CE: one more K-tile whose first column of A is 1 against a row of B holding per-column
               integer offsets.  "offset": wave quarter 1 + b mod (waves - 1) of block b sits 80 above the
               rest (the merge's exp(m_w - M) is e^-80 for every other quarter, and the maximum is never
               the first wave's); "offset_low": the whole row at -96.
    flat       CE: the columns of B inside a block are copies of the block's first, so every logit of a
               row and block is equal and sumexp == block exactly.

Expected values, from acc = the float64 product
    SwiGLU forward   g|u = bf16(acc) by bits; h: R.ref_swiglu_fwd(g, u) -- within h_bound, and the
                     sequenced bit condition (R.check_bits, h_alts, R.BIT_CAP).
    SwiGLU backward  dh = bf16(acc); dg, du: R.ref_swiglu_bwd(dh, g, u) with g|u the residual: the same
                     two-part check.
    RoPE             R.ref_rope on bf16(acc) over columns [0, rot_cols), tables on R.grid64; bf16(acc)
                     beyond.  By bits: `assert_rope_exact` checks that the unrounded a c - b s and
                     b c + a s are f32 numbers (true for ints and ints_unit at K = 64, 192, 512).
    CE statistics    per row and block b of `block` columns: max = the maximum of the expected bf16
                     logits, by bits; sumexp = the float64 sum of exp(x - max), bound below.

The sumexp bound (R's notation: E = 2^-24 one f32 rounding, HW = 2^-22 a hardware unit, gamma(n) n
roundings along one path, SECOND the second-order factor, TINY = 2^-126 a flushed result; no slack
factor).  A wave holds 64 columns of a row; m_w their maximum, t_i = exp(x_i - m_w), s_w = sum t_i:
    term      exp2(fma(x_i, log2e, -m_w log2e)): style "fma", relative ARG_i = E (|x_i| + 2 X + |d_i|),
              X = max |x| over the wave's 64 columns, d_i = x_i - m_w; plus HW for v_exp, TINY if flushed
    wave sum  8 in-lane additions (the lane's 8 columns onto 0) and 3 butterfly levels: gamma(11)
        E_w = sum_i t_i (ARG_i + HW) + gamma(11) s_w + 64 TINY
    merge     S = sum_w s_w exp(m_w - M) over the block's W = block / 64 waves: one __expf (style "sub":
              3 E |m_w - M|, + HW), one product (E) and one addition per wave (gamma(W) on the sum)
        E_S = SECOND (sum_w e^(m_w - M) (E_w + s_w (3 E |m_w - M| + HW + E)) + gamma(W) S + W TINY)
(20 first-order terms: below the 2^6 SECOND allows for.)

Emulators (fp32 torch, on the exact f32 accumulator) with one injectable fault each -- FAULTS.
"""
import functools

import torch

from tests import _gemm_ref as G
from tests import _row_ref as R

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPI_SWIGLU_FWD, EPI_SWIGLU_BWD, EPI_ROPE, EPI_CE_STATS = 5, 6, 7, 8
FAMILIES = ("ints", "ints_unit")
CE_FAMILIES = ("ints_unit", "offset", "offset_low", "flat")
HEAD = 64                  # EPI_ROPE's head_dim: the wave tile's width
OFFSET_HIGH, OFFSET_LOW = 80.0, -96.0

SWIGLU_EPI_FAULTS = ("f_on_unrounded_acc", "up_from_gate_columns", "gu_ld_as_width")
ROPE_EPI_FAULTS = ("rope_pos_tile_local", "rope_partner_16", "rope_ignores_rot_cols", "rope_boundary_block_tile")
STATS_FAULTS = ("stats_of_unrounded", "stats_row_major", "stats_drops_a_wave", "stats_max_of_first_wave")
FAULTS = SWIGLU_EPI_FAULTS + ROPE_EPI_FAULTS + STATS_FAULTS


def _exact(t64, dtype):
    out = t64.to(dtype)
    assert torch.equal(out.to(F64), t64), f"not exact in {dtype}"
    return out


# ------------------------------------------------------------------------------ families
def make_case(family, M, N, K, seed=0):
    """bf16 CPU (a [M, K], b [K, N])."""
    if family not in FAMILIES:
        raise KeyError(family)
    a, b = G.make_case("ints", M, N, K, seed)
    if family == "ints_unit":
        a = _exact(a.to(F64) * 2.0 ** -7, BF)
    return a, b


def product(a, b):
    """The float64 product, asserted to be an f32 number element by element (the exact accumulator)."""
    acc = G.ref_product(a, b)[0]
    assert torch.equal(acc.to(F32).to(F64), acc), "an accumulator is not exact in f32"
    return acc


def bf(acc):
    """bf16(acc): the epilogues' staging of an exact f32 accumulator."""
    return acc.to(F32).to(BF)


def all_g_normal():
    """R.all_g() with the bf16 subnormal patterns replaced by zero."""
    g = R.all_g()
    mag = R.ibits(g).to(torch.int32) & 0x7FFF
    return torch.where((mag != 0) & (mag < 0x0080), torch.zeros_like(g), g)


def make_all_g_fwd():
    """(a [768, 256], b [256, 512] = gate | up): see the module docstring."""
    pat = all_g_normal()
    assert not bool(R.ibits(pat[255]).any()), "row 255 of all_g is its zero padding"
    rows = torch.arange(768)
    a = torch.zeros(768, 256, dtype=F64)
    a[rows, rows % 256] = 1.0
    a[:, 255] = torch.tensor(R.ALL_G_VALUES, dtype=F64).repeat_interleave(256)
    wu = torch.zeros(256, 256, dtype=F64)
    wu[255] = 1.0
    a16, b16 = _exact(a, BF), torch.cat([pat, _exact(wu, BF)], 1)
    gu = bf(product(a16, b16))
    want_g = pat.repeat(3, 1)
    neg0 = R.ibits(want_g) == -32768
    assert torch.equal(R.ibits(gu[:, :256])[~neg0], R.ibits(want_g)[~neg0]) and not bool(R.ibits(gu[:, :256])[neg0].any())
    assert torch.equal(gu[:, 256:].to(F64), a[:, 255:256].expand(768, 256))
    return a16, b16


def make_all_g_bwd():
    """(dy [768, 256], w_down [256, 256], gu [768, 512]): dh = R.ALL_G_DH per 256-row block."""
    g, u, dh = R.make_swiglu_case("all_g")
    dy = torch.zeros(768, 256, dtype=F64)
    dy[:, 0] = torch.tensor(R.ALL_G_DH, dtype=F64).repeat_interleave(256)
    w = torch.zeros(256, 256, dtype=F64)
    w[0] = 1.0
    dy16, w16 = _exact(dy, BF), _exact(w, BF)
    assert torch.equal(R.ibits(bf(product(dy16, w16))), R.ibits(dh))
    return dy16, w16, torch.cat([g, u], 1)


def make_ce_case(family, M, N, K, block, seed=0):
    """bf16 CPU (a [M, K'], b [K', N]) of a CE family; K' = K + 64 for the offset families."""
    if family not in CE_FAMILIES:
        raise KeyError(family)
    a, b = make_case("ints_unit", M, N, K, seed)
    col = torch.arange(N)
    if family == "flat":
        return a, b[:, col // block * block].contiguous()
    if family == "ints_unit":
        return a, b
    waves = block // 64
    if family == "offset":
        off = torch.where(col % block // 64 == 1 + col // block % (waves - 1), OFFSET_HIGH, 0.0).to(F64)
    else:
        off = torch.full((N,), OFFSET_LOW, dtype=F64)
    a2 = torch.zeros(M, 64, dtype=F64)
    a2[:, 0] = 1.0
    b2 = torch.zeros(64, N, dtype=F64)
    b2[0] = off
    return torch.cat([a, _exact(a2, BF)], 1), torch.cat([b, _exact(b2, BF)], 0)


def rope_tables(seq_len, seed=0):
    """(cos, sin) [seq_len, 64] bf16 on the 1/64 grid."""
    g = R._gen("gemm-rope", seq_len, seed)
    return R.grid64((seq_len, HEAD), g), R.grid64((seq_len, HEAD), g)


# ------------------------------------------------------------------------------ expectations
def expect_swiglu_fwd(acc):
    """acc float64 [M, 2 I] = gate | up.  dict gu (bf16, by bits) + R.ref_swiglu_fwd's."""
    I = acc.shape[1] // 2
    gu = bf(acc)
    return dict(gu=gu, **R.ref_swiglu_fwd(gu[:, :I], gu[:, I:]))


def expect_swiglu_bwd(acc, gu):
    """acc float64 [M, I] = dh, gu bf16 [M, 2 I] the residual.  dict dh + R.ref_swiglu_bwd's."""
    I = acc.shape[1]
    dh = bf(acc)
    return dict(dh=dh, **R.ref_swiglu_bwd(dh, gu[:, :I], gu[:, I:]))


def assert_rope_exact(x, cos, sin, seq_len, rot_cols):
    """The unrounded a c - b s and b c + a s of every rotated pair are f32 numbers."""
    rows = x.shape[0]
    pos = torch.arange(rows) % seq_len
    c, s = (t.to(F64)[pos, :HEAD // 2][:, None, :] for t in (cos, sin))
    v = x[:, :rot_cols].to(F64).reshape(rows, -1, HEAD)
    a, b = v[..., :HEAD // 2], v[..., HEAD // 2:]
    for t in (a * c - b * s, b * c + a * s):
        assert torch.equal(t.to(F32).to(F64), t), "a rotated value is not exact in f32"


def expect_rope(acc, cos, sin, seq_len, rot_cols):
    """The whole bf16 [M, N] output, by bits."""
    x = bf(acc)
    if rot_cols == 0:
        return x
    assert_rope_exact(x, cos, sin, seq_len, rot_cols)
    return R.ref_rope(x, rot_cols // HEAD, HEAD, cos, sin, seq_len)


def expect_stats(x, block):
    """x: the expected bf16 logits [M, N].  dict max f32 [nblk, M] (by bits), sumexp float64 [nblk, M], bound."""
    M, N = x.shape
    nblk, W = N // block, block // 64
    xv = x.to(F64).reshape(M, nblk, W, 64)
    mw = xv.amax(3, keepdim=True)
    d = xv - mw
    t = torch.exp(d)
    sw = t.sum(3)
    arg = R._arg_err(xv.reshape(-1, 64), mw.reshape(-1, 1), d.reshape(-1, 64), "fma").reshape(xv.shape)
    e_w = (t * (arg + R.HW)).sum(3) + R.gamma(11) * sw + 64 * R.TINY
    mw = mw.squeeze(3)
    Mb = mw.amax(2, keepdim=True)
    dw = mw - Mb
    f = torch.exp(dw)
    S = torch.exp(xv - Mb[..., None]).sum((2, 3))
    e_S = (f * (e_w + sw * (3 * R.E * dw.abs() + R.HW + R.E))).sum(2) + R.gamma(W) * S + W * R.TINY
    return dict(max=Mb.squeeze(2).t().contiguous().to(F32), sumexp=S.t().contiguous(),
                bound=(e_S * R.SECOND).t().contiguous(), block=block)


# ------------------------------------------------------------------------------ the cases, computed once and shared
SWIGLU_FWD_SHAPES = ((256, 128, 64), (512, 384, 192))                 # (M, I, K)
SWIGLU_BWD_SHAPES = ((256, 256, 64), (512, 512, 128))                 # (M, I, H)
SWIGLU_DUAL_SHAPE = (512, 1024, 512)                                  # 8 tiles of 256 x 256 per group
ALL_G_SHAPE = (768, 256, 256)
ROPE_SHAPES = ((512, 384, 256, 128), (512, 384, 192, 64), (512, 384, 384, 512), (512, 384, 0, 128),
               (1024, 768, 512, 256))                                 # (M, N, rot_cols, seq_len)
ROPE_KS = (64, 192)
CE_SHAPES = ((256, 256, 256), (512, 512, 256), (256, 384, 128))       # (M, N, block)
CE_KS = (64, 128)


@functools.lru_cache(maxsize=None)
def fwd_case(family, M, I, K):
    """(a [M, K], b [K, 2 I] = gate | up, acc32, expectation) of the SwiGLU forward."""
    if family == "all_g":
        assert (M, I, K) == ALL_G_SHAPE
        a, b = make_all_g_fwd()
    else:
        a, b = make_case(family, M, 2 * I, K)
    acc = product(a, b)
    return a, b, acc.to(F32), expect_swiglu_fwd(acc)


@functools.lru_cache(maxsize=None)
def bwd_case(family, M, I, H):
    """(dy [M, H], w_down [H, I], g|u [M, 2 I], acc32, expectation) of the SwiGLU backward."""
    if family == "all_g":
        assert (M, I, H) == ALL_G_SHAPE
        a, b, gu = make_all_g_bwd()
    else:
        a, b = make_case(family, M, I, H)
        g, u, _ = R.make_swiglu_case("randn", M, I)
        gu = torch.cat([g, u], 1)
    acc = product(a, b)
    return a, b, gu, acc.to(F32), expect_swiglu_bwd(acc, gu)


@functools.lru_cache(maxsize=None)
def rope_case(family, M, N, K, rot_cols, seq_len):
    """(a, b, cos, sin, acc32, the expected bf16 output)."""
    a, b = make_case(family, M, N, K)
    cos, sin = rope_tables(seq_len)
    acc = product(a, b)
    return a, b, cos, sin, acc.to(F32), expect_rope(acc, cos, sin, seq_len, rot_cols)


@functools.lru_cache(maxsize=None)
def ce_case(family, M, N, K, block):
    """(a, b, acc32, the expected bf16 logits, expect_stats of them)."""
    a, b = make_ce_case(family, M, N, K, block)
    acc = product(a, b)
    x = bf(acc)
    return a, b, acc.to(F32), x, expect_stats(x, block)


# ------------------------------------------------------------------------------ checks (CPU self-test and GPU test alike)
def check_swiglu_fwd(name, h, gu, exp, tag=None):
    """g|u by bits; h within its bound and under the sequenced bit condition.  Returns the bit share."""
    G.check_exact(f"{name} g|u", gu, exp["gu"])
    R.check("h", h, exp["h_ref"], exp["h_bound"], tag)
    return R.check_bits("h", h, exp["h_want"], exp["h_alts"], exp["floor"], tag=tag)


def check_swiglu_bwd(name, dgu, exp, tag=None):
    """dg|du [M, 2 I]: both within their bounds and under the sequenced bit condition."""
    I = dgu.shape[1] // 2
    dg, du = G._cpu(dgu)[:, :I], G._cpu(dgu)[:, I:]
    R.check("dg", dg, exp["dg_ref"], exp["dg_bound"], tag)
    R.check("du", du, exp["du_ref"], exp["du_bound"], tag)
    return max(R.check_bits("du", du, exp["du_want"], exp["du_alts"], exp["floor"], tag=tag),
               R.check_bits("dg", dg, exp["dg_want"], (), exp["floor"], tag=tag))


def check_rope(name, got, want):
    return G.check_exact(name, got, want)


def check_stats(name, stats, exp, tag=None):
    """stats: the flat f32 buffer, read tile-major as [nblk, M, (max, sumexp)]: every pair written, max by
    bits, sumexp within the bound."""
    nblk, M = exp["max"].shape
    st = G._cpu(stats).reshape(nblk, M, 2)
    assert bool(torch.isfinite(st).all()), f"{name}: {int((~torch.isfinite(st)).sum())} statistics not written or not finite"
    G.check_exact(f"{name} max", st[..., 0].contiguous(), exp["max"])
    return R.check("sumexp", st[..., 1], exp["sumexp"], exp["bound"], tag)


# ------------------------------------------------------------------------------ fp32 emulators
_rne = G._rne
LOG2E = torch.tensor(1.4426950408889634, dtype=F32)


def emu_swiglu_fwd(acc32, fault=None):
    """(h, g|u) bf16 from the f32 accumulator [M, 2 I]."""
    I = acc32.shape[1] // 2
    gu = _rne(acc32)
    src = acc32 if fault == "f_on_unrounded_acc" else gu
    g, u = src[:, :I], src[:, I:]
    if fault == "up_from_gate_columns":
        u, gu = g, torch.cat([gu[:, :I], gu[:, :I]], 1)
    h, _, _ = R.emu_swiglu(g, u, torch.zeros_like(g))
    return h, gu.to(BF)


def emu_swiglu_bwd(acc32, res_full, region, fault=None):
    """dg|du bf16 [M, 2 I] from the f32 accumulator dh [M, I] and the residual g|u = res_full[region]
    (G.padded's allocation: the gaps and guard rows hold the NaN sentinel)."""
    M, I = acc32.shape
    gu = res_full[region]
    if fault == "gu_ld_as_width":
        first = region[0].start * res_full.stride(0)
        gu = res_full.reshape(-1)[first:first + M * 2 * I].reshape(M, 2 * I)
    dh = acc32 if fault == "f_on_unrounded_acc" else _rne(acc32)
    g, u = gu[:, :I].to(F32), gu[:, I:].to(F32)
    if fault == "up_from_gate_columns":
        u = g
    _, dg, du = R.emu_swiglu(g, u, dh)
    return torch.cat([dg, du], 1)


def emu_rope(acc32, cos, sin, seq_len, rot_cols, fault=None, tile_rows=128):
    """bf16 [M, N] from the f32 accumulator; tile_rows: the wave tile rope_pos_tile_local counts in."""
    M, N = acc32.shape
    x = acc32 if fault == "f_on_unrounded_acc" else _rne(acc32)
    rot = rot_cols
    if fault == "rope_ignores_rot_cols":
        rot = N
    if fault == "rope_boundary_block_tile":
        rot = min(N, -(-rot_cols // 128) * 128)
    out = _rne(acc32).clone()
    if rot == 0:
        return out.to(BF)
    rr = torch.arange(M)
    pos = rr % tile_rows % seq_len if fault == "rope_pos_tile_local" else rr % seq_len
    c, s = (t.to(F32)[pos, :HEAD // 2][:, None, :] for t in (cos, sin))
    v = x[:, :rot].reshape(M, -1, HEAD)
    ia = torch.arange(HEAD // 2)
    if fault == "rope_partner_16":
        ia = torch.cat([torch.arange(16), torch.arange(32, 48)])
    ib = ia + (16 if fault == "rope_partner_16" else HEAD // 2)
    a, b = v[..., ia], v[..., ib]
    o = torch.empty_like(v)
    o[..., ia] = a * c - b * s
    o[..., ib] = b * c + a * s
    out[:, :rot] = o.reshape(M, rot)
    return out.to(BF)


def emu_ce_stats(acc32, block, fault=None):
    """(logits bf16 [M, N], the flat f32 statistics buffer) from the f32 accumulator."""
    M, N = acc32.shape
    nblk, W = N // block, block // 64
    x = _rne(acc32)
    v = (acc32 if fault == "stats_of_unrounded" else x).reshape(M, nblk, W, 64)
    mw = v.amax(3)
    nm = -mw * LOG2E
    # fma(x, log2e, nm): the product is exact in float64, so the conversion is the fma's one rounding
    arg = (v.to(F64) * LOG2E.to(F64) + nm.to(F64)[..., None]).to(F32)
    sw = torch.exp2(arg).sum(3)
    Mb = mw[..., 0] if fault == "stats_max_of_first_wave" else mw.amax(2)
    term = sw * torch.exp(mw - Mb[..., None])
    if fault == "stats_drops_a_wave":
        term = term[..., :W - 1]
    st = torch.stack([Mb, term.sum(2)], 2)             # [M, nblk, 2]
    if fault != "stats_row_major":
        st = st.permute(1, 0, 2)                       # tile-major: stats[b * M + row]
    return x.to(BF), st.contiguous().reshape(-1)
