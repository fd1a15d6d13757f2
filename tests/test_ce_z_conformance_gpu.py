"""Per-element conformance of the z-loss entry points of csrc/cross_entropy.hip (through ctypes, as
tests/test_row_conformance_gpu.py tests their namesakes): every _z form against the float64 reference and
the derived bounds of tests/_ce_z_ref.py, on every input family, at z = 2^-2 (the value that tests the
gradient: the factor 1 + 2 z lse runs from about -59 to 61 on the offset family), 1e-4 and 0.

    fused _fwd_bwd_z      V = 8, 2040, 8200 (NC 4 / 8), 49160 (NC 32), 65544 (ce_kernel_2pass); loss-only,
                          strided sink, in place
    streaming pair        V = 8, 8200, 10232; scale_stride 0 and 1 (the backward reads the stored f32 LSE)
    _bwd_lse_shard_z      (lo, width) = (2056, 2048), (4096, 8); the target inside and outside the shard
    _fwd_stats_z          nblk 1 and 9: 33 rows with whole (-inf, 0) tiles, and every family's 8 rows
    _vp_combine_z         tp 1, 2, 8: the neg_inf family at tp > 1 (a shard of -inf columns), and every family's 8 rows
    bad targets           -1, V, 2^40: NaN row_loss, row_z and gradient row, the other rows untouched, the bit
    z = 0                 every _z form writes its plain namesake's bits and row_z = +0
    determinism           a second run of every form gives the same bits

test_zz_worst_ratio_table prints the worst |got - ref| / bound per output (run with -rA).
"""
import functools
import math

import pytest
import torch

from tests import _ce_z_ref as Z
from tests import _row_ref as R
from tests import test_row_conformance_gpu as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
IGN = R.IGNORE
ROWS = Z.CE_ROWS
call, p, dev, guarded, guards_intact, in_padded, same_bits = (T.call, T.p, T.dev, T.guarded, T.guards_intact, T.in_padded,
                                                              T.same_bits)
V_FUSED = (8, 2040, 8200, 49160, 65544)
V_STREAM = (8, 8200, 10232)


@functools.lru_cache(maxsize=8)
def ce_case(family, V):
    return Z.ce_case(family, V)


def zeros_exact(name, t):
    R.check_exact(name, t, torch.zeros(t.shape, dtype=t.dtype))


def check_ignored(grad, row_z, tgt):
    ign = tgt == IGN
    zeros_exact("ignored rows", grad.cpu()[ign])
    zeros_exact("ignored row_z", row_z.cpu()[ign])


def run_fused(x, tgt, form, z, scale=0.5, inv=None, status=None, plain=False, with_rz=True):
    """pt_cross_entropy_fwd_bwd_z (plain: its namesake): form 'loss' (dlogits NULL), 'sink', 'inplace'.
    Returns (row_loss, row_z or None, dlogits or None)."""
    rows, V = x.shape
    lf, logits = in_padded(dev(x))
    before = lf.clone()
    t = dev(tgt)
    rl_f, rl = guarded(rows, 1, F32)
    rz_f, rz = guarded(rows, 1, F32)
    invd = None if inv is None else torch.tensor([inv], dtype=F32, device=DEV)
    if form == "sink":
        df, d = guarded(rows, V, BF, gap=16)
    else:
        df, d = (lf, logits) if form == "inplace" else (None, None)
    args = (p(logits), logits.stride(0), p(t), p(d), d.stride(0) if d is not None else 0, p(rl), rows, V, scale, p(invd),
            IGN, p(status))
    if plain:
        call("pt_cross_entropy_fwd_bwd", *args)
    else:
        call("pt_cross_entropy_fwd_bwd_z", *args, z, p(rz) if with_rz else None)
    torch.cuda.synchronize()
    assert guards_intact(rl_f, rows, 1) and guards_intact(rz_f, rows, 1)
    if plain or not with_rz:
        assert guards_intact(rz_f, 0, 1), "row_z NULL: nothing written"
    if form == "inplace":
        assert guards_intact(lf, rows, V)
    else:
        assert same_bits(lf, before), "the logits are read-only out of place"
        if form == "sink":
            assert guards_intact(df, rows, V)
    return rl[:, 0], (None if plain or not with_rz else rz[:, 0]), d


@pytest.mark.parametrize("V", V_FUSED)
def test_fused_z_every_kernel(V):
    """ce_kernel<NC> and ce_kernel_2pass with the z switch on (z > 0) and off (z = 0, against the plain entry
    point by bits)."""
    inv = 1.0 / 7
    gs = torch.full((ROWS,), float(torch.tensor(0.5, dtype=F32) * torch.tensor(inv, dtype=F32)), dtype=F64)
    for family in R.CE_FAMILIES:
        x, tgt = ce_case(family, V)
        f = R.ref_ce_fwd(x, tgt)
        for z in Z.Z_VALUES:
            zf = Z.ref_z_fwd_from(f, z)
            gref, gbound = Z.ref_z_bwd(x, tgt, f["lse"], f["lse_bound"], gs, z)
            tag = f"fused z={z:g} {family}"
            loss0, rz0, _ = run_fused(x, tgt, "loss", z, inv=inv)
            R.check("row_z", rz0, zf["row_z"], zf["row_z_bound"], tag)
            R.check("loss", loss0, zf["loss"], zf["loss_bound"], tag)
            grads = {}
            for form in ("sink", "inplace"):
                loss, rz, grad = run_fused(x, tgt, form, z, inv=inv)
                assert same_bits(loss, loss0) and same_bits(rz, rz0), "loss and row_z do not depend on the form"
                R.check(f"grad {form}", grad, gref, gbound, tag)
                check_ignored(grad, rz, tgt)
                grads[form] = grad.clone()
                if z == 0:
                    ploss, _, pgrad = run_fused(x, tgt, form, 0.0, inv=inv, plain=True)
                    assert same_bits(loss, ploss) and same_bits(grad, pgrad), "z = 0 is the plain entry point by bits"
                    zeros_exact("row_z at z = 0", rz.cpu())
            assert same_bits(grads["sink"], grads["inplace"])
            loss_n, _, grad_n = run_fused(x, tgt, "sink", z, inv=inv, with_rz=False)     # row_z NULL: a second run
            assert same_bits(loss_n, loss0) and same_bits(grad_n, grads["sink"]), "run to run, with and without row_z"


def run_lse_pair(x, tgt, scale, scale_stride, z, status=None, lse_in=None, vocab_lo=None, width=None, plain=False):
    """pt_cross_entropy_fwd_lse_z + bwd_lse_z (or bwd_lse_shard_z on columns [vocab_lo, vocab_lo + width)); plain: the
    namesakes.  Returns (row_loss, row_z, row_lse, dlogits)."""
    rows, V = x.shape
    lf, logits = in_padded(dev(x))
    t = dev(tgt)
    rl_f, rl = guarded(rows, 1, F32)
    ls_f, lse = guarded(rows, 1, F32)
    rz_f, rz = guarded(rows, 1, F32)
    zargs = () if plain else (z,)
    sfx = "" if plain else "_z"
    if lse_in is None:
        args = (p(logits), logits.stride(0), p(t), p(rl), p(lse), rows, V, IGN, p(status))
        call("pt_cross_entropy_fwd_lse" + sfx, *args, *(() if plain else (z, p(rz))))
        torch.cuda.synchronize()
        assert guards_intact(rl_f, rows, 1) and guards_intact(ls_f, rows, 1) and guards_intact(rz_f, rows, 1)
        lse_c = lse[:, 0].contiguous()
    else:
        lse_c = dev(lse_in)
    sc = dev(scale.to(F32))
    if vocab_lo is None:
        df, d = guarded(rows, V, BF, gap=16)
        call("pt_cross_entropy_bwd_lse" + sfx, p(logits), logits.stride(0), p(t), p(lse_c), p(d), d.stride(0), rows, V, p(sc),
             scale_stride, IGN, *zargs)
        width = V
    else:
        df, d = guarded(rows, width, BF, gap=16)
        shard = logits[:, vocab_lo:vocab_lo + width]
        call("pt_cross_entropy_bwd_lse_shard" + sfx, p(shard), logits.stride(0), p(t), p(lse_c), p(d), d.stride(0), rows,
             width, vocab_lo, p(sc), scale_stride, IGN, *zargs)
    torch.cuda.synchronize()
    assert guards_intact(df, rows, width) and guards_intact(lf, rows, V)
    return rl[:, 0], rz[:, 0], lse_c, d


@pytest.mark.parametrize("V", V_STREAM)
def test_streaming_pair_z(V):
    """fwd_lse_z + bwd_lse_z: the forward's LSE is the plain one (saved), the backward reads it as an input."""
    steps = math.ceil(V / 8192)
    for family in R.CE_FAMILIES:
        x, tgt = ce_case(family, V)
        f = R.ref_ce_fwd(x, tgt, style="fma", steps=steps)
        for z in Z.Z_VALUES:
            zf = Z.ref_z_fwd_from(f, z)
            tag = f"stream z={z:g} {family}"
            for stride in (0, 1):
                scale = torch.tensor([0.25]) if stride == 0 else (0.125 * (1 + torch.arange(ROWS) % 3)).float()
                loss, rz, lse, grad = run_lse_pair(x, tgt, scale, stride, z)
                R.check("row_z", rz, zf["row_z"], zf["row_z_bound"], tag)
                R.check("loss", loss, zf["loss"], zf["loss_bound"], tag)
                R.check("lse", lse, f["lse"], f["lse_bound"], tag)
                gref, gbound = Z.ref_z_bwd(x, tgt, lse.cpu().double(), torch.zeros(ROWS, dtype=F64),
                                           scale.double().expand(ROWS), z, style="fma")
                R.check(f"grad stride {stride}", grad, gref, gbound, tag)
                check_ignored(grad, rz, tgt)
                if z == 0:
                    pl = run_lse_pair(x, tgt, scale, stride, 0.0, plain=True)
                    assert same_bits(loss, pl[0]) and same_bits(lse, pl[2]) and same_bits(grad, pl[3]), "z = 0: plain bits"
                    zeros_exact("row_z at z = 0", rz.cpu())
            again = run_lse_pair(x, tgt, scale, 1, z)
            assert all(same_bits(a, b) for a, b in zip(again, (loss, rz, lse, grad))), "run to run"


@pytest.mark.parametrize("lo,width", [(2056, 2048), (4096, 8)])
def test_backward_on_a_shard_z(lo, width):
    """bwd_lse_shard_z: the factor on the shard's softmax, the one-hot at target - vocab_lo only inside it."""
    V = 4104
    tgt = torch.tensor([lo, lo + width - 1, lo - 1, lo + width if lo + width < V else 0, IGN, lo + 7, 0, V - 1])
    scale = (0.125 * (1 + torch.arange(ROWS) % 3)).float()
    for family in R.CE_FAMILIES:
        x, _ = ce_case(family, V)
        lse32 = R.ref_ce_fwd(x, tgt)["lse_clean"].float()
        for z in Z.Z_VALUES:
            _, _, _, grad = run_lse_pair(x, tgt, scale, 1, z, lse_in=lse32, vocab_lo=lo, width=width)
            gref, gbound = Z.ref_z_bwd(x[:, lo:lo + width], tgt, lse32.double(), torch.zeros(ROWS, dtype=F64), scale.double(),
                                       z, style="fma", vocab_lo=lo)
            R.check("grad shard", grad, gref, gbound, f"shard z={z:g} {family}")
            zeros_exact("ignored rows", grad.cpu()[tgt == IGN])
            if z == 0:
                pgrad = run_lse_pair(x, tgt, scale, 1, 0.0, lse_in=lse32, vocab_lo=lo, width=width, plain=True)[3]
                assert same_bits(grad, pgrad), "z = 0: plain bits"
            again = run_lse_pair(x, tgt, scale, 1, z, lse_in=lse32, vocab_lo=lo, width=width)[3]
            assert same_bits(grad, again), "run to run"


def stats_forward(x, tgt, st, nblk, z, plain=False, status=None):
    rows, V = x.shape
    lf, logits = in_padded(dev(x))
    rl_f, rl = guarded(rows, 1, F32)
    ls_f, lse = guarded(rows, 1, F32)
    rz_f, rz = guarded(rows, 1, F32)
    td, sd = dev(tgt), dev(st)
    args = (p(logits), logits.stride(0), p(td), p(sd), nblk, p(rl), p(lse), rows, V, IGN, p(status))
    if plain:
        call("pt_cross_entropy_fwd_stats", *args)
    else:
        call("pt_cross_entropy_fwd_stats_z", *args, z, p(rz))
    torch.cuda.synchronize()
    assert guards_intact(rl_f, rows, 1) and guards_intact(ls_f, rows, 1) and guards_intact(rz_f, rows, 1)
    return rl[:, 0], rz[:, 0], lse[:, 0]


def stats_refs(x, tgt, m, s, z, steps=None, extra=None):
    """(lse ref, lse bound, ref_z_fwd's dict) of statistics m, s [rows, n] (float64) for the whole rows x."""
    rows = x.shape[0]
    lref, lerr = R.merge_stats(m, s, steps=steps)
    if extra is not None:
        lerr = lerr + extra
    valid = tgt != IGN
    xt = x.double()[torch.arange(rows), tgt.clamp(0, x.shape[1] - 1)]
    loss = torch.where(valid, lref - xt, torch.zeros_like(lref))
    lb = torch.where(valid, lerr + R.E * loss.abs(), torch.zeros_like(lerr))
    return lref, lerr, Z.ref_z_fwd(z, lref, lerr, valid, loss, lb)


@pytest.mark.parametrize("nblk", [1, 9])
def test_from_statistics_z(nblk):
    """fwd_stats_z on synthetic statistics with whole (-inf, 0) tiles and rows offset to lse = +-120."""
    rows, V = 33, nblk * 16
    g = R._gen("stats z", nblk, rows)
    x = (torch.randn(rows, V, generator=g) * 3 + 40.0 * (torch.arange(rows) % 7 - 3)[:, None]).to(BF)
    tiles = x.view(rows, nblk, 16)
    if nblk > 1:
        for r in range(rows):
            tiles[r, (r * 5) % nblk] = -math.inf
    tgt = torch.randint(0, V, (rows,), generator=g)
    tgt[rows // 2] = IGN
    st = T.tile_stats(x, nblk)
    m, s = st[..., 0].t().double(), st[..., 1].t().double()
    for z in Z.Z_VALUES:
        lref, lerr, zf = stats_refs(x, tgt, m, s, z)
        loss, rz, lse = stats_forward(x, tgt, st, nblk, z)
        tag = f"stats z={z:g}"
        R.check("lse", lse, lref, lerr, tag)
        R.check("row_z", rz, zf["row_z"], zf["row_z_bound"], tag)
        R.check("loss", loss, zf["loss"], zf["loss_bound"], tag)
        zeros_exact("ignored row_z", rz.cpu()[tgt == IGN])
        if z == 0:
            pl = stats_forward(x, tgt, st, nblk, 0.0, plain=True)
            assert same_bits(loss, pl[0]) and same_bits(lse, pl[2]), "z = 0: plain bits"
            zeros_exact("row_z at z = 0", rz.cpu())
        again = stats_forward(x, tgt, st, nblk, z)
        assert all(same_bits(a, b) for a, b in zip(again, (loss, rz, lse))), "run to run"


@pytest.mark.parametrize("nblk", [1, 9])
def test_from_statistics_z_every_family(nblk):
    """fwd_stats_z on the tile statistics of every family's 8 rows (make_targets' columns and the ignored row)."""
    V = nblk * 16
    for family in R.CE_FAMILIES:
        x, tgt = ce_case(family, V)
        st = T.tile_stats(x, nblk)
        m, s = st[..., 0].t().double(), st[..., 1].t().double()
        for z in Z.Z_VALUES:
            lref, lerr, zf = stats_refs(x, tgt, m, s, z)
            loss, rz, lse = stats_forward(x, tgt, st, nblk, z)
            tag = f"stats z={z:g}"
            R.check("lse", lse, lref, lerr, tag)
            R.check("row_z", rz, zf["row_z"], zf["row_z_bound"], tag)
            R.check("loss", loss, zf["loss"], zf["loss_bound"], tag)
            zeros_exact("ignored row_z", rz.cpu()[tgt == IGN])
            if z == 0:
                pl = stats_forward(x, tgt, st, nblk, 0.0, plain=True)
                assert same_bits(loss, pl[0]) and same_bits(lse, pl[2]), "z = 0: plain bits"
                zeros_exact("row_z at z = 0", rz.cpu())


def vp_forward(x, tgt, tp, Vs, nblk, z, plain=False, status=None):
    rows = x.shape[0]
    lf, logits = in_padded(dev(x))
    t = dev(tgt)
    pf, parts = guarded(tp * rows, 4, F32)
    stats, keep = [], []
    for q in range(tp):
        st = T.tile_stats(x[:, q * Vs:(q + 1) * Vs], nblk)
        stats.append(st)
        shard = logits[:, q * Vs:(q + 1) * Vs]
        sd = dev(st)
        keep.append(sd)
        call("pt_cross_entropy_vp_partial", p(shard), logits.stride(0), p(t), p(sd), nblk, p(parts[q * rows:]), rows, Vs, q * Vs)
    rl_f, rl = guarded(rows, 1, F32)
    ls_f, lse = guarded(rows, 1, F32)
    rz_f, rz = guarded(rows, 1, F32)
    args = (p(parts), tp, p(t), p(rl), p(lse), rows, tp * Vs, IGN, p(status))
    if plain:
        call("pt_cross_entropy_vp_combine", *args)
    else:
        call("pt_cross_entropy_vp_combine_z", *args, z, p(rz))
    torch.cuda.synchronize()
    assert guards_intact(pf, tp * rows, 4) and guards_intact(rl_f, rows, 1) and guards_intact(ls_f, rows, 1)
    assert guards_intact(rz_f, rows, 1)
    return rl[:, 0], rz[:, 0], lse[:, 0], torch.cat(stats, 0)


@pytest.mark.parametrize("tp", [1, 2, 8])
def test_vocab_parallel_combine_z(tp):
    """vp_partial per shard + vp_combine_z against the whole-vocabulary reference; the parts are the plain
    16 bytes per row, the z term comes from the combined LSE."""
    rows, Vs, nblk = 33, 256, 2
    V = tp * Vs
    x = R.make_ce_case("neg_inf" if tp > 1 else "offset", rows, V)
    if tp > 1:
        x[:, Vs:2 * Vs][::3] = -math.inf        # every third row: a whole shard of -inf columns
        assert bool(torch.isfinite(x.float()).any(1).all())
    tgt = R.make_targets(rows, V)
    f = R.ref_ce_fwd(x, tgt)
    for z in Z.Z_VALUES:
        loss, rz, lse, st = vp_forward(x, tgt, tp, Vs, nblk, z)
        lref, lerr = R.merge_stats(st[..., 0].t().double(), st[..., 1].t().double(), steps=9 + tp)
        lerr = lerr + 2 * R.E * (1 + f["lse_clean"].abs())         # the f32 rounding of the s_b and of xt's sum
        lb = torch.where(f["valid"], lerr + R.E * f["loss"].abs(), torch.zeros_like(lerr))
        zf = Z.ref_z_fwd(z, f["lse"], lerr, f["valid"], f["loss"], lb)
        tag = f"vp tp {tp} z={z:g}"
        R.check("lse", lse, f["lse"], lerr, tag)
        R.check("row_z", rz, zf["row_z"], zf["row_z_bound"], tag)
        R.check("loss", loss, zf["loss"], zf["loss_bound"], tag)
        zeros_exact("ignored row_z", rz.cpu()[tgt == IGN])
        if z == 0:
            pl = vp_forward(x, tgt, tp, Vs, nblk, 0.0, plain=True)
            assert same_bits(loss, pl[0]) and same_bits(lse, pl[2]), "z = 0: plain bits"
            zeros_exact("row_z at z = 0", rz.cpu())
        again = vp_forward(x, tgt, tp, Vs, nblk, z)
        assert all(same_bits(a, b) for a, b in zip(again[:3], (loss, rz, lse))), "run to run"


@pytest.mark.parametrize("tp", [1, 2, 8])
def test_vocab_parallel_combine_z_every_family(tp):
    """vp_combine_z on every family's 8 rows (make_targets) split into tp shards of 16 columns."""
    Vs, nblk = 16, 1
    V = tp * Vs
    for family in R.CE_FAMILIES:
        x, tgt = ce_case(family, V)
        f = R.ref_ce_fwd(x, tgt)
        for z in Z.Z_VALUES:
            loss, rz, lse, st = vp_forward(x, tgt, tp, Vs, nblk, z)
            lref, lerr = R.merge_stats(st[..., 0].t().double(), st[..., 1].t().double(), steps=9 + tp)
            lerr = lerr + 2 * R.E * (1 + f["lse_clean"].abs())         # the f32 rounding of the s_b and of xt's sum
            lb = torch.where(f["valid"], lerr + R.E * f["loss"].abs(), torch.zeros_like(lerr))
            zf = Z.ref_z_fwd(z, f["lse"], lerr, f["valid"], f["loss"], lb)
            tag = f"vp tp {tp} z={z:g}"
            R.check("lse", lse, f["lse"], lerr, tag)
            R.check("row_z", rz, zf["row_z"], zf["row_z_bound"], tag)
            R.check("loss", loss, zf["loss"], zf["loss_bound"], tag)
            zeros_exact("ignored row_z", rz.cpu()[tgt == IGN])
            if z == 0:
                pl = vp_forward(x, tgt, tp, Vs, nblk, 0.0, plain=True)
                assert same_bits(loss, pl[0]) and same_bits(lse, pl[2]), "z = 0: plain bits"
                zeros_exact("row_z at z = 0", rz.cpu())


@pytest.mark.parametrize("V", [8200, 65544])
def test_bad_targets_z(V):
    """-1, V and 2^40: NaN row_loss, row_z and gradient row, the status bit; the other rows bit-identical to a run
    in which those rows are ignored."""
    z = 0.25
    x, tgt = ce_case("randn3", V)
    bad, clean = tgt.clone(), tgt.clone()
    for r, t in zip((1, 3, 6), R.BAD_TARGETS):
        bad[r] = V if t == "V" else t
        clean[r] = IGN
    rb, keep = torch.tensor([1, 3, 6]), torch.tensor([0, 2, 4, 5, 7])
    kd = keep.to(DEV)

    def nan_rows(*ts):
        return all(bool(torch.isnan(t.float().cpu()[rb]).all()) for t in ts)

    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    loss_c, rz_c, grad_c = run_fused(x, clean, "sink", z, status=status)
    assert int(status.item()) == 0
    loss_b, rz_b, grad_b = run_fused(x, bad, "sink", z, status=status)
    assert int(status.item()) & 1
    assert nan_rows(loss_b, rz_b, grad_b)
    assert same_bits(loss_b[kd], loss_c[kd]) and same_bits(rz_b[kd], rz_c[kd]) and same_bits(grad_b[kd], grad_c[kd])
    # the streaming pair: NaN loss, row_z and lse from the forward, a NaN gradient row from the backward
    status.zero_()
    loss_c, rz_c, lse_c, grad_c = run_lse_pair(x, clean, torch.tensor([0.25]), 0, z, status)
    assert int(status.item()) == 0
    loss, rz, lse, grad = run_lse_pair(x, bad, torch.tensor([0.25]), 0, z, status)
    assert int(status.item()) & 1
    assert nan_rows(loss, rz, lse, grad)
    assert same_bits(loss[kd], loss_c[kd]) and same_bits(rz[kd], rz_c[kd]) and same_bits(grad[kd], grad_c[kd])
    if V > 8200:
        return
    # the backward on a shard reads the forward's NaN LSE: NaN rows, the others untouched
    lo, width = 2056, 2048
    gs_c = run_lse_pair(x, clean, torch.tensor([0.25]), 0, z, lse_in=lse_c, vocab_lo=lo, width=width)[3]
    gs_b = run_lse_pair(x, bad, torch.tensor([0.25]), 0, z, lse_in=lse, vocab_lo=lo, width=width)[3]
    assert nan_rows(gs_b) and same_bits(gs_b[kd], gs_c[kd])
    # the statistics forward and the vocab-parallel combine: the same range check
    nblk = 5
    st = T.tile_stats(x, nblk)
    status.zero_()
    loss_c, rz_c, _ = stats_forward(x, clean, st, nblk, z, status=status)
    assert int(status.item()) == 0
    loss, rz, lse = stats_forward(x, bad, st, nblk, z, status=status)
    assert int(status.item()) & 1 and nan_rows(loss, rz, lse)
    assert same_bits(loss[kd], loss_c[kd]) and same_bits(rz[kd], rz_c[kd])
    status.zero_()
    loss_c, rz_c, _, _ = vp_forward(x, clean, 5, V // 5, 1, z, status=status)
    assert int(status.item()) == 0
    loss, rz, lse, _ = vp_forward(x, bad, 5, V // 5, 1, z, status=status)
    assert int(status.item()) & 1 and nan_rows(loss, rz, lse)
    assert same_bits(loss[kd], loss_c[kd]) and same_bits(rz[kd], rz_c[kd])


def test_zz_worst_ratio_table():
    """Prints the worst |got - ref| / bound per form, z and output that this process has seen (run with -rA)."""
    worst = {}
    for (tag, name), v in R.WORST.items():
        if tag is None or " z=" not in str(tag):
            continue
        form = " ".join(str(tag).split(" ")[:-1]) if str(tag).split(" ")[0] in ("fused", "stream", "shard") else str(tag)
        key = (form, name.split(" ")[0])
        worst[key] = max(worst.get(key, 0.0), v)
    for (form, name), v in sorted(worst.items()):
        print(f"worst {form} | {name} | {v:.3g}")
