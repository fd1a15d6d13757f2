"""The AdamW kernels of csrc/adamw.hip (bf16 and f32 state, master weights, the norm pass, the clip scale)
through picotron_amd.kernels against the references of tests/_optim_ref.py, per element, on adversarial
input families and at three launch geometries.  Families, references, bounds and their derivation:
tests/_optim_ref.py (self-tested without a GPU in tests/test_optim_checker_cpu.py).

Lists (every test asserts the geometry it relies on through O.geometry, see _need):
    small  40 tensors of 0 to 20 elements: one workgroup, 35 tensors in its run, empty tensors inside and
           at the end; the ragged tail and the drain of every kernel
    mid    the six shapes of the older optimizer tests: 257 workgroups x 512 chunks, two trips per thread:
           prologue and drain of the bf16 step, one steady-state trip of the master step
    cap    13.2 M elements, 15 tensors: the step launches at their 1024-workgroup cap with 1612 chunks per
           workgroup (seven trips: the bf16 step's two-ahead steady state and rotation, the master step's
           one-ahead steady state), the norm and scale launches at their 2048 cap with 806 (the four-way
           loop); neither is a multiple of 256, so runs start in mid-tensor at odd chunk offsets; six
           tensors share one run
Every tensor of a list is carved from one sentinel-filled allocation per field with 16-byte gaps; the
gaps and the gradient buffers are compared by bits after every launch.
"""
import functools
import math

import pytest
import torch

from tests import _optim_ref as O
from tests import _row_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64

L_SMALL = [0, 1, 7, 8, 9, 16, 3, 20, 5, 12, 0, 2, 17, 4, 8, 15, 6, 19, 1, 10, 0, 13, 7, 9, 16, 11, 18, 14, 2, 8, 20, 3, 0, 5,
           16, 7, 1, 9, 12, 0]
L_MID = [2048, 1001, 512 * 2048, 37, 3 * 5 * 7, 8]
L_CAP = [10_000_136, 1001, 37, 3 * 5 * 7, 8, 0, 1_500_008, 2048, 1001, 37, 3 * 5 * 7, 8, 1_700_003, 37, 0]
LISTS = dict(small=L_SMALL, mid=L_MID, cap=L_CAP)
# t = 1, 3, 1000 x lr 3e-4, 3e-5 x wd 0.01, 0: all twelve on `small`, these four (every value once) on `mid`
SC_ALL = [O.scalars(t=t, lr=lr, wd=wd) for t in (1, 3, 1000) for lr in (3e-4, 3e-5) for wd in (0.01, 0.0)]
SC_MID = [O.scalars(1, 3e-4, 0.01), O.scalars(3, 3e-5, 0.0), O.scalars(1000, 3e-4, 0.0), O.scalars(1000, 3e-5, 0.01)]
SC_CAP = O.scalars(3, 3e-4, 0.01)


def K_():
    from picotron_amd import kernels
    return kernels


def _sync():
    if DEV == "cuda":
        torch.cuda.synchronize()


def _need(lname):
    """The geometry a test on this list relies on."""
    L = LISTS[lname]
    gs, gn = O.geometry(L, O.STEP_CAP), O.geometry(L, O.NORM_CAP)
    if lname == "small":
        assert len(L) == 40 and max(L) <= 20 and {0, 1, 7, 8, 9, 16} <= set(L) and L[-1] == 0 and 0 in L[1:-1]
        assert gs["blocks"] == gn["blocks"] == 1 and gs["run_tensors"] == sum(1 for n in L if n) == 35
    elif lname == "mid":
        assert (gs["blocks"], gs["per_block"]) == (gn["blocks"], gn["per_block"]) == (257, 512)
        assert gs["seg_full"] == 512
    else:
        assert abs(sum(L) - 13.2e6) < 1e5 and {1001, 37, 105, 8, 0} <= set(L)
        assert gs["blocks"] == 1024 and gs["per_block"] >= 1025 and gs["per_block"] % 256 != 0
        assert gn["blocks"] == 2048 and gn["per_block"] >= 769 and gn["per_block"] % 256 != 0
        assert gs["seg_full"] >= 1025 and gn["seg_full"] >= 769      # steady state / the four-way loop inside one tensor
        assert gs["run_tensors"] >= 3 and gn["run_tensors"] >= 3 and gs["mid_start"] and gn["mid_start"]
    return gs, gn


def test_geometry():
    for lname in LISTS:
        _need(lname)
    assert O.multi_grid(O.chunk_starts(L_CAP)[-1], O.STEP_CAP) == (1024, 1612)
    assert O.multi_grid(O.chunk_starts(L_CAP)[-1], O.NORM_CAP) == (2048, 806)


@functools.lru_cache(maxsize=3)
def _data(family, lname, sc, dtype, gdtype, seed=0):
    return O.make_list(family, LISTS[lname], seed, sc, dtype, gdtype)


def _bufs(data, lengths, skew=0):
    return [O.ListBuf(lengths, ts[0].dtype if ts else BF, DEV, skew).fill(ts) for ts in data]


def _status():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def _max_norm(family, sq):
    norm = math.sqrt(sq) if math.isfinite(sq) and sq > 0 else 1.0
    return (4.0 if family in O.COEF_ONE else 0.3) * norm


def _untouched(bufs, before, name):
    for b, b0 in zip(bufs, before):
        assert O.same_bits(b.flat, b0.flat), f"{name}: a skipped step wrote something"


def _sc_of(family, sc):
    return O.EXACT_S if family == "exact" else sc


# ============================================================================== bf16 state, the list form
def _list_step_bf16(lname, family, sc, clip, bufs=None, tag=None, sequenced=True):
    """One pt_adamw_step_multi(_clip) launch over the list and its check; returns the buffers after."""
    K = K_()
    L = LISTS[lname]
    sc = _sc_of(family, sc)
    name = f"bf16 list {lname} {family}{' clip' if clip else ''}"
    bufs = bufs or _bufs(_data(family, lname, sc, BF, BF), L)
    before = [b.clone() for b in bufs]
    P, G, M, V = bufs
    items = list(zip(P.views(), G.views(), M.views(), V.views()))
    coef = None
    if clip:
        sq, st = K.grad_sqnorm(items=items), _status()
        max_norm = _max_norm(family, sq.item())
        K.adamw_step_multi_clip(items, sq, max_norm, status=st, **sc.kw())
        _sync()
        coef = O.clip_coef(sq.item(), max_norm)
        if coef is None:
            assert family in ("overflow", "nan_grad") and st.item() == K.STATUS_NONFINITE_GRAD
            _untouched(bufs, before, name)
            return bufs
        assert st.item() == 0 and (coef == 1.0) == (family in O.COEF_ONE), coef
    else:
        K.adamw_step_multi(items, **sc.kw())
        _sync()
    assert O.same_bits(G.flat, before[1].flat), f"{name}: the gradients were written"
    for nm, b in zip("pmv", (P, M, V)):
        assert b.gaps_intact(), f"{name}: the kernel wrote outside the tensors of {nm}"
    g = before[1].cat() if coef is None else O.clip_grad(before[1].cat(), coef, True)
    inp = (before[0].cat(), g, before[2].cat(), before[3].cat())
    got = (P.cat(), M.cat(), V.cat())
    if family == "exact":
        O.check_exact_step(name, got, inp, sc, tag or lname)
    if sequenced:
        O.check_bf16_step(name, got, inp, sc, tag or lname)
    return bufs


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("family", O.FAMILIES)
def test_bf16_list_small(family, clip):
    _need("small")
    for sc in SC_ALL:
        _list_step_bf16("small", family, sc, clip)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("family", O.FAMILIES)
def test_bf16_list_mid(family, clip):
    _need("mid")
    _list_step_bf16("mid", family, SC_MID[O.FAMILIES.index(family) % 4], clip)


@pytest.mark.parametrize("sc", range(4))
def test_bf16_list_mid_scalars(sc):
    """every t, lr and wd of the issue at the mid geometry (randn)"""
    _need("mid")
    _list_step_bf16("mid", "randn", SC_MID[sc], bool(sc % 2))


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("family", ["exact", "randn", "cancel"])
def test_bf16_list_cap(family, clip):
    """1024 workgroups x 1612 chunks: seven trips per thread, runs that start in mid-tensor."""
    _need("cap")
    _list_step_bf16("cap", family, SC_CAP, clip, sequenced=family != "exact")


def test_bf16_list_chained_steps():
    """Three steps on the mid list, new gradients each, every step checked from the kernel's own previous output."""
    _need("mid")
    P, _, M, V = _bufs(_data("randn", "mid", SC_MID[0], BF, BF), L_MID)
    for t in (1, 2, 3):
        G = O.ListBuf(L_MID, BF, DEV).fill(O.make_list("randn", L_MID, 100 + t)[1])
        P, _, M, V = _list_step_bf16("mid", "randn", O.scalars(t=t), t == 2, bufs=[P, G, M, V], tag="chained")


# ============================================================================== single-tensor forms
SINGLE = dict(bf16_aligned=(2051, BF, 0), bf16_off2=(1001, BF, 1), f32=(100003, F32, 0))


def _single_step(name, n, dtype, skew, family, clip, sc, exact_only=False):
    K = K_()
    sc = _sc_of(family, sc)
    bufs = _bufs([[t] for t in O.make_state(family, n, 7, sc, dtype)], [n], skew)
    before = [b.clone() for b in bufs]
    p, g, m, v = (b.views()[0] for b in bufs)
    assert p.data_ptr() % 16 == skew * p.element_size()
    coef = None
    if clip:
        sq, st = K.grad_sqnorm(tensors=[g]), _status()
        max_norm = _max_norm(family, sq.item())
        K.adamw_step_clip(p, g, m, v, sq, max_norm, status=st, **sc.kw())
        _sync()
        coef = O.clip_coef(sq.item(), max_norm)
        if coef is None:
            assert st.item() == K.STATUS_NONFINITE_GRAD
            _untouched(bufs, before, name)
            return
        assert st.item() == 0
    else:
        K.adamw_step(p, g, m, v, **sc.kw())
        _sync()
    assert O.same_bits(bufs[1].flat, before[1].flat)
    assert all(bufs[i].gaps_intact() for i in (0, 2, 3)), f"{name}: a write outside the tensor"
    g0 = before[1].cat() if coef is None else O.clip_grad(before[1].cat(), coef, dtype == BF)
    inp = (before[0].cat(), g0, before[2].cat(), before[3].cat())
    got = (p.cpu(), m.cpu(), v.cpu())
    if family == "exact":
        O.check_exact_step(name, got, inp, sc, "single")
    if not exact_only:
        (O.check_bf16_step if dtype == BF else O.check_f32_step)(name, got, inp, sc, "single")


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("family", O.FAMILIES)
@pytest.mark.parametrize("kind", list(SINGLE))
def test_single_tensor(kind, family, clip):
    n, dtype, skew = SINGLE[kind]
    if dtype == BF and not skew:
        assert n // 8 == 256 and n % 8 == 3     # the vector kernel and the scalar tail
    _single_step(f"{kind} {family}{' clip' if clip else ''}", n, dtype, skew, family, clip, SC_MID[1 + clip])


@pytest.mark.parametrize("clip", [False, True])
def test_single_tensor_grid_wraps(clip):
    """adamw_bf16_kernel's grid-stride loop wraps above 2048 x 256 chunks (`exact`: no float64 pass)."""
    n = 2048 * 256 * 8 + 4099
    assert n // 8 > O.STREAM_CAP * 256 and O.grid_for(n // 8) == O.STREAM_CAP
    _single_step(f"bf16 wrap{' clip' if clip else ''}", n, BF, 0, "exact", clip, None, exact_only=True)


# ============================================================================== master weights
def _master_data(family, lname, sc, gdt):
    return _data(family, lname, sc, F32, gdt)


def _master_check(name, bufs, before, sc, coef, family, tag, bound=True):
    W, Pm, G, M, V = bufs
    assert O.same_bits(G.flat, before[2].flat), f"{name}: the gradients were written"
    for nm, b in zip(("master", "param", "m", "v"), (W, Pm, M, V)):
        assert b.gaps_intact(), f"{name}: the kernel wrote outside the tensors of {nm}"
    g = before[2].cat().to(F32)
    if coef is not None:
        g = O.clip_grad(g, coef, False)
    O.check_master_step(name, (W.cat(), Pm.cat(), M.cat(), V.cat()), (before[0].cat(), g, before[3].cat(), before[4].cat()),
                        sc, tag, bound=bound)


def _master_bufs(family, lengths, sc, gdt, data=None, skew=0):
    w, g, m, v = data or O.make_list(family, lengths, 11, sc, F32, gdt)
    return _bufs([w, [t.to(BF) for t in w], g, m, v], lengths, skew)


def _master_list(lname, family, sc, gdt, clip):
    K = K_()
    L = LISTS[lname]
    sc = _sc_of(family, sc)
    name = f"master list {lname} {family} g{'bf16' if gdt == BF else 'f32'}{' clip' if clip else ''}"
    bufs = _master_bufs(family, L, sc, gdt, _master_data(family, lname, sc, gdt))
    before = [b.clone() for b in bufs]
    items = list(zip(*(b.views() for b in bufs)))
    coef = None
    if clip:
        sq, st = K.grad_sqnorm(items=items), _status()
        max_norm = _max_norm(family, sq.item())
        K.adamw_master_step_multi_clip(items, sq, max_norm, status=st, **sc.kw())
        _sync()
        coef = O.clip_coef(sq.item(), max_norm)
        if coef is None:
            assert family in ("overflow", "nan_grad") and st.item() == K.STATUS_NONFINITE_GRAD
            _untouched(bufs, before, name)
            return
        assert st.item() == 0
    else:
        K.adamw_master_step_multi(items, **sc.kw())
        _sync()
    _master_check(name, bufs, before, sc, coef, family, lname, bound=not (family == "exact" and lname == "cap"))


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("gdt", [BF, F32], ids=["gbf16", "gf32"])
@pytest.mark.parametrize("family", O.FAMILIES)
def test_master_list_small(family, gdt, clip):
    _need("small")
    for sc in SC_ALL[::3] + SC_ALL[1::5]:
        _master_list("small", family, sc, gdt, clip)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("gdt", [BF, F32], ids=["gbf16", "gf32"])
@pytest.mark.parametrize("family", O.FAMILIES)
def test_master_list_mid(family, gdt, clip):
    _need("mid")
    _master_list("mid", family, SC_MID[(O.FAMILIES.index(family) + clip) % 4], gdt, clip)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("gdt", [BF, F32], ids=["gbf16", "gf32"])
@pytest.mark.parametrize("family", ["exact", "randn"])
def test_master_list_cap(family, gdt, clip):
    _need("cap")
    _master_list("cap", family, SC_CAP, gdt, clip)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("gdt", [BF, F32], ids=["gbf16", "gf32"])
@pytest.mark.parametrize("family", O.FAMILIES)
@pytest.mark.parametrize("skew", [0, 1], ids=["aligned", "unaligned"])
def test_master_single(skew, family, gdt, clip):
    """pt_adamw_master_step(_clip): one parameter, also 2 bytes (bf16) / 4 bytes (f32) off a 16-byte boundary."""
    K = K_()
    n = 1001
    sc = _sc_of(family, SC_MID[2 - clip])
    name = f"master single {'un' if skew else ''}aligned {family}{' clip' if clip else ''}"
    bufs = _master_bufs(family, [n], sc, gdt, skew=skew)
    before = [b.clone() for b in bufs]
    w, p, g, m, v = (b.views()[0] for b in bufs)
    assert p.data_ptr() % 16 == 2 * skew and w.data_ptr() % 16 == 4 * skew
    coef = None
    if clip:
        sq, st = K.grad_sqnorm(tensors=[g]), _status()
        max_norm = _max_norm(family, sq.item())
        K.adamw_master_step_clip(w, p, g, m, v, sq, max_norm, status=st, **sc.kw())
        _sync()
        coef = O.clip_coef(sq.item(), max_norm)
        if coef is None:
            assert st.item() == K.STATUS_NONFINITE_GRAD
            _untouched(bufs, before, name)
            return
    else:
        K.adamw_master_step(w, p, g, m, v, **sc.kw())
        _sync()
    _master_check(name, bufs, before, sc, coef, family, "single")


# ============================================================================== the norm pass
def _sq64(bufs_g):
    return float(bufs_g.cat().to(F64).pow(2).sum())


def _norm_tol(lname):
    gn = O.geometry(LISTS[lname], O.NORM_CAP)
    return R.gamma(O.sq_adds(gn["per_block"], gn["run_tensors"], gn["ragged"], gn["blocks"]))


def _norm_items(lname, family, form):
    """(items for grad_sqnorm, the gradient ListBuf): form bf16 list, or master list with bf16 / f32 gradients."""
    L = LISTS[lname]
    gdt = F32 if form == "master_f32" else BF
    g = _data(family, lname, SC_CAP, F32 if form != "list" else BF, gdt)[1]
    G = O.ListBuf(L, gdt, DEV).fill(g)
    if form == "list":
        return [(t, t, t, t) for t in G.views()], G
    W, Pm, M = (O.ListBuf(L, dt, DEV) for dt in (F32, BF, F32))
    return list(zip(W.views(), Pm.views(), G.views(), M.views(), M.views())), G


@pytest.mark.parametrize("form", ["list", "master_bf16", "master_f32"])
@pytest.mark.parametrize("lname", ["small", "cap"])
def test_norm_against_float64(lname, form):
    K = K_()
    _need(lname)
    items, G = _norm_items(lname, "randn", form)
    keep = G.clone()
    sq = K.grad_sqnorm(items=items)
    again = K.grad_sqnorm(items=items)
    _sync()
    ref, tol = _sq64(G), _norm_tol(lname)
    ratio = abs(sq.double().item() - ref) / (tol * ref)
    O._report(f"norm {lname}", form, ratio)
    print(f"sq {sq.item():.9e} float64 {ref:.9e} tol {tol:.3e}")
    assert ratio <= 1.0 and O.same_bits(sq, again) and O.same_bits(G.flat, keep.flat)
    assert K.device_status(torch.device(DEV), reset=False) == 0


@pytest.mark.parametrize("form", ["list", "master_bf16", "master_f32"])
def test_norm_overflow_and_zero(form):
    """g g overflows f32: the norm is +inf, nothing else is set; an all-zero list gives +0 by bits."""
    K = K_()
    items, G = _norm_items("small", "overflow", form)
    keep = G.clone()
    sq = K.grad_sqnorm(items=items)
    _sync()
    assert sq.item() == math.inf and O.same_bits(G.flat, keep.flat)
    assert K.device_status(torch.device(DEV), reset=False) == 0
    for lname in ("small", "cap"):
        items, G = _norm_items(lname, "randn", form)
        for t in G.views():
            t.zero_()
        sq = K.grad_sqnorm(items=items)
        _sync()
        assert O.same_bits(sq, torch.zeros(1))


@pytest.mark.parametrize("kind", ["bf16", "bf16_off2", "f32"])
def test_norm_single_tensor(kind):
    """pt_grad_sq: the cap list's largest tensor (the grid-strided four-way loop) and the small list's tensors."""
    K = K_()
    dtype, skew = (F32 if kind == "f32" else BF), int(kind == "bf16_off2")
    for n in (L_CAP[0], 20, 9, 1):
        g = O.make_state("randn", n, 3, None, dtype)[1]
        G = O.ListBuf([n], dtype, DEV, skew).fill([g])
        sq = K.grad_sqnorm(tensors=G.views())
        _sync()
        ref = _sq64(G)
        ratio = abs(sq.double().item() - ref) / (R.gamma(O.sq_adds_single(n)) * ref)
        O._report("norm single", f"{kind} n {n}", ratio)
        assert ratio <= 1.0 and G.gaps_intact()
    G = O.ListBuf([2051], dtype, DEV, skew).fill([O.make_state("overflow", 2051, 3, None, dtype)[1]])
    assert K.grad_sqnorm(tensors=G.views()).item() == math.inf
    G.views()[0].zero_()
    assert O.same_bits(K.grad_sqnorm(tensors=G.views()), torch.zeros(1))


# ============================================================================== the in-place scale
@pytest.mark.parametrize("factor", [0.3, 4.0])
def test_scale_list_cap(factor):
    """pt_grad_scale_multi at its capped geometry: bf16(g coef) by bits; coef == 1 stores nothing."""
    K = K_()
    _need("cap")
    items, G = _norm_items("cap", "randn", "list")
    keep = G.clone()
    sq, st = K.grad_sqnorm(items=items), _status()
    max_norm = factor * math.sqrt(sq.item())
    K.grad_scale_multi(items, sq, max_norm, status=st)
    _sync()
    coef = O.clip_coef(sq.item(), max_norm)
    assert st.item() == 0 and (coef == 1.0) == (factor > 1) and G.gaps_intact()
    if coef == 1.0:
        assert O.same_bits(G.flat, keep.flat)
    else:
        R.check_exact("scaled gradients", G.cat(), O.clip_grad(keep.cat(), coef, True))


@pytest.mark.parametrize("kind", ["bf16", "bf16_off2", "f32"])
def test_scale_single(kind):
    K = K_()
    dtype, skew = (F32 if kind == "f32" else BF), int(kind == "bf16_off2")
    n = L_CAP[0] if kind == "bf16" else 100003
    assert kind != "bf16" or n > O.STREAM_CAP * 256      # grad_scale_kernel's grid wraps
    G = O.ListBuf([n], dtype, DEV, skew).fill([O.make_state("randn", n, 4, None, dtype)[1]])
    keep = G.clone()
    g = G.views()[0]
    sq = K.grad_sqnorm(tensors=[g])
    for factor in (4.0, 0.3):
        st = _status()
        K.grad_scale(g, sq, factor * math.sqrt(sq.item()), status=st)
        _sync()
        coef = O.clip_coef(sq.item(), factor * math.sqrt(sq.item()))
        assert st.item() == 0 and G.gaps_intact()
        if factor > 1:
            assert coef == 1.0 and O.same_bits(G.flat, keep.flat)
        else:
            R.check_exact("scaled gradient", g, O.clip_grad(keep.cat(), coef, dtype == BF))


# ============================================================================== the descriptor cache
def test_descriptor_cache_passes_its_clear():
    """70 distinct lists in turn: _ADAM_DESC (64 entries, then cleared) hands every launch its own table."""
    K = K_()
    sc = SC_MID[0]
    lists = []
    n0 = len(K._ADAM_DESC)
    for i in range(70):
        L = [8 + i % 5, 37 + i, 0, 16, 1 + i % 9]
        lists.append(_bufs(O.make_list("randn", L, 200 + i, sc), L))

    def step_and_compare(bufs, i):
        single = [b.clone() for b in bufs]
        K.adamw_step_multi(list(zip(*(b.views() for b in bufs))), **sc.kw())
        for p, g, m, v in zip(*(b.views() for b in single)):
            if p.numel():
                K.adamw_step(p, g, m, v, **sc.kw())
        _sync()
        for a, b in zip(bufs, single):
            assert O.same_bits(a.flat, b.flat), f"list {i}: the list form differs from the per-tensor form"
    for i, bufs in enumerate(lists):
        step_and_compare(bufs, i)
    assert len(K._ADAM_DESC) < n0 + 70          # the clear happened on the way
    step_and_compare(lists[0], 0)


def test_zz_worst_ratio_table():
    for (tag, name), v in sorted(O.WORST.items(), key=lambda kv: (str(kv[0][0]), kv[0][1])):
        print(f"{str(tag):14s} {name:60s} {v:.3e}")
    by = {}
    for (tag, name), v in O.WORST.items():
        k = (str(tag), "bits" if name.endswith(" bits") else "ratio")
        by[k] = max(by.get(k, 0.0), v)
    for k, v in sorted(by.items()):
        print(f"max {k[0]:14s} {k[1]:6s} {v:.3e}")
