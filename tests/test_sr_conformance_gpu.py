"""The stochastic-rounding AdamW kernels of csrc/adamw.hip (list and single-tensor step, clipped or not, bf16
and f32 gradients, the rounding alone, the norm over the SR table) through picotron_amd.kernels against
tests/_sr_ref.py, bit for bit.  The reference, its one allowance (an f32 ulp of master_expect's fma emulation,
on at most BIT_CAP of the elements) and the checker's self-test: tests/_sr_ref.py, tests/test_sr_checker_cpu.py.

Lists: `small` and `mid` of tests/test_optim_conformance_gpu.py (one workgroup with 35 tensors in its run,
ragged tails and empty tensors; 257 workgroups x 512 chunks, two trips per thread: prologue and drain of the
two-ahead loads) and, for `randn`, `cap` (1024 workgroups x 1612 chunks: the steady state and the rotation,
runs that start in mid-tensor).  Every tensor of a list is carved from one sentinel-filled allocation per
field; gaps and gradients are compared by bits after every launch.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import _optim_ref as O
from tests import _sr_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32

L_SMALL = [0, 1, 7, 8, 9, 16, 3, 20, 5, 12, 0, 2, 17, 4, 8, 15, 6, 19, 1, 10, 0, 13, 7, 9, 16, 11, 18, 14, 2, 8, 20, 3, 0, 5,
           16, 7, 1, 9, 12, 0]
L_MID = [2048, 1001, 512 * 2048, 37, 3 * 5 * 7, 8]
L_CAP = [10_000_136, 1001, 37, 3 * 5 * 7, 8, 0, 1_500_008, 2048, 1001, 37, 3 * 5 * 7, 8, 1_700_003, 37, 0]
LISTS = dict(small=L_SMALL, mid=L_MID, cap=L_CAP)
FAMILIES = ("randn", "fresh", "tiny", "overflow", "nan_grad", "exact")
SEED = 0x123456789ABCDEF0
GDT = dict(gbf16=BF, gf32=F32)


def K_():
    from picotron_amd import kernels
    return kernels


def _streams(n):
    """distinct ids, not in list order, the largest one allowed among them"""
    return [SR.STREAMS - 1 if i == 1 else (5 * i + 3) % 997 for i in range(n)]


def _need(lname):
    """The geometry a test on this list relies on."""
    L = LISTS[lname]
    gs = O.geometry(L, O.STEP_CAP)
    if lname == "small":
        assert len(L) == 40 and max(L) <= 20 and {0, 1, 7, 8, 9, 16} <= set(L) and L[-1] == 0 and 0 in L[1:-1]
        assert gs["blocks"] == 1 and gs["run_tensors"] == sum(1 for n in L if n) == 35
    elif lname == "mid":
        assert (gs["blocks"], gs["per_block"]) == (257, 512) and gs["seg_full"] == 512
    else:
        assert gs["blocks"] == 1024 and gs["per_block"] >= 1025 and gs["per_block"] % 256 != 0
        assert gs["seg_full"] >= 1025 and gs["run_tensors"] >= 3 and gs["mid_start"]   # three trips and more: steady state
    return gs


@functools.lru_cache(maxsize=4)
def _data(family, lname, gdt, seed=0):
    """p, m, v in bf16, g in gdt (none of these families is built against the scalars)"""
    return O.make_list(family, LISTS[lname], seed, None, BF, gdt)


def _bufs(data, lengths, skew=0):
    return [O.ListBuf(lengths, ts[0].dtype if ts else BF, DEV, skew).fill(ts) for ts in data]


def _items(bufs, streams):
    return [it + (st,) for it, st in zip(zip(*(b.views() for b in bufs)), streams)]


def _status():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def _max_norm(family, sq):
    norm = math.sqrt(sq) if math.isfinite(sq) and sq > 0 else 1.0
    return (4.0 if family in O.COEF_ONE else 0.3) * norm


def _cpu(bufs):
    return [b.to("cpu") for b in bufs]


def _list_step(lname, family, sc, gdt, clip, step, bufs=None, seed=SEED):
    """One pt_adamw_sr_step_multi(_clip) launch over the list and its check; returns the buffers after."""
    K = K_()
    L = LISTS[lname]
    sc = O.EXACT_S if family == "exact" else sc
    name = f"sr list {lname} {family} g{'bf16' if gdt == BF else 'f32'}{' clip' if clip else ''} t{step}"
    bufs = bufs or _bufs(_data(family, lname, gdt), L)
    before = _cpu(bufs)
    streams = _streams(len(L))
    items = _items(bufs, streams)
    coef = None
    if clip:
        sq, st = K.grad_sqnorm(items=items), _status()
        max_norm = _max_norm(family, sq.item())
        K.adamw_sr_step_multi_clip(items, sq, max_norm, status=st, seed=seed, step=step, **sc.kw())
        torch.cuda.synchronize()
        coef = O.clip_coef(sq.item(), max_norm)
        if coef is None:
            assert family in ("overflow", "nan_grad") and st.item() == K.STATUS_NONFINITE_GRAD
            for b, b0 in zip(bufs, before):
                assert O.same_bits(b.flat, b0.flat), f"{name}: a skipped step wrote something"
            return bufs
        assert st.item() == 0 and (coef == 1.0) == (family in O.COEF_ONE), coef
    else:
        K.adamw_sr_step_multi(items, seed=seed, step=step, **sc.kw())
        torch.cuda.synchronize()
    P, G, M, V = bufs
    assert O.same_bits(G.flat, before[1].flat), f"{name}: the gradients were written"
    SR.check_sr_list(name, (P, M, V), before, streams, sc, seed, step, coef)
    if family == "exact":   # every f32 result is a bf16 value: the plain cast, bit for bit
        g = before[1].cat() if gdt == BF else before[1].cat().to(BF)
        O.check_exact_step(name, (P.cat(), M.cat(), V.cat()), (before[0].cat(), g, before[2].cat(), before[3].cat()), sc, "sr")
    return bufs


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
@pytest.mark.parametrize("gdt", list(GDT))
@pytest.mark.parametrize("family", FAMILIES)
def test_sr_list_small(family, gdt, clip):
    _need("small")
    for t in (1, 3, 1000):
        _list_step("small", family, O.scalars(t=t), GDT[gdt], clip, t)


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
@pytest.mark.parametrize("gdt", list(GDT))
@pytest.mark.parametrize("family", FAMILIES)
def test_sr_list_mid(family, gdt, clip):
    _need("mid")
    _list_step("mid", family, O.scalars(t=3, lr=3e-4, wd=0.01), GDT[gdt], clip, 3)


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
@pytest.mark.parametrize("gdt", list(GDT))
def test_sr_list_cap(gdt, clip):
    _need("cap")
    _list_step("cap", "randn", O.scalars(t=3, lr=3e-4, wd=0.01), GDT[gdt], clip, 3)


def test_sr_list_chained_steps():
    """Three steps t = 1, 2, 3 on the mid list with new gradients each: the kernel's state after each equals the
    reference chained from ITS OWN previous output."""
    K = K_()
    _need("mid")
    streams = _streams(len(L_MID))
    bufs = _bufs(_data("randn", "mid", BF), L_MID)
    ref = _cpu(bufs)
    for t in (1, 2, 3):
        g = O.make_list("randn", L_MID, 100 + t)[1]
        bufs[1] = O.ListBuf(L_MID, BF, DEV).fill(g)
        ref[1] = O.ListBuf(L_MID, BF).fill(g)
        sc = O.scalars(t=t)
        K.adamw_sr_step_multi(_items(bufs, streams), seed=SEED, step=t, **sc.kw())
        torch.cuda.synchronize()
        want16, want32, r = SR.expect_list(ref, streams, sc, SEED, t)
        SR.check_sr_step(f"chained t{t}", [bufs[i].cat() for i in (0, 2, 3)], want32, r)
        for i, w in zip((0, 2, 3), want16):
            ref[i].fill(list(torch.split(w, L_MID)))


# ============================================================================== the rounding alone
CRAFTED = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F800001, 0xFFFFFFFF, 0x7FC00000, 0xFFC00001, 0x00000001,
           0x00004000, 0x0000FFFF, 0x00010000, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x7F7F0001, 0x3F800000,
           0x3F800001, 0x3F807FFF, 0x3F808000, 0x3F80FFFF, 0xBF80FFFF]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_sr_cast_bits(which):
    """crafted patterns (every one at every position of a chunk, so with eight different draws) and 2^16 random
    finite values; a ragged length, an output 2 bytes off a 16-byte boundary"""
    K = K_()
    gen = torch.Generator().manual_seed(5 + which)
    rnd = torch.randint(-2 ** 31, 2 ** 31, (1 << 16,), generator=gen, dtype=torch.int64).to(torch.int32)
    rnd = torch.where((rnd & 0x7F800000) == 0x7F800000, rnd & ~0x40000000, rnd)   # finite
    crafted = torch.tensor(np.array(CRAFTED * 9, dtype=np.uint32).view(np.int32))   # 23 is odd: every position mod 8
    x = torch.cat([crafted, rnd, crafted[:3]]).view(F32)
    assert x.numel() % 8 and len(CRAFTED) % 2
    stream, step = 12345 + which, 7
    out = O.ListBuf([x.numel()], BF, DEV, skew=1)
    y = out.views()[0]
    assert y.data_ptr() % 16 == 2
    K.sr_cast_bf16(x.to(DEV), SEED, step, stream, which, out=y)
    torch.cuda.synchronize()
    assert out.gaps_intact()
    SR.check_sr_cast(f"cast which {which}", y.cpu(), x, SR.sr_bits(SEED, stream, step, which, x.numel()))
    z = K.sr_cast_bf16(x.to(DEV), SEED, step, stream, which)   # its own output
    assert not bool(SR.differs(z.cpu(), y.cpu()).any())


def test_sr_cast_refuses_bad_arguments():
    K = K_()
    x = torch.zeros(8, device=DEV)
    for kw in (dict(step=0), dict(stream=SR.STREAMS), dict(stream=-1), dict(which=3), dict(seed=1 << 64)):
        args = dict(seed=SEED, step=1, stream=0, which=0)
        args.update(kw)
        with pytest.raises(ValueError):
            K.sr_cast_bf16(x, **args)


# ============================================================================== geometry independence
L_GEO = [1001, 8, 17, 2048 + 5, 3, 0, 300 * 8 + 1]
S_GEO = [4, 900, 2, SR.STREAMS - 1, 77, 6, 31]


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
@pytest.mark.parametrize("gdt", list(GDT))
def test_sr_bits_do_not_depend_on_the_launch(gdt, clip):
    """the same tensors with the same stream ids: in a shuffled list, padded with other tensors, each alone
    through the single-tensor entry, and at a 2-byte-misaligned view -- all bit-identical to the list's result"""
    K = K_()
    gdt = GDT[gdt]
    sc, step = O.scalars(t=2), 2
    data = O.make_list("randn", L_GEO, 9, sc, BF, gdt)
    sq = torch.full((1,), 4.0, dtype=F32, device=DEV)   # one coefficient for every form: 0.5 / (2 + 1e-6)
    st = _status()

    def run_list(order, pad):
        bufs = _bufs(data, L_GEO)
        items = _items(bufs, S_GEO)
        items = [items[i] for i in order]
        extra = _bufs(O.make_list("randn", [40, 9], 10, sc, BF, gdt), [40, 9])
        if pad:
            more = _items(extra, [555, 556])
            items = [more[0]] + items[:3] + [more[1]] + items[3:]
        if clip:
            K.adamw_sr_step_multi_clip(items, sq, 0.5, status=st, seed=SEED, step=step, **sc.kw())
        else:
            K.adamw_sr_step_multi(items, seed=SEED, step=step, **sc.kw())
        torch.cuda.synchronize()
        return [bufs[i].cat() for i in (0, 2, 3)]

    def run_single(skew):
        outs = [[], [], []]
        for t, n in enumerate(L_GEO):
            bufs = _bufs([[d[t]] for d in data], [n], skew)
            p, g, m, v = (b.views()[0] for b in bufs)
            if n:
                assert p.data_ptr() % 16 == 2 * skew
                if clip:
                    K.adamw_sr_step_clip(p, g, m, v, S_GEO[t], sq, 0.5, status=st, seed=SEED, step=step, **sc.kw())
                else:
                    K.adamw_sr_step(p, g, m, v, S_GEO[t], seed=SEED, step=step, **sc.kw())
            torch.cuda.synchronize()
            assert all(b.gaps_intact() for b in bufs)
            for o, b in zip(outs, (bufs[0], bufs[2], bufs[3])):
                o.append(b.cat())
        return [torch.cat(o) for o in outs]

    base = run_list(range(len(L_GEO)), False)
    before = [O.ListBuf(L_GEO, d[0].dtype).fill(d) for d in data]
    _, want32, r = SR.expect_list(before, S_GEO, sc, SEED, step, O.clip_coef(4.0, 0.5) if clip else None)
    SR.check_sr_step("geometry base", base, want32, r)
    for name, got in (("shuffled", run_list([3, 0, 6, 5, 1, 4, 2], False)), ("padded", run_list(range(len(L_GEO)), True)),
                      ("single", run_single(0)), ("single, 2 bytes off", run_single(1))):
        for o, a, b in zip("pmv", got, base):
            assert O.same_bits(a, b), f"{name}: {o} differs from the list's result"
    assert st.item() == 0


def test_sr_bits_depend_on_seed_stream_and_step():
    K = K_()
    sc = O.scalars(t=2)
    data = O.make_list("randn", [4096], 3, sc)

    def run(seed, stream, step):
        bufs = _bufs(data, [4096])
        K.adamw_sr_step_multi(_items(bufs, [stream]), seed=seed, step=step, **sc.kw())
        torch.cuda.synchronize()
        return torch.cat([bufs[i].cat() for i in (0, 2, 3)])
    base = run(SEED, 5, 2)
    assert O.same_bits(run(SEED, 5, 2), base)
    for other in (run(SEED + 1, 5, 2), run(SEED ^ (1 << 63), 5, 2), run(SEED, 6, 2), run(SEED, 5, 3)):
        assert float(SR.differs(other, base).double().mean()) > 0.2   # about half of the roundings are coin flips


# ============================================================================== clip
@pytest.mark.parametrize("gdt", list(GDT))
def test_sr_nonfinite_norm_skips_the_step(gdt):
    K = K_()
    sc = O.scalars(t=1)
    n = 1001
    for bad in (math.inf, math.nan):
        sq = torch.full((1,), bad, dtype=F32, device=DEV)
        for single in (False, True):
            bufs = _bufs(O.make_list("randn", [n], 4, sc, BF, GDT[gdt]), [n], skew=int(single))
            before = _cpu(bufs)
            st = _status()
            if single:
                K.adamw_sr_step_clip(*(b.views()[0] for b in bufs), 3, sq, 1.0, status=st, seed=SEED, step=1, **sc.kw())
            else:
                K.adamw_sr_step_multi_clip(_items(bufs, [3]), sq, 1.0, status=st, seed=SEED, step=1, **sc.kw())
            torch.cuda.synchronize()
            assert st.item() == K.STATUS_NONFINITE_GRAD
            for b, b0 in zip(bufs, before):
                assert O.same_bits(b.flat, b0.flat)


@pytest.mark.parametrize("lname", ["small", "mid"])
def test_sr_norm_equals_the_plain_lists(lname):
    """pt_grad_sq_sr_multi: the same kernel over another table -- the same bits as the bf16 list's norm and as the
    master list's norm on f32 gradients"""
    K = K_()
    L = LISTS[lname]
    sc = O.scalars(t=3)
    for gdt in (BF, F32):
        bufs = _bufs(_data("randn", lname, gdt), L)
        keep = bufs[1].clone()
        sq = K.grad_sqnorm(items=_items(bufs, _streams(len(L))))
        G = bufs[1].views()
        if gdt == BF:
            other = K.grad_sqnorm(items=[(g, g, g, g) for g in G])
        else:
            W, Pm, Mm = (O.ListBuf(L, dt, DEV) for dt in (F32, BF, F32))
            other = K.grad_sqnorm(items=list(zip(W.views(), Pm.views(), G, Mm.views(), Mm.views())))
        torch.cuda.synchronize()
        assert O.same_bits(sq, other) and math.isfinite(sq.item()) and sq.item() > 0
        assert O.same_bits(bufs[1].flat, keep.flat)

