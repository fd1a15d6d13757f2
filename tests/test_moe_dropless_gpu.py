"""Dropless mixture-of-experts on the GPU: the segment plan against tests/_moe_ref.py's integer plan re-based
to 128-aligned offsets, the three segment-GEMM forms per element against the float64 product
(tests/_gemm_ref.py's families and bounds) on handcrafted segments, and functional.MoEFunction with
capacity_factor=None stage by stage against the float64 block of tests/test_moe_block_gpu.py with nothing
dropped."""
import functools

import pytest
import torch

from tests import _gemm_ref as G
from tests import _moe_ref as R
from tests import test_moe_block_gpu as B

DEV = "cuda"
pytestmark = pytest.mark.gpu
BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
A = 128


def ref_plan_dropless(idx, E):
    """(slot, src, seg, tile_expert, counts): R.ref_plan at a capacity that cannot drop, re-based."""
    T, k = idx.shape
    C = T * k
    slot0, _ = R.ref_plan(idx, E, C)
    flat = idx.reshape(-1).long()
    counts = torch.bincount(flat, minlength=E)
    seg = torch.zeros(E + 1, dtype=torch.long)
    seg[1:] = ((counts + A - 1) // A * A).cumsum(0)
    slot = seg[flat] + (slot0.reshape(-1).long() - flat * C)
    rows = A * ((T * k + E * (A - 1)) // A)
    src = torch.full((rows,), -1, dtype=torch.long)
    src[slot] = torch.arange(T * k)
    tile = torch.full((rows // A,), -1, dtype=torch.long)
    for e in range(E):
        tile[seg[e] // A:seg[e + 1] // A] = e
    return slot.reshape(T, k).to(I32), src.to(I32), seg.to(I32), tile.to(I32), counts


def _hand_idx():
    """E 4, k 1: counts 128 (no padding), 129 (one row past a multiple), 0, 5, interleaved."""
    idx = torch.tensor([0] * 128 + [1] * 129 + [3] * 5)
    return idx[torch.randperm(idx.numel(), generator=R.gen("dropless hand"))].reshape(-1, 1).to(I32), 4


PLAN_CASES = ["hand", ("dominant", 8, 60, 4), ("dominant", 1025, 60, 4), ("randn", 511, 8, 2), ("randn", 512, 8, 2),
              ("randn", 513, 8, 2), ("randn", 1000, 1, 1), ("randn", 63, 128, 8)]


@pytest.mark.parametrize("case", PLAN_CASES, ids=str)
def test_plan(case):
    from picotron_amd import kernels as K
    if case == "hand":
        idx, E = _hand_idx()
    else:
        fam, T, E, k = case
        idx = R.ref_select(R.make_logits(fam, T, E), k)
    slot, src, seg, tile, counts = ref_plan_dropless(idx, E)
    if case == "hand":
        assert counts.tolist() == [128, 129, 0, 5] and seg.tolist() == [0, 128, 384, 384, 512]
    if case != "hand" and case[1] == 8:
        assert int((counts == 0).sum()) > 0   # experts with no items
    got = [K.moe_plan_dropless(idx.to(DEV), E) for _ in range(2)]
    assert got[0][1].numel() == K.moe_dropless_rows(idx.shape[0], E, idx.shape[1])
    for name, g, g2, w in zip(("slot", "src", "seg", "tile_expert"), got[0], got[1], (slot, src, seg, tile)):
        R.check_exact(name, g, w)
        assert torch.equal(g, g2), name


# ---------------------------------------------------------------------------------------- segment GEMMs
SEG = [0, 0, 128, 512, 640]    # lengths 0, 128, 384, 128
TILE = [1, 2, 2, 2, 3, -1]     # ... and an unused tail tile
ROWS, NE = 768, 4


def _seg_dev():
    return torch.tensor(SEG, dtype=I32, device=DEV), torch.tensor(TILE, dtype=I32, device=DEV)


def _table(K, p0, p1, ld):
    return K.moe_seg_table_host([t.data_ptr() for t in p0], [t.data_ptr() for t in p1] if p1 else None, ld).to(DEV)


@pytest.mark.parametrize("family", ["ints", "randn"])
@pytest.mark.parametrize("form,N,Kc,split", [(0, 512, 192, 256), (0, 384, 64, 128), (0, 256, 128, 256),
                                             (1, 512, 192, 128), (1, 384, 64, 64)])
def test_forward_and_dx_forms(family, form, N, Kc, split):
    """form 0: split along N (gate|up); form 1: along the contraction ([Wg; Wu]); split == full: one pointer."""
    from picotron_amd import kernels as K
    seg, tile = _seg_dev()
    x = G.sentinel_cpu((ROWS, Kc), BF)   # the tail rows hold NaN: a tile of expert -1 reads nothing
    cases, w0, w1 = {}, [], []
    for e in range(NE):
        n = SEG[e + 1] - SEG[e]
        a, b = G.make_case(family, max(n, 128), N, Kc, seed=e)   # (an empty expert still has weights)
        cases[e] = (a[:n], b)
        x[SEG[e]:SEG[e + 1]] = a[:n]
        full = split == (N if form == 0 else Kc)
        if form == 0:
            w = b.t().contiguous()          # [N, K], K-contiguous
            w0.append(w[:split].contiguous().to(DEV)), w1.append(None if full else w[split:].contiguous().to(DEV))
        else:
            w0.append(b[:split].contiguous().to(DEV)), w1.append(None if full else b[split:].contiguous().to(DEV))
    table = _table(K, w0, None if w1[0] is None else w1, Kc if form == 0 else N)
    out = G.sentinel_cpu((ROWS, N), BF).to(DEV)
    K.moe_gemm_seg(form, x.to(DEV), table, seg, tile, N, Kc, split, NE, out=out)
    out = out.cpu()
    for e in range(1, NE):
        a, b = cases[e]
        G.check_case(family, out[SEG[e]:SEG[e + 1]], a, b, G.EPI_BF16, tag="moe-seg", name=f"form{form} e{e}")
    assert bool((out[SEG[NE]:].view(torch.int16) == 0).all())   # the tail: zeros


@pytest.mark.parametrize("family", ["ints", "randn"])
@pytest.mark.parametrize("epi", [G.EPI_BF16, G.EPI_BF16_ACC, G.EPI_F32, G.EPI_F32_ACC])
@pytest.mark.parametrize("Nout,Kin,parts", [(256, 256, 2), (128, 384, 1)])
def test_dw_form(family, epi, Nout, Kin, parts):
    from picotron_amd import kernels as K
    seg, _ = _seg_dev()
    dt = G.sink_dtype(epi)
    acc = epi in (G.EPI_BF16_ACC, G.EPI_F32_ACC)
    dy, x = G.sentinel_cpu((ROWS, Nout), BF), G.sentinel_cpu((ROWS, Kin), BF)
    cases, olds, sinks = {}, [], []
    for e in range(NE):
        n = SEG[e + 1] - SEG[e]
        if n:
            a, b = G.make_case(family, Nout, Kin, n, seed=e)   # a = dY_e^T [Nout, n], b = X_e [n, Kin]
            cases[e] = (a, b)
            dy[SEG[e]:SEG[e + 1]], x[SEG[e]:SEG[e + 1]] = a.t(), b
        old = G.make_old(family, Nout, Kin, dt, seed=e) if acc else G.sentinel_cpu((Nout, Kin), dt)
        olds.append(old)
        sinks.append([p.contiguous().to(DEV) for p in old.chunk(parts)])
    K.moe_experts_wgrad_seg(dy.to(DEV), x.to(DEV), sinks, seg, epi)
    got = [torch.cat([p.cpu() for p in s]) for s in sinks]
    for e, (a, b) in cases.items():
        G.check_case(family, got[e], a, b, epi, old=olds[e] if acc else None, tag="moe-seg", name=f"dW e{e} epi{epi}")
    if acc:   # the empty expert: not a bit of its sink changed
        G.check_exact("empty expert's sink", got[0], olds[0])
    else:
        assert bool((got[0] == 0).all())


# ------------------------------------------------------------------------------------------------ block
T, H, I = 192, 128, 128


@functools.lru_cache(maxsize=None)
def _block(E, k, seed=0):
    return B._run(T, H, I, E, k, None, seed=seed)


@pytest.mark.parametrize("E,k", [(8, 2), (60, 4)])
def test_block_stages_and_gradients(E, k):
    r = _block(E, k)
    st = r["st"]
    idx, gate, probs, counts, aux = R.ref_route(st["logits"], k, True)
    R.check_exact("idx", st["idx"], idx)
    slot, src, seg, tile, cnt = ref_plan_dropless(idx, E)
    for n, w in (("slot", slot), ("src", src), ("seg", seg), ("tile_expert", tile)):
        R.check_exact(n, st[n], w)
    assert bool((slot >= 0).all()) and int(cnt[B.DEAD]) == 0
    R.check_exact("xe", st["xe"], R.ref_dispatch(r["x"], src, k))
    for n in ("gu", "hh", "ye", "dgu", "dxe"):   # padding rows and the tail: zeros
        assert bool((st[n][src < 0].view(torch.int16) == 0).all()), n
    for e in range(E):
        rows = slice(int(seg[e]), int(seg[e + 1]))
        n = rows.stop - rows.start
        if n:
            B._gemm(f"gate|up e{e}", st["gu"][rows], st["xe"][rows], torch.cat([r["wgs"][e], r["wus"][e]]).t(), H)
            B._gemm(f"down e{e}", st["ye"][rows], st["hh"][rows], r["wds"][e].t(), I)
            B._gemm(f"down dX e{e}", st["dhh"][rows], st["dye"][rows], r["wds"][e], H)
            B._gemm(f"gate|up dX e{e}", st["dxe"][rows], st["dgu"][rows], torch.cat([r["wgs"][e], r["wus"][e]]), 2 * I)
            B._gemm(f"down dW e{e}", r["g_wd"][e], st["dye"][rows].t(), st["hh"][rows], n)
            B._gemm(f"gate dW e{e}", r["g_wg"][e], st["dgu"][rows, :I].t(), st["xe"][rows], n)
            B._gemm(f"up dW e{e}", r["g_wu"][e], st["dgu"][rows, I:].t(), st["xe"][rows], n)
        else:   # no token: exactly zero
            assert all(bool((g[e] == 0).all()) for g in (r["g_wd"], r["g_wg"], r["g_wu"]))
    g64 = st["gate"].to(F64)
    terms = [r["res"].to(F64)] + [g64[:, j, None] * st["ye"][slot[:, j].long()].to(F64) for j in range(k)]
    R.check_bf16("out", r["out"], R.ref_combine(st["ye"], slot, st["gate"], r["res"]), extra=B._f32_sum_allowance(terms))
    dye, dgate, mag = R.ref_combine_bwd(r["dout"], st["ye"], slot, src, st["gate"])
    R.check_bf16("dye", st["dye"], dye, zero=(src < 0)[:, None].expand_as(dye))
    R.check_dgate("dgate", st["dgate"], dgate, mag, H, slot < 0)
    ref, p = R.ref_route_bwd(st["logits"], st["idx"], st["dgate"], B.D_AUX, True)
    R.check_bf16("dlogits", st["dlogits"], ref, extra=R.route_bwd_allowance(p, st["idx"], st["dgate"], B.D_AUX, True))
    B._gemm("router dW", r["g_rw"], st["dlogits"].t(), r["x"], T)
    terms = [st["dh_router"].to(F64)] + [st["dxe"][slot[:, j].long()].to(F64) for j in range(k)]
    R.check_bf16("dh", r["dx"], R.ref_combine(st["dxe"], slot, None, st["dh_router"]), extra=B._f32_sum_allowance(terms))


def test_dominant_routing_drops_at_1_25_and_not_dropless():
    """tests/test_moe_block_gpu.py's router sends most tokens to expert 2: the capacity path at factor 1.25
    drops, the dropless path keeps every item and matches the no-drop float64 combine (checked above)."""
    cap, free = B._run(T, H, I, 8, 2, 1.25), _block(8, 2)
    assert bool((cap["st"]["slot"] < 0).any()) and bool((free["st"]["slot"] >= 0).all())
    assert torch.equal(cap["st"]["idx"], free["st"]["idx"]) and not torch.equal(cap["out"], free["out"])


def test_two_identical_calls_give_identical_bits():
    a, b = B._run(T, H, I, 8, 2, None, seed=3), B._run(T, H, I, 8, 2, None, seed=3)
    bits = lambda t: t.view(torch.int16) if t.dtype == BF else t
    for key in ("out", "aux", "dx", "g_rw"):
        assert torch.equal(bits(a[key]), bits(b[key])), key
    for key in ("g_wg", "g_wu", "g_wd"):
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a[key], b[key])), key
    for n in a["st"]:
        assert torch.equal(bits(a["st"][n]), bits(b["st"][n])), n
