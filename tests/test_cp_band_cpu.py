"""CPU tests of document masks and sliding windows under context parallelism: the per-block bounds
(kernels.attn_block_band, context_parallel.CPBand) against a brute-force [S, S] mask for every block the
schedules run, and the three schedules on gloo ranks with a band-aware torch block implementation
against dense masked attention over the whole sequence."""
import math

import pytest
import torch

from tests import _dist

SL = 8   # local tokens per rank (half-chunks of 4)


def layouts(C):
    """Document ids [n, C * SL], one layout per row: a boundary exactly on a half-chunk edge, a
    one-token document, one document spanning three ranks (all of them at C = 2), no boundary."""
    S, h = C * SL, SL // 2
    starts = [
        [0, h, 3 * h],                                # boundaries on half-chunk edges
        [0, 5, 6, S - 3],                             # a one-token document (token 5)
        [0, 6, min(S - 2, 6 + 2 * SL + 3)],           # tokens 6 .. : a document over three ranks
        [0],                                          # no boundary at all
    ]
    ids = torch.zeros(len(starts), S, dtype=torch.int64)
    for row, st in enumerate(starts):
        for s in st[1:]:
            ids[row, s:] += 1
    return ids


def windows(C):
    return [None, 1, 3, SL // 2 + 1, C * SL + 5]


def brute(ids, W):
    """vis[b, g, p]: key p visible to query g -- same document, p <= g, g - p < W."""
    B, S = ids.shape
    g = torch.arange(S)
    vis = (g[None, :] <= g[:, None])[None].expand(B, S, S).clone()
    vis &= ids[:, :, None] == ids[:, None, :]
    if W is not None:
        vis &= (g[:, None] - g[None, :] < W)[None]
    return vis


def blocks_of(C, zigzag):
    """Every (q_owner, q_slice, k_owner, k_slice, causal) the schedules run, over all ranks."""
    S, h = SL, SL // 2
    out = []
    for r in range(C):
        out.append((r, (0, S), r, (0, S), True))                       # the diagonal
        for j in range(C):
            if j == r:
                continue
            if not zigzag:
                if j < r:
                    out.append((r, (0, S), j, (0, S), False))          # the reference schedule
            elif j < r:
                out.append((r, (0, S), j, (0, h), False))              # 'kv0'
            else:
                out.append((r, (h, S), j, (0, S), False))              # 'q1' whole
                out.append((r, (h, S), j, (0, h), False))              # 'q1' as two quarters
                out.append((r, (h, S), j, (h, S), False))
    return out


@pytest.mark.parametrize("zigzag", [False, True])
@pytest.mark.parametrize("C", [2, 4])
def test_block_bounds_match_brute_force_mask(C, zigzag):
    from picotron_amd import kernels as K
    from picotron_amd.context_parallel.context_parallel import CPBand
    ids = layouts(C)
    B, S = ids.shape
    for use_docs in (True, False):
        for W in windows(C):
            if not use_docs and W is None:
                continue
            vis = brute(ids if use_docs else torch.zeros_like(ids), W)
            lo = K.attn_band(B, S, "cpu", document_ids=ids if use_docs else None, window=W).kv_lo
            # lo is the first visible key of every token
            assert torch.equal(lo.long(), vis.long().argmax(dim=2))
            band = CPBand(lo, 0, C, zigzag)
            for (qo, qs, ko, ks, causal) in blocks_of(C, zigzag):
                bb = band.block(qo, qs, ko, ks, causal)
                assert bb is band.block(qo, qs, ko, ks, causal)   # cached
                qpos = band.positions(qo)[qs[0]:qs[1]]
                kpos = band.positions(ko)[ks[0]:ks[1]]
                assert (qpos[1:] > qpos[:-1]).all() and (kpos[1:] > kpos[:-1]).all()
                assert torch.equal(qpos, kpos) if causal else kpos.max() < qpos.min()
                Sq, Sk = qpos.numel(), kpos.numel()
                want = vis[:, qpos][:, :, kpos]
                what = (C, zigzag, use_docs, W, qo, qs, ko, ks)
                assert torch.equal(bb.mask()[:, 0], want), what
                kv_lo, q_hi = bb.kv_lo, bb.q_hi
                assert kv_lo.dtype == torch.int32 and q_hi.dtype == torch.int32
                assert tuple(kv_lo.shape) == (B, Sq) and tuple(q_hi.shape) == (B, Sk)
                assert kv_lo.min() >= 0 and kv_lo.max() <= Sk and q_hi.min() >= 0 and q_hi.max() <= Sq, what
                assert (kv_lo[:, 1:] >= kv_lo[:, :-1]).all() and (q_hi[:, 1:] >= q_hi[:, :-1]).all(), what
                # q_hi is the same mask seen from the keys: the queries that see key j are [.., q_hi[j])
                j = torch.arange(Sk)
                assert torch.equal(q_hi.long(), (kv_lo[:, :, None] <= j[None, None, :]).sum(1)), what
                if causal:
                    assert (kv_lo <= torch.arange(Sq)[None]).all() and (q_hi > j[None]).all(), what


def test_position_lists():
    from picotron_amd.context_parallel.context_parallel import CPBand
    lo = torch.zeros(1, 4 * SL, dtype=torch.int32)
    zz, ct = CPBand(lo, 1, 4, True), CPBand(lo, 1, 4, False)
    h = SL // 2
    assert ct.positions(2).tolist() == list(range(2 * SL, 3 * SL))
    assert zz.positions(1).tolist() == list(range(h, 2 * h)) + list(range(6 * h, 7 * h))
    with pytest.raises(ValueError):
        CPBand(torch.zeros(1, 4 * SL + 1, dtype=torch.int32), 0, 4, True)


# ----------------------------------------------------------------------------- the schedules
class MaskedBlocks:
    """Per-block attention in torch (f32) with the HIP kernels' accumulation contract -- fwd merges into
    (acc f32 [B, S, nh, d], lse f32 [B, nh, S]), bwd accumulates -- under the block's band (band=, an
    AttnBlockBand) or, band-less, the causal flag alone."""

    calls = 0   # block calls that carried a band

    @staticmethod
    def _mask(q, k, causal, band):
        Sq, Sk = q.shape[1], k.shape[1]
        if band is not None:
            MaskedBlocks.calls += 1
            assert band.causal == bool(causal) and (band.Sq, band.Sk) == (Sq, Sk)
            return band.mask()
        m = torch.ones(Sq, Sk, dtype=torch.bool)
        return (m.tril() if causal else m)[None, None]

    @staticmethod
    def _qkv(q, k, v):
        nh = q.shape[2]
        ex = lambda t: t.float().transpose(1, 2).repeat_interleave(nh // t.shape[2], dim=1)
        return q.float().transpose(1, 2), ex(k), ex(v)

    @staticmethod
    def fwd(q, k, v, scale, causal, acc, lse, band=None):
        qq, kk, vv = MaskedBlocks._qkv(q, k, v)
        s = (qq @ kk.transpose(-1, -2) * scale).masked_fill(~MaskedBlocks._mask(q, k, causal, band), float("-inf"))
        l = torch.logsumexp(s, dim=-1)
        o = torch.exp(s - l.unsqueeze(-1)).nan_to_num(0.0) @ vv
        new = torch.logaddexp(lse, l)
        w_old = torch.exp(lse - new).nan_to_num(0.0)
        w_blk = torch.exp(l - new).nan_to_num(0.0)
        acc.mul_(w_old.transpose(1, 2).unsqueeze(-1)).add_(o.transpose(1, 2) * w_blk.transpose(1, 2).unsqueeze(-1))
        lse.copy_(new)

    @staticmethod
    def delta(do, o):
        return (do.float() * o.float()).sum(-1).transpose(1, 2).contiguous()

    @staticmethod
    def _part(do, q, k, v, lse, delta, scale, causal, dq, dk, dv, band):
        nh, nkv = q.shape[2], k.shape[2]
        qq, kk, vv = MaskedBlocks._qkv(q, k, v)
        dd = do.float().transpose(1, 2)
        s = (qq @ kk.transpose(-1, -2) * scale).masked_fill(~MaskedBlocks._mask(q, k, causal, band), float("-inf"))
        p = torch.exp(s - lse.unsqueeze(-1))
        ds = p * (dd @ vv.transpose(-1, -2) - delta.unsqueeze(-1))
        B, Sk, _, d = k.shape
        if dq is not None:
            dq += (ds @ kk * scale).transpose(1, 2)
        if dk is not None:
            dk += (ds.transpose(-1, -2) @ qq * scale).view(B, nkv, nh // nkv, Sk, d).sum(2).transpose(1, 2)
            dv += (p.transpose(-1, -2) @ dd).view(B, nkv, nh // nkv, Sk, d).sum(2).transpose(1, 2)

    @staticmethod
    def bwd(do, q, k, v, o, lse, delta, scale, causal, dq, dk, dv, band=None):
        MaskedBlocks._part(do, q, k, v, lse, delta, scale, causal, dq, dk, dv, band)

    @staticmethod
    def bwd_dq(do, q, k, v, lse, delta, scale, causal, dq, band=None):
        MaskedBlocks._part(do, q, k, v, lse, delta, scale, causal, dq, None, None, band)

    @staticmethod
    def bwd_dkdv(do, q, k, v, lse, delta, scale, causal, dk, dv, band=None):
        MaskedBlocks._part(do, q, k, v, lse, delta, scale, causal, None, dk, dv, band)


def _schedule(rank, world, schedule, W):
    from picotron_amd import kernels as K
    from picotron_amd import process_group_manager as pgm
    from picotron_amd import switches
    from picotron_amd.context_parallel import context_parallel as CP
    from picotron_amd.context_parallel.cp_communications import zigzag_exchange
    pgm.setup_process_group_manager(tp_size=1, cp_size=world, pp_size=1, dp_size=1)
    nh, nkv, d, S = 4, 2, 16, SL
    ids = layouts(world)
    B, St = ids.shape
    g = torch.Generator().manual_seed(11)
    q = torch.randn(B, St, nh, d, generator=g)
    k = torch.randn(B, St, nkv, d, generator=g)
    v = torch.randn(B, St, nkv, d, generator=g)
    do = torch.randn(B, St, nh, d, generator=g)
    scale = 1 / math.sqrt(d)
    sl = slice(rank * S, (rank + 1) * S)
    zigzag = schedule != "reference"
    lo = K.attn_band(B, St, "cpu", document_ids=ids, window=W).kv_lo
    band = CP.CPBand(lo, rank, world, zigzag)

    # dense masked attention over the whole sequence
    qr = q.transpose(1, 2).clone().requires_grad_(True)
    kr = k.transpose(1, 2).repeat_interleave(nh // nkv, 1).requires_grad_(True)
    vr = v.transpose(1, 2).repeat_interleave(nh // nkv, 1).requires_grad_(True)
    s = (qr @ kr.transpose(-1, -2) * scale).masked_fill(~brute(ids, W)[:, None], float("-inf"))
    lse_ref = torch.logsumexp(s, dim=-1)
    o_ref = torch.softmax(s, dim=-1) @ vr
    (o_ref * do.transpose(1, 2)).sum().backward()
    dk_ref = kr.grad.view(B, nkv, nh // nkv, St, d).sum(2).transpose(1, 2)[:, sl]
    dv_ref = vr.grad.view(B, nkv, nh // nkv, St, d).sum(2).transpose(1, 2)[:, sl]

    kv = torch.cat([k[:, sl].reshape(B, S, -1), v[:, sl].reshape(B, S, -1)], dim=2).contiguous()
    MaskedBlocks.calls = 0
    with switches.override(ring_mesh=0 if schedule == "zigzag_ring" else 1):
        if zigzag:
            qz, kvz, doz = zigzag_exchange([q[:, sl], kv, do[:, sl]], [1, 1, 1], True)
            kvz = kvz.reshape(B * S, -1)
            acc, lse = CP.ring_forward(qz, kvz, nkv, scale, True, blocks=MaskedBlocks, zigzag=True, band=band)
            dq, dkv = CP.ring_backward(doz, qz, kvz, acc, lse, nkv, scale, True, blocks=MaskedBlocks, zigzag=True,
                                       band=band)
            (acc,) = zigzag_exchange([acc], [1], False)
            (lse,) = zigzag_exchange([lse], [2], False)
            dq, dkv = zigzag_exchange([dq, dkv.view(B, S, -1)], [1, 1], False)
        else:
            kvc = kv.reshape(B * S, -1)
            acc, lse = CP.ring_forward(q[:, sl], kvc, nkv, scale, True, blocks=MaskedBlocks, band=band)
            dq, dkv = CP.ring_backward(do[:, sl], q[:, sl], kvc, acc, lse, nkv, scale, True, blocks=MaskedBlocks,
                                       band=band)
            dkv = dkv.view(B, S, -1)
    assert MaskedBlocks.calls > 0
    torch.testing.assert_close(acc, o_ref.transpose(1, 2)[:, sl].detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lse, lse_ref[:, :, sl].detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dq, qr.grad.transpose(1, 2)[:, sl], rtol=1e-4, atol=1e-5)
    w = nkv * d
    torch.testing.assert_close(dkv[:, :, :w].reshape(B, S, nkv, d), dk_ref, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(dkv[:, :, w:].reshape(B, S, nkv, d), dv_ref, rtol=1e-4, atol=1e-5)
    # a band built for another layout is refused before any block runs
    with pytest.raises(ValueError):
        CP.ring_forward(q[:, sl], kv.reshape(B * S, -1), nkv, scale, True, blocks=MaskedBlocks, zigzag=zigzag,
                        band=CP.CPBand(lo, rank, world, not zigzag))


@pytest.mark.parametrize("W", [None, 3])
@pytest.mark.parametrize("schedule", ["mesh", "reference", "zigzag_ring"])
@pytest.mark.parametrize("world", [2, 4])
def test_schedules_with_band_match_dense_masked_attention(world, schedule, W):
    _dist.run(_schedule, world, schedule, W)


def _gather_ids(rank, world):
    """make_cp_band: the rank's [B, S_local] chunk (all-gathered) and the full rows give the same lo."""
    from picotron_amd import kernels as K
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.context_parallel import context_parallel as CP
    pgm.setup_process_group_manager(tp_size=1, cp_size=world, pp_size=1, dp_size=1)
    ids = layouts(world)
    B, St = ids.shape
    a = CP.make_cp_band(B, SL, "cpu", ids[:, rank * SL:(rank + 1) * SL], 3)
    b = CP.make_cp_band(B, SL, "cpu", ids, 3)
    want = K.attn_band(B, St, "cpu", document_ids=ids, window=3).kv_lo
    assert torch.equal(a.lo, want) and torch.equal(b.lo, want)
    assert (a.rank, a.world, a.S) == (rank, world, SL) and CP.make_cp_band(B, SL, "cpu") is None
    assert CP.make_cp_band(B, SL, "cpu", a) is a
    with pytest.raises(NotImplementedError, match="context parallelism"):
        CP.make_cp_band(B, SL, "cpu", K.attn_band(B, SL, "cpu", window=2))
    with pytest.raises(ValueError):
        CP.make_cp_band(B, SL, "cpu", ids[:, :SL + 1])


def test_document_id_chunks_are_gathered_over_the_cp_group():
    _dist.run(_gather_ids, 2)
