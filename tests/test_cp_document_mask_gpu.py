"""Document masks and sliding windows under context parallelism on the HIP kernels: gloo ranks on
cuda:0 (tests/_dist.py).

Ring level: ring_forward / ring_backward with a CPBand on every schedule (the zig-zag full mesh, the
reference's, the zig-zag ring) against tests/_attn_ref.py's float64 reference over the whole sequence
with the brute-force mask, per element with that kit's bounds.  The backward runs from the reference's
own (o bf16, lse f32), so it is a pure function of known inputs.

Model level: the two-layer Llama of tests/test_parallel_gpu.py with each rank given its chunk of the
document ids, the cp-summed loss and parameter gradients against the oracle run document by document
(tests/test_document_mask_model_gpu.py's per_document), norm-relative 2e-2."""
import os
import types

import pytest
import torch
import torch.distributed as dist
import torch.nn.functional as F

from tests import _attn_ref as R
from tests import _dist

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TOL = 2e-2


def doc_starts(S):
    """Document starts per batch row: boundaries inside a wave, on a 128-row block edge, one document
    over several ranks | one short document and one long one."""
    return [[0, 100, 128, 128 + 33, S - 61], [0, 37]]


def doc_ids(S):
    ids = torch.zeros(2, S, dtype=torch.long)
    for b, starts in enumerate(doc_starts(S)):
        for s in starts[1:]:
            ids[b, s:] += 1
    return ids


def brute_mask(ids, W, S):
    i = torch.arange(S)
    m = (i[None, :] <= i[:, None])[None].expand(2, S, S).clone()
    if ids is not None:
        m &= ids[:, :, None] == ids[:, None, :]
    if W is not None:
        m &= (i[:, None] - i[None, :] < W)[None]
    return m[:, None]


# ---------------------------------------------------------------- ring_forward / ring_backward
def _ring(rank, world, seq, schedule, use_docs, W):
    torch.cuda.set_device(0)
    from picotron_amd import kernels as K
    from picotron_amd import process_group_manager as pgm
    from picotron_amd import switches
    from picotron_amd.context_parallel import context_parallel as CP
    from picotron_amd.context_parallel.cp_communications import zigzag_exchange
    pgm.setup_process_group_manager(tp_size=1, cp_size=world, pp_size=1, dp_size=1)
    B, H, HKV, D = 2, 4, 2, 64
    S = seq // world
    q, k, v, do = R.make_case("randn", B, seq, seq, H, HKV, D)
    scale = R.scale_of(D)
    ids = doc_ids(seq) if use_docs else None
    mask = brute_mask(ids, W, seq)
    ref = R.ref_forward(q, k, v, scale, mask)
    o16, lse32 = ref.o.to(BF), ref.lse.float()
    bwd = R.ref_backward(q, k, v, do, lse32, scale, mask, o=o16)
    sl = slice(rank * S, (rank + 1) * S)
    with switches.override(ring_mesh=0 if schedule == "zigzag_ring" else 1,
                           ring_zigzag=0 if schedule == "reference" else 1):
        zz = CP.zigzag_enabled(S, True)
        assert zz == (schedule != "reference")
        lo = K.attn_band(B, seq, "cuda", document_ids=ids, window=W).kv_lo
        band = CP.CPBand(lo, rank, world, zz)
        kv = torch.cat([k[:, sl].reshape(B, S, -1), v[:, sl].reshape(B, S, -1)], dim=2).contiguous().cuda()
        ql, ol, dol, lsel = q[:, sl].contiguous().cuda(), o16[:, sl].contiguous().cuda(), do[:, sl].contiguous().cuda(), \
            lse32[:, :, sl].contiguous().cuda()
        if zz:
            ql, kv, ol, dol = zigzag_exchange([ql, kv, ol, dol], [1, 1, 1, 1], True)
            (lsel,) = zigzag_exchange([lsel], [2], True)
        kv = kv.reshape(B * S, -1).contiguous()
        acc, lse = CP.ring_forward(ql, kv, HKV, scale, True, zigzag=zz, band=band)
        dq, dkv = CP.ring_backward(dol, ql, kv, ol, lsel.contiguous(), HKV, scale, True, zigzag=zz, band=band)
        dkv = dkv.view(B, S, -1)
        if zz:
            acc, dq, dkv = zigzag_exchange([acc, dq, dkv], [1, 1, 1], False)
            (lse,) = zigzag_exchange([lse], [2], False)
        torch.cuda.synchronize()
    tag = f"cp{world}/S{seq}/{schedule}/r{rank}"
    R.check_acc(acc, R.Ref(o=ref.o[:, sl], A=ref.A[:, sl]), tag)
    R.check_lse(lse, ref.lse[:, :, sl], tag)
    w = HKV * D
    part = R.Ref(**{n: getattr(bwd, n)[:, sl] for n in ("dq", "dk", "dv", "M_dq", "M_dk", "M_dv", "C_dq", "C_dk")})
    dk, dv = dkv[:, :, :w].reshape(B, S, HKV, D), dkv[:, :, w:].reshape(B, S, HKV, D)
    R.check_grads_f32(dq, dk, dv, part, {"dq": torch.zeros_like(dq), "dk": torch.zeros_like(dk), "dv": torch.zeros_like(dv)}, tag)


@pytest.mark.parametrize("world,seq,schedule,use_docs,W", [
    (2, 512, "mesh", True, 150),          # documents and a window together
    (4, 1024, "mesh", True, None),        # documents
    (2, 256, "reference", False, 100),    # a window (S_local 128: the reference's schedule)
    (2, 512, "zigzag_ring", True, 200),
])
def test_ring_with_band_against_reference(world, seq, schedule, use_docs, W):
    _dist.run(_ring, world, seq, schedule, use_docs, W, device="cuda")


# ---------------------------------------------------------------- the two-layer Llama
def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _llama(rank, world, tp, cp, seq, also_full_ids):
    from oracle import picotron_oracle as O
    from picotron_amd import functional as FN
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.context_parallel import context_parallel as CP
    from picotron_amd.model import Llama
    from picotron_amd.tensor_parallel.tensor_parallel import apply_tensor_parallel
    from tests.test_parallel_gpu import CFG, _shard
    os.environ["FLASH_ATTEN"] = "1"
    torch.cuda.set_device(0)
    m = pgm.setup_process_group_manager(tp_size=tp, cp_size=cp, pp_size=1, dp_size=1)
    c = dict(CFG, max_position_embeddings=seq)
    full = {k: v.to(BF) for k, v in O.init_params(dict(CFG), seed=7).items()}
    with torch.device("cuda"):
        model = Llama(types.SimpleNamespace(**c))
        if tp > 1:
            apply_tensor_parallel(model)
    CP.apply_context_parallel(model)
    model.to(BF)
    names = dict(model.named_parameters())
    with torch.no_grad():
        for n, p in names.items():
            p.copy_(_shard(full[n], p, m.tp_rank))
    CP.enable_zigzag_residual(model)    # what the data-parallel wrappers do at cp > 1
    V = CFG["vocab_size"]
    ids = torch.randint(0, V, (2, seq + 1), generator=torch.Generator().manual_seed(11))
    inp, tgt = ids[:, :-1], ids[:, 1:]
    docs = doc_ids(seq)
    # the oracle document by document, fp32 from the same bf16 weights
    pf = {k: v.float().requires_grad_(True) for k, v in full.items()}
    cos, sin = (t.float() for t in O.get_cos_sin(seq, CFG["hidden_size"] // CFG["num_attention_heads"],
                                                 base=CFG["rope_theta"]))
    spans = [list(zip(st, st[1:] + [seq])) for st in doc_starts(seq)]
    lo = torch.cat([torch.cat([O.llama_forward(inp[b:b + 1, s:e], pf, dict(CFG), cos[s:e], sin[s:e],
                                               norm=O.rmsnorm_flash_semantics) for s, e in sp], 1)
                    for b, sp in enumerate(spans)], 0)
    loss_r = F.cross_entropy(lo.reshape(-1, V), tgt.reshape(-1))
    loss_r.backward()

    s = seq // cp
    assert CP.zigzag_enabled(s, True)
    sl = slice(m.cp_rank * s, (m.cp_rank + 1) * s)
    x, t = inp[:, sl].contiguous().cuda(), tgt[:, sl].contiguous().cuda()
    logits = model(x, document_ids=docs[:, sl].contiguous().cuda())      # this rank's chunk of the ids
    loss = FN.cross_entropy(logits.view(-1, V), t.reshape(-1))
    loss.backward()
    torch.cuda.synchronize()
    assert _rel(logits, lo[:, sl]) < TOL
    lsum = loss.detach().float().cpu().view(1)
    dist.all_reduce(lsum, group=m.cp_group)
    assert abs(lsum.item() / cp - loss_r.item()) < TOL * abs(loss_r.item())
    for n, p in names.items():
        g = p.grad.detach().float().cpu()
        dist.all_reduce(g, group=m.cp_group)
        assert _rel(g / cp, _shard(pf[n].grad, p, m.tp_rank)) < TOL, n
    if also_full_ids:   # the full rows instead of the chunk (no gather): the same bits
        with torch.no_grad():
            again = model(x, document_ids=docs.cuda())
        assert torch.equal(again, logits)


@pytest.mark.parametrize("tp,cp,seq,also_full_ids", [(1, 2, 512, True), (1, 4, 1024, False), (2, 2, 512, False)])
def test_llama_with_document_id_chunks(tp, cp, seq, also_full_ids):
    _dist.run(_llama, tp * cp, tp, cp, seq, also_full_ids, device="cuda")
