"""Attention sinks against plain float64 torch on the CPU: the scores get one more column holding the head's
sink logit, softmax, the column dropped before the product with V; gradients by autograd.  Bounds: tests/_attn_ref.py's.
Those bound the backward as a function of the lse and bf16 o it is given, so dq / dk / dv go in two steps (as in
test_attn_band_gpu.py): autograd equals ref_backward on the reference's lse and o (1e-9); the kernels meet the bounds
against ref_backward on the lse and o they stored."""
import math
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import picotron_oracle as O
from picotron_amd import kernels as K, switches
from tests import _attn_ref as R

pytestmark = pytest.mark.gpu
DEV, BF, F64 = "cuda", torch.bfloat16, torch.float64
B, H, HKV = 2, 4, 2
MASKS = {"S128": (128, None, None), "S384": (384, None, None), "S200": (200, None, None),   # S, window, rows' document cut:
         "S256-w64": (256, 64, None), "S256-docs": (256, None, (70, 161))}   # one block; tiles, pairing; padded; window; documents


def band_of(S, window, cut):
    ids = None if cut is None else (torch.arange(S, device=DEV)[None] >= torch.tensor(cut, device=DEV)[:, None]).long()
    return K.attn_band(B, S, DEV, document_ids=ids, window=window)


def sink_attention(sc, sinks, v):
    """softmax over [scores | the head's sink] without the sink's column, times v; sc [b, h, q, k], v [b, h, k, d]."""
    full = torch.cat([sc, sinks[None, :, None, None].expand(*sc.shape[:3], 1)], -1)
    return torch.softmax(full, -1)[..., :-1] @ v, torch.logsumexp(full, -1)


@pytest.mark.parametrize("family", ("random", "pm20"))
@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("D", (64, 128))
def test_forward_backward_and_sink_gradient(D, name, family):
    """dsinks: attn_sink_bwd against -sum exp(sink - lse) (dO . O) in float64 on the kernel's own stored lse and O and the
    given dO.  It is one f32 sum of a head's B S D terms t = exp(sink - lse) dO O: at most 12 adds inside delta, 4 + 6 + 3
    in the partial kernel (thread, wave butterfly, wave order), B nchunk <= 4 in the reduce, two products, expf's ulp: under
    32 roundings of 2^-24; the f32 difference sink - lse moves exp by 2^-24 |sink - lse| relative.  So |error| <= 2^-24
    (32 + max |sink - lse|) sum |t|, and bf16 sinks add half a bf16 ulp (R.U relative) per rounding."""
    S, window, cut = MASKS[name]
    q, k, v, do = R.make_case("randn", B, S, S, H, HKV, D, seed=len(name))
    sinks = math.sqrt(2.0) * torch.randn(H, generator=torch.Generator().manual_seed(D + S))   # about N(0, 2)
    if family == "pm20":
        sinks[0], sinks[1] = 20.0, -20.0   # the sink dominates head 0's rows and vanishes from head 1's
    sinks, scale, band = sinks.to(BF), R.scale_of(D), band_of(S, window, cut)
    mask = band.mask().cpu()
    qd, kd, vd, dod, sd = (t.to(DEV) for t in (q, k, v, do, sinks))
    o, lse = K.attn_fwd(qd, kd, vd, scale, True, band=band if (window or cut) else None, sinks=sd)
    dq, dk, dv, delta = K.attn_bwd(dod, qd, kd, vd, o, lse, scale, True, band=band if (window or cut) else None)
    q6, k6, v6 = (t.to(F64).requires_grad_(True) for t in (q, k, v))
    kk, vv = (t.repeat_interleave(H // HKV, 2).transpose(1, 2) for t in (k6, v6))
    sc = (q6.transpose(1, 2) @ kk.transpose(-1, -2) * scale).masked_fill(~mask, float("-inf"))
    o6, lse6 = (t.transpose(1, 2) if t.dim() == 4 else t for t in sink_attention(sc, sinks.to(F64), vv))
    o6.backward(do.to(F64))
    p = torch.exp(sc - lse6[..., None]).detach()
    fwd = R.Ref(o=o6.detach(), lse=lse6.detach(), A=(p @ vv.detach().abs()).transpose(1, 2))
    exact = R.ref_backward(q, k, v, do, fwd.lse, scale, mask, o=fwd.o)
    assert max(R.norm_rel(a, b.grad) for a, b in ((exact.dq, q6), (exact.dk, k6), (exact.dv, v6))) < 1e-9
    tag = f"sink/d{D}/{name}/{family}"
    R.check_out(o, fwd, tag)
    R.check_lse(lse, fwd.lse, tag)
    bwd = R.ref_backward(q, k, v, do, lse.cpu(), scale, mask, o=o.cpu())
    R.check_delta(delta, bwd, tag)
    R.check_grads(dq, dk, dv, bwd, tag)
    x = sinks.to(F64)[None, :, None] - lse.cpu().to(F64)
    prod = (do.to(F64) * o.cpu().to(F64)).transpose(1, 2)                                        # [B, H, S, D]
    want = -(torch.exp(x) * prod.sum(-1)).sum((0, 2))
    bound = 2.0 ** -24 * (32 + float(x.abs().max())) * (torch.exp(x) * prod.abs().sum(-1)).sum((0, 2))
    g32 = K.attn_sink_bwd(lse, delta, sd, sink=K.DW_STORE_F32)
    R.check("dsinks_f32", g32, want, bound, tag)
    assert torch.equal(g32, K.attn_sink_bwd(lse, delta, sd, sink=K.DW_STORE_F32))                # two launches, equal bits
    R.check("dsinks_bf16", K.attn_sink_bwd(lse, delta, sd), want, bound + R.U * want.abs(), tag)
    g0 = torch.tensor([0.75, -1.5, 3.0, 0.01])
    acc = K.attn_sink_bwd(lse, delta, sd, out=g0.to(DEV), sink=K.DW_ACC_F32)
    R.check("dsinks_f32_acc", acc, want + g0.to(F64), bound + 2.0 ** -24 * (want + g0.to(F64)).abs(), tag)
    acc = K.attn_sink_bwd(lse, delta, sd, out=g0.to(BF).to(DEV), sink=K.DW_ACC_BF16)
    tot = want + g0.to(BF).to(F64)
    R.check("dsinks_bf16_acc", acc, tot, bound + R.U * (want.abs() + tot.abs()), tag)


@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("name", ("S384", "S256-w64"))
def test_minus_inf_sink_is_the_plain_kernel(D, name):
    """bf16 -inf is the plain initial state (m = -inf, l = 0): the plain kernel's regular launch, bit for bit."""
    S, window, _ = MASKS[name]
    q, k, v, _ = (t.to(DEV) for t in R.make_case("randn", B, S, S, H, HKV, D))
    band = band_of(S, window, None) if window else None
    with switches.override(attn_kv_chunk=0):
        o0, l0 = K.attn_fwd(q, k, v, R.scale_of(D), True, band=band)
    o1, l1 = K.attn_fwd(q, k, v, R.scale_of(D), True, band=band, sinks=torch.full((H,), float("-inf"), dtype=BF, device=DEV))
    assert torch.equal(o0.view(torch.int16), o1.view(torch.int16)) and torch.equal(l0.view(torch.int32), l1.view(torch.int32))


MS, TOL = 128, 2e-2   # tests/test_qk_norm_model_gpu.py's metric and tolerance for the same model
MCFG = dict(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_key_value_heads=2, vocab_size=512,
            rms_norm_eps=1e-5, rope_theta=10000.0, num_hidden_layers=2, max_position_embeddings=MS, attention_sinks=True)


def ref_llama(ids, p, masks, cut=None):
    """The float64 model from the oracle's pieces plus the sink column; cut: the residual stream after `cut` layers."""
    nh, nkv, d = 4, 2, 64
    cos, sin = (t.to(F64) for t in O.get_cos_sin(MS, d, base=10000.0))
    norm = lambda x, w: x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-5) * w   # noqa: E731
    x = F.embedding(ids, p["embedding.weight"])
    b, s, _ = x.shape
    for i, mask in enumerate(masks[:cut]):
        w = {n[len(f"decoder_layers.{i}."):]: t for n, t in p.items() if n.startswith(f"decoder_layers.{i}.")}
        h = norm(x, w["input_layernorm.weight"])
        q, k, v = (O.linear(h, w[f"attention.{n}_proj.weight"]).view(b, s, -1, d).transpose(1, 2) for n in "qkv")
        q, k = O.apply_rotary_pos_emb(q, cos, sin), O.apply_rotary_pos_emb(k, cos, sin).repeat_interleave(nh // nkv, 1)
        sc = (q @ k.transpose(-1, -2) / math.sqrt(d)).masked_fill(~mask, float("-inf"))
        o = sink_attention(sc, w["attention.sinks"], v.repeat_interleave(nh // nkv, 1))[0]
        x = x + O.linear(o.transpose(1, 2).reshape(b, s, nh * d), w["attention.out_proj.weight"])
        x = x + O.mlp(norm(x, w["post_attention_layernorm.weight"]), *(w[f"mlp.{n}_proj.weight"] for n in ("gate", "up", "down")))
    return x if cut else O.linear(norm(x, p["final_norm.weight"]), p["final_proj.weight"])


@pytest.mark.parametrize("alternating", (False, True), ids=("full", "alternating"))
def test_llama_two_layers(monkeypatch, alternating):
    for name, val in (("DEVICE", "cuda"), ("LOCAL_RANK", "0"), ("CONTEXT_PARALLEL", "0"), ("FLASH_ATTEN", "1")):
        monkeypatch.setenv(name, val)
    from picotron_amd import functional as FN, process_group_manager as pgm
    from picotron_amd.model import Llama
    pgm.setup_process_group_manager(1, 1, 1, 1)
    torch.manual_seed(0)
    cfg = dict(MCFG, **(dict(layer_types=["sliding_attention", "full_attention"], sliding_window=64) if alternating else {}))
    with torch.device("cuda"):
        model = Llama(types.SimpleNamespace(**cfg))
    model.to(BF)
    with torch.no_grad():
        for n, t in model.named_parameters():
            if n.endswith("attention.sinks"):
                assert t.dtype == BF and tuple(t.shape) == (4,) and float(t.float().abs().max()) < 0.2   # HF's init
                t.copy_(math.sqrt(2.0) * torch.randn(4))
    V = cfg["vocab_size"]
    ids = torch.randint(0, V, (2, MS + 1), generator=torch.Generator().manual_seed(1))
    inp, tgt = ids[:, :-1], ids[:, 1:]
    logits = model(inp.cuda())
    loss = FN.cross_entropy(logits.view(-1, V), tgt.reshape(-1).cuda())
    loss.backward()
    p = {k: v.detach().to(F64).cpu().requires_grad_(True) for k, v in model.named_parameters()}
    full, win = (K.attn_band(2, MS, DEV, window=w).mask().cpu() for w in (None, 64))
    masks = [win, full] if alternating else [full, full]
    lr = ref_llama(inp, p, masks)
    loss_r = F.cross_entropy(lr.reshape(-1, V), tgt.reshape(-1))
    loss_r.backward()
    errs = {n: R.norm_rel(t.grad, p[n].grad) for n, t in model.named_parameters()}
    print(f"sinks llama alternating={alternating}: worst grad {max(errs.values()):.3e} ({max(errs, key=errs.get)})")
    assert abs(loss.float().item() - loss_r.item()) < TOL * abs(loss_r.item()) and R.norm_rel(logits, lr.detach()) < TOL
    assert "decoder_layers.0.attention.sinks" in errs and max(errs.values()) < TOL, errs
    if alternating:   # layer 0's window cuts: its output is the windowed reference's, not the all-full one's
        with torch.no_grad():
            x0 = model.decoder_layers[0](model.embedding(inp.cuda()), document_ids=K.attn_band(2, MS, DEV, window=64))
            want, other = (ref_llama(inp, p, [m], cut=1) for m in (win, full))
        near, far = R.norm_rel(x0[:, 64:], want[:, 64:]), R.norm_rel(x0[:, 64:], other[:, 64:])
        assert R.norm_rel(x0, want) < TOL and R.norm_rel(x0[:, :64], other[:, :64]) < TOL and far > 4 * near, (near, far)
