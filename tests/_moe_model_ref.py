"""A composed fp32 reference of a decoder layer with a mixture-of-experts MLP, document masking and
QK-norm, beside tests/_model_ref.py and the oracle (oracle/picotron_oracle.py) whose ops it is built
from.  The routing decision is an input: top-k on bf16 logits is discontinuous, so the reference takes
the device's own selection (idx) and kept slots (slot >= 0) -- both proven exact on their stored
inputs in tests/test_moe_conformance_gpu.py / test_moe_block_gpu.py -- and differentiates everything
else itself: the router's softmax and renormalisation, the experts, the weighted sum, the aux loss."""
import math

import torch

from oracle import picotron_oracle as O


def ref_attention(x, p, cos, sin, nh, nkv, eps, norm, mask=None, pre=""):
    """oracle attention with the per-head q / k norms (when p has them) and a [B, 1, S, S] visibility mask."""
    b, s, _ = x.shape
    d = p[pre + "q_proj.weight"].shape[0] // nh
    q = O.linear(x, p[pre + "q_proj.weight"]).view(b, s, nh, d).transpose(1, 2)
    k = O.linear(x, p[pre + "k_proj.weight"]).view(b, s, nkv, d).transpose(1, 2)
    v = O.linear(x, p[pre + "v_proj.weight"]).view(b, s, nkv, d).transpose(1, 2)
    if pre + "q_norm.weight" in p:
        q, k = norm(q, p[pre + "q_norm.weight"], eps), norm(k, p[pre + "k_norm.weight"], eps)
    q, k = O.apply_rotary_pos_emb(q, cos, sin), O.apply_rotary_pos_emb(k, cos, sin)
    k, v = k.repeat_interleave(nh // nkv, dim=1), v.repeat_interleave(nh // nkv, dim=1)
    if mask is None:
        o = O.sdpa_causal(q, k, v)
    else:
        sc = (q @ k.transpose(-1, -2)) / math.sqrt(d)
        o = torch.softmax(sc.masked_fill(~mask, float("-inf")), -1) @ v
    return O.linear(o.transpose(1, 2).reshape(b, s, nh * d), p[pre + "out_proj.weight"])


def ref_moe(h, p, idx, keep, norm_topk=True, pre="mlp."):
    """(sum_j keep gate_j Expert_{idx_j}(h), aux) for h [T, H]; idx [T, k] long and keep [T, k] bool
    are the routing decision (fixed); gate and aux are functions of the reference's own logits."""
    T = h.shape[0]
    E, k = p[pre + "router.weight"].shape[0], idx.shape[1]
    probs = torch.softmax(O.linear(h, p[pre + "router.weight"]), dim=-1)
    sel = probs.gather(1, idx)
    gate = sel / sel.sum(1, keepdim=True) if norm_topk else sel
    out = torch.zeros_like(h)
    for e in range(E):
        ep = f"{pre}experts.{e}."
        for j in range(k):
            tok = ((idx[:, j] == e) & keep[:, j]).nonzero().flatten()
            if tok.numel():
                y = O.mlp(h[tok], p[ep + "gate_proj.weight"], p[ep + "up_proj.weight"], p[ep + "down_proj.weight"])
                out = out.index_add(0, tok, gate[tok, j, None] * y)
    f = torch.bincount(idx.reshape(-1), minlength=E).to(h.dtype) / (T * k)
    return out, E * (f * probs.mean(0)).sum()


def ref_moe_decoder_layer(x, p, cos, sin, nh, nkv, eps, norm, idx, keep, mask=None, norm_topk=True):
    """(layer output [B, S, H], aux) of RMSNorm -> attention -> residual -> RMSNorm -> MoE -> residual."""
    h = norm(x, p["input_layernorm.weight"], eps)
    x = x + ref_attention(h, p, cos, sin, nh, nkv, eps, norm, mask, pre="attention.")
    h = norm(x, p["post_attention_layernorm.weight"], eps)
    m, aux = ref_moe(h.reshape(-1, h.shape[-1]), p, idx, keep, norm_topk)
    return x + m.view_as(x), aux
