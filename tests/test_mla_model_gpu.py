"""model.MLAttention alone and a 2-layer Llama with multi-head latent attention (kv_lora_rank 64, H 4,
hidden 256, S 256, B 2), both q forms, dense and MoE (sigmoid, E 8 / k 2, dropless) MLPs, against an fp32
CPU autograd model assembled from the oracle's pieces: output, input gradient and every parameter
gradient, norm-relative 2e-2 (the suite's metric).  The MoE reference takes the device's own top-k
choice (a discontinuous function of bf16 logits) and differentiates everything else itself."""
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import picotron_oracle as O
from tests.test_qk_norm_model_gpu import _env, params_f32, randomise_norms, rel   # noqa: F401  (_env: autouse fixture)

pytestmark = pytest.mark.gpu
BF, TOL, S, B, H, EPS = torch.bfloat16, 2e-2, 256, 2, 4, 1e-5
DN, DR, DV = 128, 64, 128
CFG = dict(hidden_size=256, intermediate_size=512, num_attention_heads=H, num_key_value_heads=H, vocab_size=512,
           rms_norm_eps=EPS, rope_theta=10000.0, num_hidden_layers=2, max_position_embeddings=S, kv_lora_rank=64,
           q_lora_rank=None, qk_nope_head_dim=DN, qk_rope_head_dim=DR, v_head_dim=DV)
MOE = dict(num_experts=8, num_experts_per_tok=2, moe_scoring_func="sigmoid", moe_dropless=True, moe_intermediate_size=256)
NORM = O.rmsnorm_flash_semantics


def tables():
    return tuple(t.float() for t in O.get_cos_sin(S, DR, base=10000.0))


def ref_mla(x, p, cos, sin, pre=""):
    b, s, _ = x.shape
    if pre + "q_proj.weight" in p:
        q = O.linear(x, p[pre + "q_proj.weight"])
    else:
        q = O.linear(NORM(O.linear(x, p[pre + "q_a_proj.weight"]), p[pre + "q_a_layernorm.weight"], EPS), p[pre + "q_b_proj.weight"])
    q = q.view(b, s, H, DN + DR).transpose(1, 2)
    kva = O.linear(x, p[pre + "kv_a_proj_with_mqa.weight"])
    kvb = O.linear(NORM(kva[..., :-DR], p[pre + "kv_a_layernorm.weight"], EPS), p[pre + "kv_b_proj.weight"])
    kvb = kvb.view(b, s, H, DN + DV).transpose(1, 2)
    k_pe = O.apply_rotary_pos_emb(kva[..., -DR:].unsqueeze(1), cos, sin).expand(b, H, s, DR)
    q = torch.cat([q[..., :DN], O.apply_rotary_pos_emb(q[..., DN:], cos, sin)], -1)
    k = torch.cat([kvb[..., :DN], k_pe], -1)
    sc = (q @ k.transpose(-1, -2)) * (DN + DR) ** -0.5
    o = torch.softmax(sc.masked_fill(~torch.ones(s, s, dtype=torch.bool).tril(), float("-inf")), -1) @ kvb[..., DN:]
    return O.linear(o.transpose(1, 2).reshape(b, s, H * DV), p[pre + "out_proj.weight"])


def ref_moe_sigmoid(h, p, idx, pre="mlp."):
    sel = torch.sigmoid(O.linear(h, p[pre + "router.weight"])).gather(1, idx)
    gate = sel / sel.sum(1, keepdim=True)
    out = torch.zeros_like(h)
    for e in range(MOE["num_experts"]):
        ep = f"{pre}experts.{e}."
        for j in range(idx.shape[1]):
            tok = (idx[:, j] == e).nonzero().flatten()
            if tok.numel():
                y = O.mlp(h[tok], p[ep + "gate_proj.weight"], p[ep + "up_proj.weight"], p[ep + "down_proj.weight"])
                out = out.index_add(0, tok, gate[tok, j, None] * y)
    return out


def ref_llama(ids, params, layers, cos, sin):
    x = F.embedding(ids, params["embedding.weight"])
    for i, layer in enumerate(layers):
        pre = f"decoder_layers.{i}."
        p = {k[len(pre):]: v for k, v in params.items() if k.startswith(pre)}
        x = x + ref_mla(NORM(x, p["input_layernorm.weight"], EPS), p, cos, sin, "attention.")
        h = NORM(x, p["post_attention_layernorm.weight"], EPS)
        if layer.mlp.stages is not None:
            x = x + ref_moe_sigmoid(h.reshape(-1, h.shape[-1]), p, layer.mlp.stages["idx"].cpu().long()).view_as(x)
        else:
            x = x + O.mlp(h, p["mlp.gate_proj.weight"], p["mlp.up_proj.weight"], p["mlp.down_proj.weight"])
    return O.linear(NORM(x, params["final_norm.weight"], EPS), params["final_proj.weight"])


@pytest.mark.parametrize("q_lora_rank", [None, 96])
def test_mla_attention_module(q_lora_rank):
    from picotron_amd.model import MLAttention, get_cos_sin
    with torch.device("cuda"):
        att = MLAttention(types.SimpleNamespace(**dict(CFG, q_lora_rank=q_lora_rank)), 0)
    att.to(BF)
    randomise_norms(att)
    cos, sin = get_cos_sin(S, DR, base=10000.0)
    x, dy = torch.randn(B, S, 256).to(BF), torch.randn(B, S, 256).to(BF)
    xg = x.cuda().requires_grad_(True)
    y = att(xg, cos, sin)
    y.backward(dy.cuda())
    p = params_f32(att)
    xr = x.float().requires_grad_(True)
    yr = ref_mla(xr, p, *tables())
    yr.backward(dy.float())
    errs = {"y": rel(y, yr), "dx": rel(xg.grad, xr.grad), **{n: rel(t.grad, p[n].grad) for n, t in att.named_parameters()}}
    print(f"mla attention q_lora_rank={q_lora_rank}: {errs}")
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("moe", [False, True], ids=["dense", "moe"])
@pytest.mark.parametrize("q_lora_rank", [None, 96])
def test_mla_llama_two_layers(q_lora_rank, moe):
    from picotron_amd import functional as FN
    from picotron_amd.model import Llama
    c = dict(CFG, q_lora_rank=q_lora_rank, **(MOE if moe else {}))
    with torch.device("cuda"):
        model = Llama(types.SimpleNamespace(**c))
    model.to(BF)
    randomise_norms(model)
    for layer in model.decoder_layers:
        layer.mlp.stages = {} if moe else None
    V = c["vocab_size"]
    ids = torch.randint(0, V, (B, S + 1), generator=torch.Generator().manual_seed(1))
    inp, tgt = ids[:, :-1], ids[:, 1:]
    logits = model(inp.cuda())
    loss = FN.cross_entropy(logits.view(-1, V), tgt.reshape(-1).cuda())
    loss.backward()
    p = params_f32(model)
    lr = ref_llama(inp, p, model.decoder_layers, *tables())
    loss_r = F.cross_entropy(lr.reshape(-1, V), tgt.reshape(-1))
    loss_r.backward()
    assert abs(loss.float().item() - loss_r.item()) < TOL * abs(loss_r.item())
    errs = {"logits": rel(logits, lr), **{n: rel(q.grad, p[n].grad) for n, q in model.named_parameters()}}
    print(f"mla llama q_lora_rank={q_lora_rank} moe={moe}: worst {max(errs.values()):.3e} ({max(errs, key=errs.get)})")
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("over,grid", [
    (dict(), dict(tp=2)), (dict(), dict(cp=2)), (dict(), dict(pp=2)), (dict(qk_norm=True), {}),
    (dict(sliding_window=64), {}), (dict(qk_nope_head_dim=64), {}), (dict(v_head_dim=64), {}), (dict(qk_rope_head_dim=32), {}),
    ("document_ids", {}), ("graphed", {})])
def test_refused_layouts_raise(monkeypatch, over, grid):
    from picotron_amd import model as M
    from picotron_amd import process_group_manager as pgm
    from picotron_amd import train
    if grid:
        m = {**dict(tp=1, cp=1, pp=1), **grid}
        monkeypatch.setattr(pgm, "process_group_manager", types.SimpleNamespace(
            tp_world_size=m["tp"], cp_world_size=m["cp"], pp_world_size=m["pp"], dp_world_size=1))
    with pytest.raises(NotImplementedError):
        with torch.device("cuda"):
            layer = M.DecoderLayer(types.SimpleNamespace(**dict(CFG, **(over if isinstance(over, dict) else {}))), 0)
        if over == "document_ids":
            layer.to(BF)(torch.zeros(1, 128, 256, dtype=BF, device="cuda"), document_ids=torch.zeros(1, 128, dtype=torch.long))
        elif over == "graphed":
            train.GraphedTrainStep(layer, None, "cuda")
