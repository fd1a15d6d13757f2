"""Document-masked and sliding-window attention at the model level: DecoderLayer (both FLASH_ATTEN
flavours) and a 2-layer Llama with cross-entropy run with `document_ids`, against the unchanged
oracle run document by document -- O.decoder_layer / O.llama_forward on x[b:b+1, s:e] with
cos[s:e], sin[s:e] (positions continue across documents, as in the model), the outputs concatenated
and one backward through the whole; Attention with sliding_window against a reference assembled
here from O.linear, O.apply_rotary_pos_emb and a masked fp32 SDPA.  Metric and tolerance are those
of tests/test_model_gpu.py: norm-relative 2e-2 on outputs, the loss, the input gradient and every
parameter gradient.  The layouts a band does not cover raise NotImplementedError."""
import math
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import picotron_oracle as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TOL = 2e-2
S = 256
DOCS = [[(0, 100), (100, 256)], [(0, 256)]]     # (start, end) of each document, per batch row


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def cfg_tiny(layers=2, H=256, I=512, nh=4, nkv=2, V=512, S=S, **kw):
    return types.SimpleNamespace(hidden_size=H, intermediate_size=I, num_attention_heads=nh, num_key_value_heads=nkv,
                                 vocab_size=V, rms_norm_eps=1e-5, rope_theta=10000.0, num_hidden_layers=layers,
                                 max_position_embeddings=S, **kw)


def document_ids():
    ids = torch.zeros(len(DOCS), S, dtype=torch.long)
    for b, docs in enumerate(DOCS):
        for d, (s, e) in enumerate(docs):
            ids[b, s:e] = d
    return ids


def per_document(fn, x):
    """fn(x[b:b+1, s:e], s, e) over every document, concatenated back to x's [B, S, ...] layout."""
    return torch.cat([torch.cat([fn(x[b:b + 1, s:e], s, e) for s, e in docs], 1) for b, docs in enumerate(DOCS)], 0)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("DEVICE", "cuda")
    monkeypatch.setenv("LOCAL_RANK", "0")
    monkeypatch.setenv("CONTEXT_PARALLEL", "0")
    from picotron_amd import process_group_manager as pgm
    pgm.setup_process_group_manager(1, 1, 1, 1)
    torch.manual_seed(0)


def _params_f32(module):
    return {k: v.detach().float().cpu().requires_grad_(True) for k, v in module.named_parameters()}


@pytest.mark.parametrize("flash,nkv,d", [("1", 2, 64), ("0", 4, 64), ("1", 2, 128)])
def test_decoder_layer_with_document_ids(monkeypatch, flash, nkv, d):
    monkeypatch.setenv("FLASH_ATTEN", flash)
    from picotron_amd.model import DecoderLayer
    nh = 4
    cfg = cfg_tiny(H=nh * d, I=512, nh=nh, nkv=nkv)
    with torch.device("cuda"):
        layer = DecoderLayer(cfg, 0)
    layer.to(BF)
    for n in (layer.input_layernorm, layer.post_attention_layernorm):
        with torch.no_grad():
            n.weight.copy_(1 + 0.1 * torch.randn_like(n.weight))
    x = torch.randn(2, S, nh * d).to(BF)
    dy = torch.randn(2, S, nh * d).to(BF)
    xg = x.cuda().requires_grad_(True)
    y = layer(xg, document_ids=document_ids().cuda())
    y.backward(dy.cuda())
    p = _params_f32(layer)
    xr = x.float().requires_grad_(True)
    cos, sin = (t.float() for t in O.get_cos_sin(S, d, base=10000.0))
    norm = O.rmsnorm_flash_semantics if flash == "1" else O.rmsnorm_llama
    yr = per_document(lambda t, s, e: O.decoder_layer(t, p, cos[s:e], sin[s:e], nh, nkv, 1e-5, norm=norm), xr)
    yr.backward(dy.float())
    assert rel(y, yr) < TOL
    assert rel(xg.grad, xr.grad) < TOL
    for n, q in layer.named_parameters():
        assert rel(q.grad, p[n].grad) < TOL, n


def test_llama_loss_and_grads_with_document_ids(monkeypatch):
    monkeypatch.setenv("FLASH_ATTEN", "1")
    from picotron_amd import functional as FN
    from picotron_amd.model import Llama
    cfg = cfg_tiny(layers=2)
    with torch.device("cuda"):
        model = Llama(cfg)
    model.to(BF)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, cfg.vocab_size, (2, S + 1), generator=g)
    inp, tgt = ids[:, :-1], ids[:, 1:]
    logits = model(inp.cuda(), document_ids=document_ids().cuda())
    loss = FN.cross_entropy(logits.view(-1, cfg.vocab_size), tgt.reshape(-1).cuda())
    loss.backward()
    p = _params_f32(model)
    cos, sin = (t.float() for t in O.get_cos_sin(S, 64, base=10000.0))
    c = dict(vars(cfg))
    lr = per_document(lambda t, s, e: O.llama_forward(t, p, c, cos[s:e], sin[s:e], norm=O.rmsnorm_flash_semantics), inp)
    loss_r = F.cross_entropy(lr.reshape(-1, cfg.vocab_size), tgt.reshape(-1))
    loss_r.backward()
    assert abs(loss.float().item() - loss_r.item()) < TOL * abs(loss_r.item())
    assert rel(logits, lr) < TOL
    for n, q in model.named_parameters():
        assert rel(q.grad, p[n].grad) < TOL, n
    # an AttnBand built by the caller is taken as it is
    from picotron_amd import kernels as K
    band = K.attn_band(2, S, "cuda", document_ids=document_ids())
    assert torch.equal(model(inp.cuda(), document_ids=band), logits)


def test_attention_with_sliding_window(monkeypatch):
    monkeypatch.setenv("FLASH_ATTEN", "1")
    from picotron_amd.model import Attention, get_cos_sin
    W, nh, nkv, d = 100, 4, 2, 64
    cfg = cfg_tiny(H=nh * d, nh=nh, nkv=nkv, sliding_window=W)
    with torch.device("cuda"):
        att = Attention(cfg, 0)
    att.to(BF)
    assert att.sliding_window == W
    cos, sin = get_cos_sin(S, d, base=10000.0)
    x = torch.randn(2, S, nh * d).to(BF)
    dy = torch.randn(2, S, nh * d).to(BF)
    i = torch.arange(S)
    win = (i[None, :] <= i[:, None]) & (i[:, None] - i[None, :] < W)
    for ids in (None, document_ids()):
        att.zero_grad()
        xg = x.cuda().requires_grad_(True)
        y = att(xg, cos, sin) if ids is None else att(xg, cos, sin, document_ids=ids.cuda())
        y.backward(dy.cuda())
        p = _params_f32(att)
        xr = x.float().requires_grad_(True)
        cr, sr = cos.float().cpu(), sin.float().cpu()
        q = O.apply_rotary_pos_emb(O.linear(xr, p["q_proj.weight"]).view(2, S, nh, d).transpose(1, 2), cr, sr)
        k = O.apply_rotary_pos_emb(O.linear(xr, p["k_proj.weight"]).view(2, S, nkv, d).transpose(1, 2), cr, sr)
        v = O.linear(xr, p["v_proj.weight"]).view(2, S, nkv, d).transpose(1, 2)
        k, v = k.repeat_interleave(nh // nkv, dim=1), v.repeat_interleave(nh // nkv, dim=1)
        mask = win[None, None].expand(2, 1, S, S)
        if ids is not None:
            mask = mask & (ids[:, :, None] == ids[:, None, :])[:, None]
        s = (q @ k.transpose(-1, -2)) / math.sqrt(d)
        o = torch.softmax(s.masked_fill(~mask, float("-inf")), -1) @ v
        yr = O.linear(o.transpose(1, 2).reshape(2, S, nh * d), p["out_proj.weight"])
        yr.backward(dy.float())
        assert rel(y, yr) < TOL
        assert rel(xg.grad, xr.grad) < TOL
        for n, t in att.named_parameters():
            assert rel(t.grad, p[n].grad) < TOL, n


class _Loader:
    """One micro-batch, again and again."""

    def __init__(self, batch, grad_acc_steps=1):
        self.batch, self.grad_acc_steps = batch, grad_acc_steps

    def __next__(self):
        return self.batch


def test_train_step_passes_document_ids_through(monkeypatch):
    monkeypatch.setenv("FLASH_ATTEN", "1")
    from picotron_amd import functional as FN
    from picotron_amd import train
    from picotron_amd.model import Llama
    cfg = cfg_tiny(layers=1)
    with torch.device("cuda"):
        model = Llama(cfg)
    model.to(BF)
    ids = torch.randint(0, cfg.vocab_size, (2, S + 1), generator=torch.Generator().manual_seed(3))
    batch = {"input_ids": ids[:, :-1], "target_ids": ids[:, 1:]}
    docs = document_ids()
    wq = model.decoder_layers[0].attention.q_proj.weight
    logits = model(ids[:, :-1].cuda(), document_ids=docs.cuda())
    FN.cross_entropy(logits.view(-1, cfg.vocab_size), ids[:, 1:].reshape(-1).cuda()).backward()
    want = wq.grad.clone()
    # (the loss of a freshly initialised model barely moves with the mask: the gradient of the
    # attention's query projection tells the two apart)
    model.zero_grad(set_to_none=True)
    train.train_step(model, _Loader(dict(batch, document_ids=docs)), "cuda")
    masked = wq.grad.clone()
    model.zero_grad(set_to_none=True)
    train.train_step(model, _Loader(batch), "cuda")
    plain = wq.grad.clone()
    assert rel(masked, want) < 1e-3        # the same kernels on the same inputs
    assert rel(plain, want) > 1e-2         # without the ids every token sees the whole row


def test_unsupported_layouts_raise(monkeypatch):
    monkeypatch.setenv("FLASH_ATTEN", "1")
    from picotron_amd import functional as FN
    from picotron_amd import kernels as K
    from picotron_amd import train
    from picotron_amd.model import Llama
    from picotron_amd.pipeline_parallel.pipeline_parallel import PipelineParallel
    cfg = cfg_tiny(layers=1)
    with torch.device("cuda"):
        model = Llama(cfg)
    model.to(BF)
    ids = torch.randint(0, cfg.vocab_size, (2, S), generator=torch.Generator().manual_seed(4)).cuda()
    docs = document_ids().cuda()
    band = K.attn_band(2, S, "cuda", document_ids=docs)
    # the sequence-parallel TP layout (sp = its chunk count)
    x = torch.zeros(2, S, cfg.hidden_size, dtype=BF, device="cuda")
    with pytest.raises(NotImplementedError, match="sequence-parallel"):
        FN.DecoderLayerFunction.apply(x, *([None] * 11), 1e-5, 0, 4, 2, 64, False, 2, band)
    # GraphedTrainStep
    step = train.GraphedTrainStep(model, _Loader({"input_ids": ids, "target_ids": ids, "document_ids": docs}), "cuda")
    with pytest.raises(NotImplementedError, match="GraphedTrainStep"):
        step()
    # the pipeline engine
    pp = PipelineParallel(model, cfg)
    with pytest.raises(NotImplementedError, match="pipeline"):
        pp(ids, None, None, document_ids=docs)
    # context parallelism (the ring)
    monkeypatch.setenv("CONTEXT_PARALLEL", "1")
    with pytest.raises(NotImplementedError, match="context parallelism"):
        model(ids, document_ids=docs)
    with pytest.raises(NotImplementedError, match="context parallelism"):
        FN.AttnShape(2, S, 4, 2, 64, band=band)
    with pytest.raises(NotImplementedError, match="context parallelism"):
        model.decoder_layers[0].attention(x, None, None, document_ids=band)
