"""QK-norm at the model level: config.qk_norm through Attention (AttentionFunction), DecoderLayer
(DecoderLayerFunction) and Llama, with bands, train_step / GraphedTrainStep, DataParallelBucket, the
pipeline, optim.AdamW, and the layouts it refuses.

The reference is an fp32 CPU autograd decoder / Llama with a per-head RMSNorm of q and of k between the
projection and RoPE, assembled here from the pieces oracle.picotron_oracle exports (linear, the two
RMSNorm flavours, apply_rotary_pos_emb, sdpa_causal, mlp, get_cos_sin, init_params).  Metric and
tolerance are the suite's own (tests/test_model_gpu.py): norm-relative 2e-2.  The q_norm / k_norm weights
are set to 1 + 0.25 randn so that they are not the identity."""
import math
import os
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import picotron_oracle as O
from tests import _dist

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TOL = 2e-2
S = 256
EPS = 1e-5
PCFG = dict(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_key_value_heads=2, vocab_size=512,
            rms_norm_eps=EPS, rope_theta=10000.0, num_hidden_layers=2, max_position_embeddings=S, qk_norm=True)
SHAPES = [("1", 4, 2, 64), ("0", 4, 2, 64), ("1", 2, 1, 128)]   # (FLASH_ATTEN, heads, kv heads, head_dim)


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def cfg_of(**over):
    return types.SimpleNamespace(**dict(PCFG, **over))


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("DEVICE", "cuda")
    monkeypatch.setenv("LOCAL_RANK", "0")
    monkeypatch.setenv("CONTEXT_PARALLEL", "0")
    monkeypatch.setenv("FLASH_ATTEN", "1")
    from picotron_amd import process_group_manager as pgm
    pgm.setup_process_group_manager(1, 1, 1, 1)
    torch.manual_seed(0)


# ------------------------------------------------------------------------------ the reference
def ref_norm(flash):
    return O.rmsnorm_flash_semantics if flash == "1" else O.rmsnorm_llama


def ref_attention(x, p, cos, sin, nh, nkv, eps, norm, mask=None, pre=""):
    """oracle.attention with the per-head norms (when p has them) and an optional [B, 1, S, S] visibility mask."""
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


def ref_decoder_layer(x, p, cos, sin, nh, nkv, eps, norm, mask=None):
    h = norm(x, p["input_layernorm.weight"], eps)
    x = x + ref_attention(h, p, cos, sin, nh, nkv, eps, norm, mask, pre="attention.")
    h = norm(x, p["post_attention_layernorm.weight"], eps)
    return x + O.mlp(h, p["mlp.gate_proj.weight"], p["mlp.up_proj.weight"], p["mlp.down_proj.weight"])


def ref_llama(ids, params, cfg, cos, sin, norm, mask=None):
    x = F.embedding(ids, params["embedding.weight"])
    for i in range(cfg["num_hidden_layers"]):
        pre = f"decoder_layers.{i}."
        lp = {k[len(pre):]: v for k, v in params.items() if k.startswith(pre)}
        x = ref_decoder_layer(x, lp, cos, sin, cfg["num_attention_heads"], cfg["num_key_value_heads"],
                              cfg["rms_norm_eps"], norm, mask)
    return O.linear(norm(x, params["final_norm.weight"], cfg["rms_norm_eps"]), params["final_proj.weight"])


def params_f32(module):
    return {k: v.detach().float().cpu().requires_grad_(True) for k, v in module.named_parameters()}


def tables(d):
    return tuple(t.float() for t in O.get_cos_sin(S, d, base=10000.0))


def randomise_norms(module, seed=5):
    """Every q_norm / k_norm (and layer norm) weight to 1 + 0.25 randn: not the identity."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in module.named_parameters():
            if p.dim() == 1:
                p.copy_((1 + 0.25 * torch.randn(p.shape, generator=g)).to(p.dtype))


def full_weights(c, seed=7):
    """The oracle's init (seed) as bf16, plus the q_norm / k_norm weights of a qk_norm config."""
    full = {k: v.to(BF) for k, v in O.init_params({k: v for k, v in c.items() if k != "qk_norm"}, seed=seed).items()}
    if c.get("qk_norm"):
        g = torch.Generator().manual_seed(seed + 1)
        d = c["hidden_size"] // c["num_attention_heads"]
        for l in range(c["num_hidden_layers"]):
            for n in ("q_norm", "k_norm"):
                full[f"decoder_layers.{l}.attention.{n}.weight"] = (1 + 0.25 * torch.randn(d, generator=g)).to(BF)
    return full


def full_model(c, seed=7):
    """The one-process HIP Llama of config dict c on full_weights(c)."""
    from picotron_amd.model import Llama
    full = full_weights(c, seed)
    with torch.device("cuda"):
        model = Llama(types.SimpleNamespace(**c))
    model.to(BF)
    names = dict(model.named_parameters())
    assert sorted(names) == sorted(full)
    with torch.no_grad():
        for n, p in names.items():
            p.copy_(full[n])
    return model


# ------------------------------------------------------------------------------ modules against the reference
@pytest.mark.parametrize("flash,nh,nkv,d", SHAPES)
def test_attention_module(monkeypatch, flash, nh, nkv, d):
    monkeypatch.setenv("FLASH_ATTEN", flash)
    from picotron_amd.model import Attention, LlamaRMSNorm, TritonRMSNorm, get_cos_sin
    cfg = cfg_of(hidden_size=nh * d, num_attention_heads=nh, num_key_value_heads=nkv)
    with torch.device("cuda"):
        att = Attention(cfg, 0)
    att.to(BF)
    assert type(att.q_norm) is type(att.k_norm) is (TritonRMSNorm if flash == "1" else LlamaRMSNorm)
    assert tuple(att.q_norm.weight.shape) == tuple(att.k_norm.weight.shape) == (d,)
    assert bool((att.q_norm.weight == 1).all()) and bool((att.k_norm.weight == 1).all())
    assert [n for n, _ in att.named_parameters()][-2:] == ["q_norm.weight", "k_norm.weight"]
    randomise_norms(att)
    att.reset_parameters()
    assert bool((att.q_norm.weight == 1).all()) and bool((att.k_norm.weight == 1).all())   # reset with the rest
    randomise_norms(att)
    cos, sin = get_cos_sin(S, d, base=10000.0)
    x, dy = torch.randn(2, S, nh * d).to(BF), torch.randn(2, S, nh * d).to(BF)
    xg = x.cuda().requires_grad_(True)
    y = att(xg, cos, sin)
    y.backward(dy.cuda())
    p = params_f32(att)
    xr = x.float().requires_grad_(True)
    yr = ref_attention(xr, p, *tables(d), nh, nkv, EPS, ref_norm(flash))
    yr.backward(dy.float())
    errs = {"y": rel(y, yr), "dx": rel(xg.grad, xr.grad), **{n: rel(t.grad, p[n].grad) for n, t in att.named_parameters()}}
    print(f"qk-norm attention flash={flash} d={d}: {errs}")
    assert max(errs.values()) < TOL, errs
    assert {"q_norm.weight", "k_norm.weight"} <= set(errs)
    # it arrived: the same weights without the norms give another output and another q_proj gradient
    with torch.device("cuda"):
        plain = Attention(cfg_of(hidden_size=nh * d, num_attention_heads=nh, num_key_value_heads=nkv, qk_norm=False), 0)
    plain.to(BF)
    assert not hasattr(plain, "q_norm")
    with torch.no_grad():
        for n, t in plain.named_parameters():
            t.copy_(dict(att.named_parameters())[n])
    xp = x.cuda().requires_grad_(True)
    yp = plain(xp, cos, sin)
    yp.backward(dy.cuda())
    assert rel(y, yp) > 10 * TOL and rel(att.q_proj.weight.grad, plain.q_proj.weight.grad) > 10 * TOL


@pytest.mark.parametrize("flash,nh,nkv,d", SHAPES)
def test_decoder_layer(monkeypatch, flash, nh, nkv, d):
    monkeypatch.setenv("FLASH_ATTEN", flash)
    from picotron_amd.model import DecoderLayer
    cfg = cfg_of(hidden_size=nh * d, num_attention_heads=nh, num_key_value_heads=nkv)
    with torch.device("cuda"):
        layer = DecoderLayer(cfg, 0)
    layer.to(BF)
    randomise_norms(layer)
    x, dy = torch.randn(2, S, nh * d).to(BF), torch.randn(2, S, nh * d).to(BF)
    xg = x.cuda().requires_grad_(True)
    y = layer(xg)
    y.backward(dy.cuda())
    p = params_f32(layer)
    xr = x.float().requires_grad_(True)
    yr = ref_decoder_layer(xr, p, *tables(d), nh, nkv, EPS, ref_norm(flash))
    yr.backward(dy.float())
    errs = {"y": rel(y, yr), "dx": rel(xg.grad, xr.grad), **{n: rel(t.grad, p[n].grad) for n, t in layer.named_parameters()}}
    print(f"qk-norm decoder layer flash={flash} d={d}: {errs}")
    assert max(errs.values()) < TOL, errs
    assert {"attention.q_norm.weight", "attention.k_norm.weight"} <= set(errs)
    # frozen norm weights get no gradient, the rest is unchanged
    layer.zero_grad(set_to_none=True)
    layer.attention.q_norm.weight.requires_grad_(False)
    x2 = x.cuda().requires_grad_(True)
    layer(x2).backward(dy.cuda())
    assert layer.attention.q_norm.weight.grad is None and rel(layer.attention.k_norm.weight.grad, p["attention.k_norm.weight"].grad) < TOL
    assert rel(x2.grad, xg.grad) < 1e-3        # the same kernels on the same inputs


def _loss_and_grads(model, inp, tgt, V, **kw):
    from picotron_amd import functional as FN
    model.zero_grad(set_to_none=True)
    logits = model(inp.cuda(), **kw)
    loss = FN.cross_entropy(logits.view(-1, V), tgt.reshape(-1).cuda())
    loss.backward()
    return loss, logits


def test_llama_two_layers():
    model = full_model(PCFG)
    V = PCFG["vocab_size"]
    assert {"decoder_layers.0.attention.q_norm.weight", "decoder_layers.1.attention.k_norm.weight"} <= set(model.state_dict())
    ids = torch.randint(0, V, (2, S + 1), generator=torch.Generator().manual_seed(1))
    inp, tgt = ids[:, :-1], ids[:, 1:]
    loss, logits = _loss_and_grads(model, inp, tgt, V)
    p = params_f32(model)
    lr = ref_llama(inp, p, PCFG, *tables(64), O.rmsnorm_flash_semantics)
    loss_r = F.cross_entropy(lr.reshape(-1, V), tgt.reshape(-1))
    loss_r.backward()
    assert abs(loss.float().item() - loss_r.item()) < TOL * abs(loss_r.item())
    assert rel(logits, lr) < TOL
    errs = {n: rel(q.grad, p[n].grad) for n, q in model.named_parameters()}
    print(f"qk-norm llama: worst {max(errs.values()):.3e} ({max(errs, key=errs.get)})")
    assert max(errs.values()) < TOL, errs
    # it arrived: the same weights without the norms
    plain = full_model(dict(PCFG, qk_norm=False))
    with torch.no_grad():
        for n, t in plain.named_parameters():
            t.copy_(dict(model.named_parameters())[n])
    _loss_and_grads(plain, inp, tgt, V)
    name = "decoder_layers.0.attention.q_proj.weight"
    assert rel(dict(model.named_parameters())[name].grad, dict(plain.named_parameters())[name].grad) > 10 * TOL


def _document_ids():
    ids = torch.zeros(2, S, dtype=torch.long)
    ids[0, 100:] = 1
    return ids


def test_bands_document_ids_and_sliding_window():
    """The band's mask on the normed q, k: document ids alone (a decoder layer), and a sliding window with and
    without them (the attention module)."""
    from picotron_amd.model import Attention, DecoderLayer, get_cos_sin
    nh, nkv, d, W = 4, 2, 64, 100
    i = torch.arange(S)
    causal = (i[None, :] <= i[:, None])[None, None]
    docs = _document_ids()
    same = (docs[:, :, None] == docs[:, None, :])[:, None]
    x, dy = torch.randn(2, S, nh * d).to(BF), torch.randn(2, S, nh * d).to(BF)
    with torch.device("cuda"):
        layer = DecoderLayer(cfg_of(), 0)
    layer.to(BF)
    randomise_norms(layer)
    xg = x.cuda().requires_grad_(True)
    y = layer(xg, document_ids=docs.cuda())
    y.backward(dy.cuda())
    p = params_f32(layer)
    xr = x.float().requires_grad_(True)
    yr = ref_decoder_layer(xr, p, *tables(d), nh, nkv, EPS, O.rmsnorm_flash_semantics, mask=causal & same)
    yr.backward(dy.float())
    errs = {"y": rel(y, yr), "dx": rel(xg.grad, xr.grad), **{n: rel(t.grad, p[n].grad) for n, t in layer.named_parameters()}}
    assert max(errs.values()) < TOL, errs
    with torch.device("cuda"):
        att = Attention(cfg_of(sliding_window=W), 0)
    att.to(BF)
    randomise_norms(att)
    cos, sin = get_cos_sin(S, d, base=10000.0)
    win = causal & ((i[:, None] - i[None, :]) < W)[None, None]
    for ids, mask in ((None, win), (docs, win & same)):
        att.zero_grad(set_to_none=True)
        xg = x.cuda().requires_grad_(True)
        y = att(xg, cos, sin) if ids is None else att(xg, cos, sin, document_ids=ids.cuda())
        y.backward(dy.cuda())
        p = params_f32(att)
        xr = x.float().requires_grad_(True)
        yr = ref_attention(xr, p, *tables(d), nh, nkv, EPS, O.rmsnorm_flash_semantics, mask=mask.expand(2, 1, S, S))
        yr.backward(dy.float())
        errs = {"y": rel(y, yr), "dx": rel(xg.grad, xr.grad), **{n: rel(t.grad, p[n].grad) for n, t in att.named_parameters()}}
        assert max(errs.values()) < TOL, errs


def test_without_qk_norm_nothing_changes():
    """qk_norm absent: today's parameter names, and the forward still takes the RoPE-epilogue GEMM (one call per
    layer); with it, the plain GEMM and the fused norm + RoPE kernel instead."""
    from picotron_amd import kernels as K
    from picotron_amd.model import Llama
    c = {k: v for k, v in PCFG.items() if k != "qk_norm"}
    ids = torch.randint(0, c["vocab_size"], (2, S), generator=torch.Generator().manual_seed(2)).cuda()
    counts = {}

    def counted(name):
        orig = getattr(K, name)

        def f(*a, **kw):
            counts[name] = counts.get(name, 0) + 1
            return orig(*a, **kw)
        return orig, f
    saved = {}
    try:
        for name in ("linear_fwd_rope", "qk_norm_rope_fwd", "qk_norm_bwd"):
            saved[name], wrapped = counted(name)
            setattr(K, name, wrapped)
        with torch.device("cuda"):
            model = Llama(types.SimpleNamespace(**c))
        model.to(BF)
        assert sorted(n for n, _ in model.named_parameters()) == sorted(O.init_params(dict(c), seed=7))
        assert not any("q_norm" in n or "k_norm" in n for n in model.state_dict())
        _loss_and_grads(model, ids, ids, c["vocab_size"])
        assert counts == {"linear_fwd_rope": c["num_hidden_layers"]}, counts
        counts.clear()
        qk = full_model(PCFG)
        _loss_and_grads(qk, ids, ids, c["vocab_size"])
        assert counts == {"qk_norm_rope_fwd": PCFG["num_hidden_layers"], "qk_norm_bwd": PCFG["num_hidden_layers"]}, counts
    finally:
        for name, orig in saved.items():
            setattr(K, name, orig)


# ------------------------------------------------------------------------------ training steps
def _hand_loop(model, loader, ga, V):
    from picotron_amd import functional as FN
    tot = torch.zeros((), dtype=torch.float32, device="cuda")
    for i in range(ga):
        logits = model(input_ids=loader._inputs[i])
        loss = FN.cross_entropy(logits.view(-1, V), loader._targets[i].reshape(-1)) / ga
        loss.backward()
        tot += loss.detach().float()
    return tot.item()


@pytest.mark.parametrize("main_grad", [False, True])
def test_train_step_accumulates_the_norm_gradients(main_grad):
    """train_step with grad_acc 3 equals the hand loop: the norm weights' gradients accumulate over the
    micro-batches into a bf16 .grad, or into an f32 main_grad attribute on every parameter."""
    from picotron_amd import switches
    from picotron_amd.train import SyntheticMicroBatchDataLoader, train_step
    model = full_model(PCFG)
    dev = torch.device("cuda")
    ga, V = 3, PCFG["vocab_size"]
    loader = SyntheticMicroBatchDataLoader(2, S, ga, V, dev, seed=1234)

    def arm():
        model.zero_grad(set_to_none=True)
        if main_grad:
            for p in model.parameters():
                p.main_grad = torch.zeros(p.shape, dtype=torch.float32, device=dev)

    def grads():
        return {n: (p.main_grad if main_grad else p.grad).detach().clone() for n, p in model.named_parameters()}
    with switches.override(wgrad_pair=0):       # one weight-gradient launch per micro-batch, as the loop's
        arm()
        want = _hand_loop(model, loader, ga, V)
        gwant = grads()
        arm()
        got = train_step(model, loader, dev)
        ggot = grads()
    assert got == want
    for n in gwant:
        assert ggot[n].dtype == (torch.float32 if main_grad else BF)
        assert rel(ggot[n], gwant[n]) < TOL, n
    # the accumulated norm gradients are those of the three micro-batches together (one batch's is not)
    model.zero_grad(set_to_none=True)
    for p in model.parameters():
        if main_grad:
            del p.main_grad
    name = "decoder_layers.0.attention.q_norm.weight"
    one = _loss_and_grads(model, loader._inputs[0].cpu(), loader._targets[0].cpu(), V)
    single = dict(model.named_parameters())[name].grad.float() / ga
    assert rel(ggot[name], single) > 10 * TOL
    if main_grad:   # the reference: fp32 autograd over the three micro-batches
        p = params_f32(model)
        for i in range(ga):
            lr = ref_llama(loader._inputs[i].cpu(), p, PCFG, *tables(64), O.rmsnorm_flash_semantics)
            (F.cross_entropy(lr.reshape(-1, V), loader._targets[i].cpu().reshape(-1)) / ga).backward()
        for n in ("decoder_layers.0.attention.q_norm.weight", "decoder_layers.1.attention.k_norm.weight"):
            assert rel(ggot[n], p[n].grad) < TOL, n


def _graph_vs_eager(rank, world):
    os.environ["FLASH_ATTEN"] = "1"
    from picotron_amd import process_group_manager as pgm
    from picotron_amd import switches
    from picotron_amd.train import GraphedTrainStep, SyntheticMicroBatchDataLoader, train_step
    pgm.setup_process_group_manager(1, 1, 1, 1)
    dev = torch.device("cuda", 0)
    runs = {}
    for mode in ("eager", "graph"):
        model = full_model(PCFG)
        loader = SyntheticMicroBatchDataLoader(2, S, 4, PCFG["vocab_size"], dev, seed=7, fresh=True)
        step = GraphedTrainStep(model, loader, dev) if mode == "graph" else None
        out = []
        with switches.override(wgrad_pair=0):
            for _ in range(2):
                if step is None:
                    model.zero_grad(set_to_none=True)
                loss = step() if step is not None else train_step(model, loader, dev)
                out.append((loss, {n: p.grad.detach().clone() for n, p in model.named_parameters()}))
        torch.cuda.synchronize()
        runs[mode] = out
        if step is not None:
            assert step.graph is not None
    for (le, ge), (lg, gg) in zip(runs["eager"], runs["graph"]):
        assert le == lg, (le, lg)
        assert "decoder_layers.0.attention.q_norm.weight" in ge
        for n in ge:
            assert torch.equal(ge[n], gg[n]), n


def test_graphed_train_step_equals_eager():
    _dist.run(_graph_vs_eager, 1, device="cuda", backend="nccl")


DP_GA = 2


def _dp_ids(dp):
    return torch.randint(0, PCFG["vocab_size"], (dp, DP_GA, 2, S + 1), generator=torch.Generator().manual_seed(21))


def _dp2(rank, world, want):
    """DataParallelBucket (f32 main_grad, the bucket all-reduce on the last micro-batch), each rank its own tokens."""
    os.environ["FLASH_ATTEN"] = "1"
    torch.cuda.set_device(0)
    from picotron_amd import functional as FN
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.data_parallel.data_parallel import DataParallelBucket
    m = pgm.setup_process_group_manager(tp_size=1, cp_size=1, pp_size=1, dp_size=world)
    model = full_model(PCFG, seed=9)
    ddp = DataParallelBucket(model)
    V = PCFG["vocab_size"]
    ids = _dp_ids(world)
    for i in range(DP_GA):
        ddp.require_backward_grad_sync = (i == DP_GA - 1)
        t = ids[m.dp_rank, i]
        lo = ddp(t[:, :-1].cuda())
        (FN.cross_entropy(lo.view(-1, V), t[:, 1:].reshape(-1).cuda()) / DP_GA).backward()
    torch.cuda.synchronize()   # the step completed: the bucket was told about every gradient, the two new ones too
    for n, p in model.named_parameters():
        assert p.grad is not None and p.grad.dtype == BF, n
        assert rel(p.grad, want[n]) < TOL, n


def test_data_parallel_bucket_dp2():
    """dp = 2: every gradient is the one-process run's over both ranks' micro-batches (their mean)."""
    from picotron_amd import functional as FN
    model = full_model(PCFG, seed=9)
    V, dp = PCFG["vocab_size"], 2
    ids = _dp_ids(dp)
    for p in model.parameters():
        p.main_grad = torch.zeros(p.shape, dtype=torch.float32, device="cuda")
    for r in range(dp):
        for i in range(DP_GA):
            t = ids[r, i]
            lo = model(t[:, :-1].cuda())
            (FN.cross_entropy(lo.view(-1, V), t[:, 1:].reshape(-1).cuda()) / (DP_GA * dp)).backward()
    want = {n: p.main_grad.detach().cpu() for n, p in model.named_parameters()}
    torch.cuda.synchronize()
    _dist.run(_dp2, dp, want, device="cuda")


def _pp2(rank, world, want_loss):
    os.environ["FLASH_ATTEN"] = "1"
    torch.cuda.set_device(0)
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.model import Llama
    from picotron_amd.pipeline_parallel.pipeline_parallel import PipelineParallel, train_step_pipeline_1f1b
    from picotron_amd.train import SyntheticMicroBatchDataLoader
    m = pgm.setup_process_group_manager(tp_size=1, cp_size=1, pp_size=world, dp_size=1)
    c = dict(PCFG, num_hidden_layers=3)
    cfg = types.SimpleNamespace(**c)
    full = full_weights(c)
    with torch.device("cuda"):
        model = PipelineParallel(Llama(cfg), cfg)
    model.to(BF)
    names = dict(model.named_parameters())
    assert any("q_norm" in n for n in names) and set(names) <= set(full)
    with torch.no_grad():
        for n, p in names.items():
            p.copy_(full[n])
    loader = SyntheticMicroBatchDataLoader(2, S, 3, c["vocab_size"], torch.device("cuda"), seed=1234)
    loss = train_step_pipeline_1f1b(model, loader, (2, S, c["hidden_size"]), torch.device("cuda"), BF)
    torch.cuda.synchronize()
    if m.pp_is_last_stage:
        assert abs(loss - want_loss) < TOL * abs(want_loss), (loss, want_loss)
    assert all(p.grad is not None for p in model.parameters())


def test_pipeline_parallel_pp2():
    """One 1F1B step at pp = 2: the last stage's loss is the one-process train_step's on the same weights and batches."""
    from picotron_amd.train import SyntheticMicroBatchDataLoader, train_step
    c = dict(PCFG, num_hidden_layers=3)
    model = full_model(c)
    dev = torch.device("cuda")
    loader = SyntheticMicroBatchDataLoader(2, S, 3, c["vocab_size"], dev, seed=1234)
    want = train_step(model, loader, dev)
    assert math.isfinite(want)
    torch.cuda.synchronize()
    _dist.run(_pp2, 2, want, device="cuda")


# ------------------------------------------------------------------------------ refused layouts
def test_refused_layouts_raise_before_any_launch(monkeypatch):
    from picotron_amd import _C
    from picotron_amd import functional as FN
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.model import Attention, DecoderLayer, get_cos_sin
    with torch.device("cuda"):
        layer = DecoderLayer(cfg_of(), 0)
    layer.to(BF)
    cos, sin = get_cos_sin(S, 64, base=10000.0)
    x = torch.zeros(2, S, 256, dtype=BF, device="cuda")
    launches = []
    real_lib = _C.lib

    def no_launch():
        launches.append(1)
        return real_lib()
    monkeypatch.setattr(_C, "lib", no_launch)
    # tp = 2 (the replicated stream and the sequence-parallel layout)
    current = FN.TPContext.__dict__["current"]
    monkeypatch.setattr(FN.TPContext, "current", staticmethod(lambda: FN.TPContext(None, 2, 0)))
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        layer(x)
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        layer.attention(x, cos, sin)
    monkeypatch.setattr(FN.TPContext, "current", current)
    at = layer.attention
    w = (layer.input_layernorm.weight, layer.post_attention_layernorm.weight, *at.weights(), layer.mlp.gate_proj.weight,
         layer.mlp.up_proj.weight, layer.mlp.down_proj.weight)
    with pytest.raises(NotImplementedError, match="sequence-parallel"):
        FN.DecoderLayerFunction.apply(x, *w, cos, sin, EPS, 0, 4, 2, 64, False, 2, None, at.q_norm.weight, at.k_norm.weight)
    m = pgm.current()
    monkeypatch.setattr(m, "tp_world_size", 2)
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        Attention(cfg_of(), 0)
    monkeypatch.setattr(m, "tp_world_size", 1)
    # context parallelism
    monkeypatch.setenv("CONTEXT_PARALLEL", "1")
    with pytest.raises(NotImplementedError, match="context parallelism"):
        layer(x)
    with pytest.raises(NotImplementedError, match="context parallelism"):
        layer.attention(x, cos, sin)
    monkeypatch.setenv("CONTEXT_PARALLEL", "0")
    # head_dim 60: the module, and the Functions themselves
    with pytest.raises(NotImplementedError, match="head_dim 60"):
        Attention(cfg_of(hidden_size=240), 0)
    w60 = torch.ones(60, dtype=BF, device="cuda")
    x60 = torch.zeros(2, S, 240, dtype=BF, device="cuda")
    with pytest.raises(NotImplementedError, match="head_dim 60"):
        FN.AttentionFunction.apply(x60, None, None, None, None, cos, sin, 4, 2, 60, None, w60, w60, EPS, 0)
    with pytest.raises(NotImplementedError, match="head_dim 60"):
        FN.DecoderLayerFunction.apply(x60, *([None] * 9), cos, sin, EPS, 0, 4, 2, 60, False, 0, None, w60, w60)
    assert not launches
    # the same head_dim without qk_norm still runs (zero-padded heads), as before
    with torch.device("cuda"):
        Attention(cfg_of(hidden_size=240, qk_norm=False), 0)


# ------------------------------------------------------------------------------ the optimizer
@pytest.mark.parametrize("master", [False, True])
def test_adamw_steps_the_norm_weights(master):
    """optim.AdamW (plain, and master_weights=True) over a qk_norm attention module: after two steps the two
    [64] weights equal torch.optim.AdamW's on the same gradients (bf16 state; f32 masters and moments)."""
    from picotron_amd import optim
    from picotron_amd.model import Attention, get_cos_sin
    with torch.device("cuda"):
        att = Attention(cfg_of(), 0)
    att.to(BF)
    randomise_norms(att)
    hp = dict(lr=5e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
    ours = optim.AdamW(att.parameters(), master_weights=master, **hp)
    twins = {n: torch.nn.Parameter(p.detach().clone().to(torch.float32 if master else BF)) for n, p in att.named_parameters()}
    ref = torch.optim.AdamW(list(twins.values()), **hp)
    cos, sin = get_cos_sin(S, 64, base=10000.0)
    start = {n: p.detach().clone() for n, p in att.named_parameters()}
    for step in range(2):
        x = torch.randn(2, S, 256, generator=torch.Generator().manual_seed(step)).to(BF).cuda()
        att.zero_grad(set_to_none=True)
        att(x, cos, sin).float().pow(2).mean().backward()
        for n, p in att.named_parameters():
            twins[n].grad = p.grad.detach().clone().to(twins[n].dtype)
        ours.step()
        ref.step()
    for n in ("q_norm.weight", "k_norm.weight"):
        p = dict(att.named_parameters())[n]
        assert p.shape == (64,) and rel(p, twins[n]) < TOL, n
        assert rel(p, start[n]) > 3 * TOL, n      # and they moved: two steps of lr 0.05 on weights near 1
