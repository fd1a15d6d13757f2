"""The auxiliary z-loss at the model level: functional.cross_entropy(z_loss=, return_z_loss=) on a tiny Llama's
logits on every path it has (the lm_head statistics, the streaming kernels, a vocabulary off the 8-column grid,
[B, V, S], reductions, ignored rows), train_step and GraphedTrainStep with z_loss, the vocab-parallel path at
tp = 2 and the pipeline's last stage at pp = 2.

The torch side is fp32 on the same bf16 logits:  F.cross_entropy + z * logsumexp^2  over the valid rows, with z
the f32 value the kernels receive.  Metric and tolerance are those of tests/test_model_gpu.py: norm-relative
2e-2.  Every gradient check is paired with one that the z term arrived: the gradient differs from the z_loss = 0
gradient by more than ten times the tolerance."""
import math
import os
import types

import pytest
import torch
import torch.nn.functional as F

from tests import _ce_z_ref as Z
from tests import _dist
from tests import _row_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TOL = 2e-2
S = 256
ZL = 0.25
IGN = -100


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def cfg_tiny(layers=1, H=256, I=512, nh=4, nkv=2, V=512, S=S):
    return types.SimpleNamespace(hidden_size=H, intermediate_size=I, num_attention_heads=nh, num_key_value_heads=nkv,
                                 vocab_size=V, rms_norm_eps=1e-5, rope_theta=10000.0, num_hidden_layers=layers,
                                 max_position_embeddings=S)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("DEVICE", "cuda")
    monkeypatch.setenv("LOCAL_RANK", "0")
    monkeypatch.setenv("CONTEXT_PARALLEL", "0")
    monkeypatch.setenv("FLASH_ATTEN", "1")
    from picotron_amd import process_group_manager as pgm
    pgm.setup_process_group_manager(1, 1, 1, 1)
    torch.manual_seed(0)


def tiny_model(V=512, layers=1):
    from picotron_amd.model import Llama
    cfg = cfg_tiny(layers=layers, V=V)
    with torch.device("cuda"):
        model = Llama(cfg)
    return model.to(BF), cfg


def tokens(V, seed=1):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (2, S + 1), generator=g)
    inp, tgt = ids[:, :-1], ids[:, 1:].clone()
    tgt[0, 5:40] = IGN          # ignored rows, among them a run that spans a 32-row block of the statistics kernel
    tgt[1, -1] = IGN
    return inp, tgt


def torch_side(logits, tgt, reduction, z, gout=None):
    """(loss, z_part, dlogits) in fp32 on the bf16 logits [T, V]: F.cross_entropy + z lse^2 over the valid rows."""
    lr = logits.detach().float().cpu().requires_grad_(True)
    t = tgt.reshape(-1)
    valid = t != IGN
    zrow = Z.z32(z) * torch.logsumexp(lr, 1) ** 2 * valid
    ce = F.cross_entropy(lr, t, reduction=reduction, ignore_index=IGN)
    zp = zrow if reduction == "none" else zrow.sum() / valid.sum() if reduction == "mean" else zrow.sum()
    loss = ce + zp
    loss.backward(gout.reshape(-1) if reduction == "none" else None)
    return loss.detach(), zp.detach(), lr.grad


def run_ours(model, cfg, inp, tgt, reduction, form, z, gout=None):
    """One forward / backward of the model with functional.cross_entropy: (loss, z_part, lm_head weight gradient,
    bf16 logits [T, V], lm_head input [T, H])."""
    from picotron_amd import functional as FN
    V = cfg.vocab_size
    model.zero_grad(set_to_none=True)
    seen = {}
    h = model.final_norm.register_forward_hook(
        lambda mod, a, out: seen.update(h=FN._plain(out[0] if isinstance(out, tuple) else out).detach()))
    try:
        logits = model(inp.cuda())
    finally:
        h.remove()
    t = tgt.cuda()
    if form == "bvs":
        out = FN.cross_entropy(logits.transpose(1, 2), t, reduction=reduction, ignore_index=IGN, z_loss=z,
                               return_z_loss=True)
    else:
        out = FN.cross_entropy(logits.view(-1, V), t.reshape(-1), reduction=reduction, ignore_index=IGN, z_loss=z,
                               return_z_loss=True)
    loss, zp = out
    assert zp.dtype == torch.float32 and zp.is_cuda and not zp.requires_grad and zp.grad_fn is None
    assert loss.dtype == logits.dtype
    if reduction == "none":
        assert loss.shape == zp.shape == (t.shape if form == "bvs" else (t.numel(),))
        loss.backward(gout.cuda().to(loss.dtype).reshape(loss.shape))
    else:
        assert loss.dim() == 0 and zp.dim() == 0
        loss.backward()
    return (loss.detach(), zp, model.final_proj.weight.grad.detach().clone(), FN._plain(logits).detach().reshape(-1, V),
            seen["h"].reshape(-1, cfg.hidden_size))


@pytest.mark.parametrize("reduction,form,V", [("mean", "rows", 512), ("sum", "rows", 512), ("none", "rows", 512),
                                              ("mean", "bvs", 512), ("none", "bvs", 512), ("mean", "rows", 1001)])
def test_cross_entropy_z_against_torch(reduction, form, V):
    model, cfg = tiny_model(V)
    inp, tgt = tokens(V)
    # 'none': per-row weights of one sign, as a weighted loss has.  (With zero-mean weights the softmax term, the only
    # one z scales, averages out over the rows of a random model while the one-hot term does not: the z term is then a
    # small share of the weight gradient -- 0.17 of it here -- and the "z arrived" check below says little.)
    gout = (0.5 + torch.rand(tgt.shape, generator=torch.Generator().manual_seed(3))).to(BF) if reduction == "none" else None
    loss, zp, wgrad, logits, hid = run_ours(model, cfg, inp, tgt, reduction, form, ZL, gout)
    loss_r, zp_r, dl_r = torch_side(logits, tgt, reduction, ZL, None if gout is None else gout.float())
    wgrad_r = dl_r.t() @ hid.float().cpu()
    print(f"z-loss model {reduction} {form} V={V}: loss {rel(loss.reshape(-1), loss_r.reshape(-1)):.2e} "
          f"z {rel(zp.reshape(-1), zp_r.reshape(-1)):.2e} wgrad {rel(wgrad, wgrad_r):.2e}")
    assert rel(loss.reshape(-1), loss_r.reshape(-1)) < TOL
    assert rel(zp.reshape(-1), zp_r.reshape(-1)) < TOL
    assert rel(wgrad, wgrad_r) < TOL
    if reduction == "none":
        ign = (tgt == IGN).reshape(-1)
        assert not bool(loss.reshape(-1).cpu()[ign].any()) and not bool(zp.reshape(-1).cpu()[ign].any())
    # the z term arrived in the gradient, and the loss is not the plain one
    _, zp0, wgrad0, _, _ = run_ours(model, cfg, inp, tgt, reduction, form, 0.0, gout)
    assert not bool(zp0.any()) and zp0.shape == zp.shape
    assert rel(wgrad, wgrad0) > 10 * TOL
    assert float(zp_r.float().abs().sum()) > 10 * TOL * float(loss_r.float().abs().sum())


def test_return_convention_and_plain_call():
    """Without return_z_loss the loss alone comes back, with the term; z_loss = 0 is the call of before."""
    from picotron_amd import functional as FN
    model, cfg = tiny_model()
    inp, tgt = tokens(cfg.vocab_size)
    with torch.no_grad():
        logits = model(inp.cuda()).view(-1, cfg.vocab_size)
        t = tgt.reshape(-1).cuda()
        both = FN.cross_entropy(logits, t, z_loss=ZL, return_z_loss=True)
        alone = FN.cross_entropy(logits, t, z_loss=ZL)
        plain = FN.cross_entropy(logits, t)
        plain0 = FN.cross_entropy(logits, t, z_loss=0.0)
    assert isinstance(alone, torch.Tensor) and torch.equal(alone, both[0]) and torch.equal(plain, plain0)
    assert abs(float(both[0]) - float(plain) - float(both[1])) < TOL * float(both[0])
    # torch's own entry point on the tagged logits has no such keyword and is unchanged
    assert torch.equal(F.cross_entropy(logits, t), plain)


def test_fused_wrapper_with_z_loss():
    """kernels.cross_entropy_fwd_bwd(z_loss=): the one-read form's loss, z part and dlogits against the torch side."""
    from picotron_amd import kernels as K
    model, cfg = tiny_model()
    inp, tgt = tokens(cfg.vocab_size)
    with torch.no_grad():
        logits = FN_plain(model(inp.cuda())).reshape(-1, cfg.vocab_size).contiguous()
    t = tgt.reshape(-1).cuda()
    loss, dl, inv, zp = K.cross_entropy_fwd_bwd(logits, t, scale=0.5, ignore_index=IGN, inplace=False, z_loss=ZL)
    loss_r, zp_r, dl_r = torch_side(logits, tgt, "mean", ZL)
    assert rel(loss, loss_r) < TOL and rel(zp, zp_r) < TOL and rel(dl, 0.5 * dl_r) < TOL
    assert abs(inv.item() * int((tgt != IGN).sum()) - 1) < 1e-6
    loss0, dl0, _ = K.cross_entropy_fwd_bwd(logits, t, scale=0.5, ignore_index=IGN, inplace=False)
    assert abs(loss.item() - loss0.item() - zp.item()) < TOL * loss.item()
    # the z term arrived: off the target columns (the one-hot's -1 carries most of a logit gradient's norm and z does
    # not touch it) the gradient is the plain one times 1 + 2 z lse
    off = torch.ones_like(dl, dtype=torch.bool)
    off[torch.arange(t.numel(), device=t.device), t.clamp_min(0)] = False
    assert rel(dl * off, dl0 * off) > 10 * TOL


def FN_plain(t):
    from picotron_amd import functional as FN
    return FN._plain(t)


def test_statistics_and_streaming_paths_agree():
    """The forward fed by the lm_head GEMM's statistics and the streaming forward (switch ce_stats off), per row
    (reduction 'none'): both z parts and both losses within the per-element bounds of tests/_ce_z_ref.py of the
    float64 reference on the stored bf16 logits, and the same gradient.  The statistics' tile sums are row sums of
    at most V terms, so ref_ce_fwd's LSE bound (the larger of its two styles) covers them; merge_stats' bound covers
    their merge."""
    from picotron_amd import kernels as K
    from picotron_amd import switches
    model, cfg = tiny_model()
    V = cfg.vocab_size
    inp, tgt = tokens(V)
    gout = torch.randn(tgt.shape, generator=torch.Generator().manual_seed(3)).to(BF)
    assert K.ce_stats_fusable(tgt.numel(), V)
    runs = {}
    for name, over in (("stats", {}), ("stream", dict(ce_stats=0))):
        with switches.override(**over):
            runs[name] = run_ours(model, cfg, inp, tgt, "none", "rows", ZL, gout)
    x = runs["stats"][3].cpu()
    assert torch.equal(x, runs["stream"][3].cpu())
    t = tgt.reshape(-1)
    f = {s: R.ref_ce_fwd(x, t, style=s, steps=1) for s in ("sub", "fma")}
    e_l = torch.maximum(f["sub"]["lse_bound"], f["fma"]["lse_bound"])
    nblk = V // K.ce_stats_block(t.numel(), V)
    xv = x.double().reshape(-1, nblk, V // nblk)
    m = xv.amax(2)
    _, e_merge = R.merge_stats(m, torch.exp(xv - m[..., None]).sum(2))
    for name, e in (("stream", e_l), ("stats", e_l + e_merge)):
        fr = f["fma"]
        lb = torch.where(fr["valid"], e + R.E * fr["loss"].abs(), torch.zeros_like(e))
        zf = Z.ref_z_fwd(ZL, fr["lse"], e, fr["valid"], fr["loss"], lb)
        loss, zp = runs[name][0], runs[name][1]
        R.check("row_z", zp, zf["row_z"], zf["row_z_bound"], f"model {name}")
        R.check("loss", loss.float(), zf["loss"], R.b16(zf["loss"], zf["loss_bound"]), f"model {name}")
    assert rel(runs["stats"][2], runs["stream"][2]) < TOL


def _hand_loop(model, loader, ga, V, z):
    from picotron_amd import functional as FN
    model.zero_grad(set_to_none=True)
    tot = torch.zeros((), dtype=torch.float32, device="cuda")
    zacc = torch.zeros((), dtype=torch.float32, device="cuda")
    for i in range(ga):
        logits = model(input_ids=loader._inputs[i])
        loss, zp = FN.cross_entropy(logits.view(-1, V), loader._targets[i].reshape(-1), z_loss=z, return_z_loss=True)
        loss = loss / ga
        loss.backward()
        tot += loss.detach().float()
        zacc += zp / ga
    return tot.item(), zacc, {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def test_train_step_with_z_loss():
    from picotron_amd import switches
    from picotron_amd.train import SyntheticMicroBatchDataLoader, train_step
    model, cfg = tiny_model(layers=2)
    dev = torch.device("cuda")
    ga = 3
    loader = SyntheticMicroBatchDataLoader(2, S, ga, cfg.vocab_size, dev, seed=1234)
    with switches.override(wgrad_pair=0):       # one weight-gradient launch per micro-batch, as the loop's
        want, zwant, gwant = _hand_loop(model, loader, ga, cfg.vocab_size, ZL)
        model.zero_grad(set_to_none=True)
        got = train_step(model, loader, dev, z_loss=ZL)
        zgot = model.z_loss_part
        assert isinstance(got, float) and got == want
        assert zgot.dtype == torch.float32 and zgot.is_cuda and zgot.dim() == 0 and torch.equal(zgot, zwant)
        for n, p in model.named_parameters():
            assert rel(p.grad, gwant[n]) < TOL, n
        # read_loss=False: device scalars, the z part among them
        model.zero_grad(set_to_none=True)
        dl = train_step(model, loader, dev, read_loss=False, z_loss=ZL)
        assert isinstance(dl, torch.Tensor) and dl.is_cuda and dl.item() == want and torch.equal(model.z_loss_part, zwant)
        # z_loss = 0: the step of before, and no z part
        model.zero_grad(set_to_none=True)
        plain = train_step(model, loader, dev)
        assert model.z_loss_part is None and abs(plain + float(zwant) - want) < TOL * want
        assert float(zwant) > 10 * TOL * want


def _graph_vs_eager(rank, world):
    os.environ["FLASH_ATTEN"] = "1"
    from picotron_amd import process_group_manager as pgm
    from picotron_amd import switches
    from picotron_amd.model import Llama
    from picotron_amd.train import GraphedTrainStep, SyntheticMicroBatchDataLoader, train_step
    pgm.setup_process_group_manager(1, 1, 1, 1)
    cfg = cfg_tiny(layers=2)
    dev = torch.device("cuda", 0)
    runs = {}
    for mode in ("eager", "graph"):
        torch.manual_seed(0)
        with torch.device(dev):
            model = Llama(cfg)
        model.to(BF)
        loader = SyntheticMicroBatchDataLoader(2, S, 4, cfg.vocab_size, dev, seed=7, fresh=True)
        step = GraphedTrainStep(model, loader, dev, z_loss=ZL) if mode == "graph" else None
        out = []
        with switches.override(wgrad_pair=0):
            for _ in range(2):
                if step is None:
                    model.zero_grad(set_to_none=True)
                loss = step() if step is not None else train_step(model, loader, dev, z_loss=ZL)
                out.append((loss, model.z_loss_part.item(), [p.grad.detach().clone() for p in model.parameters()]))
        torch.cuda.synchronize()
        runs[mode] = out
        if step is not None:
            assert step.graph is not None and model.z_loss_part is step.z_acc
    for (le, ze, ge), (lg, zg, gg) in zip(runs["eager"], runs["graph"]):
        assert le == lg and ze == zg and ze > 0, (le, lg, ze, zg)
        for a, b in zip(ge, gg):
            assert torch.equal(a, b)


def test_graphed_train_step_with_z_loss():
    _dist.run(_graph_vs_eager, 1, device="cuda", backend="nccl")


PCFG = dict(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_key_value_heads=2, vocab_size=512,
            rms_norm_eps=1e-5, rope_theta=10000.0, num_hidden_layers=2, max_position_embeddings=256)


def _full_model(layers):
    """The one-process HIP Llama on the weights tests/test_parallel_gpu.py shards (oracle init, seed 7)."""
    from oracle import picotron_oracle as O
    from picotron_amd.model import Llama
    c = dict(PCFG, num_hidden_layers=layers)
    full = {k: v.to(BF) for k, v in O.init_params(dict(c), seed=7).items()}
    with torch.device("cuda"):
        model = Llama(types.SimpleNamespace(**c))
    model.to(BF)
    names = dict(model.named_parameters())
    assert sorted(names) == sorted(full)
    with torch.no_grad():
        for n, p in names.items():
            p.copy_(full[n])
    return model


def _tp2(rank, world, want_loss, want_z, want_grads):
    from picotron_amd import functional as FN
    from tests import test_parallel_gpu as TP
    m, model, names, pf, ids, lo, loss_r = TP._setup(2, 1, 256)
    V = PCFG["vocab_size"]
    x, t = ids[:, :-1].contiguous(), ids[:, 1:].contiguous()
    gathers = []
    orig_ag = FN.TPContext.all_gather_rows_into

    def counted_ag(self, out, tt, async_op=False):
        gathers.append(tuple(tt.shape))
        return orig_ag(self, out, tt, async_op)
    FN.TPContext.all_gather_rows_into = counted_ag
    try:
        logits = model(x.cuda())
        loss, zp = FN.cross_entropy(logits.view(-1, V), t.reshape(-1).cuda(), z_loss=ZL, return_z_loss=True)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        FN.TPContext.all_gather_rows_into = orig_ag
    T = t.numel()
    assert FN.vp_ce_shape_ok(T, V // 2, PCFG["hidden_size"])
    assert len([g for g in gathers if g == (T, 4)]) == 1, gathers     # the vocab-parallel path: 16 B per row, once
    assert abs(loss.item() - want_loss) < TOL * abs(want_loss) and abs(zp.item() - want_z) < TOL * abs(want_z)
    assert zp.dtype == torch.float32 and not zp.requires_grad
    for n, p in names.items():
        assert TP._rel(p.grad, TP._shard(want_grads[n], p, m.tp_rank)) < TOL, n


def test_tensor_parallel_tp2_vocab_parallel_z_loss():
    """tp = 2 takes VocabParallelCEFunction (one (T, 4) gather); loss, z part and every gradient against the
    one-rank run of the same weights and tokens."""
    from picotron_amd import functional as FN
    model = _full_model(2)
    ids = torch.randint(0, PCFG["vocab_size"], (2, 257), generator=torch.Generator().manual_seed(11))   # _setup's
    x, t = ids[:, :-1].contiguous(), ids[:, 1:].contiguous()
    grads = {}
    for z in (ZL, 0.0):
        model.zero_grad(set_to_none=True)
        logits = model(x.cuda())
        loss, zp = FN.cross_entropy(logits.view(-1, PCFG["vocab_size"]), t.reshape(-1).cuda(), z_loss=z, return_z_loss=True)
        loss.backward()
        grads[z] = {n: p.grad.detach().float().cpu() for n, p in model.named_parameters()}
        if z:
            want = (loss.item(), zp.item())
    assert rel(grads[ZL]["final_proj.weight"], grads[0.0]["final_proj.weight"]) > 10 * TOL
    torch.cuda.synchronize()
    _dist.run(_tp2, 2, want[0], want[1], grads[ZL], device="cuda")


def _pp2(rank, world, want_loss, want_z):
    os.environ["FLASH_ATTEN"] = "1"
    torch.cuda.set_device(0)
    from oracle import picotron_oracle as O
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.model import Llama
    from picotron_amd.pipeline_parallel.pipeline_parallel import PipelineParallel, train_step_pipeline_1f1b
    from picotron_amd.train import SyntheticMicroBatchDataLoader
    m = pgm.setup_process_group_manager(tp_size=1, cp_size=1, pp_size=world, dp_size=1)
    c = dict(PCFG, num_hidden_layers=3)
    cfg = types.SimpleNamespace(**c)
    full = {k: v.to(BF) for k, v in O.init_params(dict(c), seed=7).items()}
    with torch.device("cuda"):
        model = PipelineParallel(Llama(cfg), cfg)
    model.to(BF)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(full[n])
    loader = SyntheticMicroBatchDataLoader(2, 256, 3, c["vocab_size"], torch.device("cuda"), seed=1234)
    loss = train_step_pipeline_1f1b(model, loader, (2, 256, c["hidden_size"]), torch.device("cuda"), BF, z_loss=ZL)
    torch.cuda.synchronize()
    zp = model.z_loss_part
    if m.pp_is_last_stage:
        assert abs(loss - want_loss) < TOL * abs(want_loss), (loss, want_loss)
        assert zp.dtype == torch.float32 and zp.is_cuda and zp.dim() == 0 and not zp.requires_grad
        assert abs(zp.item() - want_z) < TOL * abs(want_z), (zp.item(), want_z)
    else:
        assert loss == 0.0 and zp is None
    # z_loss = 0: the step of before, no z part left over from the step above; a bad value fails on every stage
    model.zero_grad(set_to_none=True)
    plain = train_step_pipeline_1f1b(model, loader, (2, 256, c["hidden_size"]), torch.device("cuda"), BF)
    assert model.z_loss_part is None
    if m.pp_is_last_stage:
        assert abs(plain + want_z - want_loss) < TOL * abs(want_loss)
    with pytest.raises(ValueError):
        train_step_pipeline_1f1b(model, loader, (2, 256, c["hidden_size"]), torch.device("cuda"), BF, z_loss=-1.0)
    assert all(p.grad is not None for p in model.parameters())


def test_pipeline_parallel_pp2_z_loss():
    """One 1F1B step with z_loss: the last stage's logging loss and `model.z_loss_part` (the means of the micro-batch
    losses and z parts) are the one-process train_step's loss and z part (their sum over grad_acc, each divided by it) on the same weights and batches,
    and is not the plain loss."""
    from picotron_amd.train import SyntheticMicroBatchDataLoader, train_step
    model = _full_model(3)
    dev = torch.device("cuda")
    loader = SyntheticMicroBatchDataLoader(2, 256, 3, PCFG["vocab_size"], dev, seed=1234)
    want = train_step(model, loader, dev, z_loss=ZL)
    zpart = model.z_loss_part.item()
    assert zpart > 10 * TOL * want and math.isfinite(want)
    torch.cuda.synchronize()
    _dist.run(_pp2, 2, want, zpart, device="cuda")
