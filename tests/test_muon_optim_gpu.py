"""optim.Muon and optim.MuonAdamW on the GPU: a few steps of a mixed list against the kit's per-stage
references, the state_dict round trip through torch.optim.Muon, the main_grad path, a toy Llama
trained beside the CPU oracle driven by torch's own Muon + AdamW, and the shared clipping norm."""
import math
import types

import pytest
import torch
import torch.nn.functional as F

from tests import _muon_ref as M

DEV = "cuda"
pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
SHAPES = [(64, 64), (72, 40), (24, 40), (64, 128), (64, 128), (129, 127)]


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("DEVICE", "cuda")
    monkeypatch.setenv("LOCAL_RANK", "0")
    monkeypatch.setenv("CONTEXT_PARALLEL", "0")
    from picotron_amd import process_group_manager as pgm
    pgm.setup_process_group_manager(1, 1, 1, 1)
    torch.manual_seed(0)


def _params(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(s, generator=gen) * 0.02).to(BF).to(DEV)) for s in SHAPES]


def _check_steps(opt, params, steps, gdtype, main_grad, **hyper):
    gen = torch.Generator().manual_seed(11)
    for k in range(steps):
        before = []
        for p in params:
            g = (torch.randn(p.shape, generator=gen) * 0.02).to(gdtype)
            if main_grad:
                p.main_grad = g.to(DEV)
            else:
                p.grad = g.to(DEV)
            st = opt.state.get(p, {})
            buf = st["momentum_buffer"].cpu().clone() if "momentum_buffer" in st else torch.zeros(p.shape, dtype=gdtype)
            before.append((p.detach().cpu().clone(), g, buf))
        rec = []
        opt.step(stages=rec)
        torch.cuda.synchronize()
        assert len(rec) == 1   # one param group, one gradient dtype: one list
        rec = rec[0]
        sq = rec["sq"].cpu()
        for i, p in enumerate(params):
            j = next(n for n, q in enumerate(rec["params"]) if q is p)
            c = M.Case(*before[i], **hyper)
            assert opt.state[p]["momentum_buffer"].dtype == gdtype
            out = dict(buf=opt.state[p]["momentum_buffer"], sq=float(sq[j]), X0=rec["X0"][j], p=p.detach(),
                       iters=[{n: it[n][j] for n in "ASPX"} for it in rec["iters"]])
            M.check_step(c, out, tag=f"step{k} {tuple(p.shape)} ")


def test_muon_steps_against_the_kit_and_state_dict_round_trip():
    from picotron_amd.optim import Muon
    hyper = dict(lr=0.02, weight_decay=0.1, momentum=0.95, nesterov=True, ns_steps=5)
    params = _params()
    opt = Muon(params, **hyper)
    _check_steps(opt, params, 3, BF, False, **hyper)
    # into torch.optim.Muon and back
    twins = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    topt = torch.optim.Muon(twins, **hyper)
    topt.load_state_dict(opt.state_dict())
    for p, t in zip(params, twins):
        assert torch.equal(topt.state[t]["momentum_buffer"], opt.state[p]["momentum_buffer"].cpu())
    back = Muon(params, **hyper)
    back.load_state_dict(topt.state_dict())
    for p in params:
        b = back.state[p]["momentum_buffer"]
        assert b.device.type == "cuda" and torch.equal(b, opt.state[p]["momentum_buffer"])
    # One more step of both from the same state.  The two differ by lr_adj (O_hip - O_torch) and by the
    # roundings of p.  With e = torch's own relative distance to the float64 iteration on this update and
    # ours at most 2 e (tests/test_muon_conformance_gpu.py), ||O_hip - O_torch|| <= 3 e ||O64||; p is rounded
    # to bf16 twice on either side, 2^-9 relative each in the Frobenius norm at the most.
    gen = torch.Generator().manual_seed(5)
    for p, t in zip(params, twins):
        g = (torch.randn(p.shape, generator=gen) * 0.02).to(BF)
        p.grad, t.grad = g.to(DEV), g.clone()
    back.step()
    topt.step()
    torch.cuda.synchronize()
    for p, t in zip(params, twins):
        u = t.grad.lerp(topt.state[t]["momentum_buffer"], hyper["momentum"])
        o64 = M.ns_f64(u.double())
        e = M.fro_rel(M.ns_torch_bf16(u), o64)
        pn = t.detach().double().norm()
        bound = 3 * e * hyper["lr"] * M.lr_ratio(None, p.shape) * float(o64.norm()) / float(pn) + 4 * 2.0 ** -9
        d = float((p.detach().cpu().double() - t.detach().double()).norm() / pn)
        print(f"muon-vs-torch {tuple(p.shape)}: {d:.3e} bound {bound:.3e}")
        assert d <= bound, (tuple(p.shape), d, bound)


def test_muon_main_grad_runs_with_f32_buffers():
    from picotron_amd.optim import Muon
    hyper = dict(lr=0.02, weight_decay=0.1, momentum=0.9, nesterov=True, ns_steps=3)
    params = _params(1)
    opt = Muon(params, use_main_grad=True, **hyper)
    _check_steps(opt, params, 2, F32, True, **hyper)


def _cfg_tiny(layers=2, H=256, I=512, nh=4, nkv=2, V=512, S=128):
    return types.SimpleNamespace(hidden_size=H, intermediate_size=I, num_attention_heads=nh, num_key_value_heads=nkv,
                                 vocab_size=V, rms_norm_eps=1e-5, rope_theta=10000.0, num_hidden_layers=layers,
                                 max_position_embeddings=S)


@pytest.mark.parametrize("max_grad_norm", [None, 0.05], ids=["unclipped", "clipped"])
def test_muon_adamw_on_the_toy_llama_follows_the_oracle(monkeypatch, max_grad_norm):
    """20 steps of MuonAdamW on the tests' toy Llama beside the CPU oracle model stepped by
    torch.optim.Muon + torch.optim.AdamW over the same split, on bf16 leaves (so its parameters are
    rounded to bf16 after every step, as the HIP model stores them): the loss within the project's
    1 % per step, and falling.  Clipped (max_grad_norm below the model's gradient norm, so the
    coefficient is below 1 from the first step): the oracle runs torch.nn.utils.clip_grad_norm_ over
    all of its gradients in front of the two steps; last_grad_norm is the float64 norm over every
    model.parameters() gradient of the real backward, and the status word stays 0."""
    from picotron_amd import kernels as K
    from oracle import picotron_oracle as O
    monkeypatch.setenv("FLASH_ATTEN", "1")
    from picotron_amd.model import Llama
    from picotron_amd.optim import MuonAdamW, split_muon_params
    from picotron_amd.train import SyntheticMicroBatchDataLoader, train_step
    cfg = _cfg_tiny()
    dev = torch.device("cuda")
    with torch.device(dev):
        model = Llama(cfg)
    model.to(BF)
    steps, ga = 20, 1
    mk, ak = dict(lr=0.02, weight_decay=0.1), dict(lr=3e-4)
    opt = MuonAdamW(model, muon=mk, adamw=ak, max_grad_norm=max_grad_norm)
    K.device_status(dev)   # start from a clear word
    loader = SyntheticMicroBatchDataLoader(2, 128, ga, cfg.vocab_size, dev, seed=1234)

    ref = {k: v.detach().cpu().clone() for k, v in model.named_parameters()}   # bf16 leaves
    mats = {id(p) for p in split_muon_params(model)[0]}
    names = [(k, id(v) in mats) for k, v in model.named_parameters()]
    rmuon = torch.optim.Muon([ref[k] for k, m in names if m], **mk)
    radam = torch.optim.AdamW([ref[k] for k, m in names if not m], foreach=False, **ak)
    assert len(rmuon.param_groups[0]["params"]) == 14
    cos, sin = O.get_cos_sin(128, 64, base=10000.0)
    c = dict(vars(cfg))
    inputs, targets = loader._inputs.cpu(), loader._targets.cpu()

    def ref_step():
        pf = {k: v.float().requires_grad_(True) for k, v in ref.items()}
        lo = O.llama_forward(inputs[0], pf, c, cos.float(), sin.float(), norm=O.rmsnorm_flash_semantics)
        loss = F.cross_entropy(lo.reshape(-1, cfg.vocab_size), targets[0].reshape(-1))
        loss.backward()
        for k, p in ref.items():
            p.grad = pf[k].grad.to(BF)
        if max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_(list(ref.values()), max_grad_norm, foreach=False)
        rmuon.step()
        radam.step()
        return loss.item()

    ours, theirs, norms = [], [], []
    for _ in range(steps):
        opt.zero_grad()
        ours.append(train_step(model, loader, dev))
        norm64 = math.sqrt(sum(p.grad.double().pow(2).sum().item() for p in model.parameters()))
        opt.step()
        if max_grad_norm is not None:
            got = opt.last_grad_norm.item()
            # f32 sums of non-negative terms over chains of a few hundred additions: well inside 1e-5
            assert abs(got - norm64) <= 1e-5 * norm64, (got, norm64)
            norms.append(got)
        theirs.append(ref_step())
    assert K.device_status(dev) == 0
    if max_grad_norm is not None:
        print("muon-llama grad norms", [round(x, 3) for x in norms[::4]])
        assert norms[0] > 2 * max_grad_norm   # clipping is active: the coefficient is below 1/2
    dev_rel = [abs(a - b) / abs(b) for a, b in zip(ours, theirs)]
    print("muon-llama ours", [round(x, 4) for x in ours[::4]], "oracle", [round(x, 4) for x in theirs[::4]],
          "max rel", max(dev_rel))
    assert theirs[-1] < theirs[0] - 0.5, theirs
    assert ours[-1] < ours[0] - 0.5, ours
    assert max(dev_rel) < 1e-2, (max(dev_rel), ours[::4], theirs[::4])


def _split(seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)

    def mk(shape):
        p = torch.nn.Parameter((torch.randn(shape, generator=gen) * 0.02).to(BF).to(DEV))
        p.grad = ((torch.randn(shape, generator=gen) * 0.05).to(BF) * scale).to(DEV)
        return p
    return [mk(s) for s in SHAPES], [mk(s) for s in ((512,), (96, 64), (37,))]


@pytest.mark.parametrize("clips", [False, True])
def test_clipped_norm_covers_both_parts(clips):
    """Two steps.  last_grad_norm is the norm over ALL parameters; with a max_norm below it Muon's half
    shows the coefficient in its momentum buffer, and AdamW's half has the bits of a stand-alone AdamW
    whose clipped launches are handed the same squared norm and max_norm -- and, when clipping is
    active, not the bits of an unclipped AdamW (after the second step: a first AdamW step is nearly
    scale-invariant)."""
    from picotron_amd.optim import AdamW, MuonAdamW
    matrices, rest = _split(3)
    twin = [torch.nn.Parameter(p.detach().clone()) for p in rest]
    plain = [torch.nn.Parameter(p.detach().clone()) for p in rest]
    norm64 = math.sqrt(sum(p.grad.double().pow(2).sum().item() for p in matrices + rest))
    max_norm = norm64 / 4 if clips else norm64 * 4
    opt = MuonAdamW((matrices, rest), muon=dict(lr=0.02), adamw=dict(lr=1e-3), max_grad_norm=max_norm)
    topt, popt = AdamW(twin, lr=1e-3), AdamW(plain, lr=1e-3)
    for step in range(2):
        if step:   # new gradients of the same size
            gen = torch.Generator().manual_seed(77)
            for p in matrices + rest:
                p.grad = (torch.randn(p.shape, generator=gen) * 0.05).to(BF).to(DEV)
            norm64 = math.sqrt(sum(p.grad.double().pow(2).sum().item() for p in matrices + rest))
        for a, b, c in zip(rest, twin, plain):
            b.grad, c.grad = a.grad.clone(), a.grad.clone()
        before = [(p.detach().cpu().clone(), p.grad.cpu().clone(), opt.muon.state[p]["momentum_buffer"].cpu().clone()
                   if step else torch.zeros(p.shape, dtype=BF)) for p in matrices]
        opt.step()
        work, _ = topt._clip_work()
        topt._launch_clipped(work, opt.last_grad_sq, max_norm)
        popt.step()
        torch.cuda.synchronize()
        got = opt.last_grad_norm.item()
        assert abs(got - norm64) <= 1e-5 * norm64, (got, norm64)
        coef = M.clip_coef32(float(opt.last_grad_sq.cpu()), max_norm)
        assert (coef < 1) == clips and (not clips or abs(coef - 0.25) < 1e-3)
        for p, (p0, g, b0) in zip(matrices, before):
            # buf = bf16(lerp(buf, bf16(g coef), 0.05)): the ONE coefficient reached Muon's half (two bf16
            # roundings: 2^-7 relative per element at the most, on |buf| + |g|)
            st = opt.muon.state[p]["momentum_buffer"].cpu().double()
            want = b0.double() + 0.05 * (g.double() * coef - b0.double())
            scale = b0.double().abs() + 0.05 * g.double().abs() * coef
            assert bool(((st - want).abs() <= 2.0 ** -7 * scale + 1e-30).all())
            assert not torch.equal(p.detach().cpu(), p0)
        for a, b in zip(rest, twin):
            assert torch.equal(a.detach(), b.detach())
    same_as_unclipped = all(torch.equal(a.detach(), c.detach()) for a, c in zip(rest, plain))
    assert same_as_unclipped == (not clips)


def test_half_gradients_half_max_norm_same_bits():
    """Both coefficients exactly 1: every gradient scaled by 1/2 (exact in bf16) with max_norm halved gives
    the Muon matrices the bits of the unscaled run (the step normalises the update; AdamW's eps does not
    scale, so its parameters are not compared), and the reported norm is exactly halved (every square is
    exactly a quarter and the sums run in the same order)."""
    from picotron_amd.optim import MuonAdamW
    outs = []
    for scale in (1.0, 0.5):
        matrices, rest = _split(4, scale)
        opt = MuonAdamW((matrices, rest), muon=dict(lr=0.02), adamw=dict(lr=1e-3), max_grad_norm=100.0 * scale)
        opt.step()
        torch.cuda.synchronize()
        assert M.clip_coef32(float(opt.last_grad_sq.cpu()), 100.0 * scale) == 1.0
        outs.append(([p.detach().clone() for p in matrices], opt.last_grad_norm.item()))
    assert outs[1][1] == 0.5 * outs[0][1] and outs[0][1] > 0
    for a, b in zip(outs[0][0], outs[1][0]):
        assert torch.equal(a, b)
