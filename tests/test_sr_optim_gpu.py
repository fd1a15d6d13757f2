"""optim.AdamW(stochastic_rounding=True) on the GPU: a mixed parameter set against tests/_sr_ref.py step by step
(aligned bf16 through the list launch, a misaligned view and a non-contiguous parameter through the
single-tensor entry, an f32 parameter on the ordinary path; clipped or not; p.grad or f32 main_grads), a resumed
run against an unbroken one, and a tiny Llama trained twice with one seed and once with another."""
import copy
import types

import pytest
import torch

from tests import _optim_ref as O
from tests import _sr_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
LR, WD, BETAS, EPS = 3e-4, 0.01, (0.9, 0.999), 1e-8
SEED = 0xFEDCBA9876543210


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("DEVICE", "cuda")
    monkeypatch.setenv("LOCAL_RANK", "0")
    monkeypatch.setenv("CONTEXT_PARALLEL", "0")
    monkeypatch.setenv("FLASH_ATTEN", "1")
    from picotron_amd import process_group_manager as pgm
    pgm.setup_process_group_manager(1, 1, 1, 1)


def _scalars(t):
    """the seven scalars as AdamW._batches computes them"""
    beta1, beta2 = BETAS
    return O.S(decay=1 - LR * WD, w1=1 - beta1, beta2=beta2, c2=1 - beta2, bc2_sqrt=(1 - beta2 ** float(t)) ** 0.5, eps=EPS,
               step_size=(LR / (1 - beta1 ** float(t))) * -1)


def _mixed(seed=0):
    """[(name, parameter)]: two aligned bf16 tensors (one launch), a view 2 bytes off a 16-byte boundary, a transposed
    (non-contiguous) parameter, an f32 parameter."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    base = rn(1 + 515).to(BF).to(DEV)
    ps = [("aligned", rn(64, 33).to(BF).to(DEV)), ("ragged", rn(1001).to(BF).to(DEV)), ("off2", base[1:]),
          ("transposed", rn(24, 40).to(BF).to(DEV).t()), ("f32", rn(100).to(DEV))]
    assert ps[2][1].data_ptr() % 16 == 2 and not ps[3][1].is_contiguous()
    return [(n, torch.nn.Parameter(t)) for n, t in ps]


def _grads(params, t, main):
    """new gradients for step t: p.grad in the parameter's dtype, or f32 main_grads (bf16 parameters) with no p.grad"""
    g = torch.Generator().manual_seed(1000 + t)
    for _, p in params:
        x = (torch.randn(p.shape, generator=g) * 0.1).to(DEV)
        if main and p.dtype == BF:
            p.main_grad, p.grad = x, None
        else:
            p.grad = x.to(p.dtype)


def _flat(t):
    return t.detach().cpu().reshape(-1)   # the logical, row-major order


@pytest.mark.parametrize("main", [False, True], ids=["grad", "main_grad"])
@pytest.mark.parametrize("max_norm", [None, 0.5], ids=["plain", "clip"])
def test_mixed_set_equals_the_reference(max_norm, main, monkeypatch):
    from picotron_amd import kernels as K
    from picotron_amd import optim
    seen = []
    orig = optim._global_sq

    def spy(batches):
        seen.append(orig(batches))
        return seen[-1]
    monkeypatch.setattr(optim, "_global_sq", spy)
    params = _mixed()
    opt = optim.AdamW([p for _, p in params], lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, max_grad_norm=max_norm,
                      stochastic_rounding=True, sr_seed=SEED, use_main_grad=main)
    state = {n: (_flat(p), torch.zeros(p.numel(), dtype=p.dtype), torch.zeros(p.numel(), dtype=p.dtype)) for n, p in params}
    for t in (1, 2, 3):
        _grads(params, t, main)
        grads = {n: _flat(opt._grad(p)) for n, p in params}
        opt.step()
        torch.cuda.synchronize()
        coef = None
        if max_norm is not None:
            sq = seen[-1].item()
            want_sq = sum(float(g.to(F64).pow(2).sum()) for g in grads.values())
            assert abs(sq - want_sq) <= 1e-5 * want_sq, "one norm over every gradient"     # f32 sums of < 2^12 terms per thread
            assert float(opt.last_grad_norm) == pytest.approx(want_sq ** 0.5, rel=1e-5)
            coef = O.clip_coef(sq, max_norm)
            assert coef is not None and coef < 1.0
        s = _scalars(t)
        for stream, (n, p) in enumerate(params):
            st = opt.state[p]
            got = (_flat(p), _flat(st["exp_avg"]), _flat(st["exp_avg_sq"]))
            assert st["exp_avg"].dtype == st["exp_avg_sq"].dtype == p.dtype and "master_param" not in st
            assert st["step"].item() == float(t) and st["step"].device.type == "cpu"
            p0, m0, v0 = state[n]
            if p.dtype == BF:
                assert grads[n].dtype == (F32 if main else BF)
                want16, want32, r = SR.expect_step(p0, grads[n], m0, v0, s, SEED, stream, t, coef)
                SR.check_sr_step(f"{n} t{t}", got, want32, r)
                state[n] = want16 if not any(bool(SR.differs(a, b).any()) for a, b in zip(got, want16)) else got
            else:
                g = grads[n] if coef is None else O.clip_grad(grads[n], coef, False)
                O.check_f32_step(f"{n} t{t}", got, (p0, g, m0, v0), s, "sr optim")
                state[n] = got
    assert K.device_status(torch.device(DEV), reset=False) == 0


def _run(steps, params, opt, first=1):
    for t in range(first, first + steps):
        _grads(params, t, False)
        opt.step()
    torch.cuda.synchronize()


def _snapshot(params, opt):
    out = []
    for _, p in params:
        st = opt.state[p]
        out += [_flat(p), _flat(st["exp_avg"]), _flat(st["exp_avg_sq"]), st["step"].clone()]
    return out


@pytest.mark.parametrize("max_norm", [None, 0.5], ids=["plain", "clip"])
def test_resumed_run_equals_the_unbroken_one(max_norm):
    from picotron_amd import optim
    kw = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, max_grad_norm=max_norm, stochastic_rounding=True)
    a = _mixed()
    opt_a = optim.AdamW([p for _, p in a], sr_seed=SEED, **kw)
    _run(4, a, opt_a)
    b = _mixed()
    opt_b = optim.AdamW([p for _, p in b], sr_seed=SEED, **kw)
    _run(2, b, opt_b)
    checkpoint = copy.deepcopy(opt_b.state_dict())
    assert checkpoint["param_groups"][0]["sr_seed"] == SEED
    assert all(s["exp_avg"].dtype == s["exp_avg_sq"].dtype == p.dtype for s, (_, p) in zip(checkpoint["state"].values(), b))
    c = [(n, torch.nn.Parameter(p.detach().clone() if p.is_contiguous() else p.detach().t().clone().t())) for n, p in b]
    assert [p.is_contiguous() for _, p in c] == [p.is_contiguous() for _, p in b]
    opt_c = optim.AdamW([p for _, p in c], sr_seed=1, **kw)     # another seed: the checkpoint's wins
    opt_c.load_state_dict(checkpoint)
    _run(2, c, opt_c, first=3)
    for x, y in zip(_snapshot(a, opt_a), _snapshot(c, opt_c)):
        assert O.same_bits(x, y)
    # and the seed matters: the same run on another seed ends elsewhere
    d = _mixed()
    opt_d = optim.AdamW([p for _, p in d], sr_seed=SEED + 1, **kw)
    _run(4, d, opt_d)
    assert not O.same_bits(_flat(d[0][1]), _flat(a[0][1]))


def _train(seed, steps=3):
    from picotron_amd import optim
    from picotron_amd.model import Llama
    from picotron_amd.train import SyntheticMicroBatchDataLoader, train_step
    cfg = types.SimpleNamespace(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_key_value_heads=2,
                                rms_norm_eps=1e-5, max_position_embeddings=128, rope_theta=10000.0, vocab_size=256,
                                num_hidden_layers=2)
    torch.manual_seed(0)
    dev = torch.device(DEV)
    with torch.device(dev):
        model = Llama(cfg)
    model.to(BF)
    opt = optim.AdamW(model.parameters(), lr=1e-3, stochastic_rounding=True, sr_seed=seed, max_grad_norm=1.0)
    loader = SyntheticMicroBatchDataLoader(2, 128, 2, cfg.vocab_size, dev, seed=1234)
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        losses.append(train_step(model, loader, dev))
        opt.step()
    torch.cuda.synchronize()
    assert all(st["exp_avg"].dtype == BF for st in opt.state.values())
    return losses, [p.detach().cpu() for p in model.parameters()]


def test_tiny_llama_is_reproducible_per_seed():
    import math
    la, a = _train(7)
    lb, b = _train(7)
    lc, c = _train(8)
    assert all(math.isfinite(x) for x in la + lc)
    assert la == lb and all(O.same_bits(x, y) for x, y in zip(a, b))
    assert la[0] == lc[0] and not all(O.same_bits(x, y) for x, y in zip(a, c))
