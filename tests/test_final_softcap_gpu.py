"""Final-logit soft-capping (config.final_logit_softcapping, t = c tanh(raw / c)) against float64: the capped lm_head
epilogue, the cross-entropy backward with the factor 1 - (t / c)^2 folded in, the row kernels, and a model.
Tolerance of a bf16 store: half a bf16 ulp of the float64 reference plus the f32 error of the formula, the latter
measured here on the CPU as twice the worst |float32 - float64| of the same formula on the test's own inputs."""
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import picotron_oracle as O
from picotron_amd import kernels as K
from tests import _attn_ref as R
from tests.test_attn_sinks_gpu import TOL

pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
CAPS = (30.0, 2.0)


def cap_fwd(x, c):   # the kernels' expression (common.h pt_softcap) in x's precision
    return (1 - 2 / (1 + torch.exp2(x * (2.8853900817779268 / c)))) * c


def cap_grad(t, c):
    return torch.where(t == float("-inf"), torch.zeros_like(t), (c - t) * (c + t) / (c * c))


def assert_bf16(got, ref64, ref32, what):
    """|got - ref64| <= half a bf16 ulp of ref64 + 2 max|ref32 - ref64| (see the module docstring)."""
    half_ulp = torch.ldexp(torch.ones_like(ref64), torch.frexp(ref64).exponent - 9) * (ref64 != 0)
    e32 = 2 * (ref32.to(F64) - ref64).abs().max().item()
    err = (got.detach().cpu().to(F64) - ref64).abs()
    print(f"{what}: worst err {err.max().item():.3e}, f32 formula term {e32:.3e}, worst excess {(err - half_ulp).max().item():.3e}")
    assert bool((err <= half_ulp + e32).all()), what


@pytest.mark.parametrize("c", CAPS)
@pytest.mark.parametrize("M,N,Kd", [(256, 512, 128), (256, 128, 64)], ids=["block256", "block128"])
def test_capped_epilogue(M, N, Kd, c):
    block = K.ce_stats_block(M, N)
    g = torch.Generator().manual_seed(N)
    x = torch.randn(M, Kd, generator=g).to(BF)
    w = (torch.randn(N, Kd, generator=g) * (2 * c / Kd ** 0.5)).to(BF)   # |acc| reaches several c
    y, stats = K.linear_ce_stats(x.cuda(), w.cuda(), softcap=c)
    assert_bf16(y, c * torch.tanh(x.to(F64) @ w.to(F64).T / c), cap_fwd(x.float() @ w.float().T, c), "capped logits")
    # the statistics of the STORED values: equal maxima; the sum within f32 summation of `block` terms, the
    # exponent's rounding (|y - m| log2(e) <= 2.9 c, 1.5 roundings) and a few ulp of v_exp and the merge
    tiles = y.cpu().to(F64).view(M, N // block, block).transpose(0, 1)
    m, st = tiles.max(-1).values, stats.cpu().to(F64)
    s = torch.exp(tiles - m[..., None]).sum(-1)
    assert torch.equal(st[..., 0], m)
    rel = ((st[..., 1] - s).abs() / s).max().item()
    print(f"stats: worst sum rel err {rel:.3e}")
    assert rel <= (block + 3 * c + 8) * 2.0 ** -24
    (y0, s0), (y1, s1) = K.linear_ce_stats(x.cuda(), w.cuda()), K.linear_ce_stats(x.cuda(), w.cuda(), softcap=None)
    assert torch.equal(y0, y1) and torch.equal(s0, s1) and not torch.equal(y0, y)


@pytest.mark.parametrize("z", (0.0, 1e-4))
@pytest.mark.parametrize("c", CAPS)
@pytest.mark.parametrize("V,pad", [(64, 0), (520, 3), (8200, 0)], ids=["v64", "v517-padded", "v8200"])
def test_folded_backward(V, pad, c, z):
    rows, scale = 8, 0.37
    g = torch.Generator().manual_seed(V)
    t = (torch.randn(rows, V, generator=g) * c / 2).clamp(-c, c)
    t[:, 1::7], t[:, 2::11] = c, -c          # the factor is exactly 0 there
    if pad:
        t[:, V - pad:] = float("-inf")       # CrossEntropyFunction's padding of a vocabulary off the 8-column grid
    t = t.to(BF)
    tg = torch.randint(0, V - pad, (rows,), generator=g)
    tg[3] = -100
    valid = (tg != -100)
    onehot = F.one_hot(tg.clamp_min(0), V) * valid[:, None]

    def ref(dt, lse, gscale):
        x, lse = t.to(dt), lse.to(dt)[:, None]
        return (torch.exp(x - lse) * (1 + 2 * z * lse) - onehot.to(dt)) * gscale * cap_grad(x, c) * valid[:, None]

    lse64 = torch.logsumexp(t.to(F64), -1)
    lse = lse64.float()                      # the saved f32 LSE is an input of the streaming form
    dl = K.cross_entropy_grad_lse(t.cuda(), tg.cuda(), lse.cuda(), torch.tensor([scale]).cuda(), softcap=c, z_loss=z)
    assert_bf16(dl, ref(F64, lse, scale), ref(F32, lse, scale), "bwd_lse_cap")
    gs = scale / valid.sum().item()
    out = K.cross_entropy_fwd_bwd(t.cuda(), tg.cuda(), scale=scale, inplace=False, softcap=c, z_loss=z)
    assert_bf16(out[1], ref(F64, lse64, gs), ref(F32, torch.logsumexp(t.float(), -1), gs), "fwd_bwd_cap")
    for d in (dl.cpu(), out[1].cpu()):
        assert not d[t.float().abs() == c].any()                                              # factor exactly 0
        assert not d[(~valid)[:, None] | torch.isinf(t.float())].view(torch.int16).any()      # +0 by bits


@pytest.mark.parametrize("c", CAPS)
def test_row_kernels(c):
    g = torch.Generator().manual_seed(5)
    buf, dbuf = (torch.randn(5, 80, generator=g) * 2 * c).to(BF), torch.randn(5, 80, generator=g).to(BF)
    x, dy = buf[:, :72], dbuf[:, :72]        # [5, 72] views, row stride 80
    xd, dyd = buf.cuda()[:, :72], dbuf.cuda()[:, :72]
    y = K.softcap_fwd_(xd, c, out=torch.empty(5, 72, dtype=BF, device="cuda"))
    assert_bf16(y, c * torch.tanh(x.to(F64) / c), cap_fwd(x.float(), c), "softcap_fwd out of place")
    assert K.softcap_fwd_(xd, c) is xd and torch.equal(xd, y)
    assert torch.equal(xd._base[:, 72:].cpu(), buf[:, 72:])   # the view's gap is not written
    t = y.cpu()
    dx = K.softcap_bwd_(dyd, y, c, out=torch.empty(5, 72, dtype=BF, device="cuda"))
    assert_bf16(dx, dy.to(F64) * cap_grad(t.to(F64), c), dy.float() * cap_grad(t.float(), c), "softcap_bwd out of place")
    assert K.softcap_bwd_(dyd, y, c) is dyd and torch.equal(dyd, dx)


MCFG = dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_key_value_heads=1, vocab_size=512, rms_norm_eps=1e-5,
            rope_theta=10000.0, num_hidden_layers=2, max_position_embeddings=128, final_logit_softcapping=2.0)


@pytest.mark.parametrize("second", (False, True), ids=["ce-only", "second-consumer"])
def test_llama_final_softcap(monkeypatch, second):
    for name, val in (("DEVICE", "cuda"), ("LOCAL_RANK", "0"), ("CONTEXT_PARALLEL", "0"), ("FLASH_ATTEN", "1")):
        monkeypatch.setenv(name, val)
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.model import Llama
    pgm.setup_process_group_manager(1, 1, 1, 1)
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = Llama(types.SimpleNamespace(**MCFG))
    model.to(BF)
    with torch.no_grad():
        model.final_proj.weight.mul_(10.0)   # raw logits of several caps (std about 3 c)
    V, c = MCFG["vocab_size"], MCFG["final_logit_softcapping"]
    ids = torch.randint(0, V, (2, 129), generator=torch.Generator().manual_seed(1))
    inp, tgt = ids[:, :-1], ids[:, 1:].reshape(-1)

    def total(logits, ce):   # the second consumer's share of d loss / d logits is of the cross-entropy's size
        return ce + 4.0 * logits.float().square().mean() if second else ce

    calls = {"softcap_bwd_": [], "cross_entropy_grad_lse": []}
    for name, log in calls.items():
        monkeypatch.setattr(K, name, lambda *a, _f=getattr(K, name), _l=log, **k: (_l.append(k), _f(*a, **k))[1])
    logits = model(inp.cuda())
    loss = total(logits, F.cross_entropy(logits.view(-1, V), tgt.cuda()))   # (HipLogits: the HIP cross-entropy)
    loss.backward()
    # the fold is taken: the cross-entropy's share comes from the _cap kernel, the row kernel runs for the other alone
    assert [k.get("softcap") for k in calls["cross_entropy_grad_lse"]] == [c] and len(calls["softcap_bwd_"]) == int(second)
    p = {k: v.detach().float().cpu().requires_grad_(True) for k, v in model.named_parameters()}
    cos, sin = O.get_cos_sin(128, 64, base=10000.0)
    raw = O.llama_forward(inp, p, MCFG, cos.float(), sin.float(), norm=O.rmsnorm_flash_semantics)
    lr = c * torch.tanh(raw / c)
    loss_r = total(lr, F.cross_entropy(lr.reshape(-1, V), tgt))
    loss_r.backward()
    errs = {n: R.norm_rel(t.grad, p[n].grad) for n, t in model.named_parameters()}
    bite, err = R.norm_rel(raw.detach(), lr.detach()), R.norm_rel(logits, lr.detach())
    print(f"final softcap llama: loss {loss.item():.5f} vs {loss_r.item():.5f}, logits {err:.3e} (uncapped: {bite:.3e}), "
          f"worst grad {max(errs.values()):.3e} ({max(errs, key=errs.get)})")
    assert abs(loss.float().item() - loss_r.item()) < TOL * abs(loss_r.item()) and err < TOL
    assert max(errs.values()) < TOL, errs
    assert bite > 4 * err                    # the cap bites: uncapped logits are out of the tolerance's reach


def test_tp_refused_before_any_launch(monkeypatch):
    monkeypatch.setenv("DEVICE", "cuda")
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.model import Llama
    pgm.setup_process_group_manager(1, 1, 1, 1)
    monkeypatch.setattr(pgm.current(), "tp_world_size", 2)
    with pytest.raises(NotImplementedError, match="final_logit_softcapping"):
        Llama(types.SimpleNamespace(**MCFG))
