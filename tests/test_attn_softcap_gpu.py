"""Logit soft-capping against plain float64 torch on the CPU: c tanh(q k^T scale / c), masked_fill(-inf) with the
band's mask, softmax, autograd for dq / dk / dv.

Bounds of o and lse: tests/_attn_ref.py's, widened by the capping arithmetic alone.  With h = 2^-24 (f32 rounding; the
hardware exp2 and rcp are good to 1 ulp = 2 h), u = 1 - 2 rcp(1 + e), e = exp2(s k1): the rounded product s k1 and the
rounded k1 move e by |2 y| h each and exp2 by 2 h, and du / dln(e) = (1 - u^2) / 2 with |y| (1 - tanh^2 y) < 0.45, so
together < 2 h; the add 1 + e gives 2 r h <= 2 h (r <= 1), rcp 4 r h <= 4 h, the fma h |u| <= h: |du| < 9 h.  The capped
score t = u (c log2e) adds the product's and the constant's rounding, 2 h c: |dt| <= 11 h c =: CAP(c) nats.  That is a
relative error of the unnormalised P, so the lse moves by <= CAP and a normalised P by <= 2 CAP: o gets 2 CAP A more."""
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import picotron_oracle as O
from picotron_amd import kernels as K, switches
from tests import _attn_ref as R
from tests.test_attn_sinks_gpu import MASKS, MCFG, MS, TOL, band_of

pytestmark = pytest.mark.gpu
DEV, BF, F64 = "cuda", torch.bfloat16, torch.float64
B, H, HKV = 2, 4, 2
# scores well inside the cap; |s scale| = 100 c, tanh saturated; and (beyond the issue's two) y ~ N(0, 1), 1 - u^2 anywhere in (0, 1]
CAPS = {"c50-randn": (50.0, "randn"), "c2-saturated": (2.0, "offset+"), "c1-randn": (1.0, "randn")}


def capped_ref(q, k, v, do, scale, c, mask):
    """(Ref(o, lse, A), [dq, dk, dv]) in float64; c None: the plain softmax."""
    q6, k6, v6 = (t.to(F64).requires_grad_(True) for t in (q, k, v))
    kk, vv = (t.repeat_interleave(H // HKV, 2).transpose(1, 2) for t in (k6, v6))
    sc = q6.transpose(1, 2) @ kk.transpose(-1, -2) * scale
    sc = (sc if c is None else c * torch.tanh(sc / c)).masked_fill(~mask, float("-inf"))
    p = torch.softmax(sc, -1)
    o = (p @ vv).transpose(1, 2)
    o.backward(do.to(F64))
    ref = R.Ref(o=o.detach(), lse=torch.logsumexp(sc, -1).detach(), A=(p @ vv.abs()).transpose(1, 2).detach())
    return ref, [t.grad for t in (q6, k6, v6)]


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("D", (64, 128))
def test_forward_and_backward_against_float64(D, name, cap):
    """Gradients: the plain kernels' norm_rel error against their own float64 reference, same inputs and mask, is
    the yardstick; the soft-capped ones stay within 2x of it (one more rounding source on P, one on dS)."""
    (c, family), (S, window, cut) = CAPS[cap], MASKS[name]
    q, k, v, do = R.make_case(family, B, S, S, H, HKV, D, seed=len(name))
    scale, band = R.scale_of(D), band_of(S, window, cut)
    mask, kb = band.mask().cpu(), (band if (window or cut) else None)
    qd, kd, vd, dod = (t.to(DEV) for t in (q, k, v, do))
    run = lambda sc: (lambda o, lse: (o, lse) + K.attn_bwd(dod, qd, kd, vd, o, lse, scale, True, band=kb, softcap=sc)[:3])(
        *K.attn_fwd(qd, kd, vd, scale, True, band=kb, softcap=sc))   # noqa: E731
    got, again, plain = run(c), run(c), run(None)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                      # two launches, equal bits
    fwd, grads = capped_ref(q, k, v, do, scale, c, mask)
    tag, cap_err = f"softcap/d{D}/{name}/{cap}", 11 * 2.0 ** -24 * c
    R.check("out", got[0], fwd.o, R.SLACK * R.U * (fwd.A + fwd.o.abs()) + 2 * cap_err * fwd.A, tag)
    R.check("lse", got[1], fwd.lse, 2.0 ** -18 * fwd.lse.abs().clamp_min(1.0) + cap_err, tag)
    _, grads0 = capped_ref(q, k, v, do, scale, None, mask)
    for n, g, g0, want, want0 in zip(("dq", "dk", "dv"), got[2:], plain[2:], grads, grads0):
        err, err0 = R.norm_rel(g, want), R.norm_rel(g0, want0)
        R.WORST[(tag, n + "/plain")] = max(R.WORST.get((tag, n + "/plain"), 0.0), err / err0)
        print(f"attn-check {tag} {n} norm_rel {err:.3e} plain {err0:.3e} ratio {err / err0:.2f}")
        assert err <= 2 * err0, (n, err, err0)
    if family == "offset+":   # tanh = 1 in every visible score: 1 - u^2 = 0; a cap behind the mask or an inf * 0 shows here
        assert all(bool(torch.isfinite(t.float()).all()) for t in got)
        assert float(got[2].float().abs().max()) <= float(grads[0].abs().max())
        assert float(got[3].float().abs().max()) <= float(grads[1].abs().max())


def test_refusals_before_any_launch_and_none_is_the_plain_kernel(monkeypatch):
    q, k, v, do = (t.to(DEV) for t in R.make_case("randn", B, 256, 256, H, HKV, 64))
    sc = R.scale_of(64)
    for window in (None, 64):   # softcap=None / 0: the plain kernels' bits
        band = band_of(256, window, None) if window else None
        with switches.override(attn_kv_chunk=0):
            base = K.attn_fwd(q, k, v, sc, True, band=band)
        for none in (None, 0, 0.0):
            assert all(torch.equal(a, b) for a, b in zip(base, K.attn_fwd(q, k, v, sc, True, band=band, softcap=none)))
    o, lse = base
    lse3 = torch.zeros(B, H, 512, device=DEV)[:, :, :256]
    pos = torch.arange(256, device=DEV)
    bb = K.attn_block_band(K.attn_band(B, 256, DEV, window=64).kv_lo, pos, pos, True)
    q256 = torch.zeros(B, 256, H, 256, dtype=BF, device=DEV)
    monkeypatch.setattr(K._C, "lib", lambda: (_ for _ in ()).throw(AssertionError("a kernel was reached")))
    fwd = lambda **kw: K.attn_fwd(q, k, v, sc, kw.pop("causal", True), softcap=30.0, **kw)   # noqa: E731
    bwd = lambda **kw: K.attn_bwd(do, q, k, v, o, kw.pop("lse", lse), sc, True, softcap=30.0, **kw)   # noqa: E731
    refused = [lambda: K.attn_fwd(q256, q256[:, :, :HKV], q256[:, :, :HKV], sc, True, softcap=30.0),
               lambda: fwd(merge=True, out=torch.zeros(B, 256, H, 64, device=DEV), lse=lse.clone()),
               lambda: fwd(sinks=torch.zeros(H, dtype=BF, device=DEV)), lambda: fwd(causal=False), lambda: fwd(lse=lse3),
               lambda: bwd(grad_f32=True), lambda: bwd(delta=torch.zeros_like(lse)), lambda: bwd(lse=lse3),
               lambda: K.attn_fwd(q, k, v, sc, True, softcap=float("nan")), lambda: fwd(band=bb), lambda: bwd(band=bb)]
    for i, f in enumerate(refused):
        with pytest.raises((NotImplementedError, ValueError)):
            f()
            pytest.fail(f"case {i} was not refused")


def ref_llama(ids, p, masks, c):
    """The float64 model from the oracle's pieces plus the cap (test_attn_sinks_gpu.ref_llama without the sinks)."""
    nh, nkv, d = 4, 2, 64
    cos, sin = (t.to(F64) for t in O.get_cos_sin(MS, d, base=10000.0))
    norm = lambda x, w: x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-5) * w   # noqa: E731
    x = F.embedding(ids, p["embedding.weight"])
    b, s, _ = x.shape
    for i, mask in enumerate(masks):
        w = {n[len(f"decoder_layers.{i}."):]: t for n, t in p.items() if n.startswith(f"decoder_layers.{i}.")}
        h = norm(x, w["input_layernorm.weight"])
        q, k, v = (O.linear(h, w[f"attention.{n}_proj.weight"]).view(b, s, -1, d).transpose(1, 2) for n in "qkv")
        q, k = O.apply_rotary_pos_emb(q, cos, sin), O.apply_rotary_pos_emb(k, cos, sin).repeat_interleave(nh // nkv, 1)
        sc = (c * torch.tanh(q @ k.transpose(-1, -2) / d ** 0.5 / c)).masked_fill(~mask, float("-inf"))
        o = torch.softmax(sc, -1) @ v.repeat_interleave(nh // nkv, 1)
        x = x + O.linear(o.transpose(1, 2).reshape(b, s, nh * d), w["attention.out_proj.weight"])
        x = x + O.mlp(norm(x, w["post_attention_layernorm.weight"]), *(w[f"mlp.{n}_proj.weight"] for n in ("gate", "up", "down")))
    return O.linear(norm(x, p["final_norm.weight"]), p["final_proj.weight"])


def test_llama_two_layers_alternating_windows(monkeypatch):
    for name, val in (("DEVICE", "cuda"), ("LOCAL_RANK", "0"), ("CONTEXT_PARALLEL", "0"), ("FLASH_ATTEN", "1")):
        monkeypatch.setenv(name, val)
    from picotron_amd import functional as FN, process_group_manager as pgm
    from picotron_amd.model import Llama
    pgm.setup_process_group_manager(1, 1, 1, 1)
    torch.manual_seed(0)
    cfg = dict(MCFG, attention_sinks=False, attn_logit_softcapping=5.0, sliding_window=64,
               layer_types=["sliding_attention", "full_attention"])
    with torch.device("cuda"):
        model = Llama(types.SimpleNamespace(**cfg))
    model.to(BF)
    with torch.no_grad():   # the init's scores are a fraction of a nat: 4x the q and k projections, so that the cap bites
        for n, t in model.named_parameters():
            if "q_proj" in n or "k_proj" in n:
                t.mul_(4.0)
    V = cfg["vocab_size"]
    ids = torch.randint(0, V, (2, MS + 1), generator=torch.Generator().manual_seed(1))
    inp, tgt = ids[:, :-1], ids[:, 1:]
    logits = model(inp.cuda())
    loss = FN.cross_entropy(logits.view(-1, V), tgt.reshape(-1).cuda())
    loss.backward()
    p = {k: v.detach().to(F64).cpu().requires_grad_(True) for k, v in model.named_parameters()}
    lr = ref_llama(inp, p, [K.attn_band(2, MS, DEV, window=w).mask().cpu() for w in (64, None)], 5.0)
    loss_r = F.cross_entropy(lr.reshape(-1, V), tgt.reshape(-1))
    loss_r.backward()
    errs = {n: R.norm_rel(t.grad, p[n].grad) for n, t in model.named_parameters()}
    print(f"softcap llama: worst grad {max(errs.values()):.3e} ({max(errs, key=errs.get)})")
    assert abs(loss.float().item() - loss_r.item()) < TOL * abs(loss_r.item()) and R.norm_rel(logits, lr.detach()) < TOL
    assert max(errs.values()) < TOL, errs
    plain = ref_llama(inp, p, [K.attn_band(2, MS, DEV, window=w).mask().cpu() for w in (64, None)], 1e9)
    bite, err = R.norm_rel(lr.detach(), plain.detach()), R.norm_rel(logits, lr.detach())
    print(f"softcap llama: capped vs uncapped reference {bite:.3e}, model vs capped reference {err:.3e}")
    assert bite > 4 * err   # the cap bites: the uncapped model is not within the tolerance's reach
