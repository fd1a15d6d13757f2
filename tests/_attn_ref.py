"""Attention conformance kit: adversarial input families, a float64 reference, a per-element
checker and an fp32 emulator of the kernels' documented numerics (csrc/attention.hip).

Layout everywhere: q, dO, o, dq [B, Sq, H, D]; k, v, dk, dv [B, Sk, HKV, D]; lse, delta [B, H, Sq].
`scale_of(D)` = 1 / sqrt(D) is the softmax scale of every case.  All inputs are bf16 CPU tensors and
the reference is always computed from those bf16 values in float64.

Input families (`make_case`)
    randn      the baseline: scores ~ N(0, 1), nearly uniform softmax.
    peaked     q, k ~ N(0, 12): scale q.k has std 12 nats, the softmax is nearly one-hot and the row
               max jumps by far more than 2^8 between key tiles.
    offset+/-  dimension 0 of q is c and of k is +c / -c (c^2 scale ~ 200), the other dimensions
               randn: every score is +-200 plus N(0, 1) noise, the softmax is that of the noise,
               LSE ~ +-200, and the running max is very negative for offset-.
    ramp       k_j = 0.25 randn + (j / 16) e0, q_i = 0.25 randn + 0.8 sqrt(D) e0: the score rises
               0.05 nat per key, 4.6 log2 units per 64-key tile -- under the lazy rescale threshold
               (8) for one tile and over it for two.
    zeroq      q = 0: exactly uniform softmax over the visible keys; causal row i is the mean of
               V[0..i] and lse_i = log(i + 1).
    headcode   randn q, k and V[:, :, hk, :] = hk + 1: O[:, :, h, :] == h // (H / HKV) + 1 exactly.

Checker: the derivation of the bounds
    u = 2^-8 is bf16 round-to-nearest's relative error.  With p the (unnormalised) softmax weights and
    A = P |V| the normalised absolute mass:
      * forward: P is rounded to bf16 once before P V (error <= u A after normalisation; l is summed
        from the unrounded P) and the output is rounded once (<= u |ref|):  u (A + |ref|).  The f32
        merge accumulator skips the output rounding: u A.
      * backward: P (for dV) or dS (for dK, dQ) is rounded once, error <= u M with M the product of
        absolute values (M_dV = P^T |dO|, M_dK = scale |dS|^T |Q|, M_dQ = scale |dS| |K|), and the
        bf16 output once more (|ref| <= M): 2 u M; an f32 accumulator u M plus the f32 rounding of the
        add onto its initial value, 2^-22 |initial| (up to H / HKV adds of <= 2^-24 relative each).
      * dS = P (dP - D) subtracts two f32 sums of bf16 products (dP = dO.v in MFMA order, D = dO.o in
        the delta kernel's order).  Each carries f32 summation error <= 2^-20 of its absolute sum --
        the bound `delta` itself gets -- so dS has the absolute error
        P 2^-20 (|dO|.|v| + |dO|.|o|), which does not vanish where dP - D cancels exactly (zeroq's
        row 0: P = 1, o = v0, dS = 0 in exact arithmetic).  It enters the dK / dQ bounds as its own
        mass C_dK = scale E^T |Q|, C_dQ = scale E |K| with E = P (|dO|.|v| + |dO|.|o|), times 2^-20;
        relative to the bf16 terms it is 2^-12.
      * every derived bound gets the factor 1.5 for the f32 summation order and the hardware
        exp2 / log.
      * lse is f32: 2^-18 max(1, |ref|); delta: 2^-20 sum |dO| |o|.
    Every check is per element and rejects any non-finite value.

Emulator (`emu_forward`, `emu_backward`): fp32 torch, 64-key tiles, f32 scores in log2 units, the
lazy running max (moved only when a tile's max exceeds it by more than 8 log2 units, so P may reach
2^8), P rounded to bf16 for P V while l sums the unrounded P, a bf16 output; backward with P and dS
rounded to bf16, D from the bf16 o, scale applied to the f32 sums.  `fault=` injects the bugs the
checker must reject (tests/test_attn_checker_cpu.py).
"""
import math

import torch

BF = torch.bfloat16
F64 = torch.float64
U = 2.0 ** -8          # bf16 round-to-nearest
SLACK = 1.5            # f32 summation order, hardware exp2 / log
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
RESCALE_LOG2 = 8.0     # attention.hip kRescaleLog2
KT = 64                # keys per tile
FAMILIES = ("randn", "peaked", "offset+", "offset-", "ramp", "zeroq", "headcode")


def scale_of(D):
    return 1.0 / math.sqrt(D)


# ------------------------------------------------------------------------------ input families
def make_case(family, B, Sq, Sk, H, HKV, D, seed=0):
    """bf16 CPU (q [B,Sq,H,D], k, v [B,Sk,HKV,D], dO [B,Sq,H,D]) of one family; deterministic."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * FAMILIES.index(family) + D + Sq + 3 * Sk)
    q = torch.randn(B, Sq, H, D, generator=g)
    k = torch.randn(B, Sk, HKV, D, generator=g)
    v = torch.randn(B, Sk, HKV, D, generator=g)
    do = torch.randn(B, Sq, H, D, generator=g)
    if family == "peaked":
        q *= math.sqrt(12.0)
        k *= math.sqrt(12.0)
    elif family in ("offset+", "offset-"):
        c = float(torch.tensor(math.sqrt(200.0 * math.sqrt(D))).to(BF))
        q[..., 0] = c
        k[..., 0] = c if family == "offset+" else -c
    elif family == "ramp":
        q *= 0.25
        k *= 0.25
        q[..., 0] += 0.8 * math.sqrt(D)
        k[..., 0] += (torch.arange(Sk, dtype=torch.float32) / 16.0)[None, :, None]
    elif family == "zeroq":
        q.zero_()
    elif family == "headcode":
        v[:] = (torch.arange(HKV, dtype=torch.float32) + 1.0)[None, None, :, None]
    elif family != "randn":
        raise KeyError(family)
    return q.to(BF), k.to(BF), v.to(BF), do.to(BF)


def make_merge_case(family, B, S, H, HKV, D, seed=0):
    """One query shard and three key blocks whose LSEs lie > 100 nats apart: dimension 0 of q is 32
    and of block b's keys t_b, with 32 t_b scale = the family's base (0, +100, -100) + (0, +170, -170) nats.
    Block 0 is the diagonal (causal) one.  Returns q, [(k_b, v_b)] * 3, dO (bf16, CPU)."""
    base = {"peaked": 0.0, "offset+": 100.0, "offset-": -100.0}[family]
    q, k, v, do = make_case("peaked" if family == "peaked" else "randn", B, S, 3 * S, H, HKV, D, seed)
    q = q.clone()
    k = k.clone()
    q[..., 0] = 32.0
    blocks = []
    for b, shift in enumerate((0.0, 170.0, -170.0)):
        kb = k[:, b * S:(b + 1) * S].clone()
        kb[..., 0] = (base + shift) / (32.0 * scale_of(D))
        blocks.append((kb, v[:, b * S:(b + 1) * S].contiguous()))
    return q, blocks, do


def causal_mask(Sq, Sk):
    """Key j visible to query i iff j <= i."""
    return torch.arange(Sk)[None, :] <= torch.arange(Sq)[:, None]


def block_mask(Sq, blocks):
    """[Sq, sum Sk] visibility over a concatenation of key blocks, `blocks` = [(Sk, causal)]."""
    return torch.cat([causal_mask(Sq, sk) if c else torch.ones(Sq, sk, dtype=torch.bool) for sk, c in blocks], 1)


# ------------------------------------------------------------------------------ float64 reference
class Ref:
    """Named float64 results."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _expand(t, rep):   # [B, Sk, HKV, D] -> [B, Sk, H, D], query head h reads kv head h // rep
    return t.repeat_interleave(rep, dim=2)


def _scores(q, k, scale, mask):
    rep = q.shape[2] // k.shape[2]
    s = torch.einsum("bqhd,bkhd->bhqk", q.to(F64), _expand(k.to(F64), rep)) * scale
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    return s


def ref_forward(q, k, v, scale, mask=None):
    """o [B,Sq,H,D], lse [B,H,Sq], A = P |V| [B,Sq,H,D] in float64; mask [Sq,Sk] bool or None."""
    rep = q.shape[2] // k.shape[2]
    s = _scores(q, k, scale, mask)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    vv = _expand(v.to(F64), rep)
    return Ref(o=torch.einsum("bhqk,bkhd->bqhd", p, vv), lse=lse, A=torch.einsum("bhqk,bkhd->bqhd", p, vv.abs()))


def ref_backward(q, k, v, do, lse, scale, mask=None, o=None, delta=None):
    """The backward as a pure function of what the kernel is given: P = exp(S - lse),
    D = delta or sum dO o, dS = P (dP - D); dq, dk, dv, their masses M_* and cancellation masses C_*,
    and delta with its mass M_delta (when computed from o)."""
    B, Sq, H, D = q.shape
    HKV = k.shape[2]
    rep = H // HKV
    q6, do6 = q.to(F64), do.to(F64)
    kk, vv = _expand(k.to(F64), rep), _expand(v.to(F64), rep)
    p = torch.exp(_scores(q, k, scale, mask) - lse.to(F64)[..., None])
    dp = torch.einsum("bqhd,bkhd->bhqk", do6, vv)
    dp_abs = torch.einsum("bqhd,bkhd->bhqk", do6.abs(), vv.abs())
    r = Ref()
    if delta is None:
        r.delta = torch.einsum("bqhd,bqhd->bhq", do6, o.to(F64))
        r.M_delta = torch.einsum("bqhd,bqhd->bhq", do6.abs(), o.to(F64).abs())
        d_abs = r.M_delta
    else:
        r.delta = delta.to(F64)
        d_abs = r.delta.abs()
    ds = p * (dp - r.delta[..., None])
    e = p * (dp_abs + d_abs[..., None])          # f32 cancellation error of dS, in units of 2^-20

    def fold(t):   # sum a [B, Sk, H, D] gradient over a kv head's query heads
        return t.view(B, -1, HKV, rep, D).sum(3)

    r.dv = fold(torch.einsum("bhqk,bqhd->bkhd", p, do6))
    r.M_dv = fold(torch.einsum("bhqk,bqhd->bkhd", p, do6.abs()))
    r.dk = scale * fold(torch.einsum("bhqk,bqhd->bkhd", ds, q6))
    r.M_dk = scale * fold(torch.einsum("bhqk,bqhd->bkhd", ds.abs(), q6.abs()))
    r.C_dk = scale * fold(torch.einsum("bhqk,bqhd->bkhd", e, q6.abs()))
    r.dq = scale * torch.einsum("bhqk,bkhd->bqhd", ds, kk)
    r.M_dq = scale * torch.einsum("bhqk,bkhd->bqhd", ds.abs(), kk.abs())
    r.C_dq = scale * torch.einsum("bhqk,bkhd->bqhd", e, kk.abs())
    return r


# ------------------------------------------------------------------------------ checker
WORST = {}   # (tag, quantity) -> worst ratio to the bound seen in this process


def check(name, got, ref, bound, tag=None):
    """Per element: got finite and |got - ref| <= bound.  Returns the worst |got - ref| / bound (0 / 0
    counts as 0) and prints it; raises AssertionError naming the worst element otherwise."""
    g = got.detach().to("cpu").to(F64)
    ref, bound = ref.to(F64), bound.to(F64)
    assert g.shape == ref.shape, f"{name}: shape {tuple(g.shape)} != {tuple(ref.shape)}"
    finite = torch.isfinite(g)
    assert bool(finite.all()), f"{name}: {int((~finite).sum())} non-finite values, first at " \
                               f"{tuple(int(i) for i in (~finite).nonzero()[0])}"
    err = (g - ref).abs()
    ratio = torch.where(err > 0, err / bound, torch.zeros_like(err))   # x / 0 = inf for x > 0
    worst = float(ratio.max())
    key = (tag, name)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"attn-check {tag or '-'} {name} worst ratio {worst:.3f}")
    if not worst <= 1.0:
        idx = tuple(int(i) for i in (ratio == ratio.max()).nonzero()[0])
        raise AssertionError(f"{name}: {int((ratio > 1).sum())} of {ratio.numel()} elements over the bound; worst "
                             f"at {idx}: got {float(g[idx])!r} ref {float(ref[idx])!r} err {float(err[idx]):.3e} "
                             f"bound {float(bound[idx]):.3e} (ratio {worst:.2f})")
    return worst


def check_out(got, fwd, tag=None, name="out"):
    """A bf16 output: P rounded once, the output rounded once."""
    return check(name, got, fwd.o, SLACK * U * (fwd.A + fwd.o.abs()), tag)


def check_acc(got, fwd, tag=None, name="acc"):
    """The f32 merge accumulator: P rounded once."""
    return check(name, got, fwd.o, SLACK * U * fwd.A, tag)


def check_lse(got, lse_ref, tag=None, name="lse"):
    return check(name, got, lse_ref, 2.0 ** -18 * lse_ref.abs().clamp_min(1.0), tag)


def check_delta(got, bwd, tag=None, name="delta"):
    return check(name, got, bwd.delta, 2.0 ** -20 * bwd.M_delta, tag)


def _grad_bounds(bwd, f32):
    k = (1.0 if f32 else 2.0) * SLACK * U
    c = SLACK * 2.0 ** -20
    return {"dq": k * bwd.M_dq + c * bwd.C_dq, "dk": k * bwd.M_dk + c * bwd.C_dk, "dv": k * bwd.M_dv}


def check_grads(dq, dk, dv, bwd, tag=None, which=("dq", "dk", "dv")):
    """bf16 dq, dk, dv: P or dS rounded once, the output rounded once (3 u M)."""
    bounds = _grad_bounds(bwd, False)
    return {n: check(n, g, getattr(bwd, n), bounds[n], tag) for n, g in (("dq", dq), ("dk", dk), ("dv", dv))
            if n in which}


def check_grads_f32(dq, dk, dv, bwd, init, tag=None, which=("dq", "dk", "dv")):
    """f32 accumulators that held `init` = {name: tensor}: reference + initial, 1.5 u M + 2^-22 |initial|."""
    bounds = _grad_bounds(bwd, True)
    out = {}
    for n, g in (("dq", dq), ("dk", dk), ("dv", dv)):
        if n in which:
            i0 = init[n].detach().to("cpu").to(F64)
            out[n] = check(n + "_f32", g, getattr(bwd, n) + i0, bounds[n] + 2.0 ** -22 * i0.abs(), tag)
    return out


def norm_rel(got, ref):
    """The suite's older global metric: Frobenius-norm ratio."""
    got, ref = got.detach().to("cpu").to(F64), ref.to(F64)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-12))


# ------------------------------------------------------------------------------ fp32 emulator
FAULTS = ("mask_lt", "mask_le1", "no_alpha_o", "no_alpha_l", "m_init0", "kv_mod", "p_trunc", "bad_row", "bad_elem",
          "lse_off")


def _bf(x):
    return x.to(BF).float()


def _bf_trunc(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _kv_heads(t, H, fault):
    HKV = t.shape[2]
    idx = torch.arange(H) % HKV if fault == "kv_mod" else torch.arange(H) // (H // HKV)
    return t.float()[:, :, idx]


def emu_forward(q, k, v, scale, causal, fault=None, f32_out=False):
    """(o bf16 [B,Sq,H,D], lse f32 [B,H,Sq]) as the forward kernel computes them; f32_out: o unrounded,
    as the merge mode adds it to its f32 accumulator."""
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    qf = q.float().permute(0, 2, 1, 3)                                    # [B, H, Sq, D]
    kf = _kv_heads(k, H, fault).permute(0, 2, 1, 3)
    vf = _kv_heads(v, H, fault).permute(0, 2, 1, 3)
    c2 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    i = torch.arange(Sq)[:, None]
    m = torch.full((B, H, Sq), 0.0 if fault == "m_init0" else float("-inf"))
    l = torch.zeros(B, H, Sq)
    o = torch.zeros(B, H, Sq, D)
    for k0 in range(0, Sk, KT):
        j = torch.arange(k0, min(k0 + KT, Sk))[None, :]
        s = qf @ kf[:, :, k0:k0 + KT].transpose(-1, -2)
        if causal:
            vis = {"mask_lt": j < i, "mask_le1": j <= i + 1}.get(fault, j <= i)
            s = s.masked_fill(~vis, float("-inf"))
        mt = s.amax(-1) * c2
        grew = mt > m + RESCALE_LOG2
        mn = torch.where(grew, torch.maximum(m, mt), m)
        alpha = torch.exp2(m - mn)
        alpha = torch.where(m == mn, torch.ones_like(alpha), alpha)         # exp2(-inf - -inf): no key seen yet
        m = mn
        if fault != "no_alpha_l":
            l = l * alpha
        if fault != "no_alpha_o":
            o = o * alpha[..., None]
        p = torch.exp2(s * c2 - m[..., None])
        p = torch.where(torch.isneginf(s), torch.zeros_like(p), p)          # a row with no visible key yet
        l = l + p.sum(-1)
        o = o + (_bf_trunc(p) if fault == "p_trunc" else _bf(p)) @ vf[:, :, k0:k0 + KT]
    out = (o / l[..., None]).to(torch.float32 if f32_out else BF).permute(0, 2, 1, 3).contiguous()
    lse = m * LN2 + torch.log(l)
    if fault == "bad_row":        # row 64 of (batch 0, head 0) holds row 63's result
        out[0, 64, 0] = out[0, 63, 0]
    elif fault == "bad_elem":     # one element 2^-5 (4 to 8 bf16 ulps) off
        out[0, 65, 0, 3] = (out[0, 65, 0, 3].float() * (1 + 2.0 ** -5)).to(out.dtype)
    elif fault == "lse_off":
        lse = lse + 1e-3
    return out, lse


def emu_backward(q, k, v, do, o, lse, scale, causal, f32=False):
    """(dq, dk, dv, delta) as the backward kernels compute them from the bf16 o and the f32 lse;
    bf16 gradients, or f32 (to add onto an accumulator) with f32 = True."""
    B, Sq, H, D = q.shape
    Sk, HKV = k.shape[1], k.shape[2]
    rep = H // HKV
    qf, dof = q.float().permute(0, 2, 1, 3), do.float().permute(0, 2, 1, 3)
    kf = _kv_heads(k, H, None).permute(0, 2, 1, 3)
    vf = _kv_heads(v, H, None).permute(0, 2, 1, 3)
    c2 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    delta = (do.float() * o.float()).sum(-1).permute(0, 2, 1)            # [B, H, Sq]
    s = qf @ kf.transpose(-1, -2)
    p = torch.exp2(s * c2 - (lse.float() * LOG2E)[..., None])
    if causal:
        p = p.masked_fill(~causal_mask(Sq, Sk), 0.0)
    ds = _bf(p * (dof @ vf.transpose(-1, -2) - delta[..., None]))
    dv = _bf(p).transpose(-1, -2) @ dof                                    # [B, H, Sk, D]
    dk = (ds.transpose(-1, -2) @ qf) * scale
    dq = ((ds @ kf) * scale).permute(0, 2, 1, 3)
    dk, dv = (t.view(B, HKV, rep, Sk, D).sum(2).permute(0, 2, 1, 3) for t in (dk, dv))
    if f32:
        return dq.contiguous(), dk.contiguous(), dv.contiguous(), delta
    return dq.to(BF).contiguous(), dk.to(BF).contiguous(), dv.to(BF).contiguous(), delta
