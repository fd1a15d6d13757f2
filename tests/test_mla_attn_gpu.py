"""MLA attention kernels (csrc/attention_mla.hip) against a float64 reference, per element.

q / k heads are [128 nope | 64 rope], v / o heads 128 wide, k's rope columns one row per token shared
by the heads.  Inputs: tests/_attn_ref.py's families at D 192 (q, k) and D 128 (v, dO); k_pe is head
0's last 64 columns and the reference k is cat(k_nope, k_pe broadcast).  Bounds: _attn_ref's (out
1.5 u (A + |ref|); lse 2^-18 max(1, |ref|); bf16 gradients 2 * 1.5 u M + 1.5 * 2^-20 C); dk_pe's M
and C are the sums over heads of the per-head masses (f32 partials, one bf16 rounding)."""
import functools

import pytest
import torch

from tests import _attn_ref as R

pytestmark = pytest.mark.gpu

DN, DR, DV = 128, 64, 128
SCALE = R.scale_of(DN + DR)
# one block; an even block count (the paired launch); an odd block count, an odd head count, a batch stride
SHAPES = [(1, 128, 1), (1, 256, 2), (2, 384, 3)]


@functools.lru_cache(maxsize=None)
def case(family, B, S, H):
    """bf16 CPU (q, k_nope, k_pe, v, dO), the broadcast reference k and the float64 forward."""
    q, k, _, _ = R.make_case(family, B, S, S, H, H, DN + DR)
    _, _, v, do = R.make_case(family, B, S, S, H, H, DV)
    k_nope, k_pe = k[..., :DN].contiguous(), k[:, :, 0, DN:].contiguous()
    k_ref = torch.cat([k_nope, k_pe[:, :, None, :].expand(B, S, H, DR)], -1)
    return q, k_nope, k_pe, v, do, k_ref, R.ref_forward(q, k_ref, v, SCALE, R.causal_mask(S, S))


def ref_backward(q, k, v, do, o, lse, scale, mask):
    """_attn_ref.ref_backward for a v width other than q's, one k/v head per q head; dk_pe = the sum
    over heads of dk's rope columns, its masses the sums of the per-head masses."""
    F = R.F64
    q6, k6, v6, do6, o6 = (t.to(F) for t in (q, k, v, do, o))
    s = (torch.einsum("bqhd,bkhd->bhqk", q6, k6) * scale).masked_fill(~mask, float("-inf"))
    p = torch.exp(s - lse.to(F)[..., None])
    dp = torch.einsum("bqhd,bkhd->bhqk", do6, v6)
    delta = torch.einsum("bqhd,bqhd->bhq", do6, o6)
    ds = p * (dp - delta[..., None])
    e = p * (torch.einsum("bqhd,bkhd->bhqk", do6.abs(), v6.abs())
             + torch.einsum("bqhd,bqhd->bhq", do6.abs(), o6.abs())[..., None])
    r = R.Ref()
    r.dv = torch.einsum("bhqk,bqhd->bkhd", p, do6)
    r.M_dv = torch.einsum("bhqk,bqhd->bkhd", p, do6.abs())
    r.dk = scale * torch.einsum("bhqk,bqhd->bkhd", ds, q6)
    r.M_dk = scale * torch.einsum("bhqk,bqhd->bkhd", ds.abs(), q6.abs())
    r.C_dk = scale * torch.einsum("bhqk,bqhd->bkhd", e, q6.abs())
    r.dq = scale * torch.einsum("bhqk,bkhd->bqhd", ds, k6)
    r.M_dq = scale * torch.einsum("bhqk,bkhd->bqhd", ds.abs(), k6.abs())
    r.C_dq = scale * torch.einsum("bhqk,bkhd->bqhd", e, k6.abs())
    return r


def identity_tables(S):
    """cos = 1, sin = 0: the reduce pass's rotation returns its input bits."""
    return torch.ones(S, DR, dtype=R.BF, device="cuda"), torch.zeros(S, DR, dtype=R.BF, device="cuda")


def device_inputs(family, B, S, H, sliced):
    """The case on the device: contiguous, or as the module hands it over -- k_nope | v the column halves
    of a [B, S, H, 256] buffer, k_pe the last 64 columns of [B, S, 576] rows."""
    q, k_nope, k_pe, v, do = (t.cuda() for t in case(family, B, S, H)[:5])
    if sliced:
        kvb = torch.cat([k_nope, v], -1)
        kva = torch.cat([torch.full((B, S, 512), 3.0, dtype=R.BF, device="cuda"), k_pe], -1)
        k_nope, v, k_pe = kvb[..., :DN], kvb[..., DN:], kva[..., 512:]
    return q, k_nope, k_pe, v, do


def grad_sinks(B, S, H, sliced):
    if not sliced:
        return {}
    dkvb = torch.empty(B, S, H, DN + DV, dtype=R.BF, device="cuda")
    dkva = torch.empty(B, S, 576, dtype=R.BF, device="cuda")
    return dict(dk_nope=dkvb[..., :DN], dv=dkvb[..., DN:], dk_pe=dkva[..., 512:])


@pytest.mark.parametrize("sliced", [False, True], ids=["contig", "sliced"])
@pytest.mark.parametrize("B,S,H", SHAPES)
@pytest.mark.parametrize("family", ["randn", "peaked", "offset-", "zeroq"])
def test_mla_attention_matches_reference(family, B, S, H, sliced):
    from picotron_amd import kernels as K
    tag = f"mla-{family}-{B}x{S}x{H}-{'sliced' if sliced else 'contig'}"
    q, k_nope, k_pe, v, do, k_ref, fwd = case(family, B, S, H)
    dq_, dkn_, dkpe_, dv_, ddo = device_inputs(family, B, S, H, sliced)
    o, lse = K.mla_attn_fwd(dq_, dkn_, dkpe_, dv_, SCALE)
    R.check_out(o, fwd, tag)
    R.check_lse(lse, fwd.lse, tag)
    dq, dk_nope, dk_pe, dv = K.mla_attn_bwd(ddo, dq_, dkn_, dkpe_, dv_, o, lse, SCALE, *identity_tables(S),
                                            **grad_sinks(B, S, H, sliced))
    bwd = ref_backward(q, k_ref, v, do, o.cpu(), lse.cpu(), SCALE, R.causal_mask(S, S))
    k2, c = 2.0 * R.SLACK * R.U, R.SLACK * 2.0 ** -20
    R.check("dq", dq, bwd.dq, k2 * bwd.M_dq + c * bwd.C_dq, tag)
    R.check("dv", dv, bwd.dv, k2 * bwd.M_dv, tag)
    R.check("dk_nope", dk_nope, bwd.dk[..., :DN], k2 * bwd.M_dk[..., :DN] + c * bwd.C_dk[..., :DN], tag)
    R.check("dk_pe", dk_pe, bwd.dk[..., DN:].sum(2), k2 * bwd.M_dk[..., DN:].sum(2) + c * bwd.C_dk[..., DN:].sum(2), tag)


def test_mla_backward_is_deterministic():
    from picotron_amd import kernels as K
    B, S, H = SHAPES[2]
    q, k_nope, k_pe, v, do = device_inputs("randn", B, S, H, True)
    o, lse = K.mla_attn_fwd(q, k_nope, k_pe, v, SCALE)
    runs = [K.mla_attn_bwd(do, q, k_nope, k_pe, v, o, lse, SCALE, *identity_tables(S)) for _ in range(2)]
    for name, a, b in zip(("dq", "dk_nope", "dk_pe", "dv"), *runs):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("B,S,H", SHAPES)
def test_mla_rope_forward_then_inverse(B, S, H):
    """Each direction against float64 rotate_half on the bf16 tables, 2 u (|x1 cos| + |x2 sin|) per
    element; q's nope columns keep their bits."""
    from picotron_amd import kernels as K
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B * S, H * (DN + DR), generator=g).to(R.BF)
    kva = torch.randn(B * S, 576, generator=g).to(R.BF)
    ang = torch.arange(S, dtype=torch.float32)[:, None] * (1.0 / 10000.0 ** (torch.arange(0, DR, 2) / DR))[None, :]
    cos, sin = torch.cos(ang).to(R.BF).repeat(1, 2), torch.sin(ang).to(R.BF).repeat(1, 2)
    qd, kd = q.cuda(), kva.cuda()

    def rotate(x, sign):   # x [B * S, n, 64] float64 -> (rotated, bound)
        c, s = cos.to(R.F64).repeat(B, 1)[:, None, :], sign * sin.to(R.F64).repeat(B, 1)[:, None, :]
        x1, x2 = x[..., :DR // 2], x[..., DR // 2:]
        rot = torch.cat([-x2, x1], -1)
        return x * c + rot * s, 2 * R.U * ((x * c).abs() + (rot * s).abs())

    def ropes(qt, kt):    # the rotary vectors of a (q, kv_a) pair: [B * S, H + 1, 64]
        return torch.cat([qt.view(B * S, H, DN + DR)[..., DN:], kt[:, None, 512:]], 1).cpu().to(R.F64)

    for sign, inverse in ((1.0, False), (-1.0, True)):
        before = ropes(qd, kd)
        K.mla_rope_(qd, H, kd[:, 512:], cos.cuda(), sin.cuda(), S, inverse=inverse)
        ref, bound = rotate(before, sign)
        R.check("rope", ropes(qd, kd), ref, bound, f"mla-rope-{'inv' if inverse else 'fwd'}")
        assert torch.equal(qd.view(B * S, H, DN + DR)[..., :DN].cpu(), q.view(B * S, H, DN + DR)[..., :DN])
        assert torch.equal(kd[:, :512].cpu(), kva[:, :512])
