"""Attention kernels (csrc/attention.hip, through picotron_amd.kernels) against a float64 reference,
per element, on adversarial inputs.  Families, reference, bounds and their derivation: tests/_attn_ref.py
(self-tested without a GPU in tests/test_attn_checker_cpu.py).

Shapes are the smallest that reach each path of pt_attn_fwd / attn_bwd_impl's dispatch:
    d64   S 128 one query block | 256 two blocks, causal pairing on | 384 three, pairing off |
          512 eight K tiles: the 4-stage staging ring wraps
    d128  S 128 4-wave | 256 8-wave, one block | 384 4-wave, three blocks | 512 8-wave, paired
At these sizes every d64 launch has fewer than 128 workgroups, so pt_attn_split_plan would route it
to the few-head split forms; the d64 cases set attn_kv_chunk = 0 to reach the regular kernels, and
the split forms are run on purpose (chunks 2 and 4) in test_few_head_split_forms.

Worst observed |got - ref| / bound (1 = the bound) per family, over every test of this file on an
MI355X (each check prints its figure: run with -rA).  acc / lse_m: the merge mode's f32 accumulator
and merged lse; *_f32: f32 accumulation onto non-zero gradients (attn_bwd_part's tests); -: not run.

    family    out    lse    delta  dq     dk     dv     acc    lse_m  dq_f32 dk_f32 dv_f32
    randn     0.499  0.047  0.095  0.568  0.547  0.583  -      -      0.361  0.262  0.179
    peaked    0.618  0.110  0.085  0.619  0.613  0.623  0.582  0.104  0.615  0.622  0.619
    offset+   0.502  0.090  0.068  0.541  0.536  0.568  0.201  0.033  -      -      -
    offset-   0.535  0.081  0.073  0.549  0.613  0.562  0.201  0.030  -      -      -
    ramp      0.487  0.043  0.076  0.516  0.534  0.570  -      -      -      -      -
    zeroq     0.332  0.045  0.065  0.512  0.000  0.503  -      -      -      -      -
    headcode  0.000  0.042  0.024  0.004  0.001  0.505  -      -      -      -      -

No shipped kernel exceeded a bound: the margin is 1.6x or more everywhere.  zeroq's dk and headcode's
out are exact (the reference is 0, resp. the head code); headcode's dq / dk references are 0 and
their bound is the f32 cancellation term alone (_attn_ref.py).
"""
import pytest
import torch

from oracle import picotron_oracle as O
from picotron_amd import switches
from tests import _attn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN16 = 0x7FC1          # a bf16 NaN
NAN32 = 0x7FC00001      # an f32 NaN

# D, S, B, H, HKV
SHAPES = [(64, 128, 2, 4, 2), (64, 256, 1, 2, 1), (64, 384, 1, 4, 4), (64, 512, 2, 4, 2),
          (128, 128, 2, 2, 1), (128, 256, 1, 4, 2), (128, 384, 1, 2, 2), (128, 512, 2, 4, 2)]
FULL_FAMILIES = ("randn", "peaked", "offset-")
CASES = [(f, s, True) for f in R.FAMILIES for s in SHAPES] + [(f, s, False) for f in FULL_FAMILIES for s in SHAPES]


def K_():
    from picotron_amd import kernels
    return kernels


def dev(*ts):
    return [t.to(DEV) for t in ts]


def regular():
    """The regular (not few-head split) kernels at these small shapes."""
    return switches.override(attn_kv_chunk=0)


def ibits(t):
    """The bits of a bf16 / f32 tensor as an integer CPU tensor."""
    return t.detach().contiguous().view(torch.int16 if t.dtype == BF else torch.int32).cpu()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(ibits(a), ibits(b))


def sentinel(shape, dtype):
    """A device tensor whose every element is a NaN with a payload."""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.int16 if dtype == BF else torch.int32).fill_(NAN16 if dtype == BF else NAN32)
    return t


def guards_intact(buf, region):
    """Every element of `buf` outside buf[region] still holds the sentinel's bits."""
    ib = buf.view(torch.int16 if buf.dtype == BF else torch.int32).clone()
    pat = NAN16 if buf.dtype == BF else NAN32
    ib[region] = pat
    return bool((ib == pat).all())


def mask_of(Sq, Sk, causal):
    return R.causal_mask(Sq, Sk) if causal else None


def norm_ok(got, ref, tol):
    """The suite's older global metric, where the reference is not identically zero."""
    return float(ref.abs().max()) == 0.0 or R.norm_rel(got, ref) < tol


def fwd_bwd_against_reference(family, B, Sq, Sk, H, HKV, D, causal, backward=True):
    K = K_()
    q, k, v, do = R.make_case(family, B, Sq, Sk, H, HKV, D)
    scale = R.scale_of(D)
    qd, kd, vd, dod = dev(q, k, v, do)
    o, lse = K.attn_fwd(qd, kd, vd, scale, causal)
    mask = mask_of(Sq, Sk, causal)
    ref = R.ref_forward(q, k, v, scale, mask)
    R.check_out(o, ref, family)
    R.check_lse(lse, ref.lse, family)
    assert R.norm_rel(o, ref.o) < 1e-2
    if family == "zeroq" and causal:
        n = torch.arange(1, Sq + 1, dtype=torch.float64)
        R.check_lse(lse, torch.log(n).expand(B, H, Sq), family, name="lse_closed_form")
    if family == "headcode":
        code = (torch.arange(H) // (H // HKV) + 1).to(BF)[None, None, :, None].expand(B, Sq, H, D)
        assert torch.equal(o.cpu(), code)
    if not backward:
        return
    dq, dk, dv, delta = K.attn_bwd(dod, qd, kd, vd, o, lse, scale, causal)
    torch.cuda.synchronize()
    bwd = R.ref_backward(q, k, v, do, lse.cpu(), scale, mask, o=o.cpu())
    R.check_delta(delta, bwd, family)
    R.check_grads(dq, dk, dv, bwd, family)
    assert norm_ok(dq, bwd.dq, 2e-2) and norm_ok(dk, bwd.dk, 2e-2) and norm_ok(dv, bwd.dv, 2e-2)


# ---------------------------------------------------------------- a. forward and backward vs the reference
@pytest.mark.parametrize("family,shape,causal", CASES,
                         ids=[f"{f}-d{s[0]}-S{s[1]}-{'causal' if c else 'full'}" for f, s, c in CASES])
def test_fwd_bwd_vs_reference(family, shape, causal):
    D, S, B, H, HKV = shape
    if family == "headcode":
        H, HKV = 4, 2          # distinct kv heads under GQA: h // rep and h % HKV differ
    with regular():
        fwd_bwd_against_reference(family, B, S, S, H, HKV, D, causal)


# ---------------------------------------------------------------- b. non-causal Sq != Sk
@pytest.mark.parametrize("family", ["randn", "peaked"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq,Sk,backward", [(128, 192, False), (256, 128, False), (128, 384, True), (256, 128, True)])
def test_full_attention_unequal_lengths(family, D, Sq, Sk, backward):
    with regular():
        fwd_bwd_against_reference(family, 1, Sq, Sk, 4, 2, D, False, backward)


# ---------------------------------------------------------------- c. variant forms on adversarial data
VARIANT_FAMILIES = ("peaked", "offset-", "ramp")


def _fwd_bwd(K, q, k, v, do, scale, causal):
    o, lse = K.attn_fwd(q, k, v, scale, causal)
    dq, dk, dv, delta = K.attn_bwd(do, q, k, v, o, lse, scale, causal)
    torch.cuda.synchronize()
    return o, lse, dq, dk, dv, delta


@pytest.mark.parametrize("family", VARIANT_FAMILIES)
@pytest.mark.parametrize("D,S", [(64, 256), (64, 384), (128, 256), (128, 512)])
def test_dkdv_wave_pair_split_is_bit_identical(family, D, S):
    K = K_()
    q, k, v, do = dev(*R.make_case(family, 1, S, S, 4, 2, D))
    res = []
    for m in (0, 3):
        with switches.override(attn_split=m, attn_kv_chunk=0):
            res.append(_fwd_bwd(K, q, k, v, do, R.scale_of(D), True))
    for a, b in zip(res[0][2:5], res[1][2:5]):
        assert same_bits(a, b)


@pytest.mark.parametrize("family", VARIANT_FAMILIES)
@pytest.mark.parametrize("D,S", [(64, 256), (64, 512), (128, 512)])
def test_causal_pairing_is_bit_identical(family, D, S):
    K = K_()
    q, k, v, do = dev(*R.make_case(family, 1, S, S, 4, 2, D))
    res = []
    for pair in (0, 1):
        with switches.override(attn_pair=pair, attn_kv_chunk=0):
            res.append(_fwd_bwd(K, q, k, v, do, R.scale_of(D), True))
    for a, b in zip(res[0][:5], res[1][:5]):
        assert same_bits(a, b)


@pytest.mark.parametrize("family", VARIANT_FAMILIES)
@pytest.mark.parametrize("D,S", [(64, 256), (128, 256)])
def test_fused_and_separate_delta_agree_to_the_checker(family, D, S):
    K = K_()
    q, k, v, do = R.make_case(family, 2, S, S, 2, 1, D)
    qd, kd, vd, dod = dev(q, k, v, do)
    scale = R.scale_of(D)
    with regular():
        o, lse = K.attn_fwd(qd, kd, vd, scale, True)
        bwd = R.ref_backward(q, k, v, do, lse.cpu(), scale, R.causal_mask(S, S), o=o.cpu())
        for fuse in (1, 0):
            with switches.override(fuse_delta=fuse):
                dq, dk, dv, delta = K.attn_bwd(dod, qd, kd, vd, o, lse, scale, True)
            torch.cuda.synchronize()
            R.check_delta(delta, bwd, family)
            R.check_grads(dq, dk, dv, bwd, family)


@pytest.mark.parametrize("family", VARIANT_FAMILIES)
@pytest.mark.parametrize("chunk", [2, 4])
def test_few_head_split_forms(family, chunk):
    K = K_()
    B, S, H, HKV, D = 4, 512, 4, 2, 64
    q, k, v, do = R.make_case(family, B, S, S, H, HKV, D)
    qd, kd, vd, dod = dev(q, k, v, do)
    scale = R.scale_of(D)
    with switches.override(attn_kv_chunk=chunk):
        assert K._attn_split_ws(B, H, HKV, S, S, D, True, 0, qd.device) is not None   # the split forms do run
        o, lse, dq, dk, dv, delta = _fwd_bwd(K, qd, kd, vd, dod, scale, True)
    mask = R.causal_mask(S, S)
    ref = R.ref_forward(q, k, v, scale, mask)
    R.check_out(o, ref, family)           # every check rejects any non-finite element
    R.check_lse(lse, ref.lse, family)
    bwd = R.ref_backward(q, k, v, do, lse.cpu(), scale, mask, o=o.cpu())
    R.check_delta(delta, bwd, family)
    R.check_grads(dq, dk, dv, bwd, family)


# ---------------------------------------------------------------- d. merge mode
@pytest.mark.parametrize("family", ["peaked", "offset+", "offset-"])
@pytest.mark.parametrize("D,S", [(64, 128), (128, 256)])
@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)])
def test_merge_three_blocks(family, D, S, order):
    """acc = 0, lse = -inf, then the diagonal (causal) block and two full blocks whose LSEs lie 170
    nats above and below it, merged in two orders: float64 attention over the concatenation."""
    K = K_()
    B, H, HKV = 1, 4, 2
    q, blocks, _ = R.make_merge_case(family, B, S, H, HKV, D)
    scale = R.scale_of(D)
    qd = q.to(DEV)
    acc = torch.zeros(B, S, H, D, dtype=torch.float32, device=DEV)
    lse = torch.full((B, H, S), float("-inf"), device=DEV)
    for b in order:
        kb, vb = dev(*blocks[b])
        K.attn_fwd(qd, kb, vb, scale, b == 0, out=acc, lse=lse, merge=True)
    torch.cuda.synchronize()
    kc = torch.cat([kb for kb, _ in blocks], 1)
    vc = torch.cat([vb for _, vb in blocks], 1)
    ref = R.ref_forward(q, kc, vc, scale, R.block_mask(S, [(S, True), (S, False), (S, False)]))
    R.check_acc(acc, ref, family)
    R.check_lse(lse, ref.lse, family, name="lse_merged")
    assert R.norm_rel(acc, ref.o) < 1e-2


# ---------------------------------------------------------------- e. lse and delta as slices
@pytest.mark.parametrize("family", ["randn", "offset-"])
@pytest.mark.parametrize("D", [64, 128])
def test_lse_and_delta_as_slices_of_longer_rows(family, D):
    K = K_()
    B, S, H, HKV = 2, 256, 2, 1
    q, k, v, do = dev(*R.make_case(family, B, S, S, H, HKV, D))
    scale = R.scale_of(D)
    sl = (slice(None), slice(None), slice(128, 128 + S))
    with regular():
        o0, lse0 = K.attn_fwd(q, k, v, scale, True)
        delta0 = K.attn_delta(do, o0)
        g0 = K.attn_bwd(do, q, k, v, o0, lse0, scale, True, delta=delta0)[:3]
        lbuf, dbuf = sentinel((B, H, S + 256), torch.float32), sentinel((B, H, S + 256), torch.float32)
        o1, lse1 = K.attn_fwd(q, k, v, scale, True, lse=lbuf[sl])
        delta1 = K.attn_delta(do, o1, dbuf[sl])
        g1 = K.attn_bwd(do, q, k, v, o1, lbuf[sl], scale, True, delta=dbuf[sl])[:3]
    torch.cuda.synchronize()
    assert lse1.data_ptr() == lbuf[sl].data_ptr() and delta1.data_ptr() == dbuf[sl].data_ptr()
    assert same_bits(o1, o0) and same_bits(lbuf[sl], lse0) and same_bits(dbuf[sl], delta0)
    for a, b in zip(g1, g0):
        assert same_bits(a, b)
    assert guards_intact(lbuf, sl) and guards_intact(dbuf, sl)


# ---------------------------------------------------------------- f. attn_bwd_part
@pytest.mark.parametrize("family", ["randn", "peaked"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq,Sk", [(128, 256), (256, 128)])
def test_bwd_part_equals_whole_backward(family, D, Sq, Sk):
    """The context-parallel mesh backward's block shapes, non-causal: parts = 1 gives attn_bwd's dq
    and parts = 2 its dk, dv bit for bit (bf16 stores and f32 accumulation onto non-zero values),
    and the f32 accumulators hold reference + initial."""
    K = K_()
    B, H, HKV = 1, 4, 2
    q, k, v, do = R.make_case(family, B, Sq, Sk, H, HKV, D)
    qd, kd, vd, dod = dev(q, k, v, do)
    scale = R.scale_of(D)
    with regular():
        o, lse = K.attn_fwd(qd, kd, vd, scale, False)
        delta = K.attn_delta(dod, o)
        dq0, dk0, dv0, _ = K.attn_bwd(dod, qd, kd, vd, o, lse, scale, False, delta=delta)
        dq1, dk1, dv1 = torch.empty_like(dq0), torch.empty_like(dk0), torch.empty_like(dv0)
        K.attn_bwd_part(dod, qd, kd, vd, lse, delta, scale, False, dq=dq1, grad_f32=False)
        K.attn_bwd_part(dod, qd, kd, vd, lse, delta, scale, False, dk=dk1, dv=dv1, grad_f32=False)
        g = torch.Generator().manual_seed(5)
        init = {"dq": torch.randn(B, Sq, H, D, generator=g), "dk": torch.randn(B, Sk, HKV, D, generator=g),
                "dv": torch.randn(B, Sk, HKV, D, generator=g)}
        a0 = {n: t.to(DEV) for n, t in init.items()}
        a1 = {n: t.to(DEV) for n, t in init.items()}
        K.attn_bwd(dod, qd, kd, vd, o, lse, scale, False, dq=a0["dq"], dk=a0["dk"], dv=a0["dv"], grad_f32=True,
                   delta=delta)
        K.attn_bwd_part(dod, qd, kd, vd, lse, delta, scale, False, dq=a1["dq"], grad_f32=True)
        K.attn_bwd_part(dod, qd, kd, vd, lse, delta, scale, False, dk=a1["dk"], dv=a1["dv"], grad_f32=True)
    torch.cuda.synchronize()
    assert same_bits(dq1, dq0) and same_bits(dk1, dk0) and same_bits(dv1, dv0)
    for n in ("dq", "dk", "dv"):
        assert same_bits(a1[n], a0[n])
    bwd = R.ref_backward(q, k, v, do, lse.cpu(), scale, None, delta=delta.cpu())
    R.check_grads(dq1, dk1, dv1, bwd, family)
    R.check_grads_f32(a1["dq"], a1["dk"], a1["dv"], bwd, init, family)


# ---------------------------------------------------------------- g. guarded outputs
@pytest.mark.parametrize("D,chunk", [(64, 0), (64, 4), (128, 0)])
def test_strided_views_leave_their_neighbours_alone(D, chunk):
    """out, dq, dk, dv as [..., :D] views of [B, S, H, D + 8] buffers; q, k, v as column slices of one
    fused qkv buffer whose batch stride exceeds S rows; every buffer pre-filled with a NaN sentinel."""
    K = K_()
    B, S, H, HKV = 2, 256, 4, 2
    q, k, v, do = dev(*R.make_case("peaked", B, S, S, H, HKV, D))
    scale = R.scale_of(D)
    W = (H + 2 * HKV) * D
    qkv = sentinel((B, S + 3, W), BF)
    qs = qkv[:, :S, :H * D].unflatten(-1, (H, D))
    ks = qkv[:, :S, H * D:(H + HKV) * D].unflatten(-1, (HKV, D))
    vs = qkv[:, :S, (H + HKV) * D:].unflatten(-1, (HKV, D))
    qs.copy_(q)
    ks.copy_(k)
    vs.copy_(v)
    assert qs.stride(0) > S * W and not qs.is_contiguous()
    dobuf = sentinel((B, S, H, D + 8), BF)
    dos = dobuf[..., :D]
    dos.copy_(do)
    region = (Ellipsis, slice(0, D))
    with switches.override(attn_kv_chunk=chunk):
        o0, lse0, dq0, dk0, dv0, delta0 = _fwd_bwd(K, q, k, v, do, scale, True)
        obuf = sentinel((B, S, H, D + 8), BF)
        gq, gk, gv = sentinel((B, S, H, D + 8), BF), sentinel((B, S, HKV, D + 8), BF), sentinel((B, S, HKV, D + 8), BF)
        o1, lse1 = K.attn_fwd(qs, ks, vs, scale, True, out=obuf[region])
        K.attn_bwd(dos, qs, ks, vs, o1, lse1, scale, True, dq=gq[region], dk=gk[region], dv=gv[region])
        # and the separate-delta form's launches
        gq2, gk2, gv2 = (sentinel(t.shape, BF) for t in (gq, gk, gv))
        with switches.override(fuse_delta=0):
            dq2, dk2, dv2, _ = K.attn_bwd(do, q, k, v, o0, lse0, scale, True)
            K.attn_bwd(dos, qs, ks, vs, o1, lse1, scale, True, dq=gq2[region], dk=gk2[region], dv=gv2[region])
    torch.cuda.synchronize()
    assert same_bits(obuf[region], o0) and same_bits(lse1, lse0)
    assert same_bits(gq[region], dq0) and same_bits(gk[region], dk0) and same_bits(gv[region], dv0)
    assert same_bits(gq2[region], dq2) and same_bits(gk2[region], dk2) and same_bits(gv2[region], dv2)
    for buf in (obuf, gq, gk, gv, gq2, gk2, gv2, dobuf):
        assert guards_intact(buf, region)
    assert guards_intact(qkv, (slice(None), slice(0, S)))
    assert bool(torch.isfinite(o0.float()).all())


# ---------------------------------------------------------------- h. refusals
def _abi():
    from picotron_amd import _C
    return _C.lib(), _C


def _s3(t):
    from picotron_amd import _C
    return _C.i64arr([t.stride(0), t.stride(1), t.stride(2)])


@pytest.mark.parametrize("name,Sq,Sk,D,causal,ld,code", [
    ("causal Sq != Sk", 128, 256, 64, 1, 0, -3),
    ("Sq off the 128-row blocks", 192, 192, 64, 0, 0, -3),
    ("head dim 96", 128, 128, 96, 1, 0, -3),
    ("lse_ld < Sq", 128, 128, 128, 1, 64, -1),
])
def test_forward_refusals_leave_outputs_untouched(name, Sq, Sk, D, causal, ld, code):
    lib, _C = _abi()
    B, H = 1, 2
    q = torch.zeros(B, Sq, H, D, dtype=BF, device=DEV)
    k = torch.zeros(B, Sk, H, D, dtype=BF, device=DEV)
    v = torch.zeros(B, Sk, H, D, dtype=BF, device=DEV)
    o, lse = sentinel((B, Sq, H, D), BF), sentinel((B, H, Sq), torch.float32)
    rc = lib.pt_attn_fwd(q.data_ptr(), _s3(q), k.data_ptr(), _s3(k), v.data_ptr(), _s3(v), o.data_ptr(), _s3(o),
                         lse.data_ptr(), B, H, H, Sq, Sk, D, R.scale_of(D), causal, 0, ld, _C.stream_ptr(q.device))
    torch.cuda.synchronize()
    assert rc == code, name
    none = (slice(0, 0),)
    assert guards_intact(o, none) and guards_intact(lse, none)


@pytest.mark.parametrize("name,Sq,Sk,D,causal,ld,parts,null_dq,code", [
    ("causal Sq != Sk", 128, 256, 64, 1, 0, 3, False, -3),
    ("Sq off the 128-row blocks", 192, 192, 64, 0, 0, 3, False, -3),
    ("head dim 96", 128, 128, 96, 1, 0, 3, False, -3),
    ("lse_ld < Sq", 128, 128, 128, 1, 64, 3, False, -1),
    ("parts = 1 with a NULL dq", 128, 128, 64, 1, 0, 1, True, -1),
])
def test_backward_refusals_leave_outputs_untouched(name, Sq, Sk, D, causal, ld, parts, null_dq, code):
    lib, _C = _abi()
    B, H = 1, 2
    q, do = (torch.zeros(B, Sq, H, D, dtype=BF, device=DEV) for _ in range(2))
    k, v = (torch.zeros(B, Sk, H, D, dtype=BF, device=DEV) for _ in range(2))
    lse, delta = (torch.zeros(B, H, Sq, device=DEV) for _ in range(2))
    dq, dk, dv = sentinel((B, Sq, H, D), BF), sentinel((B, Sk, H, D), BF), sentinel((B, Sk, H, D), BF)
    rc = lib.pt_attn_bwd_part(q.data_ptr(), _s3(q), k.data_ptr(), _s3(k), v.data_ptr(), _s3(v), do.data_ptr(), _s3(do),
                              lse.data_ptr(), delta.data_ptr(), None if null_dq else dq.data_ptr(), _s3(dq),
                              dk.data_ptr(), _s3(dk), dv.data_ptr(), _s3(dv), B, H, H, Sq, Sk, D, R.scale_of(D), causal,
                              0, ld, parts, _C.stream_ptr(q.device))
    torch.cuda.synchronize()
    assert rc == code, name
    none = (slice(0, 0),)
    assert guards_intact(dq, none) and guards_intact(dk, none) and guards_intact(dv, none)
    if parts == 3:   # the same refusal from pt_attn_bwd and pt_attn_bwd_delta's own checks
        rc = lib.pt_attn_bwd(q.data_ptr(), _s3(q), k.data_ptr(), _s3(k), v.data_ptr(), _s3(v), do.data_ptr(), _s3(do),
                             lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), _s3(dq), dk.data_ptr(), _s3(dk),
                             dv.data_ptr(), _s3(dv), B, H, H, Sq, Sk, D, R.scale_of(D), causal, 0, None, None, 0, ld,
                             _C.stream_ptr(q.device))
        torch.cuda.synchronize()
        assert rc == code, name
        assert guards_intact(dq, none) and guards_intact(dk, none) and guards_intact(dv, none)


def test_python_entry_points_raise_on_refused_shapes():
    K = K_()
    from picotron_amd._C import HipKernelError
    q, k, v, _ = dev(*R.make_case("randn", 1, 128, 256, 2, 2, 64))
    with pytest.raises(HipKernelError, match="PT_EUNSUPPORTED"):
        K.attn_fwd(q, k, v, 0.125, True)
    lse = torch.zeros(1, 2, 256, device=DEV)
    with pytest.raises(ValueError):     # a [B, H, Sq] lse whose rows overlap: refused before the launch
        K.attn_fwd(q, k[:, :128], v[:, :128], 0.125, True, lse=lse.as_strided((1, 2, 128), (128, 64, 1)))


# ---------------------------------------------------------------- i. pt_lse_merge extremes
@pytest.mark.parametrize("lse_dtype", [torch.float32, BF])
@pytest.mark.parametrize("diff", [-100.0, 0.0, 100.0])
def test_lse_merge_extremes(lse_dtype, diff):
    """block_lse - lse = -100 / 0 / +100 against the oracle's update_out_and_lse on the same values
    (all lse values exact in bf16, and non-zero: e^-100 is then far below half an ulp of them); at
    +-100 the result is the dominant input."""
    K = K_()
    rows, D = 8, 64
    g = torch.Generator().manual_seed(11)
    out = torch.randn(1, 1, rows, D, generator=g)
    blk = torch.randn(1, 1, rows, D, generator=g).to(BF)
    lse = torch.tensor([-4.0, 2.0, 4.0, 28.0, -20.0, 12.0, 1.0, -1.0]).view(1, 1, rows).to(lse_dtype)
    blse = (lse.float() + diff).to(lse_dtype)
    assert torch.equal(blse.float(), lse.float() + diff)
    o_ref, l_ref = O.update_out_and_lse(out, lse.unsqueeze(-1), blk, blse)
    o_new, l_new = K.lse_merge(*dev(out, blk, lse, blse))
    torch.cuda.synchronize()
    o_new, l_new = o_new.cpu(), l_new.cpu()
    assert l_new.dtype == lse_dtype and bool(torch.isfinite(o_new).all()) and bool(torch.isfinite(l_new.float()).all())
    l_ref = l_ref.squeeze(-1)
    big = torch.maximum(out.abs(), blk.float().abs())   # the result is a convex combination of the two
    if lse_dtype == BF:
        assert same_bits(l_new, l_ref) and same_bits(o_new, o_ref)
    else:
        assert bool(((l_new - l_ref).abs() <= 2.0 ** -20 * l_ref.abs().clamp_min(1.0)).all())
        assert bool(((o_new - o_ref).abs() <= 2.0 ** -20 * big).all())
    if diff == 100.0:   # out - 1 * (out - block): the block up to the f32 rounding of the two subtractions
        assert bool(((o_new - blk.float()).abs() <= 2.0 ** -20 * big).all()) and torch.equal(l_new.float(), blse.float())
    elif diff == -100.0:
        assert torch.equal(o_new, out) and torch.equal(l_new.float(), lse.float())
