"""Band attention (document-masked and sliding-window causal attention: pt_attn_fwd_band /
pt_attn_bwd_band, kernels.attn_fwd / attn_bwd with band=) against the float64 reference and the
per-element bounds of tests/_attn_ref.py, unchanged; the mask is passed as [B, 1, S, S].

Shapes (D, S, B, H, HKV) are the smallest that reach each launch form: d64 S256 (two 128-row blocks,
block pairing on), d64 S512 (the 4-stage K/V ring wraps), d128 S256 (the 8-wave forward), d128 S384
(the 4-wave forward, pairing off), d128 S512 (8-wave, paired).  B = 2 with a different layout in each
batch row; H 4 over HKV 2 (GQA).  attn_kv_chunk = 0 unless stated.

Layouts:
  a  document lengths [1, 95, 33, 127] tiled to S (row 1: rotated): boundaries inside a wave (1, 33),
     inside a 64-key tile (96, 160), one past a block edge (129)
  b  documents [0, 60) [60, 170) [170, S): rows 170 .. 191 share a wave with rows of the document
     before and see no key in that wave's first tiles (running max still -inf there)
  c  boundaries on multiples of 128: whole tiles skipped
  d  every token its own document: o == v bit for bit
  e  windows 64 and 100, alone and together with layout a
"""
import functools

import pytest
import torch

from oracle import picotron_oracle as O
from picotron_amd import switches
from tests import _attn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN16 = 0x7FC1
NAN32 = 0x7FC00001

# D, S, B, H, HKV
SHAPES = [(64, 256, 2, 4, 2), (64, 512, 2, 4, 2), (128, 256, 2, 4, 2), (128, 384, 2, 4, 2), (128, 512, 2, 4, 2)]
SHAPE_IDS = [f"d{s[0]}-S{s[1]}" for s in SHAPES]
HARD = ("peaked", "offset-", "ramp")


def K_():
    from picotron_amd import kernels
    return kernels


def dev(*ts):
    return [t.to(DEV) for t in ts]


def regular():
    return switches.override(attn_kv_chunk=0)


def ibits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == BF else torch.int32).cpu()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(ibits(a), ibits(b))


def sentinel(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.int16 if dtype == BF else torch.int32).fill_(NAN16 if dtype == BF else NAN32)
    return t


def guards_intact(buf, region):
    ib = buf.view(torch.int16 if buf.dtype == BF else torch.int32).clone()
    pat = NAN16 if buf.dtype == BF else NAN32
    ib[region] = pat
    return bool((ib == pat).all())


# ---------------------------------------------------------------- layouts
def ids_from_lengths(lengths, S, tile=True):
    """Document ids of consecutive documents of `lengths` (tiled to S, or the last one running to S)."""
    ids, d = [], 0
    while len(ids) < S:
        n = lengths[d % len(lengths)] if (tile or d < len(lengths)) else S
        ids += [d] * n
        d += 1
    return torch.tensor(ids[:S])


def layout(name, S):
    """(document_ids [2, S] or None, window or None)."""
    a = torch.stack([ids_from_lengths([1, 95, 33, 127], S), ids_from_lengths([33, 127, 1, 95], S)])
    if name == "a":
        return a, None
    if name == "b":
        return torch.stack([ids_from_lengths([60, 110], S, tile=False), ids_from_lengths([100, 135], S, tile=False)]), None
    if name == "c":
        return torch.stack([ids_from_lengths([128], S), ids_from_lengths([128, S], S, tile=False)]), None
    if name == "d":
        return torch.arange(S).expand(2, S).contiguous(), None
    if name.startswith("w"):
        return (a if name.endswith("+a") else None), int(name[1:].split("+")[0])
    raise KeyError(name)


def brute_mask(ids, window, B, S):
    """[B, 1, S, S] bool from the definition (not from the band's arrays)."""
    i = torch.arange(S)
    m = (i[None, :] <= i[:, None])[None].expand(B, S, S).clone()
    if ids is not None:
        first = torch.ones(B, S, dtype=torch.bool)
        first[:, 1:] = ids[:, 1:] != ids[:, :-1]
        doc = torch.cumsum(first.long(), 1)                      # a running document number
        m &= doc[:, :, None] == doc[:, None, :]
    if window is not None:
        m &= (i[:, None] - i[None, :] < window)[None]
    return m[:, None]


@functools.lru_cache(maxsize=None)
def case(family, D, S, B, H, HKV):
    return R.make_case(family, B, S, S, H, HKV, D)


def run_band(K, q, k, v, do, scale, band, **kw):
    o, lse = K.attn_fwd(q, k, v, scale, True, band=band)
    dq, dk, dv, delta = K.attn_bwd(do, q, k, v, o, lse, scale, True, band=band, **kw)
    torch.cuda.synchronize()
    return o, lse, dq, dk, dv, delta


def band_against_reference(family, shape, name, ids=None, window=None, explicit=False):
    K = K_()
    D, S, B, H, HKV = shape
    if not explicit:
        ids, window = layout(name, S)
    q, k, v, do = case(family, D, S, B, H, HKV)
    scale = R.scale_of(D)
    qd, kd, vd, dod = dev(q, k, v, do)
    band = K.attn_band(B, S, DEV, document_ids=ids, window=window)
    mask = brute_mask(ids, window, B, S)
    assert torch.equal(band.mask().cpu(), mask)
    tag = f"{family}/{name}"
    o, lse, dq, dk, dv, delta = run_band(K, qd, kd, vd, dod, scale, band)
    ref = R.ref_forward(q, k, v, scale, mask)
    R.check_out(o, ref, tag)
    R.check_lse(lse, ref.lse, tag)
    if family == "zeroq":   # exactly uniform over the visible keys
        n = (torch.arange(S)[None] - band.kv_lo.cpu() + 1).to(torch.float64)
        R.check_lse(lse, torch.log(n)[:, None, :].expand(B, H, S), tag, name="lse_closed_form")
    bwd = R.ref_backward(q, k, v, do, lse.cpu(), scale, mask, o=o.cpu())
    R.check_delta(delta, bwd, tag)
    R.check_grads(dq, dk, dv, bwd, tag)
    return (q, k, v, do), (o, lse, dq, dk, dv, delta), bwd


# ---------------------------------------------------------------- a. the layouts against the reference
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_documents_all_families(family, shape):
    with regular():
        band_against_reference(family, shape, "a")


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("family", HARD)
@pytest.mark.parametrize("name", ["b", "c", "w64", "w100", "w64+a", "w100+a"])
def test_layouts(name, family, shape):
    with regular():
        band_against_reference(family, shape, name)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("family", HARD)
def test_every_token_its_own_document(family, shape):
    """o == v[:, :, h // rep] bit for bit, lse the scaled self-score, dv the folded dO up to the checker."""
    D, S, B, H, HKV = shape
    with regular():
        (q, k, v, do), (o, lse, dq, dk, dv, delta), bwd = band_against_reference(family, shape, "d")
    rep = H // HKV
    assert torch.equal(ibits(o), ibits(v.repeat_interleave(rep, dim=2)))
    self_score = (q.double() * k.double().repeat_interleave(rep, dim=2)).sum(-1).permute(0, 2, 1) * R.scale_of(D)
    R.check_lse(lse, self_score, family, name="lse_self_score")
    folded = do.double().view(B, S, HKV, rep, D).sum(3)
    R.check("dv_folded", dv, folded, R._grad_bounds(bwd, False)["dv"], family)


# ---------------------------------------------------------------- b. bit identity
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("family", HARD)
@pytest.mark.parametrize("how", ["one-document", "wide-window"])
def test_trivial_band_is_bit_identical_to_causal(how, family, shape):
    K = K_()
    D, S, B, H, HKV = shape
    q, k, v, do = dev(*case(family, D, S, B, H, HKV))
    scale = R.scale_of(D)
    if how == "one-document":
        band = K.attn_band(B, S, DEV, document_ids=torch.zeros(B, S, dtype=torch.long))
    else:
        band = K.attn_band(B, S, DEV, window=S + 5)
    with regular():
        got = run_band(K, q, k, v, do, scale, band)
        o, lse = K.attn_fwd(q, k, v, scale, True)
        want = (o, lse) + tuple(K.attn_bwd(do, q, k, v, o, lse, scale, True))
        torch.cuda.synchronize()
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv", "delta"), got, want):
        assert same_bits(a, b), name


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("family", HARD)
@pytest.mark.parametrize("switch,values", [("attn_pair", (0, 1)), ("attn_split", (0, 3))])
def test_variants_are_bit_identical_under_a_band(switch, values, family, shape):
    K = K_()
    D, S, B, H, HKV = shape
    q, k, v, do = dev(*case(family, D, S, B, H, HKV))
    ids, _ = layout("a", S)
    band = K.attn_band(B, S, DEV, document_ids=ids, window=100)
    res = []
    for val in values:
        with switches.override(attn_kv_chunk=0, **{switch: val}):
            res.append(run_band(K, q, k, v, do, R.scale_of(D), band))
    for a, b in zip(*res):
        assert same_bits(a, b)


@pytest.mark.parametrize("D", [64, 128])
def test_fused_rope_inverse_under_a_band(D):
    K = K_()
    B, S, H, HKV = 2, 256, 4, 2
    qkv = torch.randn(B * S, (H + 2 * HKV) * D, generator=torch.Generator().manual_seed(D)).to(BF).to(DEV)
    sh = lambda t, lo, n: t.view(B, S, -1)[:, :, lo * D:(lo + n) * D].view(B, S, n, D)
    q, k, v = sh(qkv, 0, H), sh(qkv, H, HKV), sh(qkv, H + HKV, HKV)
    do = torch.randn(B, S, H, D, generator=torch.Generator().manual_seed(D + 1)).to(BF).to(DEV)
    cos, sin = [t.to(DEV) for t in O.get_cos_sin(S, D, base=10000.0)]
    ids, _ = layout("a", S)
    band = K.attn_band(B, S, DEV, document_ids=ids, window=100)
    scale = R.scale_of(D)
    with regular():
        o, lse = K.attn_fwd(q, k, v, scale, True, band=band)
        d1, d2 = torch.empty_like(qkv), torch.empty_like(qkv)
        K.attn_bwd(do, q, k, v, o, lse, scale, True, dq=sh(d1, 0, H), dk=sh(d1, H, HKV), dv=sh(d1, H + HKV, HKV),
                   rope=(cos, sin), band=band)
        K.attn_bwd(do, q, k, v, o, lse, scale, True, dq=sh(d2, 0, H), dk=sh(d2, H, HKV), dv=sh(d2, H + HKV, HKV),
                   band=band)
        K.rope_(d2, H + HKV, D, cos, sin, S, inverse=True)
    torch.cuda.synchronize()
    assert torch.equal(d1, d2)


# ---------------------------------------------------------------- c. padded and few-head shapes
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("family", HARD)
def test_sequence_off_the_blocks(family, D):
    """S = 200 (padded to 256; every pad row its own document) with documents [70, 130]."""
    ids = torch.stack([ids_from_lengths([70, 130], 200), ids_from_lengths([130, 70], 200)])
    with regular():
        band_against_reference(family, (D, 200, 2, 4, 2), "S200", ids=ids, window=None, explicit=True)


@pytest.mark.parametrize("family", HARD)
def test_few_head_shape_keeps_the_regular_kernels(family):
    """B4 S512 H4 d64 at the default attn_kv_chunk: the causal call takes the split forms, the band call
    does not, and passes the checker."""
    K = K_()
    B, S, H, HKV, D = 4, 512, 4, 2, 64
    assert K._attn_split_ws(B, H, HKV, S, S, D, True, 0, torch.device(DEV, 0)) is not None
    a, _ = layout("a", S)
    ids = torch.cat([a, a.flip(0)])
    band_against_reference(family, (D, S, B, H, HKV), "few-head", ids=ids, window=100, explicit=True)


# ---------------------------------------------------------------- d. guarded outputs
@pytest.mark.parametrize("D", [64, 128])
def test_strided_outputs_leave_their_neighbours_alone(D):
    K = K_()
    B, S, H, HKV = 2, 256, 4, 2
    q, k, v, do = dev(*case("peaked", D, S, B, H, HKV))
    scale = R.scale_of(D)
    ids, _ = layout("a", S)
    band = K.attn_band(B, S, DEV, document_ids=ids, window=100)
    region = (Ellipsis, slice(0, D))
    with regular():
        o0, lse0, dq0, dk0, dv0, delta0 = run_band(K, q, k, v, do, scale, band)
        obuf = sentinel((B, S, H, D + 8), BF)
        gq, gk, gv = sentinel((B, S, H, D + 8), BF), sentinel((B, S, HKV, D + 8), BF), sentinel((B, S, HKV, D + 8), BF)
        lse1 = sentinel((B, H, S), torch.float32)
        o1, _ = K.attn_fwd(q, k, v, scale, True, out=obuf[region], lse=lse1, band=band)
        K.attn_bwd(do, q, k, v, o1, lse1, scale, True, dq=gq[region], dk=gk[region], dv=gv[region], band=band)
    torch.cuda.synchronize()
    assert same_bits(obuf[region], o0) and same_bits(lse1, lse0)
    assert same_bits(gq[region], dq0) and same_bits(gk[region], dk0) and same_bits(gv[region], dv0)
    for buf in (obuf, gq, gk, gv):
        assert guards_intact(buf, region)
    assert bool(torch.isfinite(o0.float()).all())


# ---------------------------------------------------------------- e. refusals
def _s3(t):
    from picotron_amd import _C
    return _C.i64arr([t.stride(0), t.stride(1), t.stride(2)])


@pytest.mark.parametrize("name,Sq,Sk,D,null,code", [
    ("Sq != Sk", 128, 256, 64, None, -3),
    ("head dim 96", 128, 128, 96, None, -3),
    ("S off the 128-row blocks", 192, 192, 64, None, -3),
    ("NULL kv_lo", 128, 128, 64, "kv_lo", -1),
    ("NULL q_hi", 128, 128, 128, "q_hi", -1),
])
def test_abi_refusals_leave_outputs_untouched(name, Sq, Sk, D, null, code):
    from picotron_amd import _C
    lib = _C.lib()
    B, H = 1, 2
    q, do = (torch.zeros(B, Sq, H, D, dtype=BF, device=DEV) for _ in range(2))
    k, v = (torch.zeros(B, Sk, H, D, dtype=BF, device=DEV) for _ in range(2))
    lo = torch.zeros(B, Sq, dtype=torch.int32, device=DEV)
    hi = torch.full((B, Sk), Sq, dtype=torch.int32, device=DEV)
    plo = None if null == "kv_lo" else lo.data_ptr()
    phi = None if null == "q_hi" else hi.data_ptr()
    o, lse = sentinel((B, Sq, H, D), BF), sentinel((B, H, Sq), torch.float32)
    stream = _C.stream_ptr(q.device)
    rc = lib.pt_attn_fwd_band(q.data_ptr(), _s3(q), k.data_ptr(), _s3(k), v.data_ptr(), _s3(v), o.data_ptr(), _s3(o),
                              lse.data_ptr(), B, H, H, Sq, Sk, D, R.scale_of(D), plo, phi, stream)
    torch.cuda.synchronize()
    assert rc == code, name
    none = (slice(0, 0),)
    assert guards_intact(o, none) and guards_intact(lse, none)
    oin, lin = torch.zeros(B, Sq, H, D, dtype=BF, device=DEV), torch.zeros(B, H, Sq, device=DEV)
    dq, dk, dv = sentinel((B, Sq, H, D), BF), sentinel((B, Sk, H, D), BF), sentinel((B, Sk, H, D), BF)
    delta = sentinel((B, H, Sq), torch.float32)
    rc = lib.pt_attn_bwd_band(q.data_ptr(), _s3(q), k.data_ptr(), _s3(k), v.data_ptr(), _s3(v), oin.data_ptr(),
                              _s3(oin), do.data_ptr(), _s3(do), lin.data_ptr(), delta.data_ptr(), dq.data_ptr(),
                              _s3(dq), dk.data_ptr(), _s3(dk), dv.data_ptr(), _s3(dv), B, H, H, Sq, Sk, D,
                              R.scale_of(D), None, None, 0, plo, phi, stream)
    torch.cuda.synchronize()
    assert rc == code, name
    for t in (dq, dk, dv, delta):
        assert guards_intact(t, none)


def test_python_entry_points_raise():
    K = K_()
    B, S, H, HKV, D = 1, 128, 2, 2, 64
    q, k, v, do = dev(*R.make_case("randn", B, S, S, H, HKV, D))
    band = K.attn_band(B, S, DEV, window=64)
    o, lse = K.attn_fwd(q, k, v, 0.125, True, band=band)
    strided = torch.zeros(B, H, 2 * S, device=DEV)[:, :, :S]
    with pytest.raises(ValueError, match="causal"):
        K.attn_fwd(q, k, v, 0.125, False, band=band)
    with pytest.raises(ValueError, match="merge"):
        K.attn_fwd(q, k, v, 0.125, True, out=torch.zeros(B, S, H, D, device=DEV),
                   lse=torch.zeros(B, H, S, device=DEV), merge=True, band=band)
    with pytest.raises(ValueError, match="dense lse"):
        K.attn_fwd(q, k, v, 0.125, True, lse=strided, band=band)
    with pytest.raises(ValueError, match="causal"):
        K.attn_bwd(do, q, k, v, o, lse, 0.125, False, band=band)
    with pytest.raises(ValueError, match="grad_f32"):
        K.attn_bwd(do, q, k, v, o, lse, 0.125, True, grad_f32=True, band=band)
    with pytest.raises(ValueError, match="dense lse"):
        K.attn_bwd(do, q, k, v, o, strided, 0.125, True, band=band)
    with pytest.raises(ValueError, match="AttnBand"):
        K.attn_fwd(q, k, v, 0.125, True, band=(band.kv_lo, band.q_hi))
    with pytest.raises(ValueError):      # a band of another shape
        K.attn_fwd(q, k, v, 0.125, True, band=K.attn_band(B, 2 * S, DEV))
    with pytest.raises(ValueError):      # a band on another device
        K.attn_fwd(q, k, v, 0.125, True, band=K.attn_band(B, S, "cpu"))
    torch.cuda.synchronize()
