"""Block bands (pt_attn_fwd_block_band / pt_attn_bwd_block_band; kernels.attn_fwd / attn_bwd /
attn_bwd_part with an AttnBlockBand): one rectangular, usually non-causal block of a context-parallel
schedule under a per-row lower bound, against the float64 reference and the per-element bounds of
tests/_attn_ref.py, unchanged (the mask is passed as [B, 1, Sq, Sk]).

Shapes: D in {64, 128}, B 2, H 4, HKV 2, Sq in {128, 256, 384}, Sk in {128, 256}; causal where
Sq == Sk.  Bound layouts (kv_lo of one batch row; the two rows of a case hold different ones):
  trivial  kv_lo = 0
  empty    kv_lo = Sk: no row sees a key
  stair    kv_lo[i] = min(i, Sk)
  mid      kv_lo = 70 (mid-tile) for rows < 37, Sk from row 37 (mid-wave) on
  blk2     the first 128-row query block full, every later one wholly empty
  last     kv_lo = Sk - 1
A kv_lo is turned into an AttnBlockBand through attn_block_band() itself: the block's keys at global
positions [0, Sk), its queries behind them (the diagonal block: the same positions), lo = kv_lo."""
import functools

import pytest
import torch

from picotron_amd import switches
from tests import _attn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN32 = 0x7FC00001
B, H, HKV = 2, 4, 2
# (Sq, Sk): square ones run causal and non-causal
BLOCKS = [(128, 128), (256, 256), (384, 256), (256, 128), (128, 256), (384, 128)]
BLOCK_IDS = [f"{a}x{b}" for a, b in BLOCKS]
LAYOUTS = ("trivial", "empty", "stair", "mid", "blk2", "last")


def K_():
    from picotron_amd import kernels
    return kernels


def regular():
    return switches.override(attn_kv_chunk=0)


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == BF else torch.int32).cpu()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def sentinel(shape):
    t = torch.empty(shape, dtype=torch.float32, device=DEV)
    t.view(torch.int32).fill_(NAN32)
    return t


def kv_lo_row(name, Sq, Sk):
    i = torch.arange(Sq)
    if name == "trivial":
        return torch.zeros(Sq, dtype=torch.int64)
    if name == "empty":
        return torch.full((Sq,), Sk, dtype=torch.int64)
    if name == "stair":
        return i.clamp(max=Sk)
    if name == "mid":
        return torch.where(i < 37, torch.tensor(70), torch.tensor(Sk))
    if name == "blk2":
        return torch.where(i < 128, torch.tensor(0), torch.tensor(Sk))
    if name == "last":
        return torch.full((Sq,), Sk - 1, dtype=torch.int64)
    raise KeyError(name)


def make_band(names, Sq, Sk, causal):
    """(AttnBlockBand on the device, kv_lo [B, Sq] on the CPU); names: one layout per batch row."""
    K = K_()
    kv_lo = torch.stack([kv_lo_row(n, Sq, Sk) for n in names])
    if causal:
        lo, qpos = kv_lo, torch.arange(Sk)
    else:
        lo, qpos = torch.cat([torch.zeros(len(names), Sk, dtype=torch.int64), kv_lo], 1), Sk + torch.arange(Sq)
    band = K.attn_block_band(lo.to(DEV), qpos, torch.arange(Sk), causal)
    assert torch.equal(band.kv_lo.cpu().long(), kv_lo)
    q_hi = (kv_lo[:, :, None] <= torch.arange(Sk)[None, None, :]).sum(1)
    assert torch.equal(band.q_hi.cpu().long(), q_hi)
    return band, kv_lo


def vis_mask(kv_lo, Sk, causal):
    """[B, 1, Sq, Sk] bool from the definition."""
    j = torch.arange(Sk)
    m = j[None, None, :] >= kv_lo[:, :, None]
    if causal:
        m = m & (j[None, None, :] <= torch.arange(kv_lo.shape[1])[None, :, None])
    return m[:, None]


def pairs(names=LAYOUTS):
    """Cases of two batch rows with different layouts: each layout with its successor."""
    return [(n, names[(i + 1) % len(names)]) for i, n in enumerate(names)]


@functools.lru_cache(maxsize=None)
def case(family, D, Sq, Sk):
    return R.make_case(family, B, Sq, Sk, H, HKV, D)


def dev(*ts):
    return [t.to(DEV) for t in ts]


def strided(shape_bhs, fill=None):
    """An f32 [B, H, Sq] view whose (b, h) rows lie Sq + 128 apart."""
    b, h, s = shape_bhs
    big = torch.zeros(b, h, s + 128, device=DEV) if fill is None else torch.full((b, h, s + 128), fill, device=DEV)
    return big[:, :, 64:64 + s]


def causal_options(Sq, Sk):
    return (False, True) if Sq == Sk else (False,)


# ---------------------------------------------------------------- a. trivial bounds: the band-less bits
@pytest.mark.parametrize("Sq,Sk", BLOCKS, ids=BLOCK_IDS)
@pytest.mark.parametrize("D", [64, 128])
def test_trivial_bounds_give_the_bandless_bits(D, Sq, Sk):
    K = K_()
    q, k, v, do = dev(*case("randn", D, Sq, Sk))
    scale = R.scale_of(D)
    g = torch.Generator().manual_seed(5)
    acc0 = torch.randn(B, Sq, H, D, generator=g).to(DEV)
    lse0 = torch.randn(B, H, Sq, generator=g).to(DEV)
    init = {n: torch.randn(B, s, h, D, generator=g).to(DEV) for n, s, h in (("dq", Sq, H), ("dk", Sk, HKV), ("dv", Sk, HKV))}
    with regular():
        for causal in causal_options(Sq, Sk):
            band, _ = make_band(("trivial", "trivial"), Sq, Sk, causal)
            for ld_strided in (False, True):
                def lse_buf(src=None):
                    t = strided((B, H, Sq)) if ld_strided else torch.zeros(B, H, Sq, device=DEV)
                    if src is not None:
                        t.copy_(src)
                    return t
                # forward, merge = 0 and 1
                got = K.attn_fwd(q, k, v, scale, causal, lse=lse_buf(), band=band)
                want = K.attn_fwd(q, k, v, scale, causal, lse=lse_buf())
                assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), ("fwd", causal, ld_strided)
                lse, o = want[1], want[0]
                ga, gl = acc0.clone(), lse_buf(lse0)
                wa, wl = acc0.clone(), lse_buf(lse0)
                K.attn_fwd(q, k, v, scale, causal, out=ga, lse=gl, merge=True, band=band)
                K.attn_fwd(q, k, v, scale, causal, out=wa, lse=wl, merge=True)
                assert same_bits(ga, wa) and same_bits(gl, wl), ("merge", causal, ld_strided)
                # backward: parts 1, 2, 3, bf16 stores and f32 accumulation onto a non-zero value
                delta = K.attn_delta(do, o, lse_buf())
                for f32 in (False, True):
                    def grads():
                        return {n: (t.clone() if f32 else torch.zeros_like(t, dtype=BF)) for n, t in init.items()}
                    for parts in (1, 2, 3):
                        a, b = grads(), grads()
                        if parts == 3:
                            K.attn_bwd(do, q, k, v, o, lse, scale, causal, grad_f32=f32, delta=delta, band=band, **a)
                            K.attn_bwd(do, q, k, v, o, lse, scale, causal, grad_f32=f32, delta=delta, **b)
                        else:
                            sel = ("dq",) if parts == 1 else ("dk", "dv")
                            K.attn_bwd_part(do, q, k, v, lse, delta, scale, causal, grad_f32=f32, band=band,
                                            **{n: a[n] for n in sel})
                            K.attn_bwd_part(do, q, k, v, lse, delta, scale, causal, grad_f32=f32,
                                            **{n: b[n] for n in sel})
                        for n in a:
                            assert same_bits(a[n], b[n]), ("bwd", n, causal, ld_strided, f32, parts)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- b. a three-block merge
@pytest.mark.parametrize("family", ["peaked", "offset+", "offset-"])
@pytest.mark.parametrize("D", [64, 128])
def test_three_block_merge_against_reference(D, family):
    K = K_()
    S = 256
    q, blocks, _ = R.make_merge_case(family, B, S, H, HKV, D)
    scale = R.scale_of(D)
    # the diagonal under a document layout (documents from 0 and 70 | from 0, 129 and 200), then two
    # non-causal blocks with empty rows
    i = torch.arange(S)
    diag = torch.stack([torch.where(i < 70, 0, 70), torch.where(i < 129, 0, torch.where(i < 200, 129, 200))])
    band0 = K.attn_block_band(diag.to(DEV), i, i, True)
    bands = [(band0, diag, True)] + [make_band(names, S, S, False) + (False,) for names in (("mid", "stair"), ("blk2", "last"))]
    acc = torch.zeros(B, S, H, D, device=DEV)
    lse = torch.full((B, H, S), float("-inf"), device=DEV)
    qd = q.to(DEV)
    for (kb, vb), (band, _, causal) in zip(blocks, bands):
        K.attn_fwd(qd, kb.to(DEV), vb.to(DEV), scale, causal, out=acc, lse=lse, merge=True, band=band)
    torch.cuda.synchronize()
    mask = torch.cat([vis_mask(kv_lo, S, causal) for _, kv_lo, causal in bands], dim=3)
    ref = R.ref_forward(q, torch.cat([b[0] for b in blocks], 1), torch.cat([b[1] for b in blocks], 1), scale, mask)
    tag = f"merge3/{family}/d{D}"
    R.check_acc(acc, ref, tag)
    R.check_lse(lse, ref.lse, tag)


# ---------------------------------------------------------------- c. rows without a visible key
@pytest.mark.parametrize("Sq,Sk", BLOCKS, ids=BLOCK_IDS)
@pytest.mark.parametrize("D", [64, 128])
def test_empty_rows_forward(D, Sq, Sk):
    K = K_()
    q, k, v, _ = case("randn", D, Sq, Sk)
    qd, kd, vd = dev(q, k, v)
    scale = R.scale_of(D)
    for causal in causal_options(Sq, Sk):
        for names in pairs():
            band, kv_lo = make_band(names, Sq, Sk, causal)
            mask = vis_mask(kv_lo, Sk, causal)
            empty = ~mask[:, 0].any(-1)                                    # [B, Sq]
            tag = f"empty/{names[0]}+{names[1]}/{'c' if causal else 'n'}/d{D}-{Sq}x{Sk}"
            # merge = 1 onto sentinels, with a finite running LSE and with -inf
            for lse_init in (0.25, float("-inf")):
                acc = sentinel((B, Sq, H, D))
                lse = torch.full((B, H, Sq), lse_init, device=DEV)
                K.attn_fwd(qd, kd, vd, scale, causal, out=acc, lse=lse, merge=True, band=band)
                torch.cuda.synchronize()
                ab, lb = bits(acc), bits(lse)
                assert bool((ab[empty] == NAN32).all()), tag
                assert torch.equal(lb.transpose(1, 2)[empty], bits(torch.full_like(lse, lse_init)).transpose(1, 2)[empty]), tag
                # the other rows took the block in: NaN * 0 stays NaN in acc, the LSE is the merged one
                assert bool(torch.isfinite(lse.cpu().transpose(1, 2)[~empty]).all()), tag
            # merge = 0: o = 0 and lse = -inf there, the reference elsewhere
            o, lse = K.attn_fwd(qd, kd, vd, scale, causal, band=band)
            torch.cuda.synchronize()
            o, lse = o.cpu(), lse.cpu()
            assert bool((o[empty] == 0).all()) and bool((lse.transpose(1, 2)[empty] == float("-inf")).all()), tag
            ref = R.ref_forward(q, k, v, scale, mask | empty[:, None, :, None])   # (empty rows: any finite stand-in)
            o, lse = o.clone(), lse.clone()
            o[empty] = ref.o[empty].to(BF)
            lse.transpose(1, 2)[empty] = ref.lse.transpose(1, 2)[empty].float()
            R.check_out(o, ref, tag)
            R.check_lse(lse, ref.lse, tag)


# ---------------------------------------------------------------- d. backward
def backward_case(family, D, Sq, Sk, causal, names):
    """The block's operands, and the global lse / delta of its queries: 128 fully visible keys ahead of
    the block keep every row's LSE finite."""
    q, kall, vall, do = R.make_case(family, B, Sq, Sk + 128, H, HKV, D)
    band, kv_lo = make_band(names, Sq, Sk, causal)
    mask = vis_mask(kv_lo, Sk, causal)
    scale = R.scale_of(D)
    full = torch.cat([torch.ones(B, 1, Sq, 128, dtype=torch.bool), mask], dim=3)
    fwd = R.ref_forward(q, kall, vall, scale, full)
    o = fwd.o.to(BF)
    lse = fwd.lse.float()
    delta = (do.float() * o.float()).sum(-1).permute(0, 2, 1).contiguous()
    k, v = kall[:, 128:].contiguous(), vall[:, 128:].contiguous()
    ref = R.ref_backward(q, k, v, do, lse, scale, mask, delta=delta)
    return (q, k, v, do, o, lse, delta), band, mask, ref


# (no "peaked" family here: against the global LSE, which the 128 keys ahead of the block dominate, a
# peaked row's weights on the block's keys fall below f32's normal range (gradients ~ 1e-39), where the
# kit's relative bounds do not hold; "offset-" keeps the very negative scores and LSE)
@pytest.mark.parametrize("family", ["randn", "offset-"])
@pytest.mark.parametrize("Sq,Sk", BLOCKS, ids=BLOCK_IDS)
@pytest.mark.parametrize("D", [64, 128])
def test_backward_parts_against_reference(D, Sq, Sk, family):
    K = K_()
    scale = R.scale_of(D)
    g = torch.Generator().manual_seed(9)
    init = {n: torch.randn(B, s, h, D, generator=g) + 3.0 for n, s, h in (("dq", Sq, H), ("dk", Sk, HKV), ("dv", Sk, HKV))}
    cases = [(c, names) for c in causal_options(Sq, Sk) for names in (("mid", "stair"), ("blk2", "last"), ("empty", "trivial"))]
    for n_case, (causal, names) in enumerate(cases):
        (q, k, v, do, o, lse, delta), band, mask, ref = backward_case(family, D, Sq, Sk, causal, names)
        qd, kd, vd, dod, od = dev(q, k, v, do, o)
        ld_strided = n_case % 2 == 1
        lsed, deld = (strided((B, H, Sq)) if ld_strided else torch.zeros(B, H, Sq, device=DEV) for _ in range(2))
        lsed.copy_(lse)
        deld.copy_(delta)
        empty_q = ~mask[:, 0].any(-1)          # [B, Sq]
        unseen_k = ~mask[:, 0].any(-2)         # [B, Sk]
        tag = f"bwd/{family}/{names[0]}+{names[1]}/{'c' if causal else 'n'}/d{D}-{Sq}x{Sk}"
        for f32 in (False, True):
            for parts in ((1, 2), (3,)):
                gr = {n: (t.to(DEV) if f32 else torch.full(t.shape, 7.0, dtype=BF, device=DEV)) for n, t in init.items()}
                for p in parts:
                    if p == 3:
                        K.attn_bwd(dod, qd, kd, vd, od, lsed, scale, causal, grad_f32=f32, delta=deld, band=band, **gr)
                    else:
                        sel = ("dq",) if p == 1 else ("dk", "dv")
                        K.attn_bwd_part(dod, qd, kd, vd, lsed, deld, scale, causal, grad_f32=f32, band=band,
                                        **{n: gr[n] for n in sel})
                torch.cuda.synchronize()
                t2 = f"{tag}/{'f32' if f32 else 'bf16'}/p{parts[0]}"
                if f32:
                    R.check_grads_f32(gr["dq"], gr["dk"], gr["dv"], ref, init, t2)
                else:
                    R.check_grads(gr["dq"], gr["dk"], gr["dv"], ref, t2)
                # empty query rows and unseen keys: exactly the initial value (bf16 stores: exactly 0)
                for n, rows in (("dq", empty_q), ("dk", unseen_k), ("dv", unseen_k)):
                    got = gr[n].cpu()[rows]
                    want = init[n][rows] if f32 else torch.zeros_like(got)
                    assert torch.equal(got, want), (t2, n)


# ---------------------------------------------------------------- e. kernel forms
@pytest.mark.parametrize("D", [64, 128])
def test_split_and_pair_forms_give_identical_bits(D):
    K = K_()
    S = 256
    scale = R.scale_of(D)
    for causal, names in ((True, ("stair", "mid")), (False, ("mid", "blk2")), (False, ("last", "empty"))):
        (q, k, v, do, o, lse, delta), band, _, _ = backward_case("randn", D, S, S, causal, names)
        qd, kd, vd, dod, od, lsed, deld = dev(q, k, v, do, o, lse, delta)
        results = []
        for split in (0, 3):
            for pair in (0, 1):
                with switches.override(attn_split=split, attn_pair=pair, attn_kv_chunk=0):
                    fo, fl = K.attn_fwd(qd, kd, vd, scale, causal, band=band)
                    dq, dk, dv, _ = K.attn_bwd(dod, qd, kd, vd, od, lsed, scale, causal, delta=deld, band=band)
                    torch.cuda.synchronize()
                results.append((fo, fl, dq, dk, dv))
        for r in results[1:]:
            for a, b in zip(results[0], r):
                assert same_bits(a, b), (causal, names)


# ---------------------------------------------------------------- f. refusals
def _s3(t):
    from picotron_amd import _C
    return _C.i64arr([t.stride(0), t.stride(1), t.stride(2)])


@pytest.mark.parametrize("name,Sq,Sk,causal,null,code", [
    ("causal with Sq != Sk", 128, 256, 1, None, -3),
    ("NULL kv_lo", 128, 128, 0, "kv_lo", -1),
    ("NULL q_hi", 256, 128, 0, "q_hi", -1),
])
def test_abi_refusals_leave_outputs_untouched(name, Sq, Sk, causal, null, code):
    from picotron_amd import _C
    lib = _C.lib()
    D, Bq, Hq = 64, 1, 2
    q, do = (torch.zeros(Bq, Sq, Hq, D, dtype=BF, device=DEV) for _ in range(2))
    k, v = (torch.zeros(Bq, Sk, Hq, D, dtype=BF, device=DEV) for _ in range(2))
    lo = torch.zeros(Bq, Sq, dtype=torch.int32, device=DEV)
    hi = torch.full((Bq, Sk), Sq, dtype=torch.int32, device=DEV)
    plo = None if null == "kv_lo" else lo.data_ptr()
    phi = None if null == "q_hi" else hi.data_ptr()
    stream = _C.stream_ptr(q.device)
    intact = lambda t: bool((bits(t) == NAN32).all())
    for merge in (0, 1):
        o, lse = sentinel((Bq, Sq, Hq, D)), sentinel((Bq, Hq, Sq))   # (f32 sentinels cover the bf16 view too)
        rc = lib.pt_attn_fwd_block_band(q.data_ptr(), _s3(q), k.data_ptr(), _s3(k), v.data_ptr(), _s3(v), o.data_ptr(),
                                        _s3(o), lse.data_ptr(), Bq, Hq, Hq, Sq, Sk, D, R.scale_of(D), causal, merge, 0,
                                        plo, phi, stream)
        torch.cuda.synchronize()
        assert rc == code, name
        assert intact(o) and intact(lse), name
    lin, din = torch.zeros(Bq, Hq, Sq, device=DEV), torch.zeros(Bq, Hq, Sq, device=DEV)
    for parts in (1, 2, 3):
        dq, dk, dv = sentinel((Bq, Sq, Hq, D)), sentinel((Bq, Sk, Hq, D)), sentinel((Bq, Sk, Hq, D))
        rc = lib.pt_attn_bwd_block_band(q.data_ptr(), _s3(q), k.data_ptr(), _s3(k), v.data_ptr(), _s3(v), do.data_ptr(),
                                        _s3(do), lin.data_ptr(), din.data_ptr(), dq.data_ptr(), _s3(dq), dk.data_ptr(),
                                        _s3(dk), dv.data_ptr(), _s3(dv), Bq, Hq, Hq, Sq, Sk, D, R.scale_of(D), causal,
                                        1, 0, parts, plo, phi, stream)
        torch.cuda.synchronize()
        assert rc == code, name
        assert intact(dq) and intact(dk) and intact(dv), name


def test_python_entry_points_refuse_mismatched_bands():
    K = K_()
    q, k, v, _ = dev(*case("randn", 64, 128, 256))
    band, _ = make_band(("trivial", "stair"), 128, 256, False)
    with pytest.raises(ValueError):       # built non-causal, called causal
        K.attn_fwd(q, q, q, 0.125, True, band=band)
    with pytest.raises(ValueError):       # a 128 x 256 band on a 128 x 128 block
        K.attn_fwd(q, k[:, :128], v[:, :128], 0.125, False, band=band)
    with pytest.raises(TypeError):
        K.AttnBlockBand(None, band.kv_lo, band.q_hi, False)
