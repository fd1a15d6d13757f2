"""Stochastic-rounding conformance kit for the AdamW step in bf16 state (csrc/adamw.hip: adamw_sr_*,
sr_cast_kernel).  CPU only: a numpy Philox4x32-10, the bits of an element, sr_bf16, the expected
bits of a step, a checker, and an emulator with injectable faults for the checker's self-test.

The bits (include/picotron_hip.h): key = the 64-bit seed's two halves; counter = (c & 0xffffffff,
c >> 32, step, (stream << 2) | which), c = i >> 3 the chunk of element i inside its tensor; element i
takes r = (w[(i & 7) >> 1] >> (16 * (i & 1))) & 0xffff of the call's four words w.

sr_bf16(x, r): inf and NaN take the plain cast; otherwise the 16-bit value (u + r) >> 16 of x's bits u.
So a bf16 value never changes, the magnitude goes up for exactly low16(u) of the 65536 values of r, -0
stays -0, and a value in the last bf16 ulp below the largest finite one may become inf.  A NaN compares
equal to any NaN (the payload of a cast NaN is the converter's business), everything else by bits.

The step (expect_step): w, m32, v32 = float(p), float(m), float(v); g32 = float(g), with clipping the
one f32 product clip_grad(g32, coef, False); tests._optim_ref.master_expect gives adam_elem_master's
f32 bits; then sr_round with which = 0, 1, 2.  master_expect's fma emulation (the float64 a b + c
rounded to f32) double-rounds on about 2^-29 of its arguments, so an f32 result may be one f32 ulp
off; check_sr_step therefore lets an element differ only if sr_round of the expected f32 value moved
one f32 ulp up or down gives the kernel's bits, and at most BIT_CAP of the elements may.  The
reference alone is far inside that: an f32-ulp move flips a store only when it crosses the rounding
threshold, about 2^-16 of the moved ones.
"""
import numpy as np
import torch

from tests import _optim_ref as O
from tests._row_ref import BF, BIT_CAP, F32, ibits

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
STREAMS = 1 << 30
PARAM, EXP_AVG, EXP_AVG_SQ = 0, 1, 2

FAULTS = ("nearest", "which_ignored", "step_ignored", "bits_by_launch", "tail_chunk0", "nan_integer", "clip_rounded")


# ------------------------------------------------------------------------------ Philox4x32-10
def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints) of one shape, key: two ints.  Returns the four output words as
    uint64 arrays holding 32-bit values."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        a = np.uint64(M0) * c[0]      # 32 x 32 -> 64: exact in uint64
        b = np.uint64(M1) * c[2]
        c = [(b >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), b & np.uint64(MASK),
             (a >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), a & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def _bits(seed, stream, step, which, chunks, n):
    """The 16-bit draws of elements 0 .. n-1 whose chunk indices are `chunks` (ceil(n / 8) of them)."""
    assert 0 <= seed < 1 << 64 and 0 <= stream < STREAMS and 1 <= step < 1 << 32 and which in (0, 1, 2)
    chunks = np.asarray(chunks, dtype=np.uint64)
    w = philox4x32_10((chunks & np.uint64(MASK), chunks >> np.uint64(32), step, (stream << 2) | which),
                      (seed & MASK, seed >> 32))
    w = np.stack(w, axis=1)                                         # [chunks, 4]
    r = np.stack([w & np.uint64(0xFFFF), w >> np.uint64(16)], axis=2)   # [chunks, word, half]: element 2 j + half
    return r.reshape(-1)[:n].astype(np.uint32)


def sr_bits(seed, stream, step, which, n):
    """r of elements 0 .. n-1 of the tensor with this stream id, as a uint32 array of 16-bit values."""
    return _bits(seed, stream, step, which, np.arange((n + 7) // 8), n)


# ------------------------------------------------------------------------------ sr_bf16
def _u32(x32):
    assert x32.dtype == F32
    return ibits(x32.detach().cpu().reshape(-1)).numpy().astype(np.int64) & MASK


def _bf_of_bits(b16):
    return torch.from_numpy(np.asarray(b16, dtype=np.uint16).view(np.int16).copy()).view(BF)


def sr_round(x32, r, fault=None):
    """sr_bf16 of an f32 tensor with the draws r (uint array of 16-bit values): a 1-D bf16 tensor.
    Faults: nearest (the plain cast everywhere), nan_integer (inf and NaN through the integer path)."""
    x32 = x32.detach().cpu().reshape(-1)
    plain = x32.to(BF)
    if fault == "nearest":
        return plain
    u = _u32(x32)
    out = _bf_of_bits((((u + np.asarray(r, dtype=np.int64)) & MASK) >> 16).astype(np.uint16))
    if fault == "nan_integer":
        return out
    special = torch.from_numpy((u & 0x7F800000) == 0x7F800000)
    return torch.where(special, plain, out)


def differs(got, want):
    """bf16 tensors: bit difference, any NaN equal to any NaN"""
    got, want = got.detach().cpu().reshape(-1), want.detach().cpu().reshape(-1)
    return (ibits(got) != ibits(want)) & ~(torch.isnan(got) & torch.isnan(want))


def check_sr_cast(name, got, x32, r):
    """got = sr_bf16(x32, r) by bits (NaN for NaN)."""
    d = differs(got, sr_round(x32, r))
    if bool(d.any()):
        i = int(d.nonzero()[0])
        u = int(_u32(x32)[i])
        raise AssertionError(f"{name}: {int(d.sum())} of {d.numel()} elements differ from sr_bf16; first at {i}: x bits "
                             f"{u:08x} r {int(r[i]):04x} got {int(ibits(got.cpu().reshape(-1))[i]) & 0xFFFF:04x}")


# ------------------------------------------------------------------------------ the step
def expect_step(p, g, m, v, s, seed, stream, step, coef=None):
    """One tensor's step.  p, m, v bf16, g bf16 or f32 (CPU, any shape), s the scalars, coef the clip
    coefficient or None.  Returns (want16, want32, r): three bf16 tensors, the three f32 tensors they were
    rounded from, and the three draw arrays, each in the order param, exp_avg, exp_avg_sq."""
    p, g, m, v = (t.detach().cpu().reshape(-1) for t in (p, g, m, v))
    g32 = g.to(F32)
    if coef is not None:
        g32 = O.clip_grad(g32, coef, False)
    want32 = O.master_expect(p.to(F32), g32, m.to(F32), v.to(F32), s)
    r = tuple(sr_bits(seed, stream, step, which, p.numel()) for which in (PARAM, EXP_AVG, EXP_AVG_SQ))
    return tuple(sr_round(x, rr) for x, rr in zip(want32, r)), want32, r


def check_sr_step(name, got, want32, r, cap=BIT_CAP):
    """got = (p, m, v) bf16 after, want32 / r from expect_step (or their concatenation over a list).  The
    NaN / inf class matches exactly; an element differs from sr_round(want32) only if sr_round of want32
    one f32 ulp up or down gives its bits; at most `cap` of the elements do.  Returns that share."""
    n = want32[0].numel()
    if n == 0:
        return 0.0
    D = torch.zeros(n, dtype=torch.bool)
    for o, gt, x, rr in zip("pmv", got, want32, r):
        gt = gt.detach().cpu().reshape(-1)
        assert gt.dtype == BF and gt.numel() == n, f"{name} {o}: {gt.dtype} x {gt.numel()}"
        w = sr_round(x, rr)
        bad = O._class_bad(gt.to(torch.float64), w.to(torch.float64))
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            raise AssertionError(f"{name} {o}: {int(bad.sum())} elements of the wrong class (NaN / inf / finite), first at "
                                 f"{i} (chunk {i // 8}): got {float(gt[i])!r} want {float(w[i])!r}")
        d = differs(gt, w)
        if bool(d.any()):
            idx = d.nonzero().reshape(-1)
            ok = torch.zeros(idx.numel(), dtype=torch.bool)
            for k in (1, -1):
                ok |= ~differs(gt[idx], sr_round(O.nbr(x[idx], k), rr[idx.numpy()]))
            if not bool(ok.all()):
                i = int(idx[(~ok).nonzero()[0]])
                raise AssertionError(f"{name} {o}: {int((~ok).sum())} of {n} elements differ from the expected bits and an f32 "
                                     f"ulp does not explain them; first at {i} (chunk {i // 8}, element {i % 8}): got "
                                     f"{float(gt[i])!r} want {float(w[i])!r} from {float(x[i])!r} r {int(rr[i]):04x}")
        D |= d
    share = float(D.double().mean())
    print(f"sr-check {name} bit-mismatch share {share:.2e}")
    assert share <= cap, f"{name}: {share:.3%} of the elements differ by bits (cap {cap:.1%})"
    return share


def expect_list(before, streams, s, seed, step, coef=None):
    """expect_step over a list: before = (P, G, M, V) ListBufs, streams the tensors' ids.  Returns (want16,
    want32, r) concatenated in list order."""
    P, G, M, V = before
    parts = [expect_step(p, g, m, v, s, seed, st, step, coef)
             for p, g, m, v, st in zip(P.views(), G.views(), M.views(), V.views(), streams)]
    cat = lambda k, j: torch.cat([x[k][j] for x in parts]) if parts else torch.zeros(0)   # noqa: E731
    want16 = tuple(cat(0, j) for j in range(3))
    want32 = tuple(cat(1, j) for j in range(3))
    r = tuple(np.concatenate([x[2][j] for x in parts]) if parts else np.zeros(0, np.uint32) for j in range(3))
    return want16, want32, r


def check_sr_list(name, after, before, streams, s, seed, step, coef=None):
    """One list step: after = (P, M, V) ListBufs, before = (P, G, M, V) as they were.  Gaps, then the bits."""
    for nm, b in zip("pmv", after):
        assert b.gaps_intact(), f"{name}: the kernel wrote outside the tensors of {nm}"
    _, want32, r = expect_list(before, streams, s, seed, step, coef)
    return check_sr_step(name, [b.cat() for b in after], want32, r)


# ------------------------------------------------------------------------------ emulator with faults
def emu_sr_list_step(P, G, M, V, streams, s, seed, step, coef=None, fault=None):
    """The list step in place on the ListBufs P, M, V, tensor by tensor.  Faults: nearest (round to nearest
    instead of stochastically), which_ignored (one draw for p, m and v), step_ignored (the bits of step 1),
    bits_by_launch (the chunk counter runs over the launch's concatenation instead of inside the tensor),
    tail_chunk0 (the ragged last chunk takes chunk 0's bits), nan_integer (NaN through the integer path),
    clip_rounded (the clipped gradient rounded to bf16).  For the checker's self-test; not a reference."""
    cs = O.chunk_starts(P.lengths)
    for t, (p, g, m, v) in enumerate(zip(P.views(), G.views(), M.views(), V.views())):
        n = p.numel()
        if n == 0:
            continue
        g32 = g.to(F32)
        if coef is not None:
            g32 = O.clip_grad(g32, coef, fault == "clip_rounded").to(F32)
        want32 = O.master_expect(p.to(F32), g32, m.to(F32), v.to(F32), s)
        for which, (dst, x) in enumerate(zip((p, m, v), want32)):
            chunks = np.arange((n + 7) // 8) + (cs[t] if fault == "bits_by_launch" else 0)
            if fault == "tail_chunk0" and n % 8:
                chunks[-1] = 0
            r = _bits(seed, streams[t], 1 if fault == "step_ignored" else step, 0 if fault == "which_ignored" else which,
                      chunks, n)
            dst.copy_(sr_round(x, r, fault))
