"""csrc/embedding.hip against its exact expectation (tests/_optim_ref.py: emu_embedding_fwd, emu_embedding_bwd;
their faults are rejected in tests/test_optim_checker_cpu.py).  The forward is a copy; the backward is the
documented order -- an f32 sum over an id's tokens in ascending position, one bf16 rounding, then the sink
-- which float32 on the CPU reproduces bit for bit, so every comparison is by bits.

    H            8 (one lane), 264 (a partly used wave), 520, 1032, 2048 (one to four trips of the column loop)
    ld           weight, output, dY and dW rows padded by 8 and by 24 columns inside sentinel-filled buffers
                 with guard rows; padding and guards intact afterwards
    sinks        bf16 store, bf16 accumulate and f32 accumulate, the last two onto non-zero old values
    vocab slice  lo > 0, ids at lo - 1, lo, hi - 1, hi; padding_idx inside the slice, outside it, absent
    ids          one id for every token, every token skipped (dW untouched by bits), every id distinct
    T            0, 1, 16384 (the one-workgroup sort's limit), 16385 (torch's stable sort), 40000 at H 8 (the
                 backward's grid of 32768 waves wraps), and a forward of 16400 x 1032 (2 115 600 chunks: the
                 forward's grid of 8192 x 256 threads wraps)
dY carries a few (X, -X, small) triples in ascending position per id and exponents spread over 2^-12 .. 2^12,
so a different summation order changes the bits.
"""
import ctypes

import pytest
import torch

from tests import _optim_ref as O
from tests import _row_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
HS = (8, 264, 520, 1032, 2048)
SINKS = (0, O.PT_DW_ACC_BF16, O.PT_DW_ACC_F32)


def K_():
    from picotron_amd import kernels
    return kernels


def _padded(t, gap):
    """t on the device inside a sentinel buffer [rows + 2, cols + gap]: (full, view)."""
    rows, cols = t.shape
    full = torch.empty(rows + 2, cols + gap, dtype=t.dtype, device=DEV)
    R.ibits(full).fill_(R.NAN16 if t.dtype == BF else R.NAN32)
    view = full[1:rows + 1, :cols]
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return full, view


def _intact(full, rows, cols):
    ib = R.ibits(full).clone()
    pat = R.NAN16 if full.dtype == BF else R.NAN32
    ib[1:rows + 1, :cols] = pat
    return bool((ib == pat).all())


def _case(T, H, V, lo, seed=0, ids=None):
    """ids [T] around the slice [lo, lo + V) (with lo - 1, lo, hi - 1, hi present when T >= 4), dY [T, H]."""
    gen = R._gen("embedding", T, H, V, seed)
    if ids is None:
        ids = torch.randint(lo - 2, lo + V + 2, (T,), generator=gen)
        if T >= 4:
            ids[torch.randperm(T, generator=gen)[:4]] = torch.tensor([lo - 1, lo, lo + V - 1, lo + V])
    dy = torch.randn(T, H, generator=gen) * torch.pow(2.0, torch.randint(-12, 13, (T, H), generator=gen).float())
    # the first two tokens of an id: X, -X with |X| 2^20 times the rest
    order = torch.sort(ids, stable=True)
    first = torch.ones(T, dtype=torch.bool)
    first[1:] = order.values[1:] != order.values[:-1]
    second = torch.zeros(T, dtype=torch.bool)
    second[1:] = first[:-1] & ~first[1:]
    a, b = order.indices[:-1][second[1:]], order.indices[1:][second[1:]]
    dy[a] = dy[a] * 2.0 ** 20
    dy = dy.to(BF)
    dy[b] = -dy[a]
    return ids, dy


def _old(V, H, sink, seed=0):
    return torch.randn(V, H, generator=R._gen("old", V, H, sink, seed)).to(F32 if sink == O.PT_DW_ACC_F32 else BF)


def _bwd(ids, dy, old, sink, lo, hi, pad=None, gap=8, name="dw"):
    K = K_()
    V, H = old.shape
    T = ids.numel()
    dyf, dyv = _padded(dy, gap) if T else (None, torch.empty(0, H, dtype=BF, device=DEV))
    dwf, dwv = _padded(old, gap)
    K.embedding_bwd(ids.to(DEV), dyv, dwv, sink, lo, hi, pad)
    torch.cuda.synchronize()
    want = O.emu_embedding_bwd(ids, dy, old, sink, lo, hi, pad)
    R.check_exact(name, dwv, want)
    assert _intact(dwf, V, H), f"{name}: dW's padding or guard rows were written"
    if T:
        keep, _ = _padded(dy, gap)
        assert O.same_bits(dyf, keep), f"{name}: dY was written"
    return want


def _fwd(ids, w, lo, hi, gap=8, name="out"):
    from picotron_amd import _C
    V, H = w.shape
    T = ids.numel()
    wf, wv = _padded(w, gap)
    of, ov = _padded(torch.zeros(T, H, dtype=BF), gap)
    R.ibits(ov).fill_(R.NAN16)
    dev_ids = ids.to(DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    rc = _C.lib().pt_embedding_fwd(p(dev_ids), T, p(wv), wv.stride(0), lo, hi, p(ov), ov.stride(0), H, _C.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    R.check_exact(name, ov, O.emu_embedding_fwd(ids, w, lo, hi))
    assert _intact(of, T, H), f"{name}: the output's padding or guard rows were written"
    keep, _ = _padded(w, gap)
    assert O.same_bits(wf, keep)


@pytest.mark.parametrize("gap", [8, 24])
@pytest.mark.parametrize("H", HS)
def test_forward(H, gap):
    V, lo = 40, 8
    ids, _ = _case(301, H, V, lo)
    w = torch.randn(V, H, generator=R._gen("w", H)).to(BF)
    _fwd(ids, w, lo, lo + V, gap)
    _fwd(ids[:1], w, lo, lo + V, gap)
    # the wrapper (dense output), also with no token at all
    out = K_().embedding_fwd(ids.to(DEV).view(7, 43), w.to(DEV), lo, lo + V)
    R.check_exact("wrapper", out.view(-1, H), O.emu_embedding_fwd(ids, w, lo, lo + V))
    assert K_().embedding_fwd(ids[:0].to(DEV), w.to(DEV), lo, lo + V).shape == (0, H)


def test_forward_grid_wraps():
    T, H, V, lo = 16400, 1032, 64, 3
    assert T * (H // 8) > 8192 * 256
    gen = R._gen("fwdwrap")
    ids = torch.randint(lo - 1, lo + V + 1, (T,), generator=gen)
    w = torch.randn(V, H, generator=gen).to(BF)
    _fwd(ids, w, lo, lo + V, 8)


@pytest.mark.parametrize("sink", SINKS)
@pytest.mark.parametrize("gap", [8, 24])
@pytest.mark.parametrize("H", HS)
def test_backward(H, gap, sink):
    V, lo = 40, 8
    ids, dy = _case(301, H, V, lo)
    old = _old(V, H, sink)
    for pad in (None, lo + 3, lo - 1, lo + V + 5):   # absent, inside the slice, outside it (twice)
        want = _bwd(ids, dy, old, sink, lo, lo + V, pad, gap, f"dw H {H} sink {sink} pad {pad}")
        if pad == lo + 3 and sink:
            assert O.same_bits(want[3], old[3])


@pytest.mark.parametrize("sink", SINKS)
def test_backward_id_patterns(sink):
    H, V, lo = 264, 600, 5
    old = _old(V, H, sink, 1)
    # one id for every token: a segment of T tokens walked by one wave
    ids, dy = _case(2000, H, V, lo, ids=torch.full((2000,), lo + 17))
    _bwd(ids, dy, old, sink, lo, lo + V, name="one id")
    # every token skipped: dW untouched by bits
    skip = torch.tensor([lo - 1, lo + V, lo + 9]).repeat(100)
    want = _bwd(skip, dy[:300].contiguous(), old, sink, lo, lo + V, pad=lo + 9, name="all skipped")
    assert O.same_bits(want, old)
    # every id distinct
    perm = torch.randperm(V, generator=R._gen("perm"))[:512] + lo
    _bwd(perm, dy[:512].contiguous(), old, sink, lo, lo + V, name="distinct")


@pytest.mark.parametrize("T", [0, 1, 16384, 16385])
def test_backward_token_counts(T):
    """Around the one-workgroup sort's limit: 16385 tokens go through torch's stable sort, the same bits."""
    H, V, lo = 24, 3000, 2
    for sink in SINKS[1:]:
        ids, dy = _case(T, H, V, lo, seed=T)
        _bwd(ids, dy, _old(V, H, sink, 2), sink, lo, lo + V, pad=lo + 1, name=f"T {T} sink {sink}")
    if T == 16384:   # one segment as long as the sort holds, and all ids distinct
        ids, dy = _case(T, 8, 4, 0, ids=torch.full((T,), 2))
        _bwd(ids, dy, _old(4, 8, 0), 0, 0, 4, name="T 16384 one id")
        ids, dy = _case(T, 8, T, 0, ids=torch.randperm(T, generator=R._gen("d")))
        _bwd(ids, dy, _old(T, 8, O.PT_DW_ACC_F32), O.PT_DW_ACC_F32, 0, T, name="T 16384 distinct")


def test_backward_grid_wraps():
    T, H, V, lo = 40000, 8, 5000, 7
    assert T > 4 * 8192          # more sorted entries than the 8192 x 4 waves of the grid
    ids, dy = _case(T, H, V, lo)
    _bwd(ids, dy, _old(V, H, O.PT_DW_ACC_BF16), O.PT_DW_ACC_BF16, lo, lo + V, pad=lo + 2, gap=24)
