"""kernels.attn_band and functional.document_ids_from_eos on CPU tensors: the two bound arrays of a
band (kv_lo per query, q_hi per key) against a brute-force mask, for document ids, sliding windows,
both together and the padded extension; their monotonicity; the refused arguments.

The brute-force mask is written from the definition, token by token: key j is visible to query i
iff j <= i, j lies in i's document (no change of document id anywhere in (j, i]) and i - j < W."""
import pytest
import torch

from picotron_amd import functional as FN
from picotron_amd import kernels as K


def doc_ids(lengths, S):
    """Document ids of `lengths` repeated until S tokens are covered."""
    ids, d = [], 0
    while len(ids) < S:
        ids += [d] * lengths[d % len(lengths)]
        d += 1
    return torch.tensor(ids[:S])


def brute_mask(S, ids=None, window=None):
    """[B, S, S] bool (query on dim 1) from the definition; ids [B, S] or None."""
    B = 1 if ids is None else ids.shape[0]
    m = torch.zeros(B, S, S, dtype=torch.bool)
    for b in range(B):
        for i in range(S):
            for j in range(i, -1, -1):
                if window is not None and i - j >= window:
                    break
                m[b, i, j] = True
                if ids is not None and j > 0 and ids[b, j] != ids[b, j - 1]:
                    break   # j is the first token of i's document
    return m


def lo_mask(band):
    j = torch.arange(band.S)
    return (j[None, None, :] >= band.kv_lo[:, :, None]) & (j[None, None, :] <= j[None, :, None])


def hi_mask(band):
    i = torch.arange(band.S)
    return (i[None, :, None] < band.q_hi[:, None, :]) & (i[None, None, :] <= i[None, :, None])


def check_band(band, want):
    assert band.kv_lo.dtype == torch.int32 and band.q_hi.dtype == torch.int32
    assert tuple(band.kv_lo.shape) == tuple(band.q_hi.shape) == (band.B, band.S)
    assert band.kv_lo.is_contiguous() and band.q_hi.is_contiguous()
    assert torch.equal(lo_mask(band), want)
    assert torch.equal(hi_mask(band), want)             # the key-side description is the same mask
    assert torch.equal(band.mask()[:, 0], want)
    i = torch.arange(band.S)
    assert bool((band.kv_lo >= 0).all()) and bool((band.kv_lo <= i).all())
    assert bool((band.q_hi > i).all()) and bool((band.q_hi <= band.S).all())
    assert bool((band.kv_lo[:, 1:] >= band.kv_lo[:, :-1]).all())   # both non-decreasing along a row
    assert bool((band.q_hi[:, 1:] >= band.q_hi[:, :-1]).all())


S = 160
IDS = torch.stack([doc_ids([1, 95, 33, 127], S), doc_ids([60, 110, 86], S)])


def test_document_ids():
    check_band(K.attn_band(2, S, "cpu", document_ids=IDS), brute_mask(S, IDS))


def test_document_ids_need_not_be_sorted_or_dense():
    ids = torch.tensor([[7, 7, 3, 3, 3, 7, 7, 0]])   # a boundary wherever the value changes
    band = K.attn_band(1, 8, "cpu", document_ids=ids)
    assert band.kv_lo.tolist() == [[0, 0, 2, 2, 2, 5, 5, 7]]
    assert band.q_hi.tolist() == [[2, 2, 5, 5, 5, 7, 7, 8]]
    check_band(band, brute_mask(8, ids))


def test_every_token_its_own_document():
    ids = torch.arange(S)[None]
    band = K.attn_band(1, S, "cpu", document_ids=ids)
    assert torch.equal(band.kv_lo[0], torch.arange(S, dtype=torch.int32))
    assert torch.equal(band.q_hi[0], torch.arange(1, S + 1, dtype=torch.int32))


@pytest.mark.parametrize("W", [1, 64, 100, S, S + 7])
def test_windows(W):
    band = K.attn_band(2, S, "cpu", window=W)
    check_band(band, brute_mask(S, None, W).expand(2, S, S))
    if W >= S:   # plain causal
        assert not bool(band.kv_lo.any()) and bool((band.q_hi == S).all())


@pytest.mark.parametrize("W", [1, 64, 100])
def test_documents_and_window(W):
    check_band(K.attn_band(2, S, "cpu", document_ids=IDS, window=W), brute_mask(S, IDS, W))


def test_neither_is_causal():
    check_band(K.attn_band(3, S, "cpu"), brute_mask(S).expand(3, S, S))


@pytest.mark.parametrize("W", [None, 50])
def test_padded_extension(W):
    """Rows past S are one-token documents: the real rows' mask is unchanged, a pad row sees itself only."""
    Sp = 256
    band = K.attn_band(2, S, "cpu", document_ids=IDS, window=W)
    ext = band.padded(Sp)
    assert ext.S == Sp and band.padded(S) is band and band.padded(Sp) is ext
    want = torch.zeros(2, Sp, Sp, dtype=torch.bool)
    want[:, :S, :S] = brute_mask(S, IDS, W)
    want[:, range(S, Sp), range(S, Sp)] = True
    check_band(ext, want)
    pad_ids = torch.cat([IDS, IDS.max() + 1 + torch.arange(Sp - S).expand(2, -1)], 1)
    assert torch.equal(want, brute_mask(Sp, pad_ids, W))


def test_bad_arguments_raise():
    with pytest.raises(ValueError):
        K.attn_band(2, S, "cpu", window=0)
    with pytest.raises(ValueError):
        K.attn_band(2, S, "cpu", window=-3)
    with pytest.raises(ValueError):
        K.attn_band(2, S, "cpu", window=64.0)
    with pytest.raises(ValueError):
        K.attn_band(2, S, "cpu", document_ids=IDS[:1])            # batch mismatch
    with pytest.raises(ValueError):
        K.attn_band(2, S - 1, "cpu", document_ids=IDS)            # length mismatch
    with pytest.raises(ValueError):
        K.attn_band(2, S, "cpu", document_ids=IDS.float())        # not integer
    with pytest.raises(ValueError):
        K.attn_band(2, S, "cpu", document_ids=IDS.tolist())       # not a tensor
    with pytest.raises(ValueError):
        K.attn_band(0, S, "cpu")
    with pytest.raises(TypeError):                                 # built only by attn_band
        K.AttnBand(None, IDS.int(), IDS.int())
    with pytest.raises(ValueError):
        K.attn_band(2, S, "cpu").padded(S - 32)


def test_document_ids_from_eos():
    eos = 9
    ids = torch.tensor([[9, 1, 2, 9, 9, 3, 4, 9],      # EOS first, doubled, last
                        [1, 2, 3, 4, 5, 6, 7, 8],      # none
                        [1, 9, 2, 2, 2, 9, 3, 3]])
    got = FN.document_ids_from_eos(ids, eos)
    assert got.dtype == torch.int32
    assert got.tolist() == [[0, 1, 1, 1, 2, 3, 3, 3],   # the EOS belongs to the document it ends
                            [0, 0, 0, 0, 0, 0, 0, 0],
                            [0, 0, 1, 1, 1, 1, 2, 2]]
    band = K.attn_band(3, 8, "cpu", document_ids=got)
    assert band.kv_lo.tolist() == [[0, 1, 1, 1, 4, 5, 5, 5], [0] * 8, [0, 0, 2, 2, 2, 2, 6, 6]]
    with pytest.raises(ValueError):
        FN.document_ids_from_eos(ids[0], eos)


def test_make_band_passes_a_ready_band_through():
    band = K.attn_band(2, S, "cpu", document_ids=IDS)
    assert FN.make_band(2, S, "cpu", band, None) is band
    assert FN.make_band(2, S, "cpu", None, None) is None
    got = FN.make_band(2, S, "cpu", IDS, 64)
    assert torch.equal(got.kv_lo, K.attn_band(2, S, "cpu", document_ids=IDS, window=64).kv_lo)
