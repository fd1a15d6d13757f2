"""Attention sinks without a GPU: the new C entries refuse before any launch (fake, never dereferenced pointers, as in
tests/test_attn_host_cpu.py), the wrappers' and model.Attention's refusals, layer_types parsing, the unchanged state_dict."""
import types

import pytest
import torch

from picotron_amd import _C, kernels as K

BF = torch.bfloat16
EINVAL, EALIGN, EUNSUP = -1, -2, -3
P = {n: 0x10000000 + i * 0x100000 for i, n in enumerate("q k v o lse sinks kv_lo q_hi delta dsinks ws".split())}
STR = _C.i64arr([256 * 4 * 64, 4 * 64, 64])
CFG = dict(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_key_value_heads=2, vocab_size=512,
           rms_norm_eps=1e-5, rope_theta=10000.0, num_hidden_layers=2, max_position_embeddings=128)
FWD, BWD = "q s k s v s o s lse sinks B H HKV Sq Sk D", "lse delta sinks dsinks ws B H Sq lse_ld delta_ld mode"


@pytest.mark.parametrize("entry,over,code", [
    (FWD, dict(sinks=None), EINVAL), (FWD, dict(sinks=P["sinks"] + 2), EALIGN), (FWD, dict(Sk=512), EUNSUP),
    (FWD, dict(D=96), EUNSUP), (FWD, dict(Sq=200, Sk=200), EUNSUP), (FWD, dict(sinks=None, D=96), EINVAL),
    (BWD, dict(sinks=None), EINVAL), (BWD, dict(mode=3), EINVAL), (BWD, dict(B=0), EINVAL), (BWD, dict(H=70000), EUNSUP),
    (BWD, dict(Sq=2 ** 31 - 1), EUNSUP), (BWD, dict(delta_ld=255), EINVAL), (BWD, dict(lse=P["lse"] + 2, mode=3), EINVAL),
    (BWD, dict(lse=P["lse"] + 2), EALIGN), (BWD, dict(dsinks=P["dsinks"] + 2, mode=K.DW_ACC_F32), EALIGN)])
def test_entries_refuse(entry, over, code):
    a = dict(P, s=STR, B=1, H=4, HKV=2, Sq=256, Sk=256, D=64, lse_ld=0, delta_ld=0, mode=0)
    a.update(over)
    args, lib = [a[n] for n in entry.split()], _C.load_library()
    if entry is BWD:
        assert lib.pt_attn_sink_bwd(*args, None) == code
        assert lib.pt_attn_sink_bwd_partials(2, 4, 1025) == 16 and lib.pt_attn_sink_bwd_partials(0, 4, 256) == EINVAL
    else:
        assert lib.pt_attn_fwd_sink(*args, 0.125, None) == code
        assert lib.pt_attn_fwd_band_sink(*args, 0.125, a["kv_lo"], a["q_hi"], None) == code


def test_wrappers_refuse():
    q, k, s = torch.zeros(1, 128, 4, 64, dtype=BF), torch.zeros(1, 128, 2, 64, dtype=BF), torch.zeros(4, dtype=BF)
    block = K.attn_block_band(K.attn_band(1, 128, "cpu").kv_lo, range(128), range(128), True)
    for kw in (dict(merge=True), dict(band=block)):
        with pytest.raises(NotImplementedError, match="exactly once"):
            K.attn_fwd(q, k, k, 0.125, True, sinks=s, **kw)
    for bad in (torch.zeros(2, dtype=BF), torch.zeros(4), torch.zeros(8, dtype=BF)[::2], torch.zeros(5, dtype=BF)[1:]):
        with pytest.raises(ValueError, match="sinks must be"):
            K.attn_fwd(q, k, k, 0.125, True, sinks=bad)
        with pytest.raises(ValueError, match="sinks must be"):
            K.attn_sink_bwd(torch.zeros(1, 4, 128), torch.zeros(1, 4, 128), bad)


def test_model_refusals_layer_types_and_state_dict(monkeypatch):
    monkeypatch.setenv("DEVICE", "cpu")
    monkeypatch.setenv("CONTEXT_PARALLEL", "0")
    from picotron_amd import process_group_manager as pgm
    from picotron_amd.model import Attention, DecoderLayer, Llama
    m = pgm.setup_process_group_manager(1, 1, 1, 1)
    ns = lambda **kw: types.SimpleNamespace(**dict(CFG, **kw))   # noqa: E731
    for axis, what in (("tp_world_size", "tensor parallelism"), ("cp_world_size", "context parallelism")):
        monkeypatch.setattr(m, axis, 2)
        with pytest.raises(NotImplementedError, match=what):
            Attention(ns(attention_sinks=True), 0)
        monkeypatch.setattr(m, axis, 1)
    with pytest.raises(NotImplementedError, match="kv_lora_rank"):
        DecoderLayer(ns(attention_sinks=True, kv_lora_rank=64), 0)
    plain = set(Llama(ns()).state_dict())
    assert set(Llama(ns(attention_sinks=False)).state_dict()) == plain
    assert set(Llama(ns(attention_sinks=True)).state_dict()) - plain == {f"decoder_layers.{i}.attention.sinks" for i in (0, 1)}
    for bad, what in ((["full_attention"], "1 entries"), (["full_attention", "chunked_attention"], "chunked_attention")):
        with pytest.raises(ValueError, match=what):
            Llama(ns(layer_types=bad, sliding_window=64))
    windows = lambda **kw: [l.attention.sliding_window for l in Llama(ns(sliding_window=64, **kw)).decoder_layers]   # noqa: E731
    assert windows(layer_types=["sliding_attention", "full_attention"]) == [64, None] and windows() == [64, 64]
