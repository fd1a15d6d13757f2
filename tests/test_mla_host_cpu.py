"""Host side of multi-head latent attention (CPU): the ABI's return codes, MLAttention's state_dict and the
Muon / AdamW parameter split -- nothing here touches a device."""
import ctypes
import types

import pytest

PTR = 1 << 20   # a non-null, 16-byte aligned address no refused call dereferences


def _config(**over):
    d = dict(hidden_size=128, intermediate_size=128, num_attention_heads=2, num_key_value_heads=2, vocab_size=256,
             rms_norm_eps=1e-5, rope_theta=10000.0, num_hidden_layers=1, max_position_embeddings=128,
             kv_lora_rank=64, q_lora_rank=None, qk_nope_head_dim=128, qk_rope_head_dim=64, v_head_dim=128)
    d.update(over)
    return types.SimpleNamespace(**d)


def _attn_args(lib_fn, q=PTR, S=128, dims=(128, 64, 128), bwd=False):
    st4, st2 = (ctypes.c_int64 * 3)(128 * 2 * 192, 2 * 192, 192), (ctypes.c_int64 * 2)(128 * 64, 64)
    views = [q, st4, PTR, st4, PTR, st2, PTR, st4, PTR, st4]            # q, k_nope, k_pe, v, o
    if bwd:                                                                # dout, lse, delta, dq, dk_nope, dv, ws
        views += [PTR, st4, PTR, PTR, PTR, st4, PTR, st4, PTR, st4, PTR]
    else:
        views += [PTR]                                                     # lse
    return lib_fn(*views, 1, 2, S, *dims, 0.07, None)


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
def test_attention_entries_refuse_before_launch(bwd):
    from picotron_amd import _C
    lib = _C.load_library()
    fn = lib.pt_mla_attn_bwd if bwd else lib.pt_mla_attn_fwd
    assert _attn_args(fn, dims=(64, 64, 128), bwd=bwd) == -1     # nope
    assert _attn_args(fn, dims=(128, 32, 128), bwd=bwd) == -1    # rope
    assert _attn_args(fn, dims=(128, 64, 192), bwd=bwd) == -1    # v
    assert _attn_args(fn, S=192, bwd=bwd) == -1                  # off the 128-row blocks
    assert _attn_args(fn, q=None, bwd=bwd) == -1


def test_row_entries_refuse_before_launch():
    from picotron_amd import _C
    lib = _C.load_library()
    rope = lambda q=PTR, cos=PTR, nope=128, rot=64: lib.pt_mla_rope(q, 384, 2, PTR, 64, 128, cos, PTR, 128, 64, nope, rot, 0, None)
    assert rope(q=None) == -1 and rope(cos=None) == -1 and rope(nope=64) == -1 and rope(rot=128) == -1
    red = lambda ws=PTR, out=PTR, rot=64, rows=128: lib.pt_mla_dkpe_reduce(ws, 2, out, 64, rows, PTR, PTR, 128, 64, rot, None)
    assert red(ws=None) == -1 and red(out=None) == -1 and red(rot=32) == -1 and red(rows=0) == -1


@pytest.mark.parametrize("q_lora_rank", [None, 96])
def test_state_dict_and_muon_split(monkeypatch, q_lora_rank):
    monkeypatch.setenv("DEVICE", "cpu")
    from picotron_amd import model as M
    from picotron_amd.optim import split_muon_params
    net = M.Llama(_config(q_lora_rank=q_lora_rank))
    at = "decoder_layers.0.attention."
    want = {"kv_a_proj_with_mqa.weight": (128, 128), "kv_a_layernorm.weight": (64,), "kv_b_proj.weight": (512, 64),
            "out_proj.weight": (128, 256)}
    if q_lora_rank is None:
        want["q_proj.weight"] = (384, 128)
    else:
        want.update({"q_a_proj.weight": (96, 128), "q_a_layernorm.weight": (96,), "q_b_proj.weight": (384, 96)})
    got = {k[len(at):]: tuple(v.shape) for k, v in net.state_dict().items() if k.startswith(at)}
    assert got == want
    assert net.decoder_layers[0].cos.shape == (128, 64)        # tables for qk_rope_head_dim
    matrices, rest = split_muon_params(net)
    names = {id(p): n for n, p in net.named_parameters()}
    muon = {names[id(p)][len(at):] for p in matrices if names[id(p)].startswith(at)}
    assert muon == {k for k, s in want.items() if len(s) == 2}
    assert all(names[id(p)].endswith("layernorm.weight") for p in rest if names[id(p)].startswith(at))
