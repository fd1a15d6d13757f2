"""model.Attention at head dim 256 (hidden 512, 2 heads on 1 kv head, B 2, S 128): output, dx and the
four weight gradients against the same module computed in float64 torch from the same bf16 weights and
tables, with tests/test_model_gpu.py's metric and tolerance for its d64 / d128 layers; and the layouts
this head dim refuses."""
import types

import pytest
import torch

from tests.test_model_gpu import TOL, _env, rel   # noqa: F401  (_env: autouse fixture)

pytestmark = pytest.mark.gpu
BF, F64 = torch.bfloat16, torch.float64
B, S, HID, NH, NKV, D = 2, 128, 512, 2, 1, 256


def cfg(**over):
    return types.SimpleNamespace(**dict(dict(
        hidden_size=HID, intermediate_size=512, num_attention_heads=NH, num_key_value_heads=NKV, vocab_size=256,
        rms_norm_eps=1e-5, rope_theta=10000.0, num_hidden_layers=1, max_position_embeddings=S), **over))


def ref_attention(x, p, cos, sin):
    def heads(w, n):
        return (x @ p[w].t()).view(B, S, n, D).transpose(1, 2)

    def rope(t):
        return t * cos + torch.cat([-t[..., D // 2:], t[..., :D // 2]], -1) * sin

    q, k, v = rope(heads("q_proj.weight", NH)), rope(heads("k_proj.weight", NKV)), heads("v_proj.weight", NKV)
    k, v = k.repeat_interleave(NH // NKV, dim=1), v.repeat_interleave(NH // NKV, dim=1)
    sc = (q @ k.transpose(-1, -2)) * D ** -0.5
    o = torch.softmax(sc.masked_fill(~torch.ones(S, S, dtype=torch.bool).tril(), float("-inf")), -1) @ v
    return o.transpose(1, 2).reshape(B, S, NH * D) @ p["out_proj.weight"].t()


def test_attention_module_matches_float64(monkeypatch):
    monkeypatch.setenv("FLASH_ATTEN", "1")
    from picotron_amd.model import Attention, get_cos_sin
    with torch.device("cuda"):
        att = Attention(cfg(), 0)
    att.to(BF)
    cos, sin = get_cos_sin(S, D, base=10000.0)
    x, dy = torch.randn(B, S, HID).to(BF), torch.randn(B, S, HID).to(BF)
    xg = x.cuda().requires_grad_(True)
    y = att(xg, cos, sin)
    y.backward(dy.cuda())
    p = {n: t.detach().cpu().to(F64).requires_grad_(True) for n, t in att.named_parameters()}
    xr = x.to(F64).requires_grad_(True)
    yr = ref_attention(xr, p, cos.cpu().to(F64), sin.cpu().to(F64))
    yr.backward(dy.to(F64))
    errs = {"y": rel(y, yr), "dx": rel(xg.grad, xr.grad), **{n: rel(t.grad, p[n].grad) for n, t in att.named_parameters()}}
    print(f"d256 attention module: {errs}")
    assert len(errs) == 6 and max(errs.values()) < TOL, errs


@pytest.mark.parametrize("what", ["document_ids", "sliding_window"])
def test_bands_raise_before_any_launch(monkeypatch, what):
    from picotron_amd import kernels as K
    from picotron_amd import model as M

    def launched(*a, **k):
        raise AssertionError("a kernel was reached")

    for name in ("attn_band", "linear_fwd", "attn_fwd"):
        monkeypatch.setattr(K, name, launched)
    with pytest.raises(NotImplementedError, match="head_dim 256"):
        with torch.device("cuda"):
            att = M.Attention(cfg(**({"sliding_window": 64} if what == "sliding_window" else {})), 0)
        att.to(BF)(torch.zeros(1, S, HID, dtype=BF, device="cuda"), *M.get_cos_sin(S, D, base=10000.0),
                   document_ids=torch.zeros(1, S, dtype=torch.long, device="cuda"))
