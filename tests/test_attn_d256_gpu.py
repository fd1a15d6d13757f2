"""Head dim 256 attention (csrc/attention_d256.hip) through kernels.attn_fwd / attn_bwd against the float64
reference of tests/_attn_ref.py at that module's own per-element bounds: out, lse, delta, dq, dk, dv
(the backward reference is a function of the o and lse the backward kernels are given).
Shapes: one 128-row block; an even block count (the paired launch) with a GQA group of 2; an odd block
count with an odd head count and a batch stride; more than one pair with two kv heads.  Layouts:
contiguous tensors, and the model's -- q|k|v column slices of one [B, S, (H + 2 HKV) * 256] buffer, the
gradients written into slices of another."""
import functools

import pytest
import torch

from tests import _attn_ref as R

pytestmark = pytest.mark.gpu
D = 256
SCALE = 0.07   # the caller's, not 256^-0.5 = 0.0625
SHAPES = [(1, 128, 1, 1), (1, 256, 2, 1), (2, 384, 3, 3), (1, 512, 4, 2)]


@functools.lru_cache(maxsize=None)
def case(family, B, S, H, HKV):
    """bf16 CPU (q, k, v, dO) and the float64 forward."""
    q, k, v, do = R.make_case(family, B, S, S, H, HKV, D)
    return q, k, v, do, R.ref_forward(q, k, v, SCALE, R.causal_mask(S, S))


def sliced(q, k, v):
    """q, k, v on the device as column slices of one [B, S, (H + 2 HKV) * D] buffer."""
    B, S, H, _ = q.shape
    HKV = k.shape[2]
    buf = torch.cat([t.reshape(B, S, -1) for t in (q, k, v)], -1).cuda()
    wq, wk = H * D, HKV * D
    return (buf[..., :wq].view(B, S, H, D), buf[..., wq:wq + wk].view(B, S, HKV, D),
            buf[..., wq + wk:].view(B, S, HKV, D))


def run(q, k, v, do, layout):
    from picotron_amd import kernels as K
    if layout == "sliced":
        qd, kd, vd = sliced(q, k, v)
        dq, dk, dv = sliced(*(torch.full_like(t, float("nan")) for t in (q, k, v)))
    else:
        qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
        dq = dk = dv = None
    out, lse = K.attn_fwd(qd, kd, vd, SCALE, True)
    dq, dk, dv, delta = K.attn_bwd(do.cuda(), qd, kd, vd, out, lse, SCALE, True, dq=dq, dk=dk, dv=dv)
    return out, lse, dq, dk, dv, delta


def check_all(got, q, k, v, do, fwd, tag):
    out, lse, dq, dk, dv, delta = got
    S = q.shape[1]
    R.check_out(out, fwd, tag)
    R.check_lse(lse, fwd.lse, tag)
    bwd = R.ref_backward(q, k, v, do, lse.cpu(), SCALE, R.causal_mask(S, S), o=out.cpu())
    R.check_delta(delta, bwd, tag)
    R.check_grads(dq, dk, dv, bwd, tag)


@pytest.mark.parametrize("layout", ["contiguous", "sliced"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("family", ["randn", "peaked", "offset-", "zeroq"])
def test_against_float64(family, shape, layout):
    q, k, v, do, fwd = case(family, *shape)
    check_all(run(q, k, v, do, layout), q, k, v, do, fwd, f"d256-{family}-{layout}")


def test_off_grid_sequence():
    """S = 200: the causal zero-padding path arrives at the kernels with S = 256."""
    q, k, v, do, fwd = case("randn", 1, 200, 2, 1)
    got = run(q, k, v, do, "contiguous")
    assert got[0].shape == q.shape and got[1].shape == (1, 2, 200) and got[3].shape == k.shape
    check_all(got, q, k, v, do, fwd, "d256-offgrid")


def test_backward_is_deterministic():
    q, k, v, do, _ = case("randn", 1, 512, 4, 2)
    a, b = run(q, k, v, do, "contiguous"), run(q, k, v, do, "contiguous")
    for name, x, y in zip(("out", "lse", "dq", "dk", "dv", "delta"), a, b):
        assert torch.equal(x, y), name


def test_refusals():
    from picotron_amd import kernels as K
    q, k, v, do = (t.cuda() for t in case("randn", 1, 128, 1, 1)[:4])
    o, lse = torch.zeros_like(q), torch.zeros(1, 1, 128, device="cuda")
    band = K.attn_band(1, 128, q.device, window=32)
    with pytest.raises(NotImplementedError, match="merge"):
        K.attn_fwd(q, k, v, SCALE, True, out=o.float(), lse=lse, merge=True)
    with pytest.raises(NotImplementedError, match="band"):
        K.attn_fwd(q, k, v, SCALE, True, band=band)
    with pytest.raises(NotImplementedError, match="sink"):
        K.attn_fwd(q, k, v, SCALE, True, sinks=torch.zeros(1, dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(ValueError, match="causal"):
        K.attn_fwd(q, k, v, SCALE, False)
    with pytest.raises(NotImplementedError, match="grad_f32"):
        K.attn_bwd(do, q, k, v, o, lse, SCALE, True, grad_f32=True)
    with pytest.raises(NotImplementedError, match="band"):
        K.attn_bwd(do, q, k, v, o, lse, SCALE, True, band=band)
