"""GeGLU on the GPU against torch float64 of gelu = g s, gelu' = s + t: s = sigmoid(z), z = 2k g (1 + c g^2),
t = g s (1 - s) z', z' = 2k (1 + 3c g^2), under the issue's bounds corrected as check() says."""
import math
import types

import pytest
import torch

from tests.test_model_gpu import _env  # noqa: F401  (DEVICE / LOCAL_RANK and the 1-rank process grid)

pytestmark = pytest.mark.gpu
BF, DEV, ACT, U = torch.bfloat16, "cuda", "gelu_tanh", 2.0 ** -8
K2, C, R, BFMAX = 2 * math.sqrt(2 / math.pi), 0.044715, 2 * U + U * U, float(torch.finfo(torch.bfloat16).max)


def check(h, dg, du, g, u, dh):
    """h, du: (R + 2^-14) |ref|; dg: R |ref| + 2^-13 |dh u| (s + |t|); R = 2U + U^2, a bf16 rounding being U = 2^-8, not
    2^-9.  Plus what an IEEE f32 transcription needs beyond a flat 2^-133 floor: 2^-134 per rounding of a subnormal
    (the first scaled by its multiplier) and, for z < -87 where e^-z leaves f32's range and s comes out 0, the lost
    s (<= 2^-126) times its factor.  Where |ref| reaches bf16's maximum inf is right: not judged."""
    g, u, dh = (t.detach().cpu().double() for t in (g, u, dh))
    z, zp = K2 * g * (1 + C * g * g), K2 * (1 + 3 * C * g * g)
    s = torch.sigmoid(z)
    t, ds = g * s * (1 - s) * zp, torch.where(z < -87, s.clamp(max=2.0 ** -126), torch.zeros_like(s)) * (1 + R)
    for name, got, want, rel, slack, lost, scale in (
            ("h", h, g * s * u, 2 ** -14, 0, ds * g * u, u), ("du", du, dh * g * s, 2 ** -14, 0, ds * g * dh, dh),
            ("dg", dg, dh * u * (s + t), 0, (dh * u).abs() * (s + t.abs()), dh * u * (ds + (ds * g * zp).abs()), s + t)):
        bound = (R + rel) * want.abs() + 2 ** -13 * slack + lost.abs() + 2.0 ** -134 * (1 + scale.abs())
        bad = (want.abs() < BFMAX * (1 - R)) & ~((got.detach().cpu().double() - want).abs() <= bound)   # (NaN: bad)
        assert not bad.any(), f"{name}: {bad.sum().item()} elements outside the bound, first at g = {g[bad][0].item()}"


@pytest.mark.parametrize("case", ["all_g", 8, 264])
def test_row_kernels_match_reference(case):
    from picotron_amd import kernels as K
    gen, n = torch.Generator().manual_seed(7), 8 if case == "all_g" else case
    gu, dd = ((torch.randn(40, 2 * n, generator=gen) * s).to(BF).to(DEV) for s in (3.0, 1.0))
    g, u, dh = gu[:, :n], gu[:, n:], dd[:, n:]   # strided halves
    if case == "all_g":   # every finite bf16 g once [8160, 8], u / dh randn
        b = torch.arange(65536, dtype=torch.int32)
        g = torch.where(b >= 0x8000, b - 0x10000, b)[(b & 0x7F80) != 0x7F80].to(torch.int16).view(BF).reshape(-1, 8)
        g, u, dh = (t.to(DEV) for t in (g, *(torch.randn(g.shape, generator=gen).to(BF) for _ in range(2))))
    dgu = torch.zeros(len(g), 2 * n, dtype=BF, device=DEV)
    dg, du = K.swiglu_bwd(dh, g, u, dg=dgu[:, :n], du=dgu[:, n:], act=ACT)
    check(K.swiglu_fwd(g, u, act=ACT), dg, du, g, u, dh)


def _operands(T, H, I):
    gen = torch.Generator().manual_seed(3)
    r, ri = (lambda *s: torch.randn(*s, generator=gen)), (lambda k, *s: torch.randint(-k, k + 1, s, generator=gen))
    # x, dY, W_gate, W_up, W_down; dY and W_down small integers (/ 64): dh is exact in any f32 summation order
    return [t.to(BF).to(DEV) for t in (r(T, H), ri(3, T, H), r(I, H) / H ** 0.5, r(I, H) / H ** 0.5, ri(4, H, I) / 64)]


@pytest.mark.parametrize("T,H,I", [(256, 64, 128), (512, 192, 384), (256, 64, 256), (512, 192, 512)])
def test_fused_epilogues_equal_row_kernels(T, H, I):
    from picotron_amd import kernels as K
    x, dm, wg, wu, wd = _operands(T, H, I)
    gu, h = K.linear_swiglu_fwd(x, wg, wu, act=ACT)
    gu_ref = K.linear_fwd(x, [wg, wu])
    assert torch.equal(gu, gu_ref) and torch.equal(h, K.swiglu_fwd(gu_ref[:, :I], gu_ref[:, I:], act=ACT))
    dh = K.linear_dgrad(dm, [wd])
    dg, du = K.swiglu_bwd(dh, gu[:, :I], gu[:, I:], act=ACT)
    if I % 256 == 0:
        assert torch.equal(K.linear_dgrad_swiglu(dm, wd, gu, act=ACT), torch.cat([dg, du], 1))
    if (T, H, I) == (256, 64, 128):
        check(h, dg, du, gu[:, :I], gu[:, I:], dh)


@pytest.mark.parametrize("T,H,I,ksplit", [(512, 512, 1024, 1), (512, 1024, 1024, 2), ("moe", 64, 256, 1)])
def test_block_forms_fused_equal_unfused(T, H, I, ksplit):   # (the dual launch at its fewest tiles; reduce mode 11)
    from picotron_amd import functional as FN, kernels as K, switches
    x, dm, *ws = _operands(512, H, I)
    assert T == "moe" or (K.swiglu_dx_ksplit(T, I, H) == ksplit and K.dual_fits((T, I), [(H, I)]))
    outs = []
    for fuse in (1, 0):
        wl = [w.clone().requires_grad_(True) for w in ws]
        with switches.override(fuse=fuse, swiglu_fuse_min_tiles=0):
            if T == "moe":   # 2 experts of capacity 256, the smallest the epilogues take
                el = [[w, w.flip(0).contiguous()] for w in ws]
                gu, hh, ye = K.moe_experts_fwd(x, *el, 256, fuse=bool(fuse), act=ACT)
                outs.append([gu, hh, ye, K.moe_experts_dgrad_down(dm, el[2], gu, 256, fuse=bool(fuse), act=ACT)[0]])
                continue
            m, saved = FN.mlp_block_fwd(x, *wl, FN.TPContext(), act=ACT)
            outs.append([m, *saved, FN.mlp_block_bwd(dm, x, saved, *wl, FN.TPContext(), act=ACT), *(w.grad for w in wl[:2])])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_model_mlp_reads_hidden_act(_env):
    from picotron_amd.model import MLP
    gen = torch.Generator().manual_seed(1)
    x, dy = (torch.randn(1, 256, 64, generator=gen).to(BF).to(DEV) for _ in range(2))

    def run(**fields):
        torch.manual_seed(0)
        with torch.device(DEV):
            mlp = MLP(types.SimpleNamespace(hidden_size=64, intermediate_size=128, **fields)).to(BF)
        xg = x.clone().requires_grad_(True)
        y = mlp(xg)
        y.backward(dy)
        return [y, xg.grad] + [p.grad for p in mlp.parameters()], mlp
    got, mlp = run(hidden_act="gelu_pytorch_tanh")
    w = [p.detach().cpu().double().requires_grad_(True) for p in mlp.parameters()]   # up, gate, down
    xr = x.cpu().double().requires_grad_(True)
    yr = (torch.nn.functional.gelu(xr @ w[1].T, approximate="tanh") * (xr @ w[0].T)) @ w[2].T
    yr.backward(dy.cpu().double())
    # norm-relative 2e-2: the SwiGLU MLP's tolerance, tests/test_model_gpu.py:17 (TOL), asserted at :96-99
    for a, b in zip(got, [yr, xr.grad] + [t.grad for t in w]):
        assert ((a.detach().cpu().double() - b).norm() / b.norm()).item() < 2e-2
    assert all(torch.equal(a, b) for a, b in zip(got, run(hidden_activation="gelu_pytorch_tanh")[0]))
    assert all(torch.equal(a, b) for a, b in zip(run()[0], run(hidden_act="silu")[0]))
    with pytest.raises(NotImplementedError, match="gelu_pytorch_tanh"):
        run(hidden_act="gelu")
