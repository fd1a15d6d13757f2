"""functional.MoEFunction on the GPU, stage by stage through its `stages=` dict: every routing stage
against tests/_moe_ref.py on that stage's own inputs, every GEMM stage against the float64 product of
its own bf16 inputs with tests/_gemm_ref.py's per-element rule, every expert's and the router's
.grad against the float64 gradient of its own stage inputs, an unused expert's gradient exactly zero,
E = 1 beside the dense MLPFunction, the epilogue-fused form beside the unfused one, and bit-identical
repeats.

Shapes: T = 192, H = 128, I = 128, E = 8, k = 2, capacity_factor 1.0 (C = 64: drops) and 4.0
(C = 192: dropless).  Expert 5 is never chosen (its router row answers a constant feature of x with
-32) and expert 2 by most tokens (+2), which overflows C = 64."""
import functools

import pytest
import torch

from tests import _gemm_ref as G
from tests import _moe_ref as R

DEV = "cuda"
pytestmark = pytest.mark.gpu
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
T, H, I, E, KTOP, DEAD = 192, 128, 128, 8, 2, 5
D_AUX = 0.3


def _weights(E_, H_, I_, seed=0):
    g = R.gen("moe block weights", E_, H_, I_, seed)
    rw = (torch.randn(E_, H_, generator=g) * 0.05)
    rw[:, 0] = 0.0
    if E_ > DEAD:
        rw[DEAD, 0] = -8.0
        rw[2, 0] = 0.5   # ... and expert 2 with +2: most tokens choose it, more than C = 64 holds
    mk = lambda r, c: ((torch.rand(r, c, generator=g) * 2 - 1) / c ** 0.5).to(BF)
    return rw.to(BF), [mk(I_, H_) for _ in range(E_)], [mk(I_, H_) for _ in range(E_)], [mk(H_, I_) for _ in range(E_)]


def _inputs(T_, H_, seed=0):
    g = R.gen("moe block inputs", T_, H_, seed)
    x = torch.randn(T_, H_, generator=g)
    x[:, 0] = 4.0
    return x.to(BF), torch.randn(T_, H_, generator=g).to(BF), torch.randn(T_, H_, generator=g).to(BF)


def _run(T_, H_, I_, E_, k, cf, norm=True, seed=0, d_aux=D_AUX):
    """One forward + backward of MoEFunction on fresh parameters; everything on the CPU."""
    from picotron_amd import functional as FN
    rw, wgs, wus, wds = _weights(E_, H_, I_, seed)
    x, res, dout = _inputs(T_, H_, seed)
    P = lambda t: torch.nn.Parameter(t.to(DEV))
    prw, pg, pu, pd = P(rw), [P(w) for w in wgs], [P(w) for w in wus], [P(w) for w in wds]
    xd, rd = x.to(DEV).requires_grad_(True), res.to(DEV).requires_grad_(True)
    stages = {}
    out, aux = FN.MoEFunction.apply(xd, rd, prw, pg, pu, pd, k, cf, norm, stages)
    torch.autograd.backward([out, aux], [dout.to(DEV), torch.tensor(d_aux, dtype=F32, device=DEV)])
    c = lambda t: t.detach().cpu()
    return dict(x=x, res=res, dout=dout, rw=rw, wgs=wgs, wus=wus, wds=wds, out=c(out), aux=c(aux), dx=c(xd.grad),
                dres=c(rd.grad), g_rw=c(prw.grad), g_wg=[c(p.grad) for p in pg], g_wu=[c(p.grad) for p in pu],
                g_wd=[c(p.grad) for p in pd], st={n: c(t) for n, t in stages.items()})


@functools.lru_cache(maxsize=None)
def _case(cf):
    return _run(T, H, I, E, KTOP, cf)


def _gemm(name, got, a, b, K_):
    """got = bf16(a [M, K] . b [K, N]) by _gemm_ref's per-element rule."""
    acc, S = G.ref_product(a, b)
    t, bound = G.target_and_bound(acc, S, K_, G.EPI_BF16)
    assert got.dtype == BF
    return G.check(name, got, t, bound, tag="moe")


def _f32_sum_allowance(terms):
    """The f32 accumulation of a combine on real (cancelling) data: at most one rounding of 2^-24
    relative per addition, each on a partial sum no larger than sum |terms|."""
    return len(terms) * 2.0 ** -24 * sum(t.abs() for t in terms)


@pytest.mark.parametrize("cf", [1.0, 4.0])
def test_forward_stages(cf):
    from picotron_amd import kernels as K
    r = _case(cf)
    st = r["st"]
    C = K.moe_capacity(T, E, KTOP, cf)
    assert C == (64 if cf == 1.0 else 192)
    _gemm("logits", st["logits"], r["x"], r["rw"].t(), H)
    idx, gate, probs, counts, aux = R.ref_route(st["logits"], KTOP, True)
    R.check_exact("idx", st["idx"], idx)
    R.check_exact("counts", st["counts"], counts)
    R.check_rel("probs", st["probs"], probs)
    R.check_rel("gate", st["gate"], gate)
    R.check_rel("aux", st["aux"], aux)
    assert torch.equal(r["aux"], st["aux"].reshape(()))
    assert int(counts[DEAD]) == 0
    slot, src = R.ref_plan(idx, E, C)
    R.check_exact("slot", st["slot"], slot)
    R.check_exact("src", st["src"], src)
    assert bool((slot < 0).any()) == (cf == 1.0)   # C = 64 drops, C = ceil64(T) cannot
    R.check_exact("xe", st["xe"], R.ref_dispatch(r["x"], src, KTOP))
    for e in range(E):
        rows = slice(e * C, (e + 1) * C)
        _gemm(f"gate|up e{e}", st["gu"][rows], st["xe"][rows], torch.cat([r["wgs"][e], r["wus"][e]]).t(), H)
        _gemm(f"down e{e}", st["ye"][rows], st["hh"][rows], r["wds"][e].t(), I)
    gu = st["gu"].to(DEV)
    assert torch.equal(K.swiglu_fwd(gu[:, :I], gu[:, I:]).cpu(), st["hh"])   # the row kernel has its own conformance test
    g64 = st["gate"].to(F64)
    terms = [r["res"].to(F64)] + [torch.where((slot[:, j] >= 0)[:, None], g64[:, j, None] * st["ye"][slot[:, j].clamp_min(0).long()].to(F64),
                                              torch.zeros(T, H, dtype=F64)) for j in range(KTOP)]
    R.check_bf16("out", st["out"], R.ref_combine(st["ye"], slot, st["gate"], r["res"]), extra=_f32_sum_allowance(terms))
    assert torch.equal(r["out"], st["out"])


@pytest.mark.parametrize("cf", [1.0, 4.0])
def test_backward_stages_and_gradients(cf):
    from picotron_amd import kernels as K
    r = _case(cf)
    st = r["st"]
    C = K.moe_capacity(T, E, KTOP, cf)
    slot, src, gate = st["slot"], st["src"], st["gate"]
    dye, dgate, mag = R.ref_combine_bwd(r["dout"], st["ye"], slot, src, gate)
    R.check_bf16("dye", st["dye"], dye, zero=(src < 0)[:, None].expand_as(dye))
    R.check_dgate("dgate", st["dgate"], dgate, mag, H, slot < 0)
    assert torch.equal(r["dres"], r["dout"])   # the residual's gradient is dout itself
    gu = st["gu"].to(DEV)
    dgu_again = K.swiglu_bwd(st["dhh"].to(DEV), gu[:, :I], gu[:, I:])
    assert torch.equal(torch.cat([t.cpu() for t in dgu_again], 1), st["dgu"])
    for e in range(E):
        rows = slice(e * C, (e + 1) * C)
        _gemm(f"down dX e{e}", st["dhh"][rows], st["dye"][rows], r["wds"][e], H)
        _gemm(f"gate|up dX e{e}", st["dxe"][rows], st["dgu"][rows], torch.cat([r["wgs"][e], r["wus"][e]]), 2 * I)
        # every expert's gradient against the float64 gradient of its own stage inputs
        _gemm(f"down dW e{e}", r["g_wd"][e], st["dye"][rows].t(), st["hh"][rows], C)
        _gemm(f"gate dW e{e}", r["g_wg"][e], st["dgu"][rows, :I].t(), st["xe"][rows], C)
        _gemm(f"up dW e{e}", r["g_wu"][e], st["dgu"][rows, I:].t(), st["xe"][rows], C)
    for g in (r["g_wd"][DEAD], r["g_wg"][DEAD], r["g_wu"][DEAD]):   # no token: exactly zero
        assert bool((g == 0).all())
    assert bool((st["xe"][DEAD * C:(DEAD + 1) * C].view(torch.int16) == 0).all())
    ref, p = R.ref_route_bwd(st["logits"], st["idx"], st["dgate"], D_AUX, True)
    R.check_bf16("dlogits", st["dlogits"], ref, extra=R.route_bwd_allowance(p, st["idx"], st["dgate"], D_AUX, True))
    _gemm("router dX", st["dh_router"], st["dlogits"], r["rw"], E)
    _gemm("router dW", r["g_rw"], st["dlogits"].t(), r["x"], T)
    terms = [st["dh_router"].to(F64)] + [torch.where((slot[:, j] >= 0)[:, None], st["dxe"][slot[:, j].clamp_min(0).long()].to(F64),
                                                     torch.zeros(T, H, dtype=F64)) for j in range(KTOP)]
    R.check_bf16("dh", st["dh"], R.ref_combine(st["dxe"], slot, None, st["dh_router"]), extra=_f32_sum_allowance(terms))
    assert torch.equal(r["dx"], st["dh"])


def test_one_expert_beside_the_dense_mlp():
    """E = 1, k = 1, capacity_factor 1 (C = T: nothing dropped, gate exactly 1) computes the dense
    MLP block.  Both paths store bf16 gate|up, swiglu and down-projection values and add the residual
    to the bf16 down projection -- the MoE in its combine, MLPFunction after it -- so the common
    float64 value is residual + float64(the stored down projection) (its gradient: the two stored dX
    parts), and each result lies within one bf16 ulp of it."""
    from picotron_amd import functional as FN
    r = _run(T, H, I, 1, 1, 1.0, d_aux=0.0)
    st = r["st"]
    assert bool((st["gate"] == 1.0).all()) and bool((st["slot"].flatten() == torch.arange(T)).all())
    P = lambda t: torch.nn.Parameter(t.to(DEV))
    wg, wu, wd = P(r["wgs"][0]), P(r["wus"][0]), P(r["wds"][0])
    xd = r["x"].to(DEV).requires_grad_(True)
    m = FN.MLPFunction.apply(xd, wg, wu, wd)
    dense = FN.K.residual_add(m.detach().contiguous(), r["res"].to(DEV)).cpu()
    m.backward(r["dout"].to(DEV))
    common = r["res"].to(F64) + st["ye"].to(F64)
    R.check_bf16("moe out", r["out"], common)
    R.check_bf16("dense out", dense, common)
    # the router's dX of one expert is exactly zero (a softmax over one logit), so dx = dxe
    assert bool((st["dlogits"] == 0).all())
    R.check_bf16("moe dx", r["dx"], st["dxe"].to(F64))
    R.check_bf16("dense dx", xd.grad.cpu(), st["dxe"].to(F64))


def test_two_identical_calls_give_identical_bits():
    a, b = _run(T, H, I, E, KTOP, 1.0, seed=3), _run(T, H, I, E, KTOP, 1.0, seed=3)
    for key in ("out", "aux", "dx", "dres", "g_rw"):
        assert torch.equal(a[key], b[key]), key
    for key in ("g_wg", "g_wu", "g_wd"):
        for x, y in zip(a[key], b[key]):
            assert torch.equal(x, y), key
    for n in a["st"]:
        assert torch.equal(a["st"][n].view(torch.int16) if a["st"][n].dtype == BF else a["st"][n],
                           b["st"][n].view(torch.int16) if b["st"][n].dtype == BF else b["st"][n]), n


def test_fused_swiglu_form_matches_the_unfused_one():
    """C = 256, I = 256 tile for the SwiGLU epilogues of the grouped expert GEMMs; switch `fuse` = 0
    runs the plain GEMMs with one strided SwiGLU call over the whole buffer.  Same bits, as for the
    dense MLP's two forms."""
    from picotron_amd import kernels as K
    from picotron_amd import switches
    assert K.moe_capacity(512, 2, 1, 1.0) == 256 and K.swiglu_fusable(256, 256, backward=True, H=128)
    fused = _run(512, 128, 256, 2, 1, 1.0, seed=7)
    with switches.override(fuse=0):
        plain = _run(512, 128, 256, 2, 1, 1.0, seed=7)
    assert "dhh" in plain["st"] and "dhh" not in fused["st"]   # the two forms did run
    for key in ("out", "dx", "g_rw"):
        assert torch.equal(fused[key], plain[key]), key
    for key in ("g_wg", "g_wu", "g_wd"):
        for x, y in zip(fused[key], plain[key]):
            assert torch.equal(x, y), key
    for n in ("gu", "hh", "ye", "dgu", "dxe"):
        assert torch.equal(fused["st"][n], plain["st"][n]), n
