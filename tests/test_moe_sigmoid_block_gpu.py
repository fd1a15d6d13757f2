"""model.MoE with the sigmoid router on the GPU (H 128, I 128, E 8, k 2, two groups of which one stays,
routed_scaling_factor 2.5, T 128; capacity E / k -- nothing drops -- and dropless; with and without a shared
expert), through its `stages`: the selection against the float64 router of tests/_moe_sigmoid_ref.py, the
output and every compared gradient against the float64 value of its own stage inputs composed from the same
weights, with the bounds of tests/test_moe_block_gpu.py."""
import functools
import types

import pytest
import torch

from tests import _gemm_ref as G
from tests import _moe_ref as R
from tests import _moe_sigmoid_ref as S
from tests.test_moe_block_gpu import _f32_sum_allowance, _gemm

pytestmark = pytest.mark.gpu
DEV, BF, F64 = "cuda", torch.bfloat16, torch.float64
T, H, I, E, KTOP, SCALE, D_AUX, RATE = 128, 128, 128, 8, 2, 2.5, 0.3, 1e-3


@functools.lru_cache(maxsize=None)
def _run(n_shared, dropless):
    from picotron_amd import functional as FN
    from picotron_amd import model as M
    torch.manual_seed(n_shared)
    mlp = M.MoE(types.SimpleNamespace(
        hidden_size=H, intermediate_size=I, num_experts=E, num_experts_per_tok=KTOP, moe_scoring_func="sigmoid", n_group=2,
        topk_group=1, routed_scaling_factor=SCALE, n_shared_experts=n_shared, moe_dropless=dropless,
        moe_capacity_factor=E / KTOP, moe_bias_update_rate=RATE)).to(DEV).to(BF)
    g = R.gen("sigmoid block", n_shared, dropless)
    mlp.e_score_correction_bias.copy_(torch.randn(E, generator=g) * 0.1)
    x, res, dout = (torch.randn(T, H, generator=g).to(BF) for _ in range(3))
    mlp.stages = st = {}
    xd, rd = x.to(DEV).requires_grad_(True), res.to(DEV).requires_grad_(True)
    out = mlp(xd, rd)
    torch.autograd.backward([out, mlp.aux_loss], [dout.to(DEV), torch.tensor(D_AUX, device=DEV)])
    r = dict(mlp=mlp, x=x, res=res, dout=dout, out=out.detach().cpu(), dx=xd.grad.cpu(), dres=rd.grad.cpu(), resin=res,
             st={n: t.cpu() for n, t in st.items()}, bias=mlp.e_score_correction_bias.cpu().clone(), load=mlp.load.cpu().clone())
    if n_shared:   # the shared branch again, alone: the same kernels on the same inputs give the same bits
        sh = mlp.shared_experts
        ws = [torch.nn.Parameter(w.detach().clone()) for w in (sh.gate_proj.weight, sh.up_proj.weight, sh.down_proj.weight)]
        x2 = x.to(DEV).requires_grad_(True)
        FN.MLPFunction.apply(x2, *ws, res.to(DEV)).backward(dout.to(DEV))
        m, (gu, hh) = FN.mlp_block_fwd(x.to(DEV), *ws, FN.TPContext.current(), residual=res.to(DEV))
        r.update(resin=m.cpu(), sh_gu=gu.cpu(), sh_hh=hh.cpu(), sh_dx=x2.grad.cpu(), sh_grads=[w.grad.cpu() for w in ws])
    FN.update_moe_router_bias(mlp)
    return r


@pytest.mark.parametrize("dropless", [False, True])
@pytest.mark.parametrize("n_shared", [0, 1])
def test_forward_and_gradients(n_shared, dropless):
    r = _run(n_shared, dropless)
    st, mlp, x = r["st"], r["mlp"], r["x"]
    _gemm("logits", st["logits"], x, mlp.router.weight.detach().cpu().t(), H)
    idx, gate, s, counts, aux, margin = S.ref_route(st["logits"], r["bias"], KTOP, 2, 1, True, SCALE)
    ok = margin >= S.MARGIN
    assert int((~ok).sum()) <= S.MAX_EXCLUDED * T
    R.check_exact("idx", st["idx"][ok], idx[ok])
    assert bool((st["idx"] // (E // 2) == st["idx"][:, :1] // (E // 2)).all())   # both choices inside one group
    _, gate, s, counts, aux, _ = S.ref_route(st["logits"], r["bias"], KTOP, 2, 1, True, SCALE, idx=st["idx"])
    R.check_exact("counts", st["counts"], counts)
    for name, ref in (("gate", gate), ("probs", s), ("aux", aux)):
        R.check_rel(name, st[name], ref)
    assert torch.equal(r["load"], st["counts"])
    e = int(st["idx"][0, 0])   # one routed expert that has tokens
    rows = slice(int(st["seg"][e]), int(st["seg"][e + 1])) if dropless else slice(e * T, (e + 1) * T)
    w = mlp.experts[e]
    wg, wu, wd = (p.detach().cpu() for p in (w.gate_proj.weight, w.up_proj.weight, w.down_proj.weight))
    _gemm("gate|up", st["gu"][rows], st["xe"][rows], torch.cat([wg, wu]).t(), H)
    _gemm("down", st["ye"][rows], st["hh"][rows], wd.t(), I)
    if n_shared:
        sg, su, sd = (p.detach().cpu() for p in (mlp.shared_experts.gate_proj.weight, mlp.shared_experts.up_proj.weight,
                                                 mlp.shared_experts.down_proj.weight))
        _gemm("shared gate|up", r["sh_gu"], x, torch.cat([sg, su]).t(), H)
        acc, mag = G.ref_product(r["sh_hh"], sd.t())
        G.check("shared down + residual", r["resin"], *G.target_and_bound(acc, mag, I, G.EPI_BF16_RES, residual=r["res"]), tag="moe")
    slot, g64 = st["slot"], st["gate"].to(F64)
    terms = [r["resin"].to(F64)] + [g64[:, j, None] * st["ye"][slot[:, j].long()].to(F64) for j in range(KTOP)]
    assert bool((slot >= 0).all())
    R.check_bf16("out", r["out"], R.ref_combine(st["ye"], slot, st["gate"], r["resin"]), extra=_f32_sum_allowance(terms))
    # backward
    dye, dgate, mag = R.ref_combine_bwd(r["dout"], st["ye"], slot, st["src"], st["gate"])
    R.check_bf16("dye", st["dye"], dye, zero=(st["src"] < 0)[:, None].expand_as(dye))
    R.check_dgate("dgate", st["dgate"], dgate, mag, H, slot < 0)
    ref_dl, allow = S.ref_route_bwd(st["logits"], st["idx"], st["dgate"], D_AUX, True, SCALE, R.F32_TOL)
    R.check_bf16("dlogits", st["dlogits"], ref_dl, extra=allow)
    _gemm("router dW", mlp.router.weight.grad.cpu(), st["dlogits"].t(), x, T)
    n = rows.stop - rows.start
    _gemm("down dW", w.down_proj.weight.grad.cpu(), st["dye"][rows].t(), st["hh"][rows], n)
    _gemm("gate dW", w.gate_proj.weight.grad.cpu(), st["dgu"][rows, :I].t(), st["xe"][rows], n)
    _gemm("up dW", w.up_proj.weight.grad.cpu(), st["dgu"][rows, I:].t(), st["xe"][rows], n)
    assert torch.equal(r["dres"], r["dout"])
    if n_shared:   # dout went down both branches: the shared expert's gradients are the lone run's, dx the two sums
        sh = mlp.shared_experts
        for p, want in zip((sh.gate_proj.weight, sh.up_proj.weight, sh.down_proj.weight), r["sh_grads"]):
            assert torch.equal(p.grad.cpu(), want)
        _gemm("shared down dW", r["sh_grads"][2], r["dout"].t(), r["sh_hh"], T)
        R.check_bf16("dx", r["dx"], st["dh"].to(F64) + r["sh_dx"].to(F64))
    else:
        assert torch.equal(r["dx"], st["dh"])


def test_bias_buffer_dtype_key_and_update():
    r = _run(1, True)
    mlp = r["mlp"]
    assert mlp.e_score_correction_bias.dtype == torch.float32 and mlp.router.weight.dtype == BF
    assert "e_score_correction_bias" in mlp.state_dict() and "load" not in mlp.state_dict()
    lc = r["load"].long()
    step = RATE * torch.sign(lc.sum() - E * lc).to(torch.float32)
    assert torch.equal(mlp.e_score_correction_bias.cpu(), r["bias"] + step) and bool((step.abs() == torch.tensor(RATE)).any())
    assert not bool(mlp.load.any())
