"""The MoE stages of tests/_moe_stage_ref.py check themselves (CPU): they accept an fp32 / float64
emulation of the MoE block rounded where the HIP path stores, and reject wiring faults at the role
where they happen.  (Like its sibling checker self-tests, this file exercises test helpers only, so it
passes with or without the feature.)"""
import types

import pytest
import torch

from tests import _gemm_ref as G
from tests import _model_ref as M
from tests import _moe_ref as MO
from tests import _moe_stage_ref as MS
from tests import _row_ref as R

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
T, H, I, E, KTOP, C = 128, 64, 64, 4, 2, 64
FAULTS = (None, "dispatch_wrong_token", "gate_unnormalised", "residual_dropped", "dW_up_reads_h2", "dx_of_dropped_kept",
          "aux_gradient_dropped", "router_dx_dropped")
ROLE = {"dispatch_wrong_token": "m_xe", "gate_unnormalised": "m_idx", "residual_dropped": "out", "dW_up_reads_h2": "m_dW_d",
        "dx_of_dropped_kept": "dh2", "aux_gradient_dropped": "m_dlogits", "router_dx_dropped": "dh2"}


def _bf(x):
    return x.to(F32).to(BF)


def _mm(a, b):
    return _bf(a.to(F64) @ b.to(F64))


def emu(fault=None):
    g = MO.gen("moe stage emu")
    mk = lambda r, c: _bf((torch.rand(r, c, generator=g) * 2 - 1) / c ** 0.5)   # noqa: E731
    c = types.SimpleNamespace(E=E, k=KTOP, C=C, I=I, norm=True, d_aux=0.4, rw=_bf(torch.randn(E, H, generator=g) * 0.3),
                              wgs=[mk(I, H) for _ in range(E)], wus=[mk(I, H) for _ in range(E)],
                              wds=[mk(H, I) for _ in range(E)])
    c.rw[0] += 0.2   # expert 0 is popular: more items than C, so some are dropped
    r = {"h2": _bf(torch.randn(T, H, generator=g)), "z": _bf(torch.randn(T, H, generator=g)),
         "dout": _bf(torch.randn(T, H, generator=g))}
    r["m_logits"] = _mm(r["h2"], c.rw.t())
    idx, gate, probs, counts, aux = MO.ref_route(r["m_logits"], KTOP, fault != "gate_unnormalised")
    r.update(m_idx=idx, m_gate=gate.to(F32), m_probs=probs.to(F32), m_counts=counts, m_aux=aux.to(F32))
    slot, src = MO.ref_plan(idx, E, C)
    assert bool((slot < 0).any())
    r.update(m_slot=slot, m_src=src)
    r["m_xe"] = MO.ref_dispatch(r["h2"].roll(1, 0) if fault == "dispatch_wrong_token" else r["h2"], src, KTOP)
    rows = [slice(e * C, (e + 1) * C) for e in range(E)]
    r["m_gu"] = torch.cat([_mm(r["m_xe"][rw], torch.cat([c.wgs[e], c.wus[e]]).t()) for e, rw in enumerate(rows)])
    r["m_hh"] = R.emu_swiglu(r["m_gu"][:, :I], r["m_gu"][:, I:], torch.zeros(E * C, I))[0]
    r["m_ye"] = torch.cat([_mm(r["m_hh"][rw], c.wds[e].t()) for e, rw in enumerate(rows)])
    r["out"] = _bf(MO.ref_combine(r["m_ye"], slot, r["m_gate"], None if fault == "residual_dropped" else r["z"]))
    dye, dgate, _ = MO.ref_combine_bwd(r["dout"], r["m_ye"], slot, src, r["m_gate"])
    r.update(m_dye=_bf(dye), m_dgate=dgate.to(F32))
    r["m_dhh"] = torch.cat([_mm(r["m_dye"][rw], c.wds[e]) for e, rw in enumerate(rows)])
    _, dg, du = R.emu_swiglu(r["m_gu"][:, :I], r["m_gu"][:, I:], r["m_dhh"])
    r["m_dgu"] = torch.cat([dg, du], 1)
    r["m_dxe"] = torch.cat([_mm(r["m_dgu"][rw], torch.cat([c.wgs[e], c.wus[e]])) for e, rw in enumerate(rows)])
    sink = lambda dy, x: dict(got=_mm(dy.t(), x), old=None, epi=G.EPI_BF16)   # noqa: E731
    r["m_dW_d"] = [sink(r["m_dye"][rw], r["h2"][:C] if fault == "dW_up_reads_h2" else r["m_hh"][rw]) for rw in rows]
    r["m_dW_g"] = [sink(r["m_dgu"][rw, :I], r["m_xe"][rw]) for rw in rows]
    r["m_dW_u"] = [sink(r["m_dgu"][rw, I:], r["m_xe"][rw]) for rw in rows]
    dl, _ = MO.ref_route_bwd(r["m_logits"], idx, r["m_dgate"], 0.0 if fault == "aux_gradient_dropped" else c.d_aux, True)
    r["m_dlogits"] = _bf(dl)
    r["m_dh_router"] = _mm(r["m_dlogits"], c.rw)
    r["m_dW_r"] = sink(r["m_dlogits"], r["h2"])
    r["dh2"] = _bf(MO.ref_combine(r["m_dxe"], slot.clamp_min(0) if fault == "dx_of_dropped_kept" else slot, None,
                                  None if fault == "router_dx_dropped" else r["m_dh_router"]))
    return r, c


@pytest.mark.parametrize("fault", FAULTS)
def test_moe_stages_accept_the_emulation_and_reject_faults(fault):
    r, c = emu(fault)
    stages = MS.MOE_FWD + MS.MOE_BWD
    if fault is None:
        res = M.check_stages(r, c, stages, "emu")
        assert set(res) == {"/".join(s.produces) for s in stages}
        return
    with pytest.raises(AssertionError, match=f"stage [^:]*{ROLE[fault]}"):
        M.check_stages(r, c, stages, "emu " + fault)


def test_a_missing_role_is_an_error_and_the_layer_stage_list_is_complete():
    r, c = emu()
    del r["m_dxe"]
    with pytest.raises(AssertionError, match="m_dxe"):
        M.check_stages(r, c, MS.MOE_FWD + MS.MOE_BWD, "emu")
    for qk in (None, 1):
        labels = ["/".join(s.produces) or "dW_qkv" for s in MS.moe_layer_stages(types.SimpleNamespace(wqn=qk))]
        assert len(labels) == len(set(labels))
        assert not {"gu", "hh", "dhh", "dgu", "dW_d", "dW_g/dW_u"} & set(labels)          # the dense MLP's stages are out
        assert {"h1/rstd1", "o/lse", "a", "z/h2/rstd2", "out", "dh2", "dz", "do", "dW_o", "dh1", "dW_qkv", "dx1", "dx"} <= set(labels)
        assert ("qk_normed/rstd_qk" in labels) == (qk is not None) and ("dqkv" in labels) == (qk is not None)
        assert labels.index("out") < labels.index("m_dye/m_dgate") < labels.index("dh2") < labels.index("dz") < labels.index("dx")
