"""tests/_model_ref.py's stage kit, extended to the decoder layer with a mixture-of-experts MLP (a new
helper: the kit itself is unchanged).  The layer is composed of separate autograd nodes
(RMSNormFunction -> AttentionFunction -> AddRMSNormFunction -> MoEFunction), so its roles come from the
same recorded kernel calls the kit reads -- `extract_moe_layer` runs the kit's own extract_attn_fwd /
extract_attn_bwd (document mask, QK-norm and their bit-identity replays included) between the norm
calls -- and the MoE half from the clones MoEFunction leaves in `layer.mlp.stages`, tied to the trace by
bits (the MoE read the h2 the norm wrote; the norm backward read the dh the MoE wrote).

Stages: the kit's LAYER / QK stages up to h2 and from dz on, with two differences the composition makes:
  * the first norm's backward carries no residual gradient (`dx1`); autograd adds the second norm's dz
    to it, bf16(dz + dx1), checked by bits (`dx`);
  * between them the MoE stages below, teacher-forced like the kit's: every reference is computed from
    the production values of the roles the stage reads, under tests/_moe_ref.py's checks (exact
    selection and plan, four times torch's f32 error for the probabilities, one bf16 ulp plus the f32
    accumulation of the terms for the combines, the f32 dot-product bound) and the GEMM kit's bound
    for every product, the experts' and the router's weight gradients through their sinks' epilogues.
"""
import types

import torch

from tests import _gemm_ref as G
from tests import _model_ref as M
from tests import _moe_ref as MO
from tests import _row_ref as R

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
Stage = M.Stage


def _rows(c, e):
    return slice(e * c.C, (e + 1) * c.C)


def _worst(vals):
    return max([float(v) for v in vals] or [0.0])


def _sum_allowance(terms):
    """The f32 accumulation of a combine on real (cancelling) data: one rounding of 2^-24 relative per
    addition, each on a partial sum no larger than sum |terms|."""
    return len(terms) * 2.0 ** -24 * sum(t.abs() for t in terms)


def _gathered(rows, slot, j, weight=None):
    kept = (slot[:, j] >= 0)[:, None]
    v = rows[slot[:, j].clamp_min(0).long()].to(F64)
    if weight is not None:
        v = weight[:, j, None].to(F64) * v
    return torch.where(kept, v, torch.zeros_like(v))


# ------------------------------------------------------------------------------ forward
def _s_logits(r, c, tag):
    return M._gemm("m_logits", r["m_logits"], r["h2"], c.rw.t(), tag)


def _s_route(r, c, tag):
    idx, gate, probs, counts, aux = MO.ref_route(r["m_logits"], c.k, c.norm)
    MO.check_exact("m_idx", r["m_idx"], idx)
    MO.check_exact("m_counts", r["m_counts"], counts)
    return {n: MO.check_rel(n, r[n], ref) / MO.F32_TOL for n, ref in (("m_probs", probs), ("m_gate", gate), ("m_aux", aux))}


def _s_plan(r, c, tag):
    slot, src = MO.ref_plan(r["m_idx"], c.E, c.C)
    MO.check_exact("m_slot", r["m_slot"], slot)
    MO.check_exact("m_src", r["m_src"], src)
    return 0.0


def _s_xe(r, c, tag):
    MO.check_exact("m_xe", r["m_xe"], MO.ref_dispatch(r["h2"], r["m_src"], c.k))
    return 0.0


def _s_gu(r, c, tag):
    return _worst(M._gemm(f"m_gu (expert {e})", r["m_gu"][_rows(c, e)], r["m_xe"][_rows(c, e)],
                          torch.cat([c.wgs[e], c.wus[e]]).t(), tag) for e in range(c.E))


def _s_hh(r, c, tag):
    f = R.ref_swiglu_fwd(r["m_gu"][:, :c.I], r["m_gu"][:, c.I:])
    return R.check("m_hh", r["m_hh"], f["h_ref"], f["h_bound"], tag)


def _s_ye(r, c, tag):
    return _worst(M._gemm(f"m_ye (expert {e})", r["m_ye"][_rows(c, e)], r["m_hh"][_rows(c, e)], c.wds[e].t(), tag)
                  for e in range(c.E))


def _s_out(r, c, tag):
    slot, gate = r["m_slot"], r["m_gate"]
    terms = [r["z"].to(F64)] + [_gathered(r["m_ye"], slot, j, gate) for j in range(c.k)]
    return MO.check_bf16("out", r["out"], MO.ref_combine(r["m_ye"], slot, gate, r["z"]), extra=_sum_allowance(terms))


MOE_FWD = [
    Stage("m_logits", "h2", _s_logits),
    Stage("m_idx m_gate m_probs m_counts m_aux", "m_logits", _s_route),
    Stage("m_slot m_src", "m_idx", _s_plan),
    Stage("m_xe", "h2 m_src", _s_xe),
    Stage("m_gu", "m_xe", _s_gu),
    Stage("m_hh", "m_gu", _s_hh),
    Stage("m_ye", "m_hh", _s_ye),
    Stage("out", "m_ye m_slot m_gate z", _s_out),
]


# ------------------------------------------------------------------------------ backward
def _s_dye(r, c, tag):
    slot, src = r["m_slot"], r["m_src"]
    dye, dgate, mag = MO.ref_combine_bwd(r["dout"], r["m_ye"], slot, src, r["m_gate"])
    return {"dye": MO.check_bf16("m_dye", r["m_dye"], dye, zero=(src < 0)[:, None].expand_as(dye)),
            "dgate": MO.check_dgate("m_dgate", r["m_dgate"], dgate, mag, r["dout"].shape[1], slot < 0)}


def _s_dhh(r, c, tag):
    return _worst(M._gemm(f"m_dhh (expert {e})", r["m_dhh"][_rows(c, e)], r["m_dye"][_rows(c, e)], c.wds[e], tag)
                  for e in range(c.E))


def _s_dgu(r, c, tag):
    f = R.ref_swiglu_bwd(r["m_dhh"], r["m_gu"][:, :c.I], r["m_gu"][:, c.I:])
    return {"dg": R.check("m_dgu (dg)", r["m_dgu"][:, :c.I], f["dg_ref"], f["dg_bound"], tag),
            "du": R.check("m_dgu (du)", r["m_dgu"][:, c.I:], f["du_ref"], f["du_bound"], tag)}


def _s_dxe(r, c, tag):
    return _worst(M._gemm(f"m_dxe (expert {e})", r["m_dxe"][_rows(c, e)], r["m_dgu"][_rows(c, e)],
                          torch.cat([c.wgs[e], c.wus[e]]), tag) for e in range(c.E))


def _s_dW_experts(r, c, tag):
    out = []
    for e in range(c.E):
        rows = _rows(c, e)
        out.append(M._wgrad(f"m_dW_d (expert {e})", r["m_dW_d"][e], r["m_dye"][rows], r["m_hh"][rows], tag))
        out.append(M._wgrad(f"m_dW_g (expert {e})", r["m_dW_g"][e], r["m_dgu"][rows, :c.I], r["m_xe"][rows], tag))
        out.append(M._wgrad(f"m_dW_u (expert {e})", r["m_dW_u"][e], r["m_dgu"][rows, c.I:], r["m_xe"][rows], tag))
    return _worst(out)


def _s_dlogits(r, c, tag):
    ref, p = MO.ref_route_bwd(r["m_logits"], r["m_idx"], r["m_dgate"], c.d_aux, c.norm)
    return MO.check_bf16("m_dlogits", r["m_dlogits"], ref,
                         extra=MO.route_bwd_allowance(p, r["m_idx"], r["m_dgate"], c.d_aux, c.norm))


def _s_dh_router(r, c, tag):
    return M._gemm("m_dh_router", r["m_dh_router"], r["m_dlogits"], c.rw, tag)


def _s_dW_router(r, c, tag):
    return M._wgrad("m_dW_r", r["m_dW_r"], r["m_dlogits"], r["h2"], tag)


def _s_dh2(r, c, tag):
    slot = r["m_slot"]
    terms = [r["m_dh_router"].to(F64)] + [_gathered(r["m_dxe"], slot, j) for j in range(c.k)]
    return MO.check_bf16("dh2", r["dh2"], MO.ref_combine(r["m_dxe"], slot, None, r["m_dh_router"]),
                         extra=_sum_allowance(terms))


def _s_dx1(r, c, tag):
    f = R.ref_norm_bwd(M.parts_bf16(r["dh1"]), r["x"], c.w1, r["rstd1"], None, c.mode)
    out = {"dx1": R.check("dx1", r["dx1"], f["dx_ref"], f["dx_bound"], tag)}
    if c.w1_grad:
        out["dw1"] = M._norm_dw("dw1", r["dw1"], f, tag)
    return out


def _s_dx(r, c, tag):
    MO.check_exact("dx", r["dx"], (r["dz"].to(F32) + r["dx1"].to(F32)).to(BF))   # autograd's bf16 add of the two paths
    return 0.0


MOE_BWD = [
    Stage("m_dye m_dgate", "dout m_ye m_slot m_src m_gate", _s_dye),
    Stage("m_dhh", "m_dye", _s_dhh),
    Stage("m_dgu", "m_dhh m_gu", _s_dgu),
    Stage("m_dxe", "m_dgu", _s_dxe),
    Stage("m_dW_d m_dW_g m_dW_u", "m_dye m_hh m_dgu m_xe", _s_dW_experts),
    Stage("m_dlogits", "m_dgate m_logits m_idx", _s_dlogits),
    Stage("m_dh_router", "m_dlogits", _s_dh_router),
    Stage("m_dW_r", "m_dlogits h2", _s_dW_router),
    Stage("dh2", "m_dxe m_dh_router m_slot", _s_dh2),
]
_MLP_FWD = ("gu", "hh", "out")
_MLP_BWD = ("dhh", "dgu", "dW_d", "dh2", "dW_g")


def moe_layer_stages(c):
    """The kit's stages of the layer (QK-norm or not) with the dense MLP's replaced by the MoE's, and the
    last norm backward split into its own stage and autograd's add."""
    qk = c.wqn is not None
    fwd = [s for s in (M.QK_FWD if qk else M.LAYER_FWD) if s.produces[0] not in _MLP_FWD] + MOE_FWD
    bwd = MOE_BWD + [s for s in (M.QK_BWD if qk else M.LAYER_BWD)
                     if (s.produces[0] if s.produces else "") not in _MLP_BWD + ("dx",)]
    return fwd + bwd + [Stage("dx1", "dh1 x rstd1", _s_dx1), Stage("dx", "dz dx1", _s_dx)]


# ------------------------------------------------------------------------------ extraction
def moe_layer_config(layer, B, S, mask=None, d_aux=0.0):
    """M.layer_config for a layer whose mlp is a model.MoE."""
    at, mlp, n1 = layer.attention, layer.mlp, layer.input_layernorm
    flash = hasattr(n1, "eps")
    w = M.cpu
    T = B * S
    from picotron_amd import kernels as K
    return types.SimpleNamespace(
        B=B, S=S, nh=at.num_local_heads, nkv=at.num_local_kv_heads, d=at.head_dim,
        I=mlp.experts[0].gate_proj.weight.shape[0], E=mlp.num_experts, k=mlp.top_k, norm=mlp.norm_topk_prob,
        C=K.moe_capacity(T, mlp.num_experts, mlp.top_k, mlp.capacity_factor), d_aux=d_aux,
        eps=n1.eps if flash else n1.variance_epsilon, mode=0 if flash else 1, mask=mask,
        w1=w(n1.weight), w2=w(layer.post_attention_layernorm.weight), wq=w(at.q_proj.weight), wk=w(at.k_proj.weight),
        wv=w(at.v_proj.weight), wo=w(at.out_proj.weight), rw=w(mlp.router.weight),
        wgs=[w(e.gate_proj.weight) for e in mlp.experts], wus=[w(e.up_proj.weight) for e in mlp.experts],
        wds=[w(e.down_proj.weight) for e in mlp.experts], cos=w(layer.cos)[:S].to(BF), sin=w(layer.sin)[:S].to(BF),
        w1_grad=True, w2_grad=True, qkv_grad=True,
        wqn=w(at.q_norm.weight) if at.qk_norm else None, wkn=w(at.k_norm.weight) if at.qk_norm else None)


def extract_moe_layer(K, layer, calls, c, y, x_grad):
    """Every role of one recorded forward + backward of the layer.  y: the layer's output, x_grad: the
    gradient autograd left on its input.  The parameters' gradients must be fresh (.grad was None)."""
    at, mlp = layer.attention, layer.mlp
    st = {n: M.cpu(t) for n, t in mlp.stages.items()}
    params = dict(w1=layer.input_layernorm.weight, w2=layer.post_attention_layernorm.weight, wq=at.q_proj.weight,
                  wk=at.k_proj.weight, wv=at.v_proj.weight, wo=at.out_proj.weight, rw=mlp.router.weight)
    if at.qk_norm:
        params.update(wqn=at.q_norm.weight, wkn=at.k_norm.weight)
    for e, ex in enumerate(mlp.experts):
        params.update({f"wg{e}": ex.gate_proj.weight, f"wu{e}": ex.up_proj.weight, f"wd{e}": ex.down_proj.weight})
    sinks = {p.grad.data_ptr(): n for n, p in params.items()}
    names = {n: n for n in params}
    wev, nev = M.sink_events(calls, sinks), M.norm_sink_events(calls, sinks)
    cur, r = M.Cursor(calls), {}
    # forward: norm1, the attention block (the kit's extraction), norm2, then the MoE's own stages
    n1 = cur.next("rmsnorm_fwd", lambda k: M._is(k.arg(1), params["w1"]) and k.kwargs.get("residual") is None, "h1")
    r["x"], r["h1"], r["rstd1"] = M.cpu(n1.arg(0).pre), M.cpu(n1.result[0].post), M.cpu(n1.result[1].post)
    M.extract_attn_fwd(K, layer, cur, c, r, n1.result[0].post)
    n2 = cur.next("rmsnorm_fwd", lambda k: M._is(k.arg(1), params["w2"]) and k.kwargs.get("residual") is not None, "h2")
    r["h2"], r["rstd2"], r["z"] = (M.cpu(t.post) for t in n2.result)
    M._bits_equal("the MoE reads the second norm's output", st["h2"], r["h2"])
    for n in ("logits", "idx", "gate", "probs", "counts", "aux", "slot", "src", "xe", "gu", "hh", "ye",
              "dye", "dgate", "dhh", "dgu", "dxe", "dlogits", "dh_router"):
        r["m_" + n] = st[n]
    r["out"] = M.cpu(y).reshape(c.B * c.S, -1)
    M._bits_equal("the layer returns the MoE's combine", st["out"], r["out"])
    # backward: the MoE, norm2, the attention block (the kit's extraction), norm1, autograd's add
    start = cur.at
    cb = cur.next("moe_combine_bwd", None, "m_dye")
    r["dout"] = M.cpu(cb.arg(0).pre)
    r["dh2"] = st["dh"]
    for e in range(c.E):
        for role, nm in (("m_dW_d", "wd"), ("m_dW_g", "wg"), ("m_dW_u", "wu")):
            r.setdefault(role, []).append(M._sink_role(M._wsink(wev, f"{nm}{e}", start, role)))
    r["m_dW_r"] = M._sink_role(M._wsink(wev, "rw", start, "m_dW_r"))
    n2b = cur.next("rmsnorm_bwd", lambda k: M._is(k.arg(2), params["w2"]), "dz")
    M._bits_equal("the second norm's backward reads the MoE's dX", n2b.arg(0).pre, st["dh"])
    r["dz"] = M.cpu(n2b.result[0].post)
    r["dw2"] = M._norm_sink(nev, "w2", n2b.result[1] if n2b.kwargs.get("defer_dw") else None, start, "dw2")
    M.extract_attn_bwd(K, layer, names, cur, c, r, wev, nev, start)
    n1b = cur.next("rmsnorm_bwd", lambda k: M._is(k.arg(2), params["w1"]), "dx1")
    assert n1b.kwargs.get("dres") is None, "the first norm's backward of the composed layer carries no residual gradient"
    r["dx1"] = M.cpu(n1b.result[0].post)
    r["dw1"] = M._norm_sink(nev, "w1", n1b.result[1] if n1b.kwargs.get("defer_dw") else None, start, "dw1")
    r["dx"] = M.cpu(x_grad).reshape(c.B * c.S, -1)
    return r
