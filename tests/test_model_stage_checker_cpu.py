"""The autograd layer's stage kit (tests/_model_ref.py) tested on itself, without a GPU.

  * the clean emulation of embedding -> decoder layer -> head passes every stage, forward and backward, with
    the dX as a bf16 tensor and as a split-K pair, in both norm modes;
  * every injected wiring fault is rejected at the stage where it was injected, and the failure names that
    role; every stage before it still passes (teacher forcing: the fault does not travel);
  * a missing role is an error, not a skip;
  * the recorder, over a stub kernel module on CPU tensors, records the pre-call contents of in-place
    arguments, the halves of SplitKParts / KPair, and identifies tensors by address, shape and stride.

What the suite's older metric (one norm-relative error < 2e-2 per tensor) makes of each fault on the faulty role
itself, against the clean emulation (1 x 128 tokens, H 256; printed by test_fault_is_rejected_at_its_stage):

    fault                         rejected at   older metric on that role
    dW_gu_x_for_z                 dW_gu         missed (0.0040)
    sink_store_for_accumulate     dW_d          caught (1.00: the prior contents are gone)
    norm_partial_row_missing      dw1           missed (0.0029: 16 of 128 rows, onto a prior gradient)
    pair_half_missing             dW_o          caught (0.98)
    ce_scale_without_inv_count    ce_scale      caught (120)
    ce_stats_of_other_logits      row_lse       at the limit (0.021; no model test compares the LSE)
    dres_omitted                  dz            caught (0.77)
    gqa_kv_head_offset            o             caught (1.44)
"""
import types

import pytest
import torch

from tests import _attn_ref as A
from tests import _gemm_ref as G
from tests import _model_ref as M
from tests import _row_ref as R

BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(autouse=True)
def _leave_the_worst_tables_alone():
    saved = [dict(t) for t in (M.WORST, G.WORST, R.WORST, A.WORST)]
    yield
    for t, s in zip((M.WORST, G.WORST, R.WORST, A.WORST), saved):
        t.clear()
        t.update(s)


@pytest.fixture(scope="module")
def clean():
    c = M.emu_config()
    return c, M.emu_model(c)


def _run(c, layer, head, only=None):
    out = M.check_stages(layer, c, M.layer_stages(c), "emu", only)
    out.update(M.check_stages(head, c, M.HEAD_FWD + M.HEAD_BWD, "emu", only))
    return out


def test_clean_emulation_passes_every_stage(clean):
    c, (layer, head) = clean
    res = _run(c, layer, head)
    want = {"/".join(s.produces) or "dW_qkv" for s in M.layer_stages(c) + M.HEAD_FWD + M.HEAD_BWD}
    assert set(res) == want


@pytest.mark.parametrize("mode,split", [(1, False), (0, True)])
def test_clean_emulation_other_forms(mode, split):
    c = M.emu_config(mode=mode, seed=1)
    layer, head = M.emu_model(c, split_dx=split)
    _run(c, layer, head)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("fault", M.FAULTS)
def test_fault_is_rejected_at_its_stage(clean, fault):
    c, (layer0, head0) = clean
    c2 = M.emu_config()
    layer, head = M.emu_model(c2, fault=fault)
    stage, role = M.FAULT_ROLE[fault]
    stages = M.layer_stages(c2) + M.HEAD_FWD + M.HEAD_BWD
    roles = dict(layer)
    roles.update(head)
    labels = ["/".join(s.produces) or "dW_qkv" for s in stages]
    assert stage in labels
    for st, label in zip(stages, labels):
        if label == stage:
            with pytest.raises(AssertionError) as e:
                M.check_stages(roles, c2, [st], "emu")
            msg = str(e.value)
            assert msg.startswith(f"stage {stage}: ") and role in msg, msg
            print(f"{fault}: {msg[:160]}")
        else:   # teacher forcing: every other stage passes on the faulty run's own values
            M.check_stages(roles, c2, [st], "emu")
    # what one norm-relative error per tensor sees of it
    key = {"dW_gu": "dW_g", "dw1": "dw1", "o": "o"}.get(role, role)
    a, b = roles[key], {**layer0, **head0}[key]
    if isinstance(a, dict):
        a, b = a["got"], b["got"]
    print(f"{fault}: older metric on {key}: {_rel(a.float(), b.float()):.4f}")


def test_missing_role_is_an_error(clean):
    c, (layer, head) = clean
    roles = {k: v for k, v in layer.items() if k != "dW_o"}
    with pytest.raises(AssertionError, match="role 'dW_o': no recorded call produces it"):
        M.check_stages(roles, c, M.layer_stages(c), "emu", only=("dW_o",))


def test_wrong_sink_dtype_is_rejected(clean):
    c, (layer, _) = clean
    roles = dict(layer)
    roles["dW_g"] = dict(layer["dW_g"], got=layer["dW_g"]["got"].to(BF))
    with pytest.raises(AssertionError, match="dW_gu"):
        M.check_stages(roles, c, M.layer_stages(c), "emu", only=("dW_g",))


def test_k_sliced_swiglu_dx(clean):
    """The down dX in K-slices: dh = bf16(the f32 sum of two K halves) passes _s_dgu_sliced although it is not the
    single-pass dh by bits everywhere; a dh from the wrong rows of dout is rejected at dgu."""
    c, (layer, _) = clean
    I, H = c.I, layer["dout"].shape[1]
    p = [G.emu_gemm(layer["dout"][:, lo:lo + H // 2], c.wd[lo:lo + H // 2], G.EPI_F32) for lo in (0, H // 2)]
    dh = (p[0] + p[1]).to(BF)
    gg, uu = layer["gu"][:, :I], layer["gu"][:, I:]
    _, dg, du = R.emu_swiglu(gg, uu, dh)
    roles = dict(layer, dgu=torch.cat([dg, du], 1), dgu_sliced=True)
    M.check_stages(roles, c, M.layer_stages(c), "emu", only=("dgu",))
    _, dg, du = R.emu_swiglu(gg, uu, dh.roll(1, 0))
    with pytest.raises(AssertionError, match="stage dgu: dgu"):
        M.check_stages(dict(roles, dgu=torch.cat([dg, du], 1)), c, M.layer_stages(c), "emu", only=("dgu",))


def test_unpaired_fallback_of_a_pair():
    """A paired group that runs as two launches (store, then accumulate) passes the sequenced bound and can fail
    the single K = 2 T bound; the second half stored over the first is rejected."""
    g = R._gen("unpaired")
    T, N, Kin = 128, 64, 64
    dy1, dy2 = ((torch.randn(T, N, generator=g)).to(BF) for _ in range(2))
    x1, x2 = ((torch.randn(T, Kin, generator=g)).to(BF) for _ in range(2))
    first = G.emu_gemm(dy1.t().contiguous(), x1, G.EPI_BF16)
    got = G.emu_gemm(dy2.t().contiguous(), x2, G.EPI_BF16_ACC, old=first)
    sink = dict(got=got, old=torch.zeros_like(got), epi=G.EPI_BF16, prev=(dy1, x1), unpaired=True)
    M._wgrad("dW", sink, dy2, x2, "emu")
    with pytest.raises(AssertionError, match="dW"):
        M._wgrad("dW", dict(sink, got=G.emu_gemm(dy2.t().contiguous(), x2, G.EPI_BF16)), dy2, x2, "emu")
    one = G.emu_gemm(torch.cat([dy1.t(), dy2.t()], 1).contiguous(), torch.cat([x1, x2]), G.EPI_BF16)
    M._wgrad("dW", dict(sink, got=one, unpaired=False), dy2, x2, "emu")


# ------------------------------------------------------------------------------ the recorder on a stub
class _Parts:
    def __init__(self, p0, p1):
        self.p0, self.p1 = p0, p1


class _KPair:
    def __init__(self, a, b):
        self.a, self.b, self.shape = a, b, (2 * a.shape[0], a.shape[1])


def _stub():
    def rope_(x, n):
        x[:, :n] += 1
        return x

    def attn_bwd(do, q, dq=None, dk=None):
        dq.copy_(do * 2)
        dk.copy_(q + 1)

    def wgrad(dy, x, outs, epilogue=0):
        a, b = (torch.cat([dy.a, dy.b]), torch.cat([x.a, x.b])) if isinstance(dy, _KPair) else (dy, x)
        outs[0] += a.t() @ b
        return outs

    def dgrad(dy, weights, keep_parts=False):
        return _Parts(dy @ weights[0], dy @ weights[0] * 0) if keep_parts else dy @ weights[0]

    return types.SimpleNamespace(rope_=rope_, attn_bwd=attn_bwd, wgrad=wgrad, dgrad=dgrad, KPair=_KPair, EPI=3)


def test_recorder_captures_in_place_arguments_and_halves():
    rec = M.Recorder(_stub())
    assert rec.EPI == 3 and rec.KPair is _KPair          # constants and classes pass through
    x = torch.arange(12.0).reshape(3, 4)
    x0 = x.clone()
    assert rec.rope_(x, 2) is x
    c = rec.calls[0]
    assert c.name == "rope_" and torch.equal(c.arg(0).pre, x0) and torch.equal(c.arg(0).post, x) and c.arg(1) == 2
    assert c.arg(0).key == (x.data_ptr(), (3, 4), (4, 1), F32) and c.result.same(c.arg(0))
    buf = torch.zeros(3, 8)
    buf[:] = 7
    rec.attn_bwd(x, x0, dq=buf[:, :4], dk=buf[:, 4:])
    c = rec.calls[1]
    assert bool((c.kwargs["dq"].pre == 7).all()) and torch.equal(c.kwargs["dq"].post, x * 2)
    assert torch.equal(c.kwargs["dk"].post, x0 + 1)
    assert c.kwargs["dq"].key != c.kwargs["dk"].key and c.kwargs["dq"].key[2] == (8, 1)   # views of one buffer
    w = torch.nn.Parameter(torch.ones(4, 4))
    sink = torch.full((4, 4), 0.5)
    pair = _KPair(x0, x)
    rec.wgrad(pair, _KPair(x0, x0), [sink], epilogue=1)
    c = rec.calls[2]
    assert isinstance(c.arg(0), M.Pair) and torch.equal(c.arg(0)[0].pre, x0) and torch.equal(c.arg(0)[1].pre, x)
    assert bool((c.arg(2)[0].pre == 0.5).all()) and torch.equal(c.arg(2)[0].post, sink) and c.kwargs["epilogue"] == 1
    out = rec.dgrad(x, [w], keep_parts=True)
    c = rec.calls[3]
    assert isinstance(out, _Parts) and isinstance(c.result, M.Parts) and torch.equal(c.result[0].post, x @ w)
    assert c.arg(1)[0].obj is w and c.arg(1)[0].pre.data_ptr() == w.data_ptr()   # a Parameter: by identity, no clone
    assert rec.names() == ["rope_", "attn_bwd", "wgrad", "dgrad"]
    ev = M.sink_events([types.SimpleNamespace(name="linear_wgrad", arg=c2.arg, args=c2.args, kwargs=c2.kwargs)
                        for c2 in rec.calls[2:3]], {sink.data_ptr(): "w"})
    assert list(ev) == ["w"] and ev["w"][0]["epi"] == 1 and bool((ev["w"][0]["old"] == 0.5).all())
    light = M.Recorder(_stub(), clone=False)
    light.rope_(x, 1)
    assert light.names() == ["rope_"] and light.calls[0].args == () and light.calls[0].result == "Tensor"
    assert isinstance(light.dgrad(x, [w], keep_parts=True), _Parts) and light.calls[1].result == "Parts"
