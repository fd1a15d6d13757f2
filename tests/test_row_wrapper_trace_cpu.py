"""The native calls the cross-entropy and RMSNorm wrappers of picotron_amd.kernels make, pinned without a GPU.

The recorder of tests/test_launch_trace_cpu.py stands in for the library; the status word is a CPU int32
tensor of the case (input 0) and kernels._status_posted is recorded as an event, as that file stubs the
stream.  Every CE wrapper runs at z_loss 0 and 0.25 and at reductions mean / sum / none where it has
one, rmsnorm_fwd with and without the residual, rmsnorm_bwd plain, from SplitKParts and with defer_dw.
Pinned: each call's entry point, every argument's value (pointers by the tensor they fall in; "fresh"
for a tensor an op made, such as inv_count), and the shapes, strides and dtypes returned.
tests/golden/row_wrapper_trace.json was written before the wrappers' shared helpers existed and is not
regenerated when the code changes (`python -m tests.test_row_wrapper_trace_cpu` writes it)."""
import json
import os

import pytest
import torch

from picotron_amd import _C
from picotron_amd import kernels as K
from tests.test_launch_trace_cpu import Trace, _TorchProxy, _bf16_rowmajor_host

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_wrapper_trace.json")
ROWS, V, NBLK, TP, NPARTS = 16, 64, 2, 2, 8
BF16, F32, I64 = torch.bfloat16, torch.float32, torch.int64
ZS = (0.0, 0.25)
REDUCTIONS = ("mean", "sum", "none")


class RowTrace(Trace):
    def ptr(self, v, strict=False):   # inv_count of the fused forms is made by torch ops, not by torch.empty
        return super().ptr(v, strict=False)


CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def _logits(tr):
    return tr.new(ROWS, V), tr.own(torch.zeros(ROWS, dtype=I64))


@case
def ce_fwd_bwd(tr):
    x, t = _logits(tr)
    for z in ZS:
        for inplace in (True, False):
            tr.note("z", z, "inplace", inplace)
            tr.call(K.cross_entropy_fwd_bwd, x, t, scale=0.5, ignore_index=-1, inplace=inplace, z_loss=z)


@case
def ce_loss_and_grad(tr):
    x, t = _logits(tr)
    tr.call(K.cross_entropy_loss, x, t, ignore_index=-1)
    tr.call(K.cross_entropy_grad, x, t, tr.new(1, dtype=F32))


@case
def ce_loss_lse(tr):
    x, t = _logits(tr)
    for z in ZS:
        for red in REDUCTIONS:
            tr.note("z", z, red)
            tr.call(K.cross_entropy_loss_lse, x, t, reduction=red, z_loss=z)
        tr.call(K.cross_entropy_loss_lse, x, t, ignore_index=-1, out_dtype=BF16, z_loss=z)
        tr.call(K.cross_entropy_loss_lse, x, t, out_dtype=BF16, reduction="none", z_loss=z)


@case
def ce_grad_lse(tr):
    x, t = _logits(tr)
    lse = tr.new(ROWS, dtype=F32)
    for z in ZS:
        for n in (1, ROWS):
            tr.note("z", z, "scale", n)
            tr.call(K.cross_entropy_grad_lse, x, t, lse, tr.new(n, dtype=F32), ignore_index=-1, z_loss=z)
            tr.call(K.cross_entropy_grad_lse_shard, x, t, lse, tr.new(n, dtype=F32), 128, z_loss=z)


@case
def ce_loss_lse_stats(tr):
    x, t = _logits(tr)
    stats = tr.new(NBLK, ROWS, 2, dtype=F32)
    for z in ZS:
        for red in REDUCTIONS:
            tr.note("z", z, red)
            tr.call(K.cross_entropy_loss_lse_stats, x, t, stats, ignore_index=-1, reduction=red, z_loss=z)


@case
def ce_vocab_parallel(tr):
    x, t = _logits(tr)
    tr.call(K.cross_entropy_vp_partial, x, t, tr.new(NBLK, ROWS, 2, dtype=F32), 128)
    parts = tr.new(TP, ROWS, 4, dtype=F32)
    for z in ZS:
        for red in REDUCTIONS:
            tr.note("z", z, red)
            tr.call(K.cross_entropy_vp_combine, parts, t, TP * V, reduction=red, z_loss=z)
        tr.call(K.cross_entropy_vp_combine, parts, t, TP * V, ignore_index=-1, out_dtype=BF16, z_loss=z)


@case
def rmsnorm(tr):
    x, w = tr.new(ROWS, V), tr.new(V)
    tr.call(K.rmsnorm_fwd, x, w, 1e-5)
    tr.call(K.rmsnorm_fwd, x, w, 1e-5, K.MODE_LLAMA, residual=tr.new(ROWS, V))
    dy, rstd, dres = tr.new(ROWS, V), tr.new(ROWS, dtype=F32), tr.new(ROWS, V)
    split = K.SplitKParts(tr.new(ROWS, V, dtype=F32), tr.new(ROWS, V, dtype=F32))
    for name, d in (("plain", dy), ("split", split)):
        tr.note(name)
        tr.rcs["pt_rmsnorm_bwd_partials"] = [NPARTS] * 4
        tr.call(K.rmsnorm_bwd, d, x, w, rstd)
        tr.call(K.rmsnorm_bwd, d, x, w, rstd, K.MODE_LLAMA, dres=dres, dw_out=tr.new(V), dw_sink=K.DW_ACC_BF16)
        tr.call(K.rmsnorm_bwd, d, x, w, rstd, dres=dres, dw_out=tr.new(V, dtype=F32), dw_sink=K.DW_ACC_F32)
        tr.call(K.rmsnorm_bwd, d, x, w, rstd, dw_out=tr.new(V), dw_sink=K.DW_ACC_BF16, defer_dw=True)
    tr.note("the width is refused")
    tr.rcs["pt_rmsnorm_bwd_partials"] = [-3]
    with pytest.raises(_C.HipKernelError, match="pt_rmsnorm_bwd_partials"):
        K.rmsnorm_bwd(dy, x, w, rstd)


def run_case(name, monkeypatch):
    tr = RowTrace()
    status = tr.own(torch.zeros(1, dtype=torch.int32))   # input 0 of every case
    monkeypatch.setattr(_C, "lib", lambda: tr)
    monkeypatch.setattr(_C, "stream_ptr", lambda device=None: None)
    monkeypatch.setattr(K, "_bf16_rowmajor", _bf16_rowmajor_host)
    monkeypatch.setattr(K, "status_word", lambda device: status)
    monkeypatch.setattr(K, "_status_posted", lambda device: tr.note("status_posted"))
    monkeypatch.setattr(K, "torch", _TorchProxy(tr))
    CASES[name](tr)
    return json.loads(json.dumps(tr.events))


def _load():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_holds_exactly_the_cases():
    assert sorted(_load()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_row_wrapper_trace(name, monkeypatch):
    got, want = run_case(name, monkeypatch), _load()[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: event {i} differs"
    assert len(got) == len(want), f"{name}: {len(got)} events, the pinned trace has {len(want)}"


def test_every_wrapper_under_test_made_a_native_call():
    """The golden file names each plain entry point and, for the CE forms with a z term, its _z namesake."""
    seen = {e[0] for events in _load().values() for e in events if e[0].startswith("pt_")}
    plain = {"pt_cross_entropy_fwd_bwd", "pt_cross_entropy_fwd_lse", "pt_cross_entropy_bwd_lse", "pt_cross_entropy_fwd_stats",
             "pt_cross_entropy_vp_combine", "pt_cross_entropy_bwd_lse_shard"}
    assert seen >= plain | {n + "_z" for n in plain} | {"pt_cross_entropy_mean", "pt_cross_entropy_vp_partial",
                                                        "pt_rmsnorm_fwd", "pt_rmsnorm_bwd", "pt_rmsnorm_bwd_splitk",
                                                        "pt_rmsnorm_bwd_partials"}


def _write():
    out = {}
    for name in sorted(CASES):
        mp = pytest.MonkeyPatch()
        try:
            out[name] = run_case(name, mp)
        finally:
            mp.undo()
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(
            json.dumps(k) + ": [\n" + ",\n".join("  " + json.dumps(e, separators=(",", ":")) for e in out[k]) + "\n]"
            for k in sorted(out)) + "\n}\n")


if __name__ == "__main__":
    _write()
