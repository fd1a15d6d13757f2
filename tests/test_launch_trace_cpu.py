"""The native GEMM calls picotron_amd.kernels / functional make, pinned without a GPU.

The library is replaced by a recorder (every pt_* call is logged and returns 0), the stream is None
and the device clause of kernels._bf16_rowmajor is dropped, so linear_fwd / linear_dgrad /
linear_wgrad / linear_wgrad_grouped / linear_dgrad_dual / linear_dgrad_swiglu and the functional
dispatchers run on torch.empty CPU tensors.  Every recorded call is decoded -- flags, epilogue, tile,
order, each problem's sizes, bounds and leading dimensions, and every pointer as "in<i>+<bytes>" (inside
the i-th tensor the case made) or "tmp<k>:<bytes>+<offset>" (the k-th temporary the code allocated, in
order of first appearance) -- and compared with tests/golden/launch_trace.json.  That file pins the
launches a refactor of the host code must keep: it is not regenerated when the code changes
(`python -m tests.test_launch_trace_cpu NAME ...` rewrites only the named cases)."""
import ctypes
import json
import os
import sys

import pytest
import torch

from picotron_amd import _C, switches
from picotron_amd import functional as FN
from picotron_amd import kernels as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_trace.json")
T, H, I, V = 4096, 2048, 8192, 49152          # the shapes of tests/test_launch_shapes_cpu.py
Hs, Qs, Is = H // 8, 3 * H // 8, I // 8          # TP = 8 shard widths
BF16, F32 = torch.bfloat16, torch.float32

ARGS = {
    "pt_gemm": "A lda a_kcontig B ldb b_bounds nb b_kcontig b_seg_dim C ldc c_bounds nc M N K epilogue residual ldr "
               "tile stream",
    "pt_gemm_grouped": "problems n a_kcontig b_kcontig epilogue tile stream",
    "pt_gemm_dual": "dx_problems dx_n dx_a_kcontig dx_b_kcontig dx_epilogue dw_problems dw_n dw_a_kcontig "
                    "dw_b_kcontig dw_epilogue order stream",
    "pt_gemm_splitk_reduce": "parts ksplit kpart_stride M N outs ldc bounds nc mode residual ldr stream",
    "pt_gemm_splitk_sum": "p0 p1 residual out numel stream",
}


class Trace:
    """The recorder standing in for the library, and the registry that names pointers."""

    def __init__(self):
        self.events, self.inputs, self.allocs, self.tmps, self.rcs = [], [], [], {}, {}

    # ---- tensors
    def new(self, *shape, dtype=BF16):
        """An input tensor of the case (uninitialised: nothing reads it)."""
        return self.own(torch.empty(*shape, dtype=dtype))

    def own(self, t):
        self.inputs.append(t)
        return t

    def param(self, *shape, requires_grad=True):
        p = torch.nn.Parameter(self.new(*shape), requires_grad=requires_grad)
        p._pt_grad_ready = lambda q: self.events.append(["grad_ready", self.ptr(q.data_ptr())])
        return p

    def track(self, t):
        self.allocs.append(t)   # kept alive, so no two temporaries of a case share an address
        return t

    @staticmethod
    def _span(t):
        s = t.untyped_storage()
        return s.data_ptr(), s.data_ptr() + s.nbytes()

    def ptr(self, v, strict=True):
        if isinstance(v, ctypes.c_void_p):
            v = v.value
        if not v:
            return None
        for i, t in enumerate(self.inputs):
            lo, hi = self._span(t)
            if lo <= v < hi:
                return f"in{i}+{v - lo}"
        for t in self.allocs:
            lo, hi = self._span(t)
            if lo <= v < hi:
                k = self.tmps.setdefault(lo, len(self.tmps))
                return f"tmp{k}:{hi - lo}+{v - lo}"
        assert not strict, f"pointer {v:#x} is in no tensor the case made and no temporary of the code"
        return "fresh"

    # ---- the library
    def __getattr__(self, name):
        if not name.startswith("pt_"):
            raise AttributeError(name)

        def call(*args):
            types = _C.SIGNATURES[name][1]
            assert len(args) == len(types), f"{name}: {len(args)} arguments, the ABI takes {len(types)}"
            names = ARGS[name].split() if name in ARGS else [str(i) for i in range(len(args))]
            self.events.append([name, {n: self._arg(args, i, types[i]) for i, n in enumerate(names)}])
            q = self.rcs.get(name)
            return q.pop(0) if q else 0
        return call

    def _arg(self, args, i, ctype):
        v = args[i]
        if isinstance(v, ctypes.Array):
            if v._type_ is _C.GemmProblem:
                return [self._problem(v[j]) for j in range(args[i + 1])]
            return [self.ptr(x) for x in v] if v._type_ is ctypes.c_void_p else list(v)
        return self.ptr(v) if ctype is ctypes.c_void_p else v

    def _problem(self, p):
        return {"A": self.ptr(p.A), "lda": p.lda, "A2": self.ptr(p.A2), "a_k2": p.a_k2,
                "B": [self.ptr(p.B[j]) for j in range(p.nb)], "ldb": list(p.ldb[:p.nb]),
                "b_bounds": list(p.b_bounds[:p.nb + 1]), "nb": p.nb, "b_seg_dim": p.b_seg_dim,
                "C": [self.ptr(p.C[j]) for j in range(p.nc)], "ldc": list(p.ldc[:p.nc]),
                "c_bounds": list(p.c_bounds[:p.nc + 1]), "nc": p.nc, "M": p.M, "N": p.N, "K": p.K,
                "residual": self.ptr(p.residual), "ldr": p.ldr, "ksplit": p.ksplit, "kpart_stride": p.kpart_stride}

    # ---- results
    def ret(self, r):
        if isinstance(r, torch.Tensor):
            return {"ptr": self.ptr(r.data_ptr(), strict=False), "shape": list(r.shape), "stride": list(r.stride()),
                    "dtype": str(r.dtype)}
        if isinstance(r, K.SplitKParts):
            return {"p0": self.ret(r.p0), "p1": self.ret(r.p1)}
        if isinstance(r, (list, tuple)):
            return [self.ret(x) for x in r]
        assert r is None
        return None

    def call(self, fn, *a, **kw):
        """Run one entry point; its native calls are recorded as they happen, then what it returns."""
        self.events.append(["call", fn.__name__])
        self.events.append(["ret", self.ret(fn(*a, **kw))])

    def note(self, *what):
        self.events.append(list(what))


class _TorchProxy:
    """torch for the modules under test, with the allocations registered as temporaries."""

    def __init__(self, tr):
        self._tr = tr

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *a, **kw):
        return self._tr.track(torch.empty(*a, **kw))

    def zeros(self, *a, **kw):
        return self._tr.track(torch.zeros(*a, **kw))

    def empty_like(self, *a, **kw):
        return self._tr.track(torch.empty_like(*a, **kw))


def _bf16_rowmajor_host(t, name):
    """kernels._bf16_rowmajor without its device clause (the tensors here are CPU tensors)."""
    if isinstance(t, K.KPair):
        _bf16_rowmajor_host(t.a, name)
        _bf16_rowmajor_host(t.b, name)
        return
    K._req(t.dtype == BF16, f"{name}: expected bfloat16, got {t.dtype}")
    K._req(t.dim() == 2 and t.stride(1) == 1, f"{name}: expected a 2-D row-major view")


CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


SINKS = {"bf16": (K.EPI_BF16, BF16), "bf16acc": (K.EPI_BF16_ACC, BF16), "f32acc": (K.EPI_F32_ACC, F32)}


def _attn(tr, q=H, o=H, T=T, dtype=BF16, pair=False):
    """The q|k|v + o_proj weight-gradient jobs: widths q per projection, o_proj's input width o."""
    def act(n):
        return K.KPair(tr.new(T, n), tr.new(T, n)) if pair else tr.new(T, n)
    dqkv, x, da, ao = act(3 * q), act(H), act(H), act(o)
    return [(dqkv, x, [tr.new(q, H, dtype=dtype) for _ in range(3)]), (da, ao, [tr.new(H, o, dtype=dtype)])]


# ------------------------------------------------------------------------------------ TP = 1
@case
def tp1_qkvo_dw(tr):
    for name, (epi, dt) in SINKS.items():
        tr.note("sink", name)
        tr.call(K.linear_wgrad_grouped, _attn(tr, dtype=dt), epilogue=epi)


@case
def tp1_forwards(tr):
    x, res = tr.new(T, H), tr.new(T, H)
    tr.call(K.linear_fwd, x, [tr.new(H, H) for _ in range(3)])
    tr.call(K.linear_fwd, x, [tr.new(H, H)], residual=res)
    tr.call(K.linear_fwd, tr.new(T, I), [tr.new(H, I)], residual=res)


@case
def tp1_gate_up_dx(tr):
    dgu, h2, ws = tr.new(T, 2 * I), tr.new(T, H), [tr.new(I, H), tr.new(I, H)]
    tr.call(K.linear_dgrad, dgu, ws)
    tr.call(K.linear_dgrad, dgu, ws, keep_parts=True)
    sinks = [tr.new(I, H), tr.new(I, H)]
    tr.call(K.linear_dgrad_dual, dgu, ws, [(dgu, h2, sinks)], K.EPI_BF16_ACC, keep_parts=True, order=1)
    tr.call(K.linear_dgrad_dual, dgu, ws, [(dgu, h2, sinks)], K.EPI_BF16_ACC)
    tr.call(K.linear_dgrad_dual, dgu, ws, [(dgu, h2, sinks)], K.EPI_BF16_ACC, split_min=1 << 30)


@case
def tp1_qkv_dx(tr):
    jobs = _attn(tr)
    dqkv, ws = jobs[0][0], [tr.new(H, H) for _ in range(3)]
    tr.call(K.linear_dgrad, dqkv, ws)
    tr.call(K.linear_dgrad, dqkv, ws, keep_parts=True, split_min=1024)
    tr.call(K.linear_dgrad_dual, dqkv, ws, jobs, K.EPI_BF16, keep_parts=True, split_min=1024)
    tr.call(K.linear_dgrad_dual, dqkv, ws, jobs, K.EPI_BF16_ACC, split_min=1024)


@case
def tp1_down_dx_swiglu(tr):
    dm, wd, gu, hh = tr.new(T, H), tr.new(H, I), tr.new(T, 2 * I), tr.new(T, I)
    tr.call(K.linear_dgrad_swiglu, dm, wd, gu)
    tr.call(K.linear_dgrad_dual, dm, [wd], [(dm, hh, [tr.new(H, I, dtype=F32)])], K.EPI_F32_ACC, gu=gu)
    tr.call(K.linear_dgrad_dual, dm, [wd], [(dm, hh, [tr.new(H, I)])], K.EPI_BF16, gu=gu, order=0)


@case
def tp1_lm_head_dx(tr):
    tr.call(K.linear_dgrad, tr.new(T, V), [tr.new(V, H)])
    out = tr.new(T, H)
    tr.call(K.linear_dgrad, tr.new(T, H), [tr.new(H, H)], out=out, accumulate=True)


# ------------------------------------------------------------------------------------ TP = 8
@case
def tp8_qkvo_dw(tr):
    for name, (epi, dt) in SINKS.items():
        tr.note("sink", name)
        tr.call(K.linear_wgrad_grouped, _attn(tr, Hs, Hs, dtype=dt), epilogue=epi)
    tr.note("f32 store: no K-slices")
    tr.call(K.linear_wgrad_grouped, _attn(tr, Hs, Hs, dtype=F32), epilogue=K.EPI_F32)
    tr.note("a tile asked for")
    tr.call(K.linear_wgrad_grouped, _attn(tr, Hs, Hs), epilogue=K.EPI_BF16, tile=12)


@case
def tp8_gate_up_dw(tr):
    dgu, h2 = tr.new(T, 2 * Is), tr.new(T, H)
    tr.call(K.linear_wgrad, dgu, h2, [tr.new(Is, H), tr.new(Is, H)], K.EPI_BF16_ACC)
    tr.call(K.linear_wgrad, dgu, h2, [tr.new(Is, H, dtype=F32), tr.new(Is, H, dtype=F32)], K.EPI_F32_ACC)
    tr.note("the down_proj dW alone: 2 K-slices on tile 15")
    tr.call(K.linear_wgrad, tr.new(T, H), tr.new(T, Is), [tr.new(H, Is)], K.EPI_BF16)
    tr.call(K.linear_wgrad, tr.new(T, H), tr.new(T, Is), [tr.new(H, Is)], K.EPI_BF16, tile=13)


@case
def tp8_down_dual(tr):
    dm, wd, gu, hh = tr.new(T, H), tr.new(H, Is), tr.new(T, 2 * Is), tr.new(T, Is)
    tr.call(K.linear_dgrad_dual, dm, [wd], [(dm, hh, [tr.new(H, Is)])], K.EPI_BF16_ACC, gu=gu)
    tr.call(K.linear_dgrad_dual, dm, [wd], [(dm, hh, [tr.new(H, Is, dtype=F32)])], K.EPI_F32_ACC, gu=gu)


@case
def tp8_few_tile_fwd_dx(tr):
    x = tr.new(T, H)
    tr.call(K.linear_fwd, x, [tr.new(Hs, H) for _ in range(3)])               # tile 15
    tr.call(K.linear_dgrad, x, [tr.new(H, Hs)])                                # o_proj dX: tile 15
    tr.call(K.linear_fwd, tr.new(T, Hs), [tr.new(H, Hs)], residual=x)         # o_proj forward: the auto tile
    x2 = tr.new(T, 2 * H)
    tr.call(K.linear_fwd, x2, [tr.new(Hs, 2 * H)], residual=tr.new(T, Hs))    # 2 K-slices on tile 15
    tr.call(K.linear_dgrad, x2, [tr.new(2 * H, Hs)])
    tr.call(K.linear_dgrad, x2, [tr.new(2 * H, Hs)], out=tr.new(T, Hs), accumulate=True)


@case
def small_wgrad_ksplit(tr):
    """Shapes the 128x128 form leaves alone and wgrad_ksplit slices (256x256 tiles)."""
    dy, x = tr.new(1024, 1024), tr.new(1024, 256)
    tr.call(K.linear_wgrad, dy, x, [tr.new(512, 256), tr.new(512, 256)], K.EPI_BF16_ACC)
    tr.call(K.linear_wgrad_grouped, [(dy, x, [tr.new(1024, 256)]), (x, dy, [tr.new(256, 1024)])], K.EPI_BF16)


# ------------------------------------------------------------------------------------ paired
@case
def paired(tr):
    jobs = _attn(tr, pair=True)
    tr.call(K.linear_wgrad, *jobs[0], K.EPI_BF16_ACC)
    tr.call(K.linear_wgrad_grouped, jobs, K.EPI_BF16)
    ws = [tr.new(H, H) for _ in range(3)]
    tr.call(K.linear_dgrad_dual, jobs[0][0].b, ws, jobs, K.EPI_BF16, keep_parts=True, split_min=1024)
    tr.note("one job paired, one not")
    tr.call(K.linear_wgrad_grouped, [jobs[0], _attn(tr)[1]], K.EPI_BF16_ACC)
    tr.note("TP = 8 widths: a pair takes no K-slices")
    tr.call(K.linear_wgrad_grouped, _attn(tr, Hs, Hs, pair=True), K.EPI_BF16_ACC)
    dm, wd, gu = tr.new(T, H), tr.new(H, Is), tr.new(T, 2 * Is)
    tr.call(K.linear_dgrad_dual, dm, [wd], [(K.KPair(tr.new(T, H), dm), K.KPair(tr.new(T, Is), tr.new(T, Is)),
                                            [tr.new(H, Is)])], K.EPI_BF16_ACC, gu=gu)


@case
def paired_halves_off_grid(tr):
    """T = 96: 2 T is on the 64-grid, each micro-batch's T is not."""
    dy, x = K.KPair(tr.new(96, 128), tr.new(96, 128)), K.KPair(tr.new(96, 128), tr.new(96, 128))
    tr.call(K.linear_wgrad, dy, x, [tr.new(128, 128)], K.EPI_BF16)


# ------------------------------------------------------------------------------------ off the 64-grid
@case
def off_grid(tr):
    t, k, ns = 100, 72, [40, 24]
    x, ws = tr.new(t, k), [tr.new(n, k) for n in ns]
    tr.call(K.linear_fwd, x, ws)
    tr.call(K.linear_fwd, x, ws, residual=tr.new(t, sum(ns)))
    dy = tr.new(t, sum(ns))
    tr.call(K.linear_dgrad, dy, ws)
    tr.call(K.linear_dgrad, dy, ws, out=tr.new(t, k), accumulate=True)
    for name, (epi, dt) in SINKS.items():
        tr.note("sink", name)
        tr.call(K.linear_wgrad, dy, x, [tr.new(n, k, dtype=dt) for n in ns], epi)
    tr.note("pair")
    tr.call(K.linear_wgrad, K.KPair(dy, tr.new(t, sum(ns))), K.KPair(x, tr.new(t, k)), [tr.new(n, k) for n in ns],
            K.EPI_BF16)
    tr.note("grouped")
    tr.call(K.linear_wgrad_grouped, [(dy, x, [tr.new(n, k) for n in ns]),
                                     (tr.new(128, 64), tr.new(128, 64), [tr.new(64, 64)])], K.EPI_BF16_ACC)


# ------------------------------------------------------------------------------------ sink fallbacks
def _misaligned(tr, rows, cols, dtype=BF16):
    buf = tr.new(rows * cols + 8, dtype=dtype)
    off = 1 if dtype == BF16 else 2                       # 2-B (bf16) / 8-B (f32) off the chunk
    return buf[off:off + rows * cols].view(rows, cols)


@case
def misaligned_sinks_keep_unsplit(tr):
    jobs = _attn(tr, Hs, Hs)
    jobs[1] = (jobs[1][0], jobs[1][1], [_misaligned(tr, H, Hs)])
    tr.call(K.linear_wgrad_grouped, jobs, K.EPI_BF16_ACC)
    tr.call(K.linear_wgrad, jobs[1][0], jobs[1][1], jobs[1][2], K.EPI_BF16_ACC)
    tr.call(K.linear_wgrad, tr.new(1024, 1024), tr.new(1024, 256), [_misaligned(tr, 1024, 256, F32)], K.EPI_F32_ACC)
    dm, wd, gu, hh = tr.new(T, H), tr.new(H, Is), tr.new(T, 2 * Is), tr.new(T, Is)
    tr.call(K.linear_dgrad_dual, dm, [wd], [(dm, hh, [_misaligned(tr, H, Is)])], K.EPI_BF16_ACC, gu=gu)
    x2 = tr.new(T, 2 * H)
    tr.call(K.linear_fwd, x2, [tr.new(Hs, 2 * H)], residual=_misaligned(tr, T, Hs))
    tr.call(K.linear_dgrad, x2, [tr.new(2 * H, Hs)], out=_misaligned(tr, T, Hs))


@case
def library_refuses(tr):
    """PT_EUNSUPPORTED (-3) from the dual launch: None, nothing else launched; from a paired grouped
    launch: each micro-batch's half on its own."""
    jobs = _attn(tr)
    tr.rcs["pt_gemm_dual"] = [-3]
    tr.call(K.linear_dgrad_dual, jobs[0][0], [tr.new(H, H) for _ in range(3)], jobs, K.EPI_BF16)
    tr.rcs["pt_gemm_grouped"] = [-3]
    tr.call(K.linear_wgrad_grouped, _attn(tr, pair=True), K.EPI_BF16)


# ------------------------------------------------------------------------------------ switches
@case
def switch_ksplit_0(tr):
    with switches.override(ksplit=0):
        tr.call(K.linear_wgrad_grouped, _attn(tr, Hs, Hs), K.EPI_BF16_ACC)


@case
def switch_swiglu_splitk_0(tr):
    dm, wd, gu, hh = tr.new(T, H), tr.new(H, Is), tr.new(T, 2 * Is), tr.new(T, Is)
    with switches.override(swiglu_splitk=0):
        tr.call(K.linear_dgrad_dual, dm, [wd], [(dm, hh, [tr.new(H, Is)])], K.EPI_BF16_ACC, gu=gu)


@case
def switch_splitk2_0(tr):
    dgu, h2, ws = tr.new(T, 2 * I), tr.new(T, H), [tr.new(I, H), tr.new(I, H)]
    with switches.override(splitk2=0):
        tr.call(K.linear_dgrad, dgu, ws, keep_parts=True)
        tr.call(K.linear_dgrad_dual, dgu, ws, [(dgu, h2, [tr.new(I, H), tr.new(I, H)])], K.EPI_BF16_ACC,
                keep_parts=True, order=1)


@case
def switch_dual_0(tr):
    L = _Layer(tr)
    with switches.override(dual=0):
        L.backward()


# ------------------------------------------------------------------------------------ functional
class _Layer:
    """One decoder layer's weight-gradient calls as functional.attn_block_bwd / mlp_block_bwd make
    them at tp = 1: the down dual, the gate|up dual, the q|k|v + o_proj dual."""

    def __init__(self, tr, T=T, sinks="grad"):
        self.tr, self.T = tr, T
        self.wq, self.wk, self.wv, self.wo = (tr.param(H, H) for _ in range(4))
        self.wg, self.wu, self.wd = tr.param(I, H), tr.param(I, H), tr.param(H, I)
        if sinks != "grad":
            for p in self.params():
                p.main_grad = tr.new(*p.shape, dtype=F32 if sinks == "main_grad_f32" else BF16)

    def params(self):
        return [self.wq, self.wk, self.wv, self.wo, self.wg, self.wu, self.wd]

    def backward(self, notify=True):
        tr, t = self.tr, self.T
        dm, hh, gu = tr.new(t, H), tr.new(t, I), tr.new(t, 2 * I)
        tr.call(FN.dgrad_with_wgrad, dm, [self.wd], [(dm, hh, [self.wd])], gu=gu, notify=notify)
        dgu, h2 = tr.new(t, 2 * I), tr.new(t, H)
        tr.call(FN.dgrad_with_wgrad, dgu, [self.wg, self.wu], [(dgu, h2, [self.wg, self.wu])], keep_parts=True,
                split_min=None, order=FN.GU_DUAL_ORDER)
        dqkv, da, o = tr.new(t, 3 * H), tr.new(t, H), tr.new(t, H)
        tr.call(FN.dgrad_with_wgrad, dqkv, [self.wq, self.wk, self.wv],
                [(dqkv, h2, [self.wq, self.wk, self.wv]), (da, o, [self.wo])], keep_parts=True, split_min=1024)

    def separate(self, notify=True):
        """The same weight gradients through wgrad / wgrad_group (the TP > 1 calls)."""
        tr, t = self.tr, self.T
        tr.call(FN.wgrad, tr.new(t, H), tr.new(t, I), [self.wd], notify)
        tr.call(FN.wgrad, tr.new(t, 2 * I), tr.new(t, H), [self.wg, self.wu], notify)
        tr.call(FN.wgrad_group, [(tr.new(t, 3 * H), tr.new(t, H), [self.wq, self.wk, self.wv]),
                                 (tr.new(t, H), tr.new(t, H), [self.wo])], notify)


def _phases(tr, seq, run):
    """run() under each pairing phase of seq in turn, then phase None and the flush (train_step)."""
    old = FN.wgrad_pairing(None)
    try:
        for ph in seq:
            tr.note("phase", ph)
            FN.wgrad_pairing(ph)
            run()
            tr.note("pending", len(FN.WgradPairing.pending))
        FN.wgrad_pairing(None)
        tr.note("flush")
        FN.flush_wgrad_pairs()
        tr.note("pending", len(FN.WgradPairing.pending))
    finally:
        FN.wgrad_pairing(old)
        FN.WgradPairing.pending.clear()


@case
def fn_dual_phases(tr):
    L = _Layer(tr)
    _phases(tr, [None, 0, 1], L.backward)


@case
def fn_separate_phases(tr):
    L = _Layer(tr)
    _phases(tr, [None, 0, 1], L.separate)


@case
def fn_main_grad_f32_phases(tr):
    L = _Layer(tr, sinks="main_grad_f32")
    _phases(tr, [0, 1], L.backward)
    _phases(tr, [None], L.separate)


@case
def fn_main_grad_bf16(tr):
    L = _Layer(tr, sinks="main_grad_bf16")
    _phases(tr, [None], L.backward)


@case
def fn_odd_micro_batch_flushes(tr):
    """A deferring micro-batch nobody completes: the flush launches its jobs unpaired."""
    L = _Layer(tr)
    _phases(tr, [0], L.backward)
    _phases(tr, [0], lambda: L.separate(notify=False))


@case
def fn_pair_layout_differs(tr):
    """The completing micro-batch has another token count: the older job on its own first."""
    L = _Layer(tr)
    old = FN.wgrad_pairing(0)
    try:
        L.separate()
        L.T = T // 2
        _phases(tr, [1], L.separate)
    finally:
        FN.wgrad_pairing(old)


@case
def fn_frozen(tr):
    L = _Layer(tr)
    L.wk.requires_grad_(False)
    L.wu.requires_grad_(False)
    _phases(tr, [None, 0, 1], L.backward)
    _phases(tr, [None, 0, 1], L.separate)


@case
def fn_mixed_sinks(tr):
    """One .grad present, the others not: one launch per parameter."""
    def fresh():
        L = _Layer(tr)
        L.wq.grad, L.wg.grad = tr.new(H, H), tr.new(I, H)
        return L
    _phases(tr, [None], fresh().backward)
    _phases(tr, [None], fresh().separate)
    _phases(tr, [0, 1], fresh().backward)
    _phases(tr, [0, 1], fresh().separate)


@case
def fn_dual_refused_or_untileable(tr):
    """pt_gemm_dual answers -3: the same sinks through separate launches; shapes dual_fits refuses."""
    L = _Layer(tr)
    tr.rcs["pt_gemm_dual"] = [-3, -3, -3]
    L.backward()
    w = tr.param(72, 40)
    dy = tr.new(100, 72)
    tr.call(FN.dgrad_with_wgrad, dy, [w], [(dy, tr.new(100, 40), [w])])


@case
def fn_deferred_twice(tr):
    """Two deferring backwards on one parameter with no completing one between them."""
    w = tr.param(H, H)
    jobs = [(tr.new(T, H), tr.new(T, H)) for _ in range(2)]
    _phases(tr, [0], lambda: [tr.call(FN.wgrad, dy, x, [w]) for dy, x in jobs])


# ------------------------------------------------------------------------------------ the test
def run_case(name, monkeypatch):
    tr = Trace()
    monkeypatch.setattr(_C, "lib", lambda: tr)
    monkeypatch.setattr(_C, "stream_ptr", lambda device=None: None)
    monkeypatch.setattr(K, "_bf16_rowmajor", _bf16_rowmajor_host)
    proxy = _TorchProxy(tr)
    monkeypatch.setattr(K, "torch", proxy)
    monkeypatch.setattr(FN, "torch", proxy)
    CASES[name](tr)
    return json.loads(json.dumps(tr.events))


def _load():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_holds_exactly_the_cases():
    assert sorted(_load()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_trace(name, monkeypatch):
    got, want = run_case(name, monkeypatch), _load()[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: event {i} differs"
    assert len(got) == len(want), f"{name}: {len(got)} events, the pinned trace has {len(want)}"


def test_paired_launch_refused_for_its_k_segment_runs_as_halves(monkeypatch):
    """PT_EINVAL (-1) from a paired grouped launch falls back as PT_EUNSUPPORTED (-3) does: each
    micro-batch's half on its own, the second accumulating."""
    def refused(rc):
        def run(tr):
            tr.rcs["pt_gemm_grouped"] = [rc]
            tr.call(K.linear_wgrad_grouped, _attn(tr, pair=True), K.EPI_BF16)
        monkeypatch.setitem(CASES, "refused", run)
        return run_case("refused", monkeypatch)
    assert refused(-1) == refused(-3)
    assert [e[1]["epilogue"] for e in refused(-1) if e[0] == "pt_gemm_grouped"] == \
        [K.EPI_BF16, K.EPI_BF16, K.EPI_BF16_ACC, K.EPI_BF16, K.EPI_BF16_ACC]


def _write(names):
    out = _load() if names else {}
    for name in names or sorted(CASES):
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
    _write(sys.argv[1:])
