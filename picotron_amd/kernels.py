"""Tensor-level wrappers over the C ABI: validation, output allocation (by torch's caching
allocator -- kernels never allocate) and launch on torch's current stream.

Every function here runs the gfx950 kernels and nothing else; there is no CPU or eager
fallback.  Shapes/dtypes/strides are validated in Python before the call, as the reference
validates with asserts (e.g. picotron/model.py:95-96, tensor_parallel.py:81,151,226).
"""
import ctypes
import math

import sys

import torch

from . import _C
from .switches import S as SW

BF16 = torch.bfloat16


def _ptr(t):
    return None if t is None else t.data_ptr()


def _req(cond, msg):
    if not cond:
        raise ValueError(msg)


def _bf16_rowmajor(t, name):
    if isinstance(t, KPair):
        _bf16_rowmajor(t.a, name)
        _bf16_rowmajor(t.b, name)
        return
    _req(t.dtype == BF16, f"{name}: expected bfloat16, got {t.dtype}")
    _req(t.is_cuda, f"{name}: expected a device tensor")
    _req(t.dim() == 2 and t.stride(1) == 1, f"{name}: expected a 2-D row-major view")


# --------------------------------------------------------------------------------- RMSNorm
MODE_TRITON = 0   # flash-attn layer_norm_fn(is_rms_norm=True): bf16(x * rstd * w)
MODE_LLAMA = 1    # LlamaRMSNorm: w * bf16(x * rstd)


def rmsnorm_fwd(x, weight, eps, mode=MODE_TRITON, residual=None):
    """x [rows, cols] bf16 contiguous.  Returns (y, rstd, z) where z = bf16(x + residual) (or None)."""
    _bf16_rowmajor(x, "x")
    x = x.contiguous()
    rows, cols = x.shape
    lib = _C.lib()
    y = torch.empty_like(x)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    z = None
    if residual is not None:
        residual = residual.contiguous()
        _req(residual.shape == x.shape and residual.dtype == BF16, "residual shape/dtype")
        z = torch.empty_like(x)
    rc = lib.pt_rmsnorm_fwd(_ptr(x), _ptr(residual), _ptr(weight), _ptr(y), _ptr(z), _ptr(rstd), rows, cols,
                            float(eps), int(mode), _C.stream_ptr(x.device))
    _C.check(rc, "pt_rmsnorm_fwd")
    return y, rstd, z


DW_ACC_BF16, DW_ACC_F32 = 4, 8   # pt_rmsnorm_bwd dweight sinks (include/picotron_hip.h)


class SplitKParts:
    """A split-K dX GEMM's result before its sum pass: two f32 K halves [rows, cols] whose
    bf16(p0 + p1) is the dX (linear_dgrad_dual(keep_parts=True)).  rmsnorm_bwd takes it as its dy
    and sums in the norm kernel; anything else calls .sum() for the bf16 tensor."""

    def __init__(self, p0, p1):
        self.p0, self.p1 = p0, p1
        self.shape, self.device = p0.shape, p0.device

    def sum(self, out=None, residual=None):
        """bf16(p0 + p1 (+ residual)) into out (a new tensor when None)."""
        if out is None:
            out = torch.empty(self.shape, dtype=BF16, device=self.device)
        rc = _C.lib().pt_gemm_splitk_sum(_ptr(self.p0), _ptr(self.p1), _ptr(residual), _ptr(out), out.numel(),
                                         _C.stream_ptr(self.device))
        _C.check(rc, "pt_gemm_splitk_sum")
        return out


class KPair:
    """Two [T, n] row blocks a, b of one layout standing for their concatenation [2 T, n] along the
    token (K) dimension of a weight gradient: two micro-batches' dY (or X).  The wgrad launches take
    it as a K-segmented operand (pt_gemm_problem.A2 / b_seg_dim 1): dW = dY_a^T X_a + dY_b^T X_b in
    one K = 2 T GEMM (functional.pair_jobs).  Column slices stay pairs."""

    def __init__(self, a, b):
        _req(a.shape == b.shape and a.stride() == b.stride() and a.dtype == b.dtype and a.device == b.device,
             "KPair: two row blocks of one shape and layout")
        self.a, self.b = a, b
        self.shape = (2 * a.shape[0], a.shape[1])
        self.dtype, self.device = a.dtype, a.device

    def stride(self, i=None):
        return self.a.stride() if i is None else self.a.stride(i)

    def __getitem__(self, idx):
        return KPair(self.a[idx], self.b[idx])


def rmsnorm_bwd(dy, z, weight, rstd, mode=MODE_TRITON, dres=None, dw_out=None, dw_sink=0, defer_dw=False):
    """Returns (dx, dweight).  dres (same shape as dy) is added into dx when given.
    dw_out/dw_sink: write the weight gradient into an existing buffer -- 0 store (bf16),
    DW_ACC_BF16 accumulate into a bf16 .grad, DW_ACC_F32 accumulate into an f32 main_grad.
    defer_dw: no column sum; returns (dx, partial) -- the f32 per-block partial rows, to be summed
    into the sink later by rmsnorm_colsum_batch.  dy may be a SplitKParts (summed in the kernel)."""
    split = isinstance(dy, SplitKParts)
    if not split:
        dy = dy.contiguous()
    rows, cols = z.shape
    lib = _C.lib()
    nparts = lib.pt_rmsnorm_bwd_partials(rows, cols)
    _C.check(0 if nparts > 0 else nparts, "pt_rmsnorm_bwd_partials")
    partial = torch.empty(nparts, cols, dtype=torch.float32, device=z.device)
    dx = torch.empty_like(z)
    if defer_dw:
        dw_out, dw_sink = None, 0
    elif dw_out is None:
        dw_out, dw_sink = torch.empty(cols, dtype=BF16, device=z.device), 0
    if dw_out is not None:
        _req(dw_out.is_contiguous() and dw_out.numel() == cols, "dweight buffer must be contiguous [cols]")
        _req(dw_out.dtype == (torch.float32 if dw_sink == DW_ACC_F32 else BF16), "dweight buffer dtype")
    if dres is not None:
        dres = dres.contiguous()
    if split:
        _req(dy.p0.is_contiguous() and dy.p1.is_contiguous() and tuple(dy.shape) == (rows, cols), "split dy parts")
        rc = lib.pt_rmsnorm_bwd_splitk(_ptr(dy.p0), _ptr(dy.p1), _ptr(z), _ptr(weight), _ptr(rstd), _ptr(dres), _ptr(dx),
                                       _ptr(dw_out), _ptr(partial), rows, cols, int(mode) | int(dw_sink),
                                       _C.stream_ptr(z.device))
        _C.check(rc, "pt_rmsnorm_bwd_splitk")
    else:
        rc = lib.pt_rmsnorm_bwd(_ptr(dy), _ptr(z), _ptr(weight), _ptr(rstd), _ptr(dres), _ptr(dx), _ptr(dw_out),
                                _ptr(partial), rows, cols, int(mode) | int(dw_sink), _C.stream_ptr(z.device))
        _C.check(rc, "pt_rmsnorm_bwd")
    return dx, (partial if defer_dw else dw_out)


def rmsnorm_colsum_batch(jobs):
    """jobs: [(partial [nparts, cols] f32, dw_out, dw_sink)], all of one width, <= 32: the deferred
    weight-gradient sums of rmsnorm_bwd(defer_dw=True), one launch."""
    _req(0 < len(jobs) <= 32, "rmsnorm_colsum_batch: 1..32 jobs")
    cols = jobs[0][0].shape[1]
    for part, out, sink in jobs:
        _req(part.dtype == torch.float32 and part.is_contiguous() and part.shape[1] == cols, "partials [n, cols] f32")
        _req(out.is_contiguous() and out.numel() == cols, "dweight buffer must be contiguous [cols]")
        _req(out.dtype == (torch.float32 if sink == DW_ACC_F32 else BF16), "dweight buffer dtype")
    rc = _C.lib().pt_rmsnorm_colsum_batch(_C.ptrarr([_ptr(p) for p, _, _ in jobs]),
                                          _C.i32arr([p.shape[0] for p, _, _ in jobs]),
                                          _C.ptrarr([_ptr(o) for _, o, _ in jobs]),
                                          _C.i32arr([s for _, _, s in jobs]), len(jobs), cols,
                                          _C.stream_ptr(jobs[0][0].device))
    _C.check(rc, "pt_rmsnorm_colsum_batch")


# ------------------------------------------------------------------------------- embedding
def embedding_fwd(ids, weight, vocab_lo=0, vocab_hi=None):
    """out[t] = weight[ids[t] - vocab_lo] (zero rows for ids outside [vocab_lo, vocab_hi))."""
    _req(weight.dtype == BF16 and weight.stride(1) == 1, "embedding table: bf16 rows")
    vocab_hi = vocab_lo + weight.shape[0] if vocab_hi is None else vocab_hi
    flat = ids.reshape(-1).contiguous().to(torch.int64)
    H = weight.shape[1]
    out = torch.empty(flat.numel(), H, dtype=BF16, device=weight.device)
    if flat.numel() == 0:   # an empty tensor has no address to hand to the kernel's argument check
        return out.view(*ids.shape, H)
    rc = _C.lib().pt_embedding_fwd(_ptr(flat), flat.numel(), _ptr(weight), weight.stride(0), int(vocab_lo),
                                   int(vocab_hi), _ptr(out), out.stride(0), H, _C.stream_ptr(weight.device))
    _C.check(rc, "pt_embedding_fwd")
    return out.view(*ids.shape, H)


def embedding_bwd(ids, dy2d, dweight, sink, vocab_lo=0, vocab_hi=None, padding_idx=None):
    """Sum the dY rows of every id into dweight (sink: 0 / DW_ACC_BF16 / DW_ACC_F32); ids outside
    [vocab_lo, vocab_hi) and padding_idx contribute nothing (F.embedding's backward)."""
    _bf16_rowmajor(dy2d, "dy")
    flat = ids.reshape(-1).to(torch.int64).contiguous()
    vocab_hi = vocab_lo + dweight.shape[0] if vocab_hi is None else vocab_hi
    T = flat.numel()
    if T == 0:   # no token: nothing to add (and no address to hand to the kernels' argument checks)
        return
    sorted_ids = torch.empty(T, dtype=torch.int64, device=flat.device)
    perm = torch.empty(T, dtype=torch.int64, device=flat.device)
    rc = _C.lib().pt_embedding_sort(_ptr(flat), T, int(vocab_lo), int(vocab_hi), int(padding_idx is not None),
                                    int(padding_idx if padding_idx is not None else 0), _ptr(sorted_ids), _ptr(perm),
                                    _C.stream_ptr(flat.device))
    if rc == -3:   # more tokens than the one-workgroup sort holds: torch's (stable) device sort
        skip = (flat < vocab_lo) | (flat >= vocab_hi)
        if padding_idx is not None:
            skip = skip | (flat == padding_idx)
        sorted_ids, perm = torch.sort(torch.where(skip, torch.full_like(flat, -1), flat), stable=True)
    else:
        _C.check(rc, "pt_embedding_sort")
    rc = _C.lib().pt_embedding_bwd(_ptr(sorted_ids), _ptr(perm), flat.numel(), _ptr(dy2d), dy2d.stride(0),
                                   int(vocab_lo), _ptr(dweight), dweight.stride(0), dy2d.shape[1], int(sink),
                                   _C.stream_ptr(dy2d.device))
    _C.check(rc, "pt_embedding_bwd")


# ----------------------------------------------------------------------------------- AdamW
def _grad_dtype(t, what):
    _req(t.is_cuda and t.is_contiguous(), f"{what}: a contiguous device tensor")
    if t.dtype == BF16:
        return 0
    if t.dtype == torch.float32:
        return 1
    raise _C.HipKernelError(f"{what}: unsupported dtype {t.dtype}")


def _sq_ok(sq, device):
    _req(sq.dtype == torch.float32 and sq.numel() == 1 and sq.device == device, "grad_sq: one f32 on the device")


class _clip_status:
    """The status word of a clip consumer's launch.  A caller that issues several of them for one
    step (optim.AdamW) passes its own word (status_word(device), fetched once) and posts it once
    after the last (_status_posted), so the poll in front of a launch never raises mid-step for a
    bit the same step's earlier launch set."""

    def __init__(self, device, status):
        self.device, self.own = device, status is None
        self.word = status_word(device) if status is None else status

    def __enter__(self):
        return _ptr(self.word)

    def __exit__(self, exc_type, exc, tb):
        if self.own and exc_type is None:
            _status_posted(self.device)


def _adam_launch(name, dev, lead, scalars=(), clip=None, ints=()):
    """Entry `name`(*lead, *scalars as f32, *ints, stream) on dev's current stream, its return code
    checked.  clip = (sq, max_norm, status): a clip consumer -- sq is validated, the entry runs under
    _clip_status and takes (sq, max_norm, status word) in front of the stream."""
    sc = [float(x) for x in scalars] + [int(x) for x in ints]
    if clip is None:
        _C.check(getattr(_C.lib(), name)(*lead, *sc, _C.stream_ptr(dev)), name)
        return
    sq, max_norm, status = clip
    _sq_ok(sq, dev)
    with _clip_status(dev, status) as st:
        _C.check(getattr(_C.lib(), name)(*lead, *sc, _ptr(sq), float(max_norm), st, _C.stream_ptr(dev)), name)


def _adam_single_ok(p, grad, exp_avg, exp_avg_sq):
    """One (param, grad, exp_avg, exp_avg_sq) of adamw_step / adamw_step_clip; returns the dtype code."""
    for t, nm in ((grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _req(t.dtype == p.dtype and t.numel() == p.numel() and t.device == p.device, f"adamw: {nm} must match param")
        _req(t.is_contiguous(), "adamw: dense tensors")
    _req(p.is_contiguous(), "adamw: param must be contiguous")
    return _grad_dtype(p, "adamw")


def adamw_step(p, grad, exp_avg, exp_avg_sq, decay, w1, beta2, c2, bc2_sqrt, eps, step_size):
    """One fused AdamW update of tensor p in place (bf16 or f32, any alignment; torch foreach semantics)."""
    dt = _adam_single_ok(p, grad, exp_avg, exp_avg_sq)
    _adam_launch("pt_adamw_step", p.device, (_ptr(p), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), p.numel(), dt),
                 (decay, w1, beta2, c2, bc2_sqrt, eps, step_size))


def adamw_step_clip(p, grad, exp_avg, exp_avg_sq, sq, max_norm, decay, w1, beta2, c2, bc2_sqrt, eps, step_size, status=None):
    """adamw_step on the clipped gradient (one tensor, bf16 or f32, any alignment)."""
    dt = _adam_single_ok(p, grad, exp_avg, exp_avg_sq)
    _adam_launch("pt_adamw_step_clip", p.device, (_ptr(p), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), p.numel(), dt),
                 (decay, w1, beta2, c2, bc2_sqrt, eps, step_size), (sq, max_norm, status))


_ADAM_DESC = {}


def _is_sr(items):
    """A stochastic-rounding list: (param, grad, exp_avg, exp_avg_sq, stream id) tuples."""
    return len(items[0]) == 5 and not torch.is_tensor(items[0][4])


def _adam_desc(items):
    """(device descriptor table, device chunk_start, total chunks) of a list of tensor tuples:
    4-tuples make the pt_adam_tensor table, 5-tuples the pt_adam_master_tensor table, (param, grad,
    exp_avg, exp_avg_sq, stream id) the pt_adam_sr_tensor table with the id in the row and in the
    key.  Cached per pointer set: the tensors of a model stay put across steps, a re-allocated
    gradient makes a new table.  A new table is staged in pinned host memory and copied on the
    current stream without a host sync (the caching host allocator keeps the staging buffer alive
    until that copy has run)."""
    if _is_sr(items):
        rows = tuple(tuple(t.data_ptr() for t in it[:4]) + (it[0].numel(), int(it[4])) for it in items)
        key = ("sr",) + rows
    else:
        key = rows = tuple(tuple(t.data_ptr() for t in it) + (it[0].numel(),) for it in items)
    ent = _ADAM_DESC.get(key)
    if ent is None:
        dev = items[0][0].device
        chunks = [0]
        for it in items:
            chunks.append(chunks[-1] + (it[0].numel() + 7) // 8)
        desc_h = torch.tensor([list(k) for k in rows], dtype=torch.int64).pin_memory()
        chunk_h = torch.tensor(chunks, dtype=torch.int64).pin_memory()
        ent = (desc_h.to(dev, non_blocking=True), chunk_h.to(dev, non_blocking=True), chunks[-1])
        if len(_ADAM_DESC) > 64:
            _ADAM_DESC.clear()
        _ADAM_DESC[key] = ent
    return ent


def _adam_list(items, *extra):
    """The leading arguments of a list entry: table, chunk_start, ntensors, total_chunks (, extra)."""
    desc, chunk_t, total = _adam_desc(items)
    return (_ptr(desc), _ptr(chunk_t), len(items), int(total)) + extra


def _adam_items_ok(items):
    _req(len(items) > 0, "adamw multi: an empty tensor list")
    for p, g, m, v in items:
        for t in (p, g, m, v):
            _req(t.dtype == BF16 and t.is_contiguous() and t.numel() == p.numel() and t.data_ptr() % 16 == 0,
                 "adamw multi: contiguous, 16-byte aligned bf16 tensors of one length per parameter")


def adamw_step_multi(items, decay, w1, beta2, c2, bc2_sqrt, eps, step_size):
    """One launch of the fused AdamW update over a list of bf16 (param, grad, exp_avg, exp_avg_sq)
    tuples (pt_adamw_step_multi), on the cached descriptor table of _adam_desc."""
    _adam_items_ok(items)
    _adam_launch("pt_adamw_step_multi", items[0][0].device, _adam_list(items),
                 (decay, w1, beta2, c2, bc2_sqrt, eps, step_size))


def adamw_step_multi_clip(items, sq, max_norm, decay, w1, beta2, c2, bc2_sqrt, eps, step_size, status=None):
    """adamw_step_multi on the clipped gradients bf16(grad * coef), coef as in grad_scale_multi,
    applied where the kernel loads the gradient: bit-identical to grad_scale_multi followed by
    adamw_step_multi, and the gradients are not modified.  A non-finite sq skips the update."""
    _adam_items_ok(items)
    _adam_launch("pt_adamw_step_multi_clip", items[0][0].device, _adam_list(items),
                 (decay, w1, beta2, c2, bc2_sqrt, eps, step_size), (sq, max_norm, status))


# ----------------------------------------------------- AdamW, fp32 master weights and moments
def _adam_master_ok(w, p, g, m, v, what):
    """One (master, param, grad, exp_avg, exp_avg_sq) entry; returns the gradient's dtype code."""
    _req(p.dtype == BF16 and w.dtype == m.dtype == v.dtype == torch.float32,
         f"{what}: a bf16 parameter with f32 master, exp_avg and exp_avg_sq")
    _req(g.dtype in (BF16, torch.float32), f"{what}: bf16 or f32 gradients")
    for t in (w, p, g, m, v):
        _req(t.is_cuda and t.device == p.device and t.is_contiguous() and t.numel() == p.numel(),
             f"{what}: contiguous device tensors of one length per parameter")
    return 0 if g.dtype == BF16 else 1


def _adam_master_items_ok(items):
    _req(len(items) > 0, "adamw master multi: an empty tensor list")
    gdt = None
    for it in items:
        d = _adam_master_ok(*it, "adamw master multi")
        _req(gdt in (None, d), "adamw master multi: the gradients of one launch share a dtype")
        gdt = d
        _req(all(t.data_ptr() % 16 == 0 for t in it), "adamw master multi: 16-byte aligned tensors")
    return gdt


def adamw_master_step_multi(items, decay, w1, beta2, c2, bc2_sqrt, eps, step_size):
    """One launch of the AdamW update with f32 master weights and moments over a list of (master f32,
    param bf16, grad bf16 | f32, exp_avg f32, exp_avg_sq f32) tuples (pt_adamw_master_step_multi):
    torch's foreach f32 AdamW on the masters, then param = bf16(master).  The gradients of one list
    share a dtype.  The descriptor table is cached as adamw_step_multi's."""
    gdt = _adam_master_items_ok(items)
    _adam_launch("pt_adamw_master_step_multi", items[0][0].device, _adam_list(items, gdt),
                 (decay, w1, beta2, c2, bc2_sqrt, eps, step_size))


def adamw_master_step_multi_clip(items, sq, max_norm, decay, w1, beta2, c2, bc2_sqrt, eps, step_size, status=None):
    """adamw_master_step_multi on float(grad) * coef, coef as in grad_scale_multi: one f32 product,
    not rounded to bf16; the gradients are not modified.  A non-finite sq skips the update."""
    gdt = _adam_master_items_ok(items)
    _adam_launch("pt_adamw_master_step_multi_clip", items[0][0].device, _adam_list(items, gdt),
                 (decay, w1, beta2, c2, bc2_sqrt, eps, step_size), (sq, max_norm, status))


def adamw_master_step(master, p, grad, exp_avg, exp_avg_sq, decay, w1, beta2, c2, bc2_sqrt, eps, step_size):
    """adamw_master_step_multi for one parameter at any alignment (element by element, the same math)."""
    gdt = _adam_master_ok(master, p, grad, exp_avg, exp_avg_sq, "adamw master")
    _adam_launch("pt_adamw_master_step", p.device,
                 (_ptr(master), _ptr(p), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), p.numel(), gdt),
                 (decay, w1, beta2, c2, bc2_sqrt, eps, step_size))


def adamw_master_step_clip(master, p, grad, exp_avg, exp_avg_sq, sq, max_norm, decay, w1, beta2, c2, bc2_sqrt, eps,
                           step_size, status=None):
    """adamw_master_step on the clipped gradient."""
    gdt = _adam_master_ok(master, p, grad, exp_avg, exp_avg_sq, "adamw master")
    _adam_launch("pt_adamw_master_step_clip", p.device,
                 (_ptr(master), _ptr(p), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), p.numel(), gdt),
                 (decay, w1, beta2, c2, bc2_sqrt, eps, step_size), (sq, max_norm, status))


# ---------------------------------------------- AdamW, bf16 state with stochastic rounding
SR_STREAMS = 1 << 30   # stream ids are below this
SR_PARAM, SR_EXP_AVG, SR_EXP_AVG_SQ = 0, 1, 2   # `which` of the three stores


def _sr_key(seed, step):
    """(seed_lo, seed_hi, step) as the entries take them: a 64-bit seed, a step count t >= 1."""
    _req(int(seed) == seed and 0 <= int(seed) < 1 << 64, "stochastic rounding: the seed is an unsigned 64-bit integer")
    _req(int(step) == step and 1 <= int(step) < 1 << 32, "stochastic rounding: the step count is an integer >= 1")
    seed = int(seed)
    return seed & 0xFFFFFFFF, seed >> 32, int(step)


def _sr_stream_ok(stream):
    _req(isinstance(stream, int) and 0 <= stream < SR_STREAMS, "stochastic rounding: a stream id in [0, 2^30)")
    return stream


def _adam_sr_ok(p, g, m, v, what):
    """One (param, grad, exp_avg, exp_avg_sq) entry; returns the gradient's dtype code."""
    _req(p.dtype == m.dtype == v.dtype == BF16, f"{what}: bf16 param, exp_avg and exp_avg_sq")
    _req(g.dtype in (BF16, torch.float32), f"{what}: bf16 or f32 gradients")
    for t in (p, g, m, v):
        _req(t.is_cuda and t.device == p.device and t.is_contiguous() and t.numel() == p.numel(),
             f"{what}: contiguous device tensors of one length per parameter")
    return 0 if g.dtype == BF16 else 1


def _adam_sr_items_ok(items):
    _req(len(items) > 0, "adamw sr multi: an empty tensor list")
    gdt = None
    for it in items:
        _req(len(it) == 5, "adamw sr multi: (param, grad, exp_avg, exp_avg_sq, stream id) tuples")
        d = _adam_sr_ok(*it[:4], "adamw sr multi")
        _req(gdt in (None, d), "adamw sr multi: the gradients of one launch share a dtype")
        gdt = d
        _req(all(t.data_ptr() % 16 == 0 for t in it[:4]), "adamw sr multi: 16-byte aligned tensors")
        _sr_stream_ok(it[4])
    return gdt


def adamw_sr_step_multi(items, decay, w1, beta2, c2, bc2_sqrt, eps, step_size, seed, step):
    """One launch of the AdamW update in bf16 state with stochastic rounding over a list of (param
    bf16, grad bf16 | f32, exp_avg bf16, exp_avg_sq bf16, stream id) tuples (pt_adamw_sr_step_multi):
    adamw_master_step's f32 sequence on the widened values, the three results stored with sr_bf16
    on the Philox bits of (seed, stream id, step, element index, which output) -- see
    include/picotron_hip.h.  The gradients of one list share a dtype; the table is cached as
    adamw_step_multi's, stream ids included."""
    gdt = _adam_sr_items_ok(items)
    _adam_launch("pt_adamw_sr_step_multi", items[0][0].device, _adam_list(items, gdt),
                 (decay, w1, beta2, c2, bc2_sqrt, eps, step_size), ints=_sr_key(seed, step))


def adamw_sr_step_multi_clip(items, sq, max_norm, decay, w1, beta2, c2, bc2_sqrt, eps, step_size, seed, step,
                             status=None):
    """adamw_sr_step_multi on float(grad) * coef, coef as in grad_scale_multi: one f32 product, not
    rounded to bf16; the gradients are not modified.  A non-finite sq skips the update."""
    gdt = _adam_sr_items_ok(items)
    _adam_launch("pt_adamw_sr_step_multi_clip", items[0][0].device, _adam_list(items, gdt),
                 (decay, w1, beta2, c2, bc2_sqrt, eps, step_size), (sq, max_norm, status), ints=_sr_key(seed, step))


def adamw_sr_step(p, grad, exp_avg, exp_avg_sq, stream, decay, w1, beta2, c2, bc2_sqrt, eps, step_size, seed, step):
    """adamw_sr_step_multi for one parameter at any alignment: the same bits."""
    gdt = _adam_sr_ok(p, grad, exp_avg, exp_avg_sq, "adamw sr")
    _adam_launch("pt_adamw_sr_step", p.device, (_ptr(p), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), p.numel(), gdt),
                 (decay, w1, beta2, c2, bc2_sqrt, eps, step_size), ints=_sr_key(seed, step) + (_sr_stream_ok(stream),))


def adamw_sr_step_clip(p, grad, exp_avg, exp_avg_sq, stream, sq, max_norm, decay, w1, beta2, c2, bc2_sqrt, eps,
                       step_size, seed, step, status=None):
    """adamw_sr_step on the clipped gradient."""
    gdt = _adam_sr_ok(p, grad, exp_avg, exp_avg_sq, "adamw sr")
    _adam_launch("pt_adamw_sr_step_clip", p.device, (_ptr(p), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), p.numel(), gdt),
                 (decay, w1, beta2, c2, bc2_sqrt, eps, step_size), (sq, max_norm, status),
                 ints=_sr_key(seed, step) + (_sr_stream_ok(stream),))


def sr_cast_bf16(x, seed, step, stream, which, out=None):
    """bf16 of an f32 tensor by stochastic rounding alone (pt_sr_cast_bf16): element i of the flattened
    x is rounded with the draw the AdamW step gives element i of output `which` (SR_PARAM, SR_EXP_AVG,
    SR_EXP_AVG_SQ) of the parameter with this stream id at this step.  E[out] = x; a bf16 value
    comes out unchanged; inf and NaN take the plain cast."""
    _req(x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(), "sr_cast_bf16: a contiguous f32 device tensor")
    _req(which in (SR_PARAM, SR_EXP_AVG, SR_EXP_AVG_SQ), "sr_cast_bf16: which is 0, 1 or 2")
    if out is None:
        out = torch.empty(x.shape, dtype=BF16, device=x.device)
    _req(out.dtype == BF16 and out.is_contiguous() and out.numel() == x.numel() and out.device == x.device,
         "sr_cast_bf16: a contiguous bf16 output of x's length")
    key = _sr_key(seed, step)
    if x.numel():   # an empty tensor has no address to hand to the entry's argument check
        _C.check(_C.lib().pt_sr_cast_bf16(_ptr(x), _ptr(out), x.numel(), *key, _sr_stream_ok(stream), int(which),
                                          _C.stream_ptr(x.device)), "pt_sr_cast_bf16")
    return out


# -------------------------------------------------------------- global gradient-norm clipping
_GRAD_WS = {}   # device index -> f32 workspace of the norm pass (one partial per workgroup)


def _grad_ws(device):
    i = _dev_index(device)
    w = _GRAD_WS.get(i)
    if w is None:
        w = _GRAD_WS[i] = torch.empty(_C.lib().pt_grad_sq_workspace(), dtype=torch.float32,
                                      device=torch.device("cuda", i))
    return w


def grad_sqnorm(items=(), tensors=(), out=None, accumulate=False, weight=1.0):
    """out[0] (+)= weight * sum of g^2, in f32 and bit-reproducible (csrc/adamw.hip: per-workgroup
    partials, then one workgroup sums them in a fixed order).  items: bf16 (param, grad, exp_avg,
    exp_avg_sq) tuples as adamw_step_multi takes them -- one launch over the list on the SAME cached
    table, of which only the grad field is read (gradients alone: (g, g, g, g)), or the (master, param,
    grad, exp_avg, exp_avg_sq) tuples of adamw_master_step_multi or the (param, grad, exp_avg, exp_avg_sq,
    stream id) tuples of adamw_sr_step_multi, bf16 or f32 gradients; tensors: single
    gradients of what the list form does not take (f32, unaligned bf16).  Everything accumulates
    into the one device scalar in stream order; returns it (a [1] f32 tensor)."""
    items, tensors = list(items), list(tensors)
    _req(items or tensors, "grad_sqnorm: nothing to sum")
    dev = (items[0][1] if items else tensors[0]).device
    if out is None:
        _req(not accumulate, "grad_sqnorm: accumulate needs the scalar to add to")
        out = torch.empty(1, dtype=torch.float32, device=dev)
    _sq_ok(out, dev)
    ws, acc = _grad_ws(dev), bool(accumulate)
    if items:
        if _is_sr(items):
            name, extra = "pt_grad_sq_sr_multi", (_adam_sr_items_ok(items),)
        elif len(items[0]) == 5:   # the master-weight list: its entry takes the gradients' dtype as well
            name, extra = "pt_grad_sq_master_multi", (_adam_master_items_ok(items),)
        else:
            _adam_items_ok(items)
            name, extra = "pt_grad_sq_multi", ()
        _adam_launch(name, dev, _adam_list(items, *extra) + (float(weight), int(acc), _ptr(ws), _ptr(out)))
        acc = True
    for g in tensors:
        _req(g.device == dev, "grad_sqnorm: gradients on one device")
        _adam_launch("pt_grad_sq", dev, (_ptr(g), g.numel(), _grad_dtype(g, "grad_sqnorm"), float(weight), int(acc),
                                         _ptr(ws), _ptr(out)))
        acc = True
    return out


def grad_scale_multi(items, sq, max_norm, status=None):
    """grad = bf16(grad * coef) in place over the list (items as in grad_sqnorm), coef = min(1,
    max_norm / (sqrt(sq[0]) + 1e-6)) computed on the device; a non-finite sq leaves the gradients
    alone and posts STATUS_NONFINITE_GRAD (status: see _clip_status)."""
    _adam_items_ok(items)
    _adam_launch("pt_grad_scale_multi", items[0][1].device, _adam_list(items), clip=(sq, max_norm, status))


def grad_scale(grad, sq, max_norm, status=None):
    """grad_scale_multi for one tensor of any alignment, bf16 or f32."""
    _adam_launch("pt_grad_scale", grad.device, (_ptr(grad), grad.numel(), _grad_dtype(grad, "grad_scale")),
                 clip=(sq, max_norm, status))


# ------------------------------------------------------------------------------------ Muon
# Everything of a Muon step (csrc/muon.hip) and the host scheduler of its Newton-Schulz iteration.
# An item is (param, grad, momentum_buffer, x, lr_ratio): 2-D views with unit column stride; x is
# the matrix's workspace image from muon_x_workspace ([up(R), up(C)] bf16, zero outside [R, C]),
# where the scale kernel leaves X0, muon_newton_schulz leaves O and the apply kernel reads it.
MUON_GROUP = 4   # pt_gemm_grouped / pt_muon_poly take at most 4 problems
_MUON_DESC = {}
_MUON_WS = {}    # (up(R), up(C), device index) -> the iteration's shared buffers
_MUON_PART = {}  # device index -> f32 block partials of the momentum kernel


def muon_lr_ratio(adjust_lr_fn, shape):
    """torch.optim._muon._adjust_lr's ratio for a parameter shape: lr_adj = lr * ratio."""
    R, C = int(shape[0]), int(shape[1])
    if adjust_lr_fn is None or adjust_lr_fn == "original":
        return math.sqrt(max(1, R / C))
    if adjust_lr_fn == "match_rms_adamw":
        return 0.2 * math.sqrt(max(R, C))
    raise ValueError(f"Adjust learning rate function {adjust_lr_fn} is not supported")


def muon_x_workspace(shape, device):
    """The zero-filled [up(R), up(C)] bf16 image of one [R, C] matrix (its X0 / O)."""
    return torch.zeros(_up(shape[0]), _up(shape[1]), dtype=BF16, device=device)


def muon_group_plan(shapes):
    """Pure: [(shape, [indices])] -- the matrices of one shape, in order of first appearance, cut into
    launches of at most MUON_GROUP problems."""
    by_shape = {}
    for i, s in enumerate(shapes):
        by_shape.setdefault((int(s[0]), int(s[1])), []).append(i)
    return [(s, idx[k:k + MUON_GROUP]) for s, idx in by_shape.items() for k in range(0, len(idx), MUON_GROUP)]


def _f32_bits(x):
    """The bit pattern of f32(x): a float field of a descriptor row built from int64s."""
    return ctypes.c_uint32.from_buffer_copy(ctypes.c_float(float(x))).value


def _muon_items_ok(items):
    """The gradients' dtype code of a list of Muon items."""
    _req(len(items) > 0, "muon: an empty tensor list")
    gdt = None
    for p, g, buf, x, _ in items:
        _req(p.dim() == 2 and p.dtype == BF16 and p.is_cuda, "muon: 2-D bf16 device parameters")
        _req(g.dtype in (BF16, torch.float32) and buf.dtype == g.dtype, "muon: bf16 or f32 gradients, buffers alike")
        _req(x.dtype == BF16 and x.is_contiguous() and x.data_ptr() % 16 == 0 and
             tuple(x.shape) == (_up(p.shape[0]), _up(p.shape[1])), "muon: x is muon_x_workspace(param.shape)")
        for t in (p, g, buf):
            _req(t.shape == p.shape and t.device == p.device and t.stride(1) == 1 and t.stride(0) >= p.shape[1],
                 "muon: [R, C] views with unit column stride on one device")
        d = 0 if g.dtype == BF16 else 1
        _req(gdt in (None, d), "muon: the gradients of one launch share a dtype")
        gdt = d
    return gdt


def _muon_desc(items):
    """(device pt_muon_tensor table, device block_start, total blocks), cached per pointer set like
    _adam_desc's.  sq_slot is the item's position."""
    key = tuple((p.data_ptr(), g.data_ptr(), b.data_ptr(), x.data_ptr(), p.numel(), p.shape[1], p.stride(0),
                 g.stride(0), b.stride(0), x.stride(0), _f32_bits(r) | (i << 32))
                for i, (p, g, b, x, r) in enumerate(items))
    ent = _MUON_DESC.get(key)
    if ent is None:
        dev = items[0][0].device
        per = _C.lib().pt_muon_block_chunks()
        blocks = [0]
        for it in items:
            blocks.append(blocks[-1] + -(-((it[0].numel() + 7) // 8) // per))
        desc_h = torch.tensor([list(k) for k in key], dtype=torch.int64).pin_memory()
        block_h = torch.tensor(blocks, dtype=torch.int64).pin_memory()
        ent = (desc_h.to(dev, non_blocking=True), block_h.to(dev, non_blocking=True), blocks[-1])
        if len(_MUON_DESC) > 64:
            _MUON_DESC.clear()
        _MUON_DESC[key] = ent
    return ent


def _muon_list(items, *extra):
    desc, block_t, total = _muon_desc(items)
    return (_ptr(desc), _ptr(block_t), len(items), int(total)) + extra


def muon_momentum(items, momentum, nesterov, clip=None):
    """buf = lerp(buf, g, 1 - momentum) in place for every item and sq[i] = sum u_i^2 (f32, over the
    bf16 u = lerp(g, buf, momentum) | buf; bit-reproducible, independent of the item's position) --
    one launch over the list plus the final sum.  clip = (global sq, max_norm, status): on the
    clipped gradients; a non-finite global norm writes nothing (sq then stays the zeros it is handed).
    Returns sq, [len(items)] f32."""
    gdt = _muon_items_ok(items)
    dev = items[0][0].device
    lead = _muon_list(items, gdt)
    i = _dev_index(dev)
    part = _MUON_PART.get(i)
    if part is None or part.numel() < lead[3]:
        part = _MUON_PART[i] = torch.empty(max(lead[3], 4096), dtype=torch.float32, device=dev)
    sq = (torch.zeros if clip else torch.empty)(len(items), dtype=torch.float32, device=dev)
    tail = (float(1 - momentum), float(momentum), int(bool(nesterov)), _ptr(part), _ptr(sq))
    _adam_launch("pt_muon_momentum" + ("_clip" if clip else ""), dev, lead + tail, clip=clip)
    return sq


def muon_scale(items, sq, momentum, nesterov, eps, clip=None):
    """x_i[:R, :C] = bf16(u_i / max(sqrt(sq[i]), eps)), u recomputed from (g, buf): X0 of every item."""
    gdt = _muon_items_ok(items)
    dev = items[0][0].device
    _req(sq.dtype == torch.float32 and sq.numel() == len(items) and sq.device == dev, "muon_scale: sq of muon_momentum")
    _adam_launch("pt_muon_scale" + ("_clip" if clip else ""), dev,
                 _muon_list(items, gdt) + (float(momentum), int(bool(nesterov)), _ptr(sq), float(eps)), clip=clip)


def muon_apply(items, lr, weight_decay, clip=None):
    """p = bf16(bf16(p * (1 - lr wd)) - lr * lr_ratio * x[:R, :C]) for every item."""
    _muon_items_ok(items)
    _adam_launch("pt_muon_apply" + ("_clip" if clip else ""), items[0][0].device,
                 _muon_list(items) + (float(1 - lr * weight_decay), float(lr)), clip=clip)


def muon_poly(As, Ss, Ps, a, b, c):
    """P_i = bf16(a I + b A_i + c S_i) for up to 4 dense [m, m] matrices (A, P bf16; S f32)."""
    _req(1 <= len(As) <= MUON_GROUP and len(As) == len(Ss) == len(Ps), "muon_poly: 1 to 4 matrices")
    m = As[0].shape[0]
    for A, S, P in zip(As, Ss, Ps):
        _req(A.dtype == BF16 and P.dtype == BF16 and S.dtype == torch.float32, "muon_poly: A, P bf16 and S f32")
        _req(all(tuple(t.shape) == (m, m) and t.is_contiguous() and t.is_cuda for t in (A, S, P)),
             "muon_poly: dense [m, m] device matrices of one size")
    rc = _C.lib().pt_muon_poly(_C.ptrarr([_ptr(t) for t in As]), _C.ptrarr([_ptr(t) for t in Ss]),
                               _C.ptrarr([_ptr(t) for t in Ps]), len(As), m, float(a), float(b), float(c),
                               _C.stream_ptr(As[0].device))
    _C.check(rc, "pt_muon_poly")


def _muon_ws(Rp, Cp, device):
    key = (Rp, Cp, _dev_index(device))
    ws = _MUON_WS.get(key)
    if ws is None:
        m = min(Rp, Cp)
        ws = _MUON_WS[key] = dict(
            T=[torch.zeros(MUON_GROUP, Rp, Cp, dtype=BF16, device=device) for _ in range(2)],
            A=torch.zeros(MUON_GROUP, m, m, dtype=BF16, device=device),
            S=torch.zeros(MUON_GROUP, m, m, dtype=torch.float32, device=device),
            P=torch.zeros(MUON_GROUP, m, m, dtype=BF16, device=device))
    return ws


def _muon_gemm(label, probs, a_kcontig, b_kcontig, epilogue, mnk, dev):
    M, N, K = mnk
    n = len(probs)
    arr = (_C.GemmProblem * n)(*probs)
    rc = _timed(f"muon {label} {n}x{M}x{N}x{K}", 2.0 * n * M * N * K, float(n * _alg_bytes(M, N, K, epilogue)),
                _C.lib().pt_gemm_grouped, arr, n, int(a_kcontig), int(b_kcontig), int(epilogue), -1, _C.stream_ptr(dev))
    _C.check(rc, f"pt_gemm_grouped(muon {label}: {n} x M={M}, N={N}, K={K}, a_k={a_kcontig}, b_k={b_kcontig})")


def muon_newton_schulz(xs, ns_coefficients, ns_steps, stages=None):
    """The Newton-Schulz iteration of torch's _zeropower_via_newtonschulz on every image of xs
    (muon_x_workspace buffers holding X0; O replaces it), ns_steps times, on the GEMM launch layer:

        A = bf16(X X^T)   [m, m], m = the image's smaller side; X^T X where it has more rows than
                          columns (the wgrad layout, no transpose; images are padded to the 64-grid)
        S = f32(A A)
        P' = bf16(a I + b A + c S)                       pt_muon_poly
        X <- bf16(P' X)   (X P' for R > C)

    Images of one shape run up to MUON_GROUP per launch (muon_group_plan) through pt_gemm_grouped
    with the tile picked automatically; A, S, P' and two ping-pong X buffers are allocated once per
    shape and shared by the groups.  Nothing synchronises with the host.  stages: a dict that
    receives clones of the intermediates -- stages["X0"][i] and stages["iters"][k][name][i] for
    name in A, S, P, X and image i (the padded buffers)."""
    a, b, c = (float(v) for v in ns_coefficients)
    ns_steps = int(ns_steps)
    _req(0 <= ns_steps < 100, "muon_newton_schulz: 0 <= ns_steps < 100")
    for x in xs:
        _req(x.dtype == BF16 and x.dim() == 2 and x.is_contiguous() and x.is_cuda and _on_grid(*x.shape),
             "muon_newton_schulz: dense bf16 images on the 64-grid (muon_x_workspace)")
    if stages is not None:
        stages["X0"] = [x.clone() for x in xs]
        stages["iters"] = [{k: [None] * len(xs) for k in "ASPX"} for _ in range(ns_steps)]
    for (Rp, Cp), idx in muon_group_plan([x.shape for x in xs]):
        dev = xs[idx[0]].device
        ws = _muon_ws(Rp, Cp, dev)
        tall = Rp > Cp
        m = min(Rp, Cp)
        n = len(idx)
        own = [xs[i] for i in idx]
        A, S, P = ([ws[k][j] for j in range(n)] for k in "ASP")
        for it in range(ns_steps):
            src = own if it == 0 else [ws["T"][(it - 1) % 2][j] for j in range(n)]
            last = it == ns_steps - 1
            dst = own if last and it > 0 else [ws["T"][it % 2][j] for j in range(n)]
            if tall:   # A = X^T X: both operands stored [K = R, m]
                _muon_gemm("gram", [_problem(x, Cp, [x], [Cp], [0, m], 0, [g], [m], [0, m], m, m, Rp)
                                    for x, g in zip(src, A)], 0, 0, EPI_BF16, (m, m, Rp), dev)
            else:      # A = X X^T: the forward layout, X as activations and as weights
                _muon_gemm("gram", [_problem(x, Cp, [x], [Cp], [0, m], 0, [g], [m], [0, m], m, m, Cp)
                                    for x, g in zip(src, A)], 1, 1, EPI_BF16, (m, m, Cp), dev)
            _muon_gemm("square", [_problem(g, m, [g], [m], [0, m], 0, [s], [m], [0, m], m, m, m)
                                  for g, s in zip(A, S)], 1, 0, EPI_F32, (m, m, m), dev)
            muon_poly(A, S, P, a, b, c)
            if tall:   # X <- X P'
                _muon_gemm("update", [_problem(x, Cp, [p], [m], [0, m], 0, [y], [Cp], [0, Rp], Rp, m, m)
                                      for x, p, y in zip(src, P, dst)], 1, 0, EPI_BF16, (Rp, m, m), dev)
            else:      # X <- P' X
                _muon_gemm("update", [_problem(p, m, [x], [Cp], [0, Cp], 0, [y], [Cp], [0, m], m, Cp, m)
                                      for x, p, y in zip(src, P, dst)], 1, 0, EPI_BF16, (m, Cp, m), dev)
            if last and it == 0:   # a single iteration cannot write its own input: through T[0]
                for o, d in zip(own, dst):
                    o.copy_(d)
            if stages is not None:
                for k, ts in (("A", A), ("S", S), ("P", P), ("X", own if last else dst)):
                    for i, t in zip(idx, ts):
                        stages["iters"][it][k][i] = t.clone()
    return xs


# ------------------------------------------------------------------------------------ RoPE
def rope_(x2d, nheads, head_dim, cos, sin, seq_len, inverse=False):
    """In-place rotate the first `nheads` heads of every row of x2d ([rows, row_stride] view)."""
    _req(x2d.dtype == BF16 and x2d.stride(-1) == 1, "rope: bf16 row-major view expected")
    _req(cos.dtype == BF16 and sin.dtype == BF16 and cos.stride(-1) == 1, "rope: bf16 cos/sin tables")
    _req(cos.shape[0] >= seq_len, "rope: table shorter than the sequence")
    rows = x2d.shape[0]
    rc = _C.lib().pt_rope(_ptr(x2d), rows, x2d.stride(0), nheads, head_dim, _ptr(cos), _ptr(sin), seq_len,
                          cos.stride(0), 1 if inverse else 0, _C.stream_ptr(x2d.device))
    _C.check(rc, "pt_rope")
    return x2d


# ------------------------------------------------------------------------- QK-norm (+ RoPE)
def _qk_rows(t, nq, nk, d, name):
    _req(t.dtype == BF16 and t.is_cuda and t.dim() == 2 and t.stride(1) == 1, f"{name}: bf16 row-major device view")
    _req(t.shape[1] >= (nq + nk) * d, f"{name}: rows narrower than {nq} + {nk} heads of {d}")


def _qk_weight(w, d, name):
    _req(w.dtype == BF16 and w.is_contiguous() and w.numel() == d, f"{name}: contiguous bf16 [{d}]")


def qk_norm_rope_fwd(qkv, nq, nk, d, wq, wk, eps, mode, cos, sin, seq_len, out=None):
    """Per-head RMSNorm of the first nq + nk heads of every row of qkv ([T, >= (nq + nk) d] bf16 view;
    wq / wk [d]: the q heads' and the k heads' weight), then RoPE on the bf16 result (cos = sin = None:
    norm only).  Later columns (v) are neither read nor written.  out: where y goes -- a new
    [T, (nq + nk) d] tensor when None; may be qkv itself.  Returns (y, rstd [T, nq + nk] f32)."""
    _qk_rows(qkv, nq, nk, d, "qkv")
    _qk_weight(wq, d, "q_norm weight")
    _qk_weight(wk, d, "k_norm weight")
    T = qkv.shape[0]
    if out is None:
        out = torch.empty(T, (nq + nk) * d, dtype=BF16, device=qkv.device)
    _qk_rows(out, nq, nk, d, "out")
    _req(out.shape[0] == T, "out: one row per row of qkv")
    _req((cos is None) == (sin is None), "qk_norm_rope_fwd: cos and sin together, or neither")
    if cos is not None:
        _req(cos.dtype == BF16 and sin.dtype == BF16 and cos.stride(-1) == 1 and sin.stride() == cos.stride(),
             "qk_norm_rope_fwd: bf16 cos/sin tables of one layout")
        _req(cos.shape[0] >= seq_len, "qk_norm_rope_fwd: table shorter than the sequence")
    rstd = torch.empty(T, nq + nk, dtype=torch.float32, device=qkv.device)
    rc = _C.lib().pt_qk_norm_rope_fwd(_ptr(qkv), qkv.stride(0), _ptr(out), out.stride(0), _ptr(wq), _ptr(wk), _ptr(rstd),
                                      T, nq, nk, d, float(eps), int(mode), _ptr(cos), _ptr(sin), seq_len,
                                      cos.stride(0) if cos is not None else 0, _C.stream_ptr(qkv.device))
    _C.check(rc, "pt_qk_norm_rope_fwd")
    return out, rstd


def qk_norm_bwd(dy, x, wq, wk, rstd, nq, nk, d, mode, dx=None, need_dw=(True, True)):
    """Backward of the norm of qk_norm_rope_fwd on dy = the gradient with respect to the normed,
    un-rotated y (the first nq + nk heads of every row of dy), from the pre-norm x and the saved rstd.
    dx: where the input gradient goes (new [T, (nq + nk) d] when None; may be dy itself).  Returns
    (dx, partial_q, partial_k): the f32 per-workgroup partial rows of the two weight gradients, to be
    summed into their sinks by rmsnorm_colsum_batch (None where need_dw says the weight takes none)."""
    _qk_rows(dy, nq, nk, d, "dy")
    _qk_rows(x, nq, nk, d, "x")
    _qk_weight(wq, d, "q_norm weight")
    _qk_weight(wk, d, "k_norm weight")
    T = x.shape[0]
    _req(dy.shape[0] == T, "dy: one row per row of x")
    _req(rstd.dtype == torch.float32 and rstd.is_contiguous() and tuple(rstd.shape) == (T, nq + nk), "rstd [T, nq + nk] f32")
    if dx is None:
        dx = torch.empty(T, (nq + nk) * d, dtype=BF16, device=x.device)
    _qk_rows(dx, nq, nk, d, "dx")
    _req(dx.shape[0] == T, "dx: one row per row of x")
    lib = _C.lib()
    nparts = lib.pt_qk_norm_bwd_partials(T, nq, nk, d)
    _C.check(0 if nparts > 0 else nparts, "pt_qk_norm_bwd_partials")
    pq, pk = (torch.empty(nparts, d, dtype=torch.float32, device=x.device) if need else None for need in need_dw)
    rc = lib.pt_qk_norm_bwd(_ptr(dy), dy.stride(0), _ptr(x), x.stride(0), _ptr(wq), _ptr(wk), _ptr(rstd), _ptr(dx),
                            dx.stride(0), _ptr(pq), _ptr(pk), T, nq, nk, d, int(mode), _C.stream_ptr(x.device))
    _C.check(rc, "pt_qk_norm_bwd")
    return dx, pq, pk


# ---------------------------------------------------------------------------------- SwiGLU
def swiglu_fwd(g, u, out=None):
    rows, cols = g.shape
    h = out if out is not None else torch.empty(rows, cols, dtype=BF16, device=g.device)
    rc = _C.lib().pt_swiglu_fwd(_ptr(g), g.stride(0), _ptr(u), u.stride(0), _ptr(h), h.stride(0), rows, cols,
                                _C.stream_ptr(g.device))
    _C.check(rc, "pt_swiglu_fwd")
    return h


def swiglu_bwd(dh, g, u, dg=None, du=None):
    rows, cols = g.shape
    dh = dh if dh.stride(-1) == 1 else dh.contiguous()
    dg = dg if dg is not None else torch.empty(rows, cols, dtype=BF16, device=g.device)
    du = du if du is not None else torch.empty(rows, cols, dtype=BF16, device=g.device)
    rc = _C.lib().pt_swiglu_bwd(_ptr(dh), dh.stride(0), _ptr(g), g.stride(0), _ptr(u), u.stride(0), _ptr(dg),
                                dg.stride(0), _ptr(du), du.stride(0), rows, cols, _C.stream_ptr(g.device))
    _C.check(rc, "pt_swiglu_bwd")
    return dg, du


def residual_add(x, r):
    """bf16(x + r) of two contiguous bf16 tensors of one shape (model.py:208's residual add)."""
    _req(x.dtype == BF16 and r.dtype == BF16 and x.shape == r.shape and x.is_contiguous() and r.is_contiguous(),
         "residual_add: contiguous bf16 tensors of one shape")
    out = torch.empty_like(x)
    rc = _C.lib().pt_residual_add(_ptr(x), _ptr(r), _ptr(out), x.numel(), _C.stream_ptr(x.device))
    _C.check(rc, "pt_residual_add")
    return out


# --------------------------------------------------------------------- mixture-of-experts routing
MOE_MAX_EXPERTS, MOE_MAX_TOPK = 128, 8   # csrc/moe.hip: two experts per lane of a wave; k choices in registers
# (kind, words, device index) -> the route / plan workspace.  Every MoE layer of a device shares them: a
# workspace lives only between the launches of ONE moe_route / moe_plan call, so calls ordered on one stream
# (the training loop's: forward and backward run on torch's current stream) cannot meet in it.  MoE calls
# on two streams of one device at the same time are not supported (as for the Muon and gradient-norm
# workspaces above).
_MOE_WS = {}


def moe_capacity(T, E, k, capacity_factor):
    """Rows C each expert owns of the [E C, H] buffers: min(ceil64(T), max(64, ceil64(cf T k / E))).
    Items past an expert's C are dropped.  cf >= E / k gives ceil64(T), which never drops (a token
    picks an expert at most once): the dropless setting, at E / k times the GEMM work."""
    T, E, k = int(T), int(E), int(k)
    _req(T >= 1 and E >= 1 and 1 <= k <= E, "moe_capacity: T >= 1 and 1 <= k <= E")
    _req(capacity_factor > 0 and math.isfinite(capacity_factor), "moe_capacity: a finite capacity_factor > 0")
    return min(_up(T), max(GRID, _up(math.ceil(capacity_factor * T * k / E))))


def _moe_sizes(E, k, what):
    _req(1 <= E <= MOE_MAX_EXPERTS, f"{what}: 1 <= num_experts <= {MOE_MAX_EXPERTS}, got {E}")
    _req(1 <= k <= min(E, MOE_MAX_TOPK), f"{what}: 1 <= k <= min(num_experts, {MOE_MAX_TOPK}), got {k}")


def _moe_ws(kind, words, device):
    key = (kind, int(words), _dev_index(device))
    ws = _MOE_WS.get(key)
    if ws is None:
        ws = _MOE_WS[key] = torch.empty(int(words), dtype=torch.int32, device=device)
    return ws


def _moe_rows(t, H, name):
    _req(t.dtype == BF16 and t.is_cuda and t.dim() == 2 and t.stride(1) == 1 and t.shape[1] == H,
         f"{name}: bf16 row-major device view [rows, {H}]")


def _moe_items(t, T, k, dtype, name):
    _req(t.dtype == dtype and t.is_cuda and t.is_contiguous() and tuple(t.shape) == (T, k),
         f"{name}: contiguous {dtype} [{T}, {k}]")


def moe_route(logits, k, norm_topk_prob=True):
    """logits [T, E] bf16 (a row-major view; stride >= E) -> (idx int32 [T, k], gate f32 [T, k],
    probs f32 [T, E], counts int32 [E], aux f32 [1]): the f32 softmax over all E stored values, the k
    largest stored values (ties to the lower expert, best first), their probabilities (divided by
    their sum under norm_topk_prob), the selections per expert and the Switch load-balancing loss
    aux = E sum_e (counts_e / (T k)) mean_t probs[t, e] (HF Mixtral's value is k times this)."""
    _req(logits.dtype == BF16 and logits.is_cuda and logits.dim() == 2 and logits.stride(1) == 1,
         "moe_route: logits as a bf16 row-major device view [T, E]")
    T, E = logits.shape
    k = int(k)
    _req(T >= 1, "moe_route: at least one token")
    _moe_sizes(E, k, "moe_route")
    dev = logits.device
    lib = _C.lib()
    idx = torch.empty(T, k, dtype=torch.int32, device=dev)
    gate = torch.empty(T, k, dtype=torch.float32, device=dev)
    probs = torch.empty(T, E, dtype=torch.float32, device=dev)
    counts = torch.empty(E, dtype=torch.int32, device=dev)
    aux = torch.empty(1, dtype=torch.float32, device=dev)
    words = lib.pt_moe_route_workspace(T, E)
    _C.check(0 if words > 0 else words, "pt_moe_route_workspace")
    rc = lib.pt_moe_route(_ptr(logits), logits.stride(0), T, E, k, int(bool(norm_topk_prob)), _ptr(idx), _ptr(gate),
                          _ptr(probs), _ptr(counts), _ptr(aux), _ptr(_moe_ws("route", words, dev)), _C.stream_ptr(dev))
    _C.check(rc, "pt_moe_route")
    return idx, gate, probs, counts, aux


def moe_plan(idx, E, C):
    """idx int32 [T, k] -> (slot int32 [T, k], src int32 [E C]).  Item i = t k + j takes position
    pos = the number of earlier items with its expert; slot = e C + pos, or -1 when pos >= C (dropped);
    src[slot] = i, -1 for the rows nobody fills."""
    _req(idx.dim() == 2, "moe_plan: idx [T, k]")
    T, k = idx.shape
    E, C = int(E), int(C)
    _moe_items(idx, T, k, torch.int32, "idx")
    _req(T >= 1 and C >= 1, "moe_plan: at least one token and one row per expert")
    _moe_sizes(E, k, "moe_plan")
    dev = idx.device
    lib = _C.lib()
    slot = torch.empty(T, k, dtype=torch.int32, device=dev)
    src = torch.empty(E * C, dtype=torch.int32, device=dev)
    words = lib.pt_moe_plan_workspace(T, E, k)
    _C.check(0 if words > 0 else words, "pt_moe_plan_workspace")
    rc = lib.pt_moe_plan(_ptr(idx), T, E, k, C, _ptr(slot), _ptr(src), _ptr(_moe_ws("plan", words, dev)),
                         _C.stream_ptr(dev))
    _C.check(rc, "pt_moe_plan")
    return slot, src


def moe_dispatch(x, src, k, out=None):
    """xe[r] = x[src[r] // k] (a bit copy of token rows into their experts' rows), zeros where
    src[r] < 0.  x [T, H] bf16, H % 64 == 0 -> xe [len(src), H]."""
    _req(x.dim() == 2, "moe_dispatch: x [T, H]")
    T, H = x.shape
    _moe_rows(x, H, "x")
    _req(H % GRID == 0, f"moe_dispatch: H % {GRID} == 0")
    _req(src.dtype == torch.int32 and src.is_cuda and src.dim() == 1 and src.is_contiguous(), "src: contiguous int32 [E C]")
    R = src.shape[0]
    xe = out if out is not None else torch.empty(R, H, dtype=BF16, device=x.device)
    _moe_rows(xe, H, "out")
    _req(xe.shape[0] == R, "out: one row per entry of src")
    rc = _C.lib().pt_moe_dispatch(_ptr(x), x.stride(0), _ptr(src), _ptr(xe), xe.stride(0), T, int(k), R, H,
                                  _C.stream_ptr(x.device))
    _C.check(rc, "pt_moe_dispatch")
    return xe


def moe_combine(ye, slot, gate=None, residual=None):
    """y[t] = bf16(residual[t] + sum_j gate[t, j] ye[slot[t, j]]) over the kept items (slot >= 0), f32
    in j order, one rounding.  gate None: weights of 1 -- the backward of moe_dispatch,
    dx[t] = sum_j dxe[slot[t, j]]."""
    _req(ye.dim() == 2 and slot.dim() == 2, "moe_combine: ye [E C, H], slot [T, k]")
    R, H = ye.shape
    T, k = slot.shape
    _moe_rows(ye, H, "ye")
    _req(H % GRID == 0, f"moe_combine: H % {GRID} == 0")
    _moe_items(slot, T, k, torch.int32, "slot")
    if gate is not None:
        _moe_items(gate, T, k, torch.float32, "gate")
    if residual is not None:
        _moe_rows(residual, H, "residual")
        _req(residual.shape[0] == T, "residual: one row per token")
    y = torch.empty(T, H, dtype=BF16, device=ye.device)
    rc = _C.lib().pt_moe_combine(_ptr(ye), ye.stride(0), _ptr(slot), _ptr(gate), _ptr(residual),
                                 residual.stride(0) if residual is not None else 0, _ptr(y), H, T, k, R, H,
                                 _C.stream_ptr(ye.device))
    _C.check(rc, "pt_moe_combine")
    return y


def moe_combine_bwd(dy, ye, slot, src, gate):
    """Backward of moe_combine's weighted sum: (dye [E C, H] = bf16(gate[item] dy[token]) per filled
    row, zeros for empty ones; dgate f32 [T, k] = <dy[t], ye[slot[t, j]]>, 0 for dropped items)."""
    _req(ye.dim() == 2 and slot.dim() == 2, "moe_combine_bwd: ye [E C, H], slot [T, k]")
    R, H = ye.shape
    T, k = slot.shape
    _moe_rows(ye, H, "ye")
    _moe_rows(dy, H, "dy")
    _req(H % GRID == 0, f"moe_combine_bwd: H % {GRID} == 0")
    _req(dy.shape[0] == T, "dy: one row per token")
    _moe_items(slot, T, k, torch.int32, "slot")
    _moe_items(gate, T, k, torch.float32, "gate")
    _req(src.dtype == torch.int32 and src.is_cuda and src.is_contiguous() and tuple(src.shape) == (R,),
         "src: contiguous int32 [E C]")
    dye = torch.empty(R, H, dtype=BF16, device=ye.device)
    dgate = torch.empty(T, k, dtype=torch.float32, device=ye.device)
    rc = _C.lib().pt_moe_combine_bwd(_ptr(dy), dy.stride(0), _ptr(ye), ye.stride(0), _ptr(slot), _ptr(src), _ptr(gate),
                                     _ptr(dye), H, _ptr(dgate), T, k, R, H, _C.stream_ptr(ye.device))
    _C.check(rc, "pt_moe_combine_bwd")
    return dye, dgate


def moe_route_bwd(dgate, probs, idx, counts, d_aux=None, norm_topk_prob=True):
    """dlogits bf16 [T, E]: the backward of moe_route's gate (selection fixed at idx, renormalisation,
    softmax) on dgate [T, k], plus d_aux (an f32 device scalar, read on the device; None: 0) times
    the gradient of aux, which flows through the mean probabilities only."""
    _req(probs.dim() == 2 and idx.dim() == 2, "moe_route_bwd: probs [T, E], idx [T, k]")
    T, E = probs.shape
    k = idx.shape[1]
    _moe_sizes(E, k, "moe_route_bwd")
    _moe_items(probs, T, E, torch.float32, "probs")
    _moe_items(idx, T, k, torch.int32, "idx")
    _moe_items(dgate, T, k, torch.float32, "dgate")
    _req(counts.dtype == torch.int32 and counts.is_cuda and counts.is_contiguous() and counts.numel() == E,
         "counts: contiguous int32 [E]")
    if d_aux is not None:
        _req(d_aux.dtype == torch.float32 and d_aux.is_cuda and d_aux.numel() == 1, "d_aux: an f32 device scalar")
    dlogits = torch.empty(T, E, dtype=BF16, device=probs.device)
    rc = _C.lib().pt_moe_route_bwd(_ptr(dgate), _ptr(probs), _ptr(idx), _ptr(counts), _ptr(d_aux),
                                   int(bool(norm_topk_prob)), _ptr(dlogits), E, T, E, k, _C.stream_ptr(probs.device))
    _C.check(rc, "pt_moe_route_bwd")
    return dlogits


# ---------------------------------------------------------------------------- device status
STATUS_BAD_TARGET = 1   # PT_STATUS_BAD_TARGET (include/picotron_hip.h)
STATUS_NONFINITE_GRAD = 2   # PT_STATUS_NONFINITE_GRAD
_STATUS = {}


def _dev_index(device):
    device = torch.device(device) if device is not None else torch.device("cuda")
    return device.index if device.index is not None else torch.cuda.current_device()


def status_word(device):
    """The per-device int32 status word data-validating kernels OR their error bits into."""
    _status_poll(device)   # an error an earlier launch posted raises before the next launch
    w = _STATUS.get(_dev_index(device))
    if w is None:
        w = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", _dev_index(device)))
        _STATUS[_dev_index(device)] = w
    return w


_STATUS_HOST = {}   # device index -> pinned int32 mirror of the status word (async D2H copies)


def _status_posted(device):
    """After a validating launch: copy the status word into its pinned host mirror on the same
    stream, without a host sync.  The next validating call reads the mirror (see _status_poll), so a
    bad target raises one call later even on the drop-in path, whose train.py never calls
    check_device_status -- as torch's own asynchronous device-side assert surfaces at a later op."""
    i = _dev_index(device)
    h = _STATUS_HOST.get(i)
    if h is None:
        h = _STATUS_HOST[i] = torch.zeros(1, dtype=torch.int32).pin_memory()
    h.copy_(status_word(device), non_blocking=True)


def _status_poll(device):
    """Raise if a copy that has already landed in the pinned mirror carries an error bit."""
    h = _STATUS_HOST.get(_dev_index(device))
    if h is not None and int(h[0]):
        check_device_status(device)


def device_status(device=None, reset=True):
    """Read (a host synchronisation) and optionally clear the status word of `device`."""
    w = _STATUS.get(_dev_index(device))
    if w is None:
        return 0
    v = int(w.item())
    if reset and v:
        w.zero_()
        h = _STATUS_HOST.get(_dev_index(device))
        if h is not None:
            h.zero_()   # every copy into it was enqueued before the item() sync above
    return v


def check_device_status(device=None):
    """Raise what torch's device-side asserts would have: called where the host synchronises anyway
    (train.train_step after the step's loss read) or by anyone after a suspicious NaN."""
    v = device_status(device)
    if v & STATUS_BAD_TARGET:
        raise _C.HipKernelError("cross_entropy: a target index is outside [0, vocab) and is not ignore_index "
                                "(torch: 'Assertion `t >= 0 && t < n_classes` failed'); its row loss and "
                                "gradient were set to NaN")
    if v & STATUS_NONFINITE_GRAD:
        raise _C.HipKernelError("gradient clipping: the global gradient norm is not finite (inf or NaN); the "
                                "optimizer step (or the in-place scale) it belonged to was skipped")
    if v:
        raise _C.HipKernelError(f"device status word {v:#x}")


# ---------------------------------------------------------------------------- cross entropy
# Auxiliary z-loss: every wrapper below takes z_loss (a finite Python float >= 0; the kernels get it as
# an f32).  With z_loss == 0 a wrapper calls and returns exactly what it did without the keyword; with
# z_loss > 0 it calls the _z entry point, the loss includes z_loss * lse^2 per valid row, and the
# wrappers that produce a loss return one more element: the z part, f32, reduced like the loss.
def z_coef(z_loss):
    """z_loss as the float the kernels receive (its f32 value); ValueError unless finite and >= 0."""
    if isinstance(z_loss, bool) or not isinstance(z_loss, (int, float)):
        raise ValueError(f"cross_entropy: z_loss must be a Python float (float(x) of a numpy scalar or a tensor), got "
                         f"{type(z_loss).__name__} {z_loss!r}")
    if not math.isfinite(z_loss) or z_loss < 0:
        raise ValueError(f"cross_entropy: z_loss must be a finite float >= 0, got {z_loss!r}")
    z = ctypes.c_float(z_loss).value
    if not math.isfinite(z):
        raise ValueError(f"cross_entropy: z_loss {z_loss!r} is not finite in f32")
    return z


def _ce_native(name, device, args, z=0.0, row_z=None, what=None):
    """One CE native call on torch's current stream: name(*args, stream) when z == 0; with z > 0 its _z
    namesake, which takes z (and row_z [rows] f32, where the entry point writes one) between args and
    the stream."""
    if z > 0:
        name, args = name + "_z", (*args, z) if row_z is None else (*args, z, _ptr(row_z))
    rc = getattr(_C.lib(), name)(*args, _C.stream_ptr(device))
    _C.check(rc, what or name)


def _ce_fwd_args(rows, targets, stats=None, vocab=None):
    """The forward forms' shared checks: int64 targets [rows] (returned contiguous) and, where given,
    the lm_head GEMM's statistics f32 [nblk, rows, 2] with nblk dividing vocab."""
    _req(targets.dtype == torch.int64 and targets.numel() == rows, "targets: int64 [rows]")
    if stats is not None:
        _req(stats.dtype == torch.float32 and stats.is_contiguous() and stats.dim() == 3 and stats.shape[1:] == (rows, 2)
             and vocab % stats.shape[0] == 0, "stats: f32 [nblk, rows, 2]")
    return targets.contiguous()


def _ce_bwd_args(rows, targets, row_lse, scale_dev):
    """The LSE backward forms' shared checks: an f32 scale (one element or [rows]) and the saved f32
    row_lse [rows]; returns (targets, scale_dev) contiguous."""
    targets = targets.contiguous()
    _req(scale_dev.dtype == torch.float32 and scale_dev.numel() in (1, rows), "scale: f32 device scalar or [rows]")
    _req(row_lse.dtype == torch.float32 and row_lse.is_contiguous() and row_lse.numel() == rows, "row_lse: f32 [rows]")
    return targets, scale_dev.contiguous()


def cross_entropy_fwd_bwd(logits, targets, scale=1.0, ignore_index=-100, inplace=True, z_loss=0.0):
    """logits [rows, V] bf16, targets [rows] int64.  Returns (loss (f32 scalar tensor, mean over
    valid rows, *not* multiplied by scale), dlogits (aliases logits when inplace), inv_count); with
    z_loss > 0 the loss and dlogits carry the z term and a fourth element is the mean z part."""
    z = z_coef(z_loss)
    _bf16_rowmajor(logits, "logits")
    targets = targets.contiguous().to(torch.int64)
    rows, vocab = logits.shape
    valid = (targets != ignore_index)
    inv_count = (1.0 / valid.sum().clamp_min(1).to(torch.float32)).reshape(1)
    row_loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
    dlogits = logits if inplace else torch.empty_like(logits)
    row_z = torch.empty(rows, dtype=torch.float32, device=logits.device) if z > 0 else None
    _ce_native("pt_cross_entropy_fwd_bwd", logits.device,
               (_ptr(logits), logits.stride(0), _ptr(targets), _ptr(dlogits), dlogits.stride(0), _ptr(row_loss), rows,
                vocab, float(scale), _ptr(inv_count), int(ignore_index), _ptr(status_word(logits.device))), z, row_z)
    _status_posted(logits.device)
    loss = row_loss.sum() * inv_count[0]
    return (loss, dlogits, inv_count) if row_z is None else (loss, dlogits, inv_count, row_z.sum() * inv_count[0])


def cross_entropy_loss(logits, targets, ignore_index=-100):
    """Forward only: (mean loss f32 scalar tensor, inv_count [1] f32) -- one read of the logits."""
    _bf16_rowmajor(logits, "logits")
    rows, vocab = logits.shape
    targets = _ce_fwd_args(rows, targets)
    inv_count = (1.0 / (targets != ignore_index).sum().clamp_min(1).to(torch.float32)).reshape(1)
    row_loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
    _ce_native("pt_cross_entropy_fwd_bwd", logits.device,
               (_ptr(logits), logits.stride(0), _ptr(targets), None, 0, _ptr(row_loss), rows, vocab, 1.0, None,
                int(ignore_index), _ptr(status_word(logits.device))), what="pt_cross_entropy_fwd_bwd(loss)")
    _status_posted(logits.device)
    return row_loss.sum() * inv_count[0], inv_count


def _ce_mean(row_loss, targets, ignore_index, out_dtype, reduce_sum=False):
    """(mean loss over the valid rows in out_dtype, inv_count [1] f32) in one launch
    (reduce_sum: the sum of the row losses, inv_count 1)."""
    rows = row_loss.numel()
    _req(out_dtype in (BF16, torch.float32), "cross_entropy: loss dtype bf16 / f32")
    inv_count = torch.empty(1, dtype=torch.float32, device=row_loss.device)
    loss = torch.empty((), dtype=out_dtype, device=row_loss.device)
    rc = _C.lib().pt_cross_entropy_mean(_ptr(row_loss), _ptr(targets), rows, int(ignore_index), None, _ptr(inv_count),
                                        _ptr(loss), int(out_dtype == BF16), int(bool(reduce_sum)),
                                        _C.stream_ptr(row_loss.device))
    _C.check(rc, "pt_cross_entropy_mean")
    return loss, inv_count


def _ce_reduce(row_loss, targets, ignore_index, out_dtype, reduction):
    """F.cross_entropy's reduction of the per-row losses (ignored rows hold 0): 'mean' / 'sum' in one
    launch -> (loss scalar, inv_count [1]); 'none' -> (row losses in out_dtype, None)."""
    if reduction == "none":
        return (row_loss if out_dtype == torch.float32 else row_loss.to(out_dtype)), None
    _req(reduction in ("mean", "sum"), f"cross_entropy: reduction {reduction!r}")
    return _ce_mean(row_loss, targets, ignore_index, out_dtype, reduce_sum=reduction == "sum")


def _ce_lse_result(row_loss, row_lse, row_z, targets, ignore_index, out_dtype, reduction):
    """What the forward forms that save the LSE return: (loss, inv_count, row_lse) by _ce_reduce and, when
    there is a z part (row_z), its f32 reduction as a fourth element."""
    # no clamp: every target ignored gives 0 * inf = nan, as F.cross_entropy's mean does (grads 0)
    loss, inv_count = _ce_reduce(row_loss, targets, ignore_index, out_dtype, reduction)
    if row_z is None:
        return loss, inv_count, row_lse
    return loss, inv_count, row_lse, _ce_reduce(row_z, targets, ignore_index, torch.float32, reduction)[0]


def cross_entropy_loss_lse(logits, targets, ignore_index=-100, out_dtype=torch.float32, reduction="mean", z_loss=0.0):
    """Forward of the autograd pair: (mean loss f32 scalar tensor, inv_count [1] f32, row_lse [rows]
    f32) from one streaming read of the logits (online max / sum-exp); z_loss > 0: (loss with the z
    term, inv_count, row_lse, z_part)."""
    z = z_coef(z_loss)
    _bf16_rowmajor(logits, "logits")
    rows, vocab = logits.shape
    targets = _ce_fwd_args(rows, targets)
    row_loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
    row_lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
    row_z = torch.empty(rows, dtype=torch.float32, device=logits.device) if z > 0 else None
    _ce_native("pt_cross_entropy_fwd_lse", logits.device,
               (_ptr(logits), logits.stride(0), _ptr(targets), _ptr(row_loss), _ptr(row_lse), rows, vocab,
                int(ignore_index), _ptr(status_word(logits.device))), z, row_z)
    _status_posted(logits.device)
    return _ce_lse_result(row_loss, row_lse, row_z, targets, ignore_index, out_dtype, reduction)


def cross_entropy_grad_lse(logits, targets, row_lse, scale_dev, ignore_index=-100, z_loss=0.0):
    """dlogits = (exp(x - row_lse) - onehot) * scale_dev[0] (one f32 device scalar) or
    * scale_dev[row] (f32 [rows]: reduction='none'): elementwise, no row reduction.  z_loss > 0: the
    softmax term times 1 + 2 z_loss row_lse."""
    z = z_coef(z_loss)
    _bf16_rowmajor(logits, "logits")
    rows, vocab = logits.shape
    targets, scale_dev = _ce_bwd_args(rows, targets, row_lse, scale_dev)
    dl = torch.empty(rows, vocab, dtype=BF16, device=logits.device)
    _ce_native("pt_cross_entropy_bwd_lse", logits.device,
               (_ptr(logits), logits.stride(0), _ptr(targets), _ptr(row_lse), _ptr(dl), dl.stride(0), rows, vocab,
                _ptr(scale_dev), int(scale_dev.numel() != 1), int(ignore_index)), z)
    return dl


def cross_entropy_grad(logits, targets, scale_dev, ignore_index=-100):
    """dlogits = (softmax - onehot) * scale_dev[0] (a device scalar, e.g. grad_output / #valid)."""
    _bf16_rowmajor(logits, "logits")
    rows, vocab = logits.shape
    targets = targets.contiguous()
    _req(scale_dev.dtype == torch.float32 and scale_dev.numel() == 1, "scale: f32 device scalar")
    scale_dev = scale_dev.contiguous()
    dl = torch.empty(rows, vocab, dtype=BF16, device=logits.device)
    row_loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
    _ce_native("pt_cross_entropy_fwd_bwd", logits.device,
               (_ptr(logits), logits.stride(0), _ptr(targets), _ptr(dl), dl.stride(0), _ptr(row_loss), rows, vocab, 1.0,
                _ptr(scale_dev), int(ignore_index), _ptr(status_word(logits.device))), what="pt_cross_entropy_fwd_bwd(grad)")
    _status_posted(logits.device)
    return dl


# ------------------------------------------------------------------------------------ GEMM
EPI_BF16, EPI_BF16_ACC, EPI_F32, EPI_F32_ACC, EPI_BF16_RES = 0, 1, 2, 3, 4


class GemmProbe:
    """Live timing of every GEMM launch (bench.py's roofline): a pair of HIP events recorded on
    the launch stream around each pt_gemm call, plus its algorithmic FLOPs (2*M*N*K)."""

    def __init__(self, only=None):
        self.records = []
        self.only = only   # a launch label: time only launches of that kind (bench.py's timed steps)

    def __enter__(self):
        global _PROBE
        _PROBE = self
        return self

    def __exit__(self, *exc):
        global _PROBE
        _PROBE = None

    def summary(self):
        torch.cuda.synchronize()
        ms = [r[0].elapsed_time(r[1]) for r in self.records]
        flops = [r[2] for r in self.records]
        byts = [r[3] for r in self.records]
        n = len(ms)
        return {"launches": n, "total_ms": sum(ms), "total_flop": sum(flops),
                "avg_ms": sum(ms) / max(n, 1), "avg_flop": sum(flops) / max(n, 1),
                "avg_alg_bytes": sum(byts) / max(n, 1)}

    def label_stats(self, label):
        """Launches of one label: {launches, total_ms, avg_ms, avg_flop, avg_alg_bytes}."""
        torch.cuda.synchronize()
        rs = [r for r in self.records if r[4] == label]
        n = max(len(rs), 1)
        ms = [r[0].elapsed_time(r[1]) for r in rs]
        return {"launches": len(rs), "total_ms": sum(ms), "avg_ms": sum(ms) / n,
                "avg_flop": sum(r[2] for r in rs) / n, "avg_alg_bytes": sum(r[3] for r in rs) / n}

    def by_label(self):
        """{label: (launches, total ms, TF/s)} -- which GEMM shapes / launch kinds take the time."""
        torch.cuda.synchronize()
        out = {}
        for r in self.records:
            n, t, f = out.get(r[4], (0, 0.0, 0.0))
            out[r[4]] = (n + 1, t + r[0].elapsed_time(r[1]), f + r[2])
        return {k: (n, round(t, 4), round(f / (t * 1e-3) / 1e12, 1)) for k, (n, t, f) in
                sorted(out.items(), key=lambda kv: -kv[1][1])}


def _alg_bytes(M, N, K, epilogue):
    """Algorithmic HBM bytes of one GEMM launch: A and B read once, C written once (read too when
    accumulating / adding a residual; f32 for the main_grad epilogues; the SwiGLU epilogues move
    two [M, N] bf16 tensors more)."""
    elem = 4 if epilogue in (EPI_F32, EPI_F32_ACC) else 2
    c = M * N * elem * (2 if epilogue in (EPI_BF16_ACC, EPI_F32_ACC, EPI_BF16_RES) else 1)
    if epilogue == 5:      # gate|up: reads x, Wg, Wu; writes g|u and h
        c = M * N * 2 + M * (N // 2) * 2
    elif epilogue == 6:    # down dX: reads g|u, writes dg|du
        c = 4 * M * N * 2
    return 2 * (M * K + N * K) + c


_PROBE = None


def _timed(label, flops, nbytes, launch, *args):
    """launch(*args), between two HIP events on the current stream when a GemmProbe is active and
    times this label -- the one place a probe record is made.  Without a probe: one global read and
    a branch.  nbytes: the launch's algorithmic bytes, or the (M, N, K, epilogue) _alg_bytes takes, worked
    out only for a record.  A launch that raises leaves no record."""
    p = _PROBE
    if p is None or (p.only is not None and p.only != label):
        return launch(*args)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = launch(*args)
    ev1.record()
    p.records.append((ev0, ev1, flops, _alg_bytes(*nbytes) if isinstance(nbytes, tuple) else nbytes, label))
    return out


def _gemm(A, lda, a_kcontig, Bs, ldbs, b_bounds, b_kcontig, b_seg_dim, Cs, ldcs, c_bounds, M, N, K, epilogue,
          tile=-1, residual=None, ldr=0):
    rc = _timed(f"gemm {M}x{N}x{K} e{epilogue} t{tile}", 2.0 * M * N * K, (M, N, K, epilogue), _C.lib().pt_gemm, _ptr(A), lda, int(a_kcontig), _C.ptrarr([_ptr(b) for b in Bs]), _C.i64arr(ldbs),
                _C.i64arr(b_bounds), len(Bs), int(b_kcontig), int(b_seg_dim), _C.ptrarr([_ptr(c) for c in Cs]),
                _C.i64arr(ldcs), _C.i64arr(c_bounds), len(Cs), M, N, K, int(epilogue), _ptr(residual), int(ldr),
                int(tile), _C.stream_ptr(A.device))
    _C.check(rc, f"pt_gemm(M={M}, N={N}, K={K}, a_k={a_kcontig}, b_k={b_kcontig}, epi={epilogue})")


def _bounds(sizes):
    out = [0]
    for s in sizes:
        out.append(out[-1] + int(s))
    return out


# ------------------------------------------------------------------ shapes off the 64-element grid
# Every GEMM tile is a multiple of 64 in M, N and K (the smallest tile is 64x64, the K-tile 64), so a
# projection whose T, width or K is not (Llama-2-7B at tp 8: a vocab shard of 4000, an intermediate
# shard of 1376; an odd token count) runs on zero-padded copies: the padding adds zero products
# (the real outputs are the unpadded kernel's, bit for bit, K-order unchanged) and is sliced off.  The
# layer shapes of picotron's configs tile and never take this path.
GRID = 64


def _up(n):
    return -(-int(n) // GRID) * GRID


def _on_grid(*dims):
    return all(int(d) % GRID == 0 for d in dims)


def _pad2(t, rows, cols):
    """A zero-padded contiguous [rows, cols] copy of a 2-D tensor (or the tensor when it fits)."""
    if tuple(t.shape) == (rows, cols) and t.is_contiguous():
        return t
    out = torch.zeros(rows, cols, dtype=t.dtype, device=t.device)
    out[:t.shape[0], :t.shape[1]] = t
    return out


def _pad_cols_segments(t, rows, ns):
    """[r, sum ns] with column segments of widths ns -> [rows, sum _up(n)], each segment at its
    padded offset (the segments of a stacked q|k|v or gate|up output)."""
    out = torch.zeros(rows, sum(_up(n) for n in ns), dtype=t.dtype, device=t.device)
    src = dst = 0
    for n in ns:
        out[:t.shape[0], dst:dst + n] = t[:, src:src + n]
        src, dst = src + n, dst + _up(n)
    return out


def _unpad_cols_segments(tp, rows, ns):
    """Inverse of _pad_cols_segments: the real columns of every segment, [rows, sum ns] (a copy)."""
    if len(ns) == 1:
        return tp[:rows, :ns[0]]
    parts, off = [], 0
    for n in ns:
        parts.append(tp[:rows, off:off + n])
        off += _up(n)
    return torch.cat(parts, dim=1)


def _linear_fwd_padded(x2d, weights, out, residual):
    T, K = x2d.shape
    ns = [w.shape[0] for w in weights]
    Tp, Kp = _up(T), _up(K)
    rp = None if residual is None else _pad_cols_segments(residual, Tp, ns)
    yp = linear_fwd(_pad2(x2d, Tp, Kp), [_pad2(w, _up(n), Kp) for w, n in zip(weights, ns)], residual=rp)
    y = _unpad_cols_segments(yp, T, ns)
    if out is None:
        return y.contiguous()
    out.copy_(y)
    return out


def _linear_dgrad_padded(dy2d, weights, out, accumulate):
    T = dy2d.shape[0]
    Kin = weights[0].shape[1]
    ns = [w.shape[0] for w in weights]
    Tp, Kp = _up(T), _up(Kin)
    dxp = linear_dgrad(_pad_cols_segments(dy2d, Tp, ns), [_pad2(w, _up(n), Kp) for w, n in zip(weights, ns)])
    dx = dxp[:T, :Kin]
    if out is None:
        return dx.contiguous()
    if accumulate:   # EPI_BF16_ACC's bf16(old + bf16(new)): dx is already the bf16 product
        out.copy_(out + dx)
    else:
        out.copy_(dx)
    return out


def _linear_wgrad_padded(dy2d, x2d, outs, epilogue):
    """dW_i into the sinks outs with the epilogue's semantics: EPI_BF16 store, EPI_BF16_ACC
    bf16(old + bf16(new)), EPI_F32 store / EPI_F32_ACC old + new in f32 (the f32 product, unrounded)."""
    T = dy2d.shape[0]
    Kin = x2d.shape[1]
    ns = [o.shape[0] for o in outs]
    Tp, Kp = _up(T), _up(Kin)
    f32 = epilogue in (EPI_F32, EPI_F32_ACC)
    tmp = [torch.empty(_up(n), Kp, dtype=torch.float32 if f32 else BF16, device=dy2d.device) for n in ns]
    linear_wgrad(_pad_cols_segments(dy2d, Tp, ns), _pad2(x2d, Tp, Kp), tmp, EPI_F32 if f32 else EPI_BF16)
    for o, t, n in zip(outs, tmp, ns):
        if epilogue in (EPI_BF16_ACC, EPI_F32_ACC):
            o.copy_(o + t[:n, :Kin])
        else:
            o.copy_(t[:n, :Kin])
    return outs


def _problem(A, lda, Bs, ldbs, b_bounds, b_seg_dim, Cs, ldcs, c_bounds, M, N, K):
    pr = _C.GemmProblem()
    pr.A, pr.lda = _ptr(A), int(lda)
    for i, (b, ld) in enumerate(zip(Bs, ldbs)):
        pr.B[i], pr.ldb[i] = _ptr(b), int(ld)
    for i, v in enumerate(b_bounds):
        pr.b_bounds[i] = int(v)
    pr.nb, pr.b_seg_dim = len(Bs), int(b_seg_dim)
    for i, (c, ld) in enumerate(zip(Cs, ldcs)):
        pr.C[i], pr.ldc[i] = _ptr(c), int(ld)
    for i, v in enumerate(c_bounds):
        pr.c_bounds[i] = int(v)
    pr.nc = len(Cs)
    pr.M, pr.N, pr.K = int(M), int(N), int(K)
    return pr


def _ksplit_enabled():
    return SW.ksplit != 0


def wgrad_ksplit(mnks, extra_tiles=0):
    """K-slices for a group of wgrad problems [(M, N, K)] (K = the token count) that leaves CUs idle:
    the TP-shard weight gradients (TP = 8 at SmolLM-1.7B: q|k|v dW 24 + o_proj dW 8 tiles of 256x256,
    down_proj dW 32, gate|up dW 64, on 256 CUs) run as ksplit slices of K / ksplit -- the largest
    power of two keeping every slice >= 512 deep and the launch within one round of the 256 CUs
    (2 ... 16) -- into f32 partials that pt_gemm_splitk_reduce sums into the sink.  1 = unsplit:
    shapes that already fill half the CUs, or do not tile by 256.  extra_tiles: tiles of other
    problems sharing the launch (a dual launch's dX), counted in the round."""
    if not _ksplit_enabled() or any(m % 256 or n % 256 for m, n, _ in mnks):
        return 1
    tiles = sum((m // 256) * (n // 256) for m, n, _ in mnks)
    if tiles >= 128:
        return 1
    s = 1
    while s < 16 and tiles * s * 2 + extra_tiles <= 256 and \
            all(k % (s * 2 * 64) == 0 and k // (s * 2) >= 512 for _, _, k in mnks):
        s *= 2
    return s


def swiglu_dx_ksplit(T, I, H):
    """K-slices for the down_proj dX with the SwiGLU backward (dual launch beside the down_proj dW)
    when its 256x256 tiles fill under half the CUs -- the TP shards (TP = 8 at SmolLM-1.7B: 64
    tiles with K 2048, the launch's critical path beside 128 dW slices of K 1024): the largest power
    of two keeping the dX slices within half a round and >= 512 deep, the SwiGLU backward then in
    the reduce pass (pt_gemm_splitk_reduce mode 6).  1 = unsplit (the fused epilogue)."""
    if not _ksplit_enabled() or not SW.swiglu_splitk or T % 256 or I % 256:
        return 1
    tiles = (T // 256) * (I // 256)
    s = 1
    while s < 8 and tiles * s * 2 <= 128 and H % (s * 2 * 64) == 0 and H // (s * 2) >= 512:
        s *= 2
    return s


def hq_form(mnks, extra_tiles=0):
    """K-slices (1 or 2) for a group of few-tile problems [(M, N, K)] on the 128x128 k-substep tile
    (15), or 0 when it does not apply.  It applies where the phased 256x256 tiles leave most of the 256
    CUs idle -- fewer than 96 of them over the group: the TP shards (TP = 8 at SmolLM-1.7B: the q|k|v
    forward 48 tiles, the o_proj dX 16, the q|k|v + o_proj dW 32, gate|up dW 64) -- and every problem
    tiles by 128.  A 128x128 tile puts four times the workgroups on the CUs at the same K, so most
    of these fill the chip without K-slices; 2 slices where the 128x128 tiles still fill at most half
    a round and K >= 4096 (the q|k|v + o_proj and down_proj dW: 128 tiles).  Measured per launch
    (tools/tp_gemm_ab.py, profiles/r05/tp_gemm_ab_r05c.log), against the 256x256 K-slice forms:
    q|k|v forward 22.1 vs 34.4 us, o_proj dX 20.7 vs 25.8, q|k|v + o dW 34.4 vs 42.6, gate|up dW
    40.6 vs 49.9, down_proj dW 31.6 vs 38.6."""
    if not _ksplit_enabled() or any(m % 128 or n % 128 for m, n, _ in mnks):
        return 0
    t12 = sum((m // 256) * (n // 256) if m % 256 == 0 and n % 256 == 0 else (m * n) // 65536 for m, n, _ in mnks)
    if t12 >= 96 or any(m < 2048 and k < 2048 for m, _, k in mnks):
        return 0
    t15 = sum((m // 128) * (n // 128) for m, n, _ in mnks) + extra_tiles
    if t15 * 2 <= 256 and all(k >= 4096 and k % 256 == 0 for _, _, k in mnks):
        return 2
    return 1


def _gemm_ksplit(A, lda, a_kcontig, Bs, ldbs, b_bounds, b_kcontig, b_seg_dim, out, M, N, K, s, tile, epilogue,
                 residual=None, ldr=0):
    """C = A . B as s K-slices into f32 partials (one grouped launch of `tile`), then the reduce
    pass through `epilogue` (EPI_BF16 / EPI_BF16_ACC / EPI_BF16_RES) into out [M, N]."""
    dev = A.device
    ws = torch.empty(s * M * N, dtype=torch.float32, device=dev)
    probs = (_C.GemmProblem * 1)()
    pr = _problem(A, lda, Bs, ldbs, b_bounds, b_seg_dim, [ws], [N], [0, M], M, N, K)
    pr.ksplit, pr.kpart_stride = s, M * N
    probs[0] = pr
    _timed(f"gemm {M}x{N}x{K} ks{s}", 2.0 * M * N * K, (M, N, K, epilogue), _ksplit_launch, probs, 1, a_kcontig,
           b_kcontig, tile, [([out], [0, M], epilogue, residual, ldr)], dev)
    return out


def _reduce_sink_ok(out, residual=None):
    """pt_gemm_splitk_reduce writes 16-B (f32) / 8-B (bf16) row chunks and reads the residual the same
    way: a sink (or residual) it cannot address so -- a misaligned view -- keeps the unsplit GEMM,
    decided before anything is launched (the reduce pass would refuse it after the partial GEMM)."""
    for t in (out,) if residual is None else (out, residual):
        if t.stride(1) != 1 or t.stride(0) % 4 or t.data_ptr() % (16 if t.dtype == torch.float32 else 8):
            return False
    return True


def _splitk_reduce(pr, sink, stream):
    """The reduce pass of a K-sliced problem pr (its C[0] the f32 partials, ksplit slices kpart_stride
    apart) into its real sink (outs, row bounds, epilogue, residual, ldr): the partials summed in
    slice order over the whole chip, through the GEMM's own epilogue."""
    outs, bounds, mode, residual, ldr = sink
    rc = _C.lib().pt_gemm_splitk_reduce(ctypes.c_void_p(pr.C[0]), pr.ksplit, pr.kpart_stride, pr.M, pr.N,
                                        _C.ptrarr([_ptr(o) for o in outs]), _C.i64arr([o.stride(0) for o in outs]),
                                        _C.i64arr(bounds), len(outs), int(mode), _ptr(residual), int(ldr), stream)
    _C.check(rc, f"pt_gemm_splitk_reduce(epi {mode})")


def _ksplit_launch(probs, n, a_kcontig, b_kcontig, tile, sinks, dev):
    """The split-K problems (f32 partials, one grouped launch), then one reduce pass per problem into
    its sink (_splitk_reduce).  (Finishing a tile inside the launch -- its last-arriving slice
    summing the partials, tools/diag/ksplit_fused.patch -- measured 12-20 % slower at TP = 8: one
    workgroup per tile then does the whole reduction after the other slices have left the CUs.)"""
    stream = _C.stream_ptr(dev)
    rc = _C.lib().pt_gemm_grouped(probs, n, int(a_kcontig), int(b_kcontig), EPI_F32, int(tile), stream)
    _C.check(rc, f"pt_gemm_grouped({n} problems, split-K {probs[0].ksplit})")
    for j in range(n):
        _splitk_reduce(probs[j], sinks[j], stream)


def _wgrad_ksplit_run(jobs, epilogue, s, tile=-1):
    """The wgrad jobs [(dy2d, x2d, outs)] as s-way split-K problems of ONE grouped launch (f32
    partials in one workspace; tile -1: the auto pick), then one reduce pass per job into its outs
    through `epilogue`."""
    dev = jobs[0][0].device
    ws = torch.empty(s * sum(dy.shape[1] * x.shape[1] for dy, x, _ in jobs), dtype=torch.float32, device=dev)
    probs = (_C.GemmProblem * len(jobs))()
    base = 0
    for j, (dy2d, x2d, outs) in enumerate(jobs):
        n = s * dy2d.shape[1] * x2d.shape[1]
        probs[j] = _wgrad_problem(dy2d, x2d, outs, ws[base:base + n], s)
        base += n
    _timed("_wgrad_ksplit_run", *_wgrad_cost(jobs, epilogue), _ksplit_launch, probs, len(jobs), 0, 0, tile,
           [_wgrad_sink(outs, epilogue) for _, _, outs in jobs], dev)


def _wgrad_sink(outs, epilogue):
    """A K-sliced weight gradient's real sink, as _splitk_reduce takes it."""
    return outs, _bounds([o.shape[0] for o in outs]), epilogue, None, 0


def _wgrad_cost(jobs, epilogue):
    """(FLOPs, algorithmic bytes) of the wgrad jobs, for the probe."""
    mnks = [(dy.shape[1], x.shape[1], dy.shape[0]) for dy, x, _ in jobs]
    return sum(2.0 * m * n * k for m, n, k in mnks), float(sum(_alg_bytes(m, n, k, epilogue) for m, n, k in mnks))


def _wgrad_problem(dy2d, x2d, outs, part=None, s=1):
    """The GemmProblem of dW = dY^T X into outs (row segments of dW): dY and X plain [T, n] or KPair
    (two micro-batches: A K-segmented at T through A2, B through two K-segments).  part: the f32
    partials [s, N, Kin] of an s-way K-sliced launch, which then writes them instead of outs
    (_splitk_reduce finishes it)."""
    _bf16_rowmajor(dy2d, "dy")
    _bf16_rowmajor(x2d, "x")
    Nw, Kin = dy2d.shape[1], x2d.shape[1]
    ns = [o.shape[0] for o in outs]
    _req(sum(ns) == Nw and x2d.shape[0] == dy2d.shape[0], "wgrad: output rows must cover dY's width")
    if part is not None:
        Cs, ldcs, cb = [part], [Kin], [0, Nw]
    else:
        Cs, ldcs, cb = outs, [o.stride(0) for o in outs], _bounds(ns)
    if isinstance(dy2d, KPair):
        _req(isinstance(x2d, KPair) and part is None, "wgrad: dY and X paired together, unsliced")
        t = dy2d.a.shape[0]
        pr = _problem(dy2d.a, dy2d.stride(0), [x2d.a, x2d.b], [x2d.stride(0)] * 2, [0, t, 2 * t], 1, Cs, ldcs, cb,
                      Nw, Kin, 2 * t)
        pr.A2, pr.a_k2 = _ptr(dy2d.b), t
        return pr
    pr = _problem(dy2d, dy2d.stride(0), [x2d], [x2d.stride(0)], [0, Kin], 0, Cs, ldcs, cb, Nw, Kin, dy2d.shape[0])
    if part is not None:
        pr.ksplit, pr.kpart_stride = s, Nw * Kin
    return pr


def _is_paired(jobs):
    return any(isinstance(dy, KPair) for dy, _, _ in jobs)


_WGRAD_SLICED = (EPI_BF16, EPI_BF16_ACC, EPI_F32_ACC)   # the sinks the reduce pass writes


def wgrad_form(jobs, epilogue, tile=-1):
    """(tile, K-slices) of the one launch of the wgrad jobs [(dy2d, x2d, outs)], or None when a job
    is off the 64-grid (each job then runs on its own: padded, a pair as its two halves).  A pure
    function of the shapes, the sinks' alignment and the switches; `tile` is the caller's request
    (-1: the auto pick), which also keeps the launch unsliced.
      * the grid test of a KPair is on each micro-batch's T (its K-segment), not on their sum;
      * a pair runs on tile 12 (the K-segmented A: the 256x256 8-phase kernel only), unsliced;
      * few-tile groups (TP shards) on the 128x128 tile 15, in 2 K-slices where hq_form says so,
        else in wgrad_ksplit's slices of the 256x256 tiles -- slices only into sinks the reduce
        pass can address (_reduce_sink_ok), decided here, before anything is launched."""
    for dy, x, outs in jobs:
        t = dy.a.shape[0] if isinstance(dy, KPair) else dy.shape[0]
        if not _on_grid(t, x.shape[1], *[o.shape[0] for o in outs]):
            return None
    if _is_paired(jobs):
        return 12, 1
    if tile < 0 and epilogue in _WGRAD_SLICED:
        mnks = [(dy.shape[1], x.shape[1], dy.shape[0]) for dy, x, _ in jobs]
        hq = hq_form(mnks) if all(o.shape[0] % 128 == 0 for _, _, outs in jobs for o in outs) else 0
        sinks_ok = all(_reduce_sink_ok(o) for _, _, outs in jobs for o in outs)
        if hq == 2 and sinks_ok:
            return 15, 2
        if hq == 1:
            return 15, 1
        s = wgrad_ksplit(mnks)
        if s > 1 and sinks_ok:
            return -1, s
    return tile, 1


_ACC_OF = {EPI_BF16: EPI_BF16_ACC, EPI_BF16_ACC: EPI_BF16_ACC, EPI_F32: EPI_F32_ACC, EPI_F32_ACC: EPI_F32_ACC}


def _wgrad_unpaired(jobs, epilogue):
    """Paired wgrad jobs as two launches each: the first micro-batch's half through `epilogue`, the
    second's accumulating onto it."""
    for dy, x, outs in jobs:
        if isinstance(dy, KPair):
            linear_wgrad_grouped([(dy.a, x.a, outs)], epilogue)
            linear_wgrad_grouped([(dy.b, x.b, outs)], _ACC_OF[epilogue])
        else:
            linear_wgrad_grouped([(dy, x, outs)], epilogue)


def linear_wgrad_grouped(jobs, epilogue=EPI_BF16, tile=-1):
    """Several wgrad GEMMs (dW_i = dY_i^T X for each job (dy2d, x2d, outs)) in ONE launch
    (pt_gemm_grouped): e.g. dW of q|k|v (192 tiles) + dW of o_proj (64 tiles) fill 256 CUs.  A group
    that would leave most CUs idle (TP shards) runs split-K (wgrad_ksplit)."""
    form = wgrad_form(jobs, epilogue, tile)
    if form is None:   # a job off the 64-grid: every job on its own (linear_wgrad pads; a pair as its two halves)
        if _is_paired(jobs):
            _wgrad_unpaired(jobs, epilogue)
        else:
            for dy, x, outs in jobs:
                linear_wgrad(dy, x, outs, epilogue)
        return
    tile, s = form
    if s > 1:
        return _wgrad_ksplit_run(jobs, epilogue, s, tile)
    probs = (_C.GemmProblem * len(jobs))(*[_wgrad_problem(*job) for job in jobs])
    _timed("linear_wgrad_grouped", *_wgrad_cost(jobs, epilogue), _wgrad_grouped_launch, probs, jobs, epilogue, tile)


def _wgrad_grouped_launch(probs, jobs, epilogue, tile):
    rc = _C.lib().pt_gemm_grouped(probs, len(jobs), 0, 0, int(epilogue), int(tile), _C.stream_ptr(jobs[0][0].device))
    if rc in (-1, -3) and _is_paired(jobs):
        # a shape the 256x256 tile does not cover (PT_EUNSUPPORTED), or a K-segment it refuses
        # (PT_EINVAL): each micro-batch's half on its own
        return _wgrad_unpaired(jobs, epilogue)
    _C.check(rc, f"pt_gemm_grouped({len(jobs)} problems, epi={epilogue})")


def linear_fwd(x2d, weights, out=None, tile=-1, residual=None):
    """Y = x . [W_0; W_1; ...]^T  -> [T, sum N_i] (one launch; F.linear of model.py:124-126,186).
    residual [T, N]: Y = residual + x W^T (the residual add of model.py:208 in the epilogue)."""
    _bf16_rowmajor(x2d, "x")
    T, K = x2d.shape
    for w in weights:
        _req(w.dtype == BF16 and w.is_contiguous() and w.shape[1] == K, "weight must be contiguous [N, K] bf16")
    ns = [w.shape[0] for w in weights]
    N = sum(ns)
    if not _on_grid(T, K, *ns):
        if residual is not None:
            _req(tuple(residual.shape) == (T, N), "residual shape")
        return _linear_fwd_padded(x2d, weights, out, residual)
    y = out if out is not None else torch.empty(T, N, dtype=BF16, device=x2d.device)
    _req(y.stride(1) == 1 and y.shape == (T, N), "out shape")
    epi, ldr = EPI_BF16, 0
    if residual is not None:
        _bf16_rowmajor(residual, "residual")
        _req(tuple(residual.shape) == (T, N), "residual shape")
        epi, ldr = EPI_BF16_RES, residual.stride(0)
    if out is None and tile < 0 and _splitk_enabled() and len(weights) <= 4 and \
            (residual is None or residual.is_contiguous()):
        h = _splitk_halves(T, N, K)
        if h is not None:
            return _linear_fwd_splitk(x2d, weights, h, y, residual)
    hq = hq_form([(T, N, K)]) if tile < 0 and all(n % 128 == 0 for n in ns) else 0
    if hq == 1:
        tile = 15
    elif hq == 2 and _reduce_sink_ok(y, residual):
        return _gemm_ksplit(x2d, x2d.stride(0), 1, weights, [K] * len(weights), _bounds(ns), 1, 0, y, T, N, K, 2, 15,
                            epi, residual=residual, ldr=ldr)
    _gemm(x2d, x2d.stride(0), 1, weights, [K] * len(weights), _bounds(ns), 1, 0, [y], [y.stride(0)], [0, T],
          T, N, K, epi, tile, residual=residual, ldr=ldr)
    return y


EPI_SWIGLU_FWD, EPI_SWIGLU_BWD = 5, 6


def rope_fusable(T, head_dim, seq_len, widths=()):
    """The RoPE-fused q|k|v projection tiles head_dim 64 (the wave tile width) with T % 256, and the
    phased kernels need every q / k / v segment boundary on a 128-column tile edge (e.g. TP shards
    of 2 q heads + 1 kv head of 64 do not tile: the separate RoPE kernel runs instead)."""
    return head_dim == 64 and T % 256 == 0 and T % seq_len == 0 and all(w % 128 == 0 for w in widths)


# fewer 256x256 tiles than this: q|k|v + RoPE as a plain GEMM + rope kernel (PICOTRON_ROPE_FUSE_MIN_TILES)


def linear_fwd_rope(x2d, weights, cos, sin, seq_len, rot_heads, head_dim):
    """Y = x . [W_0; ...]^T with the first rot_heads heads of every row rotated by RoPE in the GEMM
    epilogue (model.py:124-126 + 136-137: the q|k|v projection, then apply_rotary_emb on q and k)."""
    _bf16_rowmajor(x2d, "x")
    T, K = x2d.shape
    for w in weights:
        _req(w.dtype == BF16 and w.is_contiguous() and w.shape[1] == K, "weight must be contiguous [N, K] bf16")
    _req(cos.dtype == BF16 and sin.dtype == BF16 and cos.stride(-1) == 1 and sin.stride(0) == cos.stride(0),
         "rope tables: bf16 [S, d]")
    _req(cos.shape[0] >= seq_len and rope_fusable(T, head_dim, seq_len), "linear_fwd_rope: shape")
    ns = [w.shape[0] for w in weights]
    N = sum(ns)
    if (T // 256) * (N // 256) < SW.rope_fuse_min_tiles:
        # a TP shard's q|k|v (TP = 8: N 768, 48 tiles of 256x256 on 256 CUs): the phased kernels
        # the RoPE epilogue needs would leave most CUs idle; the plain GEMM picks a smaller tile and
        # csrc/rope.hip rotates q|k after it (bit-identical to the fused epilogue)
        y = linear_fwd(x2d, weights)
        return rope_(y, rot_heads, head_dim, cos, sin, seq_len)
    y = torch.empty(T, N, dtype=BF16, device=x2d.device)
    rc = _timed("linear_fwd_rope", 2.0 * T * N * K, (T, N, K, EPI_BF16), _C.lib().pt_gemm_rope, _ptr(x2d), x2d.stride(0),
                _C.ptrarr([_ptr(w) for w in weights]), _C.i64arr([K] * len(weights)), _C.i64arr(_bounds(ns)),
                len(weights), _ptr(y), y.stride(0), T, N, K, _ptr(cos), _ptr(sin), cos.stride(0), seq_len,
                rot_heads * head_dim, head_dim, -1, _C.stream_ptr(x2d.device))
    _C.check(rc, "pt_gemm_rope")
    return y


EPI_CE_STATS = 8


def ce_stats_block(T, V):
    """Column tile of the lm_head GEMM's CE statistics: 256 (8-phase 256x256 kernel) when V divides,
    else 128 (4-phase 256x128); None when the shape does not tile (T % 256)."""
    if T % 256:
        return None
    return 256 if V % 256 == 0 else (128 if V % 128 == 0 else None)


def ce_stats_fusable(T, V):
    return ce_stats_block(T, V) is not None


def linear_ce_stats(x2d, weight):
    """lm_head (model.py:270) with the CE forward's statistics in the GEMM epilogue: returns (logits
    [T, V] bf16, stats [V / block, T, 2] f32 = per column tile and row (max, sum exp(x - max)) of
    the stored bf16 logits)."""
    _bf16_rowmajor(x2d, "x")
    T, K = x2d.shape
    V = weight.shape[0]
    _req(weight.dtype == BF16 and weight.is_contiguous() and weight.shape[1] == K, "weight must be contiguous [V, K] bf16")
    block = ce_stats_block(T, V)
    _req(block is not None and K % 64 == 0, "linear_ce_stats: T % 256, V % 128, K % 64")
    y = torch.empty(T, V, dtype=BF16, device=x2d.device)
    stats = torch.empty(V // block, T, 2, dtype=torch.float32, device=x2d.device)
    rc = _timed("linear_ce_stats", 2.0 * T * V * K, (T, V, K, EPI_BF16), _C.lib().pt_gemm_ce_stats, _ptr(x2d),
                x2d.stride(0), _ptr(weight), K, _ptr(y), y.stride(0), _ptr(stats), block, T, V, K,
                _C.stream_ptr(x2d.device))
    _C.check(rc, "pt_gemm_ce_stats")
    return y, stats


def cross_entropy_loss_lse_stats(logits, targets, stats, ignore_index=-100, out_dtype=torch.float32,
                                 reduction="mean", z_loss=0.0):
    """cross_entropy_loss_lse from the lm_head GEMM's statistics (linear_ce_stats): same outputs,
    the logits are not streamed again (only x[row, target] is read)."""
    z = z_coef(z_loss)
    _bf16_rowmajor(logits, "logits")
    rows, vocab = logits.shape
    targets = _ce_fwd_args(rows, targets, stats, vocab)
    row_loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
    row_lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
    row_z = torch.empty(rows, dtype=torch.float32, device=logits.device) if z > 0 else None
    _ce_native("pt_cross_entropy_fwd_stats", logits.device,
               (_ptr(logits), logits.stride(0), _ptr(targets), _ptr(stats), stats.shape[0], _ptr(row_loss), _ptr(row_lse),
                rows, vocab, int(ignore_index), _ptr(status_word(logits.device))), z, row_z)
    _status_posted(logits.device)
    return _ce_lse_result(row_loss, row_lse, row_z, targets, ignore_index, out_dtype, reduction)


def cross_entropy_vp_partial(logits_shard, targets, stats, vocab_lo):
    """One tp rank's share of the vocab-parallel CE: per row float4 (max, sum exp(x - max), x[target]
    or 0, 1 or 0: the target in this shard) of the shard logits [rows, Vs] (columns vocab_lo ..), from
    the lm_head GEMM's statistics (linear_ce_stats) -- the logits are read at x[target] only."""
    _bf16_rowmajor(logits_shard, "logits")
    rows, vs = logits_shard.shape
    targets = _ce_fwd_args(rows, targets, stats, vs)
    part = torch.empty(rows, 4, dtype=torch.float32, device=logits_shard.device)
    _ce_native("pt_cross_entropy_vp_partial", logits_shard.device,
               (_ptr(logits_shard), logits_shard.stride(0), _ptr(targets), _ptr(stats), stats.shape[0], _ptr(part), rows, vs,
                int(vocab_lo)))
    return part


def cross_entropy_vp_combine(parts, targets, vocab, ignore_index=-100, out_dtype=torch.float32, reduction="mean",
                             z_loss=0.0):
    """Every tp rank's partials [tp, rows, 4] (rank order) -> (loss, inv_count, row_lse) as
    cross_entropy_loss_lse_stats returns them for the whole [rows, vocab] logits (z_loss > 0: the z
    term from the combined LSE, and z_part as a fourth element)."""
    z = z_coef(z_loss)
    _req(parts.dtype == torch.float32 and parts.is_contiguous() and parts.dim() == 3 and parts.shape[2] == 4,
         "parts: f32 [tp, rows, 4]")
    tp, rows = parts.shape[0], parts.shape[1]
    targets = _ce_fwd_args(rows, targets)
    row_loss = torch.empty(rows, dtype=torch.float32, device=parts.device)
    row_lse = torch.empty(rows, dtype=torch.float32, device=parts.device)
    row_z = torch.empty(rows, dtype=torch.float32, device=parts.device) if z > 0 else None
    _ce_native("pt_cross_entropy_vp_combine", parts.device,
               (_ptr(parts), tp, _ptr(targets), _ptr(row_loss), _ptr(row_lse), rows, int(vocab), int(ignore_index),
                _ptr(status_word(parts.device))), z, row_z)
    _status_posted(parts.device)
    return _ce_lse_result(row_loss, row_lse, row_z, targets, ignore_index, out_dtype, reduction)


def cross_entropy_grad_lse_shard(logits_shard, targets, row_lse, scale_dev, vocab_lo, ignore_index=-100, z_loss=0.0):
    """cross_entropy_grad_lse on a vocab shard (columns vocab_lo ..): the one-hot only where the
    target falls in the shard; row_lse is the whole vocabulary's."""
    z = z_coef(z_loss)
    _bf16_rowmajor(logits_shard, "logits")
    rows, vs = logits_shard.shape
    targets, scale_dev = _ce_bwd_args(rows, targets, row_lse, scale_dev)
    dl = torch.empty(rows, vs, dtype=BF16, device=logits_shard.device)
    _ce_native("pt_cross_entropy_bwd_lse_shard", logits_shard.device,
               (_ptr(logits_shard), logits_shard.stride(0), _ptr(targets), _ptr(row_lse), _ptr(dl), dl.stride(0), rows, vs,
                int(vocab_lo), _ptr(scale_dev), int(scale_dev.numel() != 1), int(ignore_index)), z)
    return dl


def swiglu_fusable(T, I, backward=False, H=None):
    """Shapes the SwiGLU-fused projections tile (8-phase kernel: T % 256, I % 128 (fwd) / 256 (bwd),
    and the hidden size H -- the GEMM's K -- on the 64 K-tile grid)."""
    return T % 256 == 0 and I % (256 if backward else 128) == 0 and (H is None or H % GRID == 0)


# fewer 256-row x (128 fwd / 256 bwd)-column tiles than this: the SwiGLU runs as its own kernel
# beside a plain GEMM (whose auto tile fills the CUs) -- a TP shard's I (TP = 8: 1024; 128 tiles
# on 256 CUs); bit-identical either way.  The backward keeps its fused dual launch at every width
# (TP = 8 proxy: 8.95 vs 9.08 ms per micro-batch split).  PICOTRON_SWIGLU_FUSE_MIN_TILES / _BWD_MIN_TILES.


def swiglu_fuse_pays(T, I, backward=False, H=None):
    """swiglu_fusable and enough tiles that the fused (8-phase 256x256) launch fills the CUs."""
    tiles = (T // 256) * (I // (256 if backward else 128))
    return swiglu_fusable(T, I, backward, H) and \
        tiles >= (SW.swiglu_bwd_min_tiles if backward else SW.swiglu_fuse_min_tiles)


def linear_swiglu_fwd(x2d, wg, wu):
    """gate|up projection with SwiGLU in the GEMM epilogue (model.py:186): returns (gu [T, 2I] =
    [x Wg^T | x Wu^T], h = bf16(bf16(silu(g)) * u) [T, I]) in one launch."""
    _bf16_rowmajor(x2d, "x")
    T, K = x2d.shape
    I = wg.shape[0]
    for w in (wg, wu):
        _req(w.dtype == BF16 and w.is_contiguous() and tuple(w.shape) == (I, K), "gate/up weights [I, K] bf16")
    _req(swiglu_fusable(T, I, H=x2d.shape[1]), "linear_swiglu_fwd: T % 256, I % 128 and H % 64 required")
    gu = torch.empty(T, 2 * I, dtype=BF16, device=x2d.device)
    h = torch.empty(T, I, dtype=BF16, device=x2d.device)
    _gemm(x2d, x2d.stride(0), 1, [wg, wu], [K, K], [0, I, 2 * I], 1, 0, [h, gu], [I, 2 * I], [0, T], T, 2 * I, K,
          EPI_SWIGLU_FWD)
    return gu, h


def linear_dgrad_swiglu(dy2d, wd, gu):
    """dh = dY W_down (model.py:186 backward) with the SwiGLU backward in the epilogue: returns
    dgu = [dg | du] [T, 2I] (dh is never materialised)."""
    _bf16_rowmajor(dy2d, "dy")
    _bf16_rowmajor(gu, "gu")
    T, H = dy2d.shape
    I = wd.shape[1]
    _req(wd.dtype == BF16 and wd.is_contiguous() and wd.shape[0] == H, "down weight [H, I] bf16")
    _req(tuple(gu.shape) == (T, 2 * I), "gu must be [T, 2I]")
    _req(swiglu_fusable(T, I, backward=True, H=dy2d.shape[1]), "linear_dgrad_swiglu: T % 256, I % 256 and H % 64 required")
    dgu = torch.empty(T, 2 * I, dtype=BF16, device=dy2d.device)
    _gemm(dy2d, dy2d.stride(0), 1, [wd], [I], [0, I], 0, 0, [dgu], [dgu.stride(0)], [0, T], T, I, H, EPI_SWIGLU_BWD,
          residual=gu, ldr=gu.stride(0))
    return dgu


# ------------------------------------------------------------------ MoE expert GEMMs (grouped)
# Expert e's tokens are rows [e C, (e + 1) C) of the [E C, *] buffers (moe_dispatch), C on the
# 64-grid, so every expert is one plain same-layout problem: MOE_GROUP of them per pt_gemm_grouped
# launch, the tile picked over the group.  The SwiGLU rides in the epilogues where the 8-phase tile
# takes the shape (swiglu_fusable on C), else it is one strided call over the whole buffer; the two
# forms give the same bits, as for the dense MLP.
MOE_GROUP = 4   # pt_gemm_grouped takes at most 4 problems


def _moe_gemm(label, probs, a_kcontig, b_kcontig, epilogue, mnk, dev):
    M, N, K = mnk
    for lo in range(0, len(probs), MOE_GROUP):
        grp = probs[lo:lo + MOE_GROUP]
        n = len(grp)
        arr = (_C.GemmProblem * n)(*grp)
        rc = _timed(f"moe {label} {n}x{M}x{N}x{K}", 2.0 * n * M * N * K, float(n * _alg_bytes(M, N, K, epilogue)),
                    _C.lib().pt_gemm_grouped, arr, n, int(a_kcontig), int(b_kcontig), int(epilogue), -1,
                    _C.stream_ptr(dev))
        _C.check(rc, f"pt_gemm_grouped(moe {label}: {n} x M={M}, N={N}, K={K}, epi={epilogue})")


def _moe_expert_shapes(buf, ws, C, what):
    """E of an expert buffer [E C, cols] against its per-expert weights."""
    _bf16_rowmajor(buf, what)
    E = len(ws)
    _req(E >= 1 and buf.shape[0] == E * C and buf.is_contiguous(), f"{what}: contiguous [E C, cols], E = {E}, C = {C}")
    _req(C % GRID == 0 and buf.shape[1] % GRID == 0, f"{what}: C and the row width on the {GRID}-grid")
    return E


def _moe_weights(ws, shape, what):
    for w in ws:
        _req(w.dtype == BF16 and w.is_contiguous() and tuple(w.shape) == tuple(shape), f"{what}: contiguous bf16 {shape}")


def moe_experts_fwd(xe, wgs, wus, wds, C, fuse=True):
    """xe [E C, H] -> (gu [E C, 2I] = [x Wg_e^T | x Wu_e^T], hh [E C, I] = swiglu, ye [E C, H] =
    hh Wd_e^T), each expert on its own C rows."""
    E = _moe_expert_shapes(xe, wgs, C, "xe")
    H, I = xe.shape[1], wgs[0].shape[0]
    _req(len(wus) == E and len(wds) == E and I % GRID == 0, f"moe_experts_fwd: E weights each, I % {GRID} == 0")
    _moe_weights(list(wgs) + list(wus), (I, H), "gate / up weights")
    _moe_weights(wds, (H, I), "down weights")
    dev = xe.device
    gu = torch.empty(E * C, 2 * I, dtype=BF16, device=dev)
    hh = torch.empty(E * C, I, dtype=BF16, device=dev)
    ye = torch.empty(E * C, H, dtype=BF16, device=dev)
    rows = [slice(e * C, (e + 1) * C) for e in range(E)]
    if fuse and swiglu_fusable(C, I, H=H):
        _moe_gemm("gate|up+swiglu", [_problem(xe[r], H, [wg, wu], [H, H], [0, I, 2 * I], 0, [hh[r], gu[r]], [I, 2 * I],
                                              [0, C], C, 2 * I, H) for r, wg, wu in zip(rows, wgs, wus)],
                  1, 1, EPI_SWIGLU_FWD, (C, 2 * I, H), dev)
    else:
        _moe_gemm("gate|up", [_problem(xe[r], H, [wg, wu], [H, H], [0, I, 2 * I], 0, [gu[r]], [2 * I], [0, C], C, 2 * I, H)
                              for r, wg, wu in zip(rows, wgs, wus)], 1, 1, EPI_BF16, (C, 2 * I, H), dev)
        swiglu_fwd(gu[:, :I], gu[:, I:], out=hh)
    _moe_gemm("down", [_problem(hh[r], I, [wd], [I], [0, H], 0, [ye[r]], [H], [0, C], C, H, I)
                       for r, wd in zip(rows, wds)], 1, 1, EPI_BF16, (C, H, I), dev)
    return gu, hh, ye


def moe_experts_dgrad_down(dye, wds, gu, C, fuse=True):
    """dye [E C, H] -> (dgu [E C, 2I] = the SwiGLU backward of dhh = dye Wd_e on the saved gate|up,
    dhh [E C, I] or None where the epilogue-fused form never stores it)."""
    E = _moe_expert_shapes(dye, wds, C, "dye")
    H, I = dye.shape[1], wds[0].shape[1]
    _moe_weights(wds, (H, I), "down weights")
    _bf16_rowmajor(gu, "gu")
    _req(tuple(gu.shape) == (E * C, 2 * I) and gu.is_contiguous() and I % GRID == 0, "gu: contiguous [E C, 2I]")
    dev = dye.device
    dgu = torch.empty_like(gu)
    rows = [slice(e * C, (e + 1) * C) for e in range(E)]
    if fuse and swiglu_fusable(C, I, backward=True, H=H):
        probs = []
        for r, wd in zip(rows, wds):
            pr = _problem(dye[r], H, [wd], [I], [0, I], 0, [dgu[r]], [2 * I], [0, C], C, I, H)
            pr.residual, pr.ldr = _ptr(gu[r]), 2 * I
            probs.append(pr)
        _moe_gemm("down dX+swiglu", probs, 1, 0, EPI_SWIGLU_BWD, (C, I, H), dev)
        return dgu, None
    dhh = torch.empty(E * C, I, dtype=BF16, device=dev)
    _moe_gemm("down dX", [_problem(dye[r], H, [wd], [I], [0, H], 1, [dhh[r]], [I], [0, C], C, I, H)
                          for r, wd in zip(rows, wds)], 1, 0, EPI_BF16, (C, I, H), dev)
    swiglu_bwd(dhh, gu[:, :I], gu[:, I:], dg=dgu[:, :I], du=dgu[:, I:])
    return dgu, dhh


def moe_experts_dgrad_gate_up(dgu, wgs, wus, C):
    """dgu [E C, 2I] -> dxe [E C, H] = dg Wg_e + du Wu_e."""
    E = _moe_expert_shapes(dgu, wgs, C, "dgu")
    I, H = wgs[0].shape
    _req(len(wus) == E and dgu.shape[1] == 2 * I, "moe_experts_dgrad_gate_up: dgu [E C, 2I], E weights each")
    _moe_weights(list(wgs) + list(wus), (I, H), "gate / up weights")
    dev = dgu.device
    dxe = torch.empty(E * C, H, dtype=BF16, device=dev)
    _moe_gemm("gate|up dX", [_problem(dgu[e * C:(e + 1) * C], 2 * I, [wg, wu], [H, H], [0, I, 2 * I], 1,
                                      [dxe[e * C:(e + 1) * C]], [H], [0, C], C, H, 2 * I)
                             for e, (wg, wu) in enumerate(zip(wgs, wus))], 1, 0, EPI_BF16, (C, H, 2 * I), dev)
    return dxe


def _splitk_enabled():
    return SW.splitk2 != 0


def _splitk_min():
    return SW.splitk2_min


def _splitk_halves(M, N, K, min_half=None):
    """K of each half when C [M, N] = A [M, K] . B pays to split in two K halves (None if not): one
    round of 256x256 tiles for both halves together and at least PICOTRON_SPLITK2_MIN (8192) of K per
    half -- where the 256x256 8-phase rate (~17 % above the 256x128 one at long K) pays for the f32
    partials and the sum pass.  min_half overrides that floor (a caller whose halves share a launch
    with other work and whose consumer sums them)."""
    if M % 256 or N % 256 or 2 * (M // 256) * (N // 256) > 256 or K % 128:
        return None
    h = K // 2
    return h if h >= (_splitk_min() if min_half is None else min_half) else None


def _segments(sizes, lo, hi):
    """(index, offset inside it, length) of the pieces of the concatenation of `sizes` in [lo, hi)"""
    out, base = [], 0
    for i, n in enumerate(sizes):
        a, b = max(lo, base), min(hi, base + n)
        if a < b:
            out.append((i, a - base, b - a))
        base += n
    return out


def _splitk_launch(probs, b_kcontig, parts, residual, out):
    """The two K halves (f32, 256x256 tiles, one grouped launch), then the sum pass into out (none
    when out is None: the halves are left to a consumer that sums them)."""
    rc = _C.lib().pt_gemm_grouped(probs, 2, 1, b_kcontig, EPI_F32, 12, _C.stream_ptr(parts.device))
    _C.check(rc, "pt_gemm_grouped(split-K halves)")
    return parts if out is None else parts.sum(out, residual)


def _dx_halves(dy2d, weights, h):
    """dX = dY . [W_0; W_1; ...] as its two K halves dY[:, :h] . W[:h] and dY[:, h:] . W[h:] (the
    halves may cut through a weight): the two problems and their f32 results (SplitKParts)."""
    T, N = dy2d.shape
    Kin = weights[0].shape[1]
    ns = [w.shape[0] for w in weights]
    parts = [torch.empty(T, Kin, dtype=torch.float32, device=dy2d.device) for _ in range(2)]
    probs = (_C.GemmProblem * 2)()
    for i, (lo, hi) in enumerate(((0, h), (h, N))):
        segs = _segments(ns, lo, hi)
        bs = [weights[j][a:a + n] for j, a, n in segs]
        probs[i] = _problem(dy2d[:, lo:], dy2d.stride(0), bs, [Kin] * len(bs), _bounds([n for _, _, n in segs]), 1,
                            [parts[i]], [Kin], [0, T], T, Kin, hi - lo)
    return probs, SplitKParts(*parts)


def _dx_splits(T, Kin, N, weights, ns, split_min):
    """K of each half when the dX [T, Kin] = dY [T, N] . W runs as two K halves (_splitk_halves, and
    weights the halves can cut through), else None."""
    h = _splitk_halves(T, Kin, N, split_min) if _splitk_enabled() else None
    if h is not None and all(w.dtype == BF16 and w.is_contiguous() for w in weights) and all(n % 64 == 0 for n in ns):
        return h
    return None


def _linear_dgrad_splitk(dy2d, weights, h, dx, keep_parts=False):
    """dX = bf16(sum of _dx_halves) into dx: one grouped launch, then the sum pass (keep_parts: no
    sum pass, the SplitKParts for a consumer that sums them)."""
    T, N = dy2d.shape
    Kin = weights[0].shape[1]
    probs, parts = _dx_halves(dy2d, weights, h)
    if keep_parts:
        return _splitk_launch(probs, 0, parts, None, None)
    return _timed("_splitk_run", 2.0 * T * Kin * N, (T, Kin, N, EPI_BF16), _splitk_launch, probs, 0, parts, None, dx)


def _linear_fwd_splitk(x2d, weights, h, y, residual):
    """Y = bf16(x[:, :h] . W[:, :h]^T + x[:, h:] . W[:, h:]^T) (+ residual as EPI_BF16_RES): two f32
    problems on 256x256 tiles in one grouped launch, then the sum pass (which adds the residual)."""
    T, K = x2d.shape
    ns = [w.shape[0] for w in weights]
    N = sum(ns)
    parts = [torch.empty(T, N, dtype=torch.float32, device=x2d.device) for _ in range(2)]
    probs = (_C.GemmProblem * 2)()
    for i, (lo, hi) in enumerate(((0, h), (h, K))):
        probs[i] = _problem(x2d[:, lo:], x2d.stride(0), [w[:, lo:] for w in weights], [K] * len(weights), _bounds(ns),
                            0, [parts[i]], [N], [0, T], T, N, hi - lo)
    return _timed("_splitk_run", 2.0 * T * N * K, (T, N, K, EPI_BF16), _splitk_launch, probs, 1, SplitKParts(*parts),
                  residual, y)


def linear_dgrad(dy2d, weights, out=None, accumulate=False, tile=-1, keep_parts=False, split_min=None):
    """dX = dY . [W_0; W_1; ...]  where dY = [dY_0 | dY_1 | ...] is [T, sum N_i].  split_min / keep_parts
    as linear_dgrad_dual's (the dX of a dual launch whose weight gradients were deferred)."""
    _bf16_rowmajor(dy2d, "dy")
    T, N = dy2d.shape
    Kin = weights[0].shape[1]
    ns = [w.shape[0] for w in weights]
    _req(sum(ns) == N, "dgrad: dY width must equal the stacked weight rows")
    if not _on_grid(T, Kin, *ns):
        return _linear_dgrad_padded(dy2d, weights, out, accumulate)
    if out is None and not accumulate and tile < 0 and len(weights) <= 3:
        h = _dx_splits(T, Kin, N, weights, ns, split_min)
        if h is not None:
            return _linear_dgrad_splitk(dy2d, weights, h, torch.empty(T, Kin, dtype=BF16, device=dy2d.device),
                                        keep_parts=keep_parts)
    dx = out if out is not None else torch.empty(T, Kin, dtype=BF16, device=dy2d.device)
    hq = hq_form([(T, Kin, N)]) if tile < 0 and all(n % 64 == 0 for n in ns) else 0
    if hq == 1:
        tile = 15
    elif hq == 2 and _reduce_sink_ok(dx):
        return _gemm_ksplit(dy2d, dy2d.stride(0), 1, weights, [Kin] * len(weights), _bounds(ns), 0, 1, dx, T, Kin,
                            N, 2, 15, EPI_BF16_ACC if accumulate else EPI_BF16)
    _gemm(dy2d, dy2d.stride(0), 1, weights, [Kin] * len(weights), _bounds(ns), 0, 1, [dx], [dx.stride(0)],
          [0, T], T, Kin, N, EPI_BF16_ACC if accumulate else EPI_BF16, tile)
    return dx


def dual_enabled():
    """PICOTRON_DUAL=0 launches a layer's dX and dW GEMMs separately (A/B measurement only)."""
    return SW.dual != 0


# the dual launch's XCD order unless a caller picks one: 0 = dX tiles first in every XCD, 1 = dW
# first, 2 = staggered -- even XCDs dX first, odd XCDs dW first, so half the chip is in the dX tiles'
# HBM-bound SwiGLU-backward tail at a time (+0.8 % on the step over 0 / 1, profiles/r03/dual_order_ab.txt)
DUAL_ORDER = 2


def dual_fits(dgrad_mn, wgrad_mns):
    """Whether pt_gemm_dual tiles these problems: every [M, N] by 256 x 256 and each group's tile
    count a multiple of 8 (equal shares per XCD)."""
    def ok(mns):
        return all(m % 256 == 0 and n % 256 == 0 for m, n in mns) and sum(m * n for m, n in mns) // 65536 % 8 == 0
    return ok([dgrad_mn]) and ok(wgrad_mns)


def norm_splitk_enabled():
    """The post-attention norm backward takes the gate|up dX's split-K halves directly
    (PICOTRON_NORM_SPLITK=0: the sum pass + the plain norm backward, A/B only)."""
    return SW.norm_splitk != 0


class _DualRefused(Exception):
    """pt_gemm_dual answered PT_EUNSUPPORTED: nothing was launched."""


def linear_dgrad_dual(dy2d, weights, wjobs, wepilogue, gu=None, order=None, keep_parts=False, split_min=None):
    """dX = dY . [W_0; ...] (or, with gu, the SwiGLU backward dg|du of the down_proj dX:
    linear_dgrad_swiglu) AND the wgrads wjobs [(dy2d, x2d, outs)] (linear_wgrad, epilogue
    wepilogue) in ONE launch (pt_gemm_dual).  Returns dX / dg|du, or None (nothing launched) when
    the problems do not tile for it -- the caller then launches them separately."""
    _bf16_rowmajor(dy2d, "dy")
    T, N = dy2d.shape
    dev = dy2d.device
    parts = dxsink = None   # the dX as two f32 K halves / the real sink of a K-sliced SwiGLU dX
    if gu is not None:
        wd = weights[0]
        ncols = I = wd.shape[1]
        _bf16_rowmajor(gu, "gu")
        _req(len(weights) == 1 and wd.is_contiguous() and wd.shape[0] == N and tuple(gu.shape) == (T, 2 * I),
             "dual: down weight [H, I], gu [T, 2I]")
        dx = torch.empty(T, 2 * I, dtype=BF16, device=dev)
        dxs = swiglu_dx_ksplit(T, I, N)
        if dxs > 1:   # TP shard widths: dh as K-slices into f32 partials beside the dW slices,
            # dg|du = the SwiGLU backward of the summed dh slices in the reduce pass
            dxpart = torch.empty(dxs * T * I, dtype=torch.float32, device=dev)
            p0 = _problem(dy2d, dy2d.stride(0), [wd], [I], [0, I], 0, [dxpart], [I], [0, T], T, I, N)
            p0.ksplit, p0.kpart_stride = dxs, T * I
            e0, dxsink = EPI_F32, ([dx], [0, T], EPI_SWIGLU_BWD, gu, gu.stride(0))
        else:
            p0 = _problem(dy2d, dy2d.stride(0), [wd], [I], [0, I], 0, [dx], [dx.stride(0)], [0, T], T, I, N)
            p0.residual, p0.ldr = _ptr(gu), gu.stride(0)
            e0 = EPI_SWIGLU_BWD
        p0s = (_C.GemmProblem * 1)(p0)
        flops, nbytes = 2.0 * T * I * N, _alg_bytes(T, I, N, EPI_SWIGLU_BWD)
    else:
        ncols = Kin = weights[0].shape[1]
        ns = [w.shape[0] for w in weights]
        _req(sum(ns) == N, "dgrad: dY width must equal the stacked weight rows")
        dx = torch.empty(T, Kin, dtype=BF16, device=dev)
        e0, flops, nbytes = EPI_BF16, 2.0 * T * Kin * N, _alg_bytes(T, Kin, N, EPI_BF16)
        h = _dx_splits(T, Kin, N, weights, ns, split_min)
        if h is not None:   # the dX as two f32 K halves (split-K, finished by the sum pass after the launch)
            p0s, parts = _dx_halves(dy2d, weights, h)
            e0 = EPI_F32
        else:
            p0s = (_C.GemmProblem * 1)(_problem(dy2d, dy2d.stride(0), weights, [Kin] * len(weights), _bounds(ns), 1,
                                                [dx], [dx.stride(0)], [0, T], T, Kin, N))
    # the probe's label of this launch kind (bench.py's roofline picks the dominant kernel by label)
    label = f"dual dX {T}x{ncols}x{N} e{e0} + dW " + \
        ",".join(f"{dy.shape[1]}x{x.shape[1]}x{dy.shape[0]}" for dy, x, _ in wjobs) + f" e{wepilogue}"
    # the TP shards' few-tile dW as split-K slices beside the dX tiles (f32 partials, reduced after
    # the launch) -- only into sinks the reduce pass can address (_reduce_sink_ok: a misaligned
    # .grad / main_grad view keeps the unsplit dW), decided before anything is launched
    ws = 1
    if wepilogue in _WGRAD_SLICED and not _is_paired(wjobs):
        dx_tiles = sum(p.M // 256 * (p.N // 256) * max(1, p.ksplit) for p in p0s)
        ws = wgrad_ksplit([(dy.shape[1], x.shape[1], dy.shape[0]) for dy, x, _ in wjobs], extra_tiles=dx_tiles)
        if ws > 1 and not all(_reduce_sink_ok(o) for _, _, outs in wjobs for o in outs):
            ws = 1
    p1s = (_C.GemmProblem * len(wjobs))()
    for j, (wdy, x2d, outs) in enumerate(wjobs):   # a KPair: K = 2 T on the 8-phase tile (A2)
        part = torch.empty(ws * wdy.shape[1] * x2d.shape[1], dtype=torch.float32, device=dev) if ws > 1 else None
        p1s[j] = _wgrad_problem(wdy, x2d, outs, part, ws)
    wflops, wbytes = _wgrad_cost(wjobs, wepilogue)
    if order is None:
        order = DUAL_ORDER
        # unsplit dX tiles longer (in K) than the dW tiles: dX first on every XCD, the dW tiles
        # chaining on the other CUs around them (a dW-first XCD would start its dX tiles last)
        if e0 == EPI_BF16 and wjobs and N > max(dy.shape[0] for dy, _, _ in wjobs):
            order = 0

    def launch():
        stream = _C.stream_ptr(dev)
        rc = _C.lib().pt_gemm_dual(p0s, len(p0s), 1, 0, e0, p1s, len(wjobs), 0, 0, EPI_F32 if ws > 1 else int(wepilogue),
                                   int(order), stream)
        if rc == -3:   # PT_EUNSUPPORTED: outside the dual tiling (e.g. C segments not on 256 rows)
            raise _DualRefused
        _C.check(rc, f"pt_gemm_dual(dX epi {e0}, {len(wjobs)} wgrads epi {wepilogue}, split {ws})")
        if ws > 1:
            for j, (_, _, outs) in enumerate(wjobs):
                _splitk_reduce(p1s[j], _wgrad_sink(outs, wepilogue), stream)
        if dxsink is not None:
            _splitk_reduce(p0s[0], dxsink, stream)
        elif parts is not None:   # keep_parts: the consumer (rmsnorm_bwd) sums the halves
            return parts if keep_parts else parts.sum(dx)
        return dx
    try:
        return _timed(label, flops + wflops, nbytes + wbytes, launch)
    except _DualRefused:
        return None


def linear_wgrad(dy2d, x2d, outs, epilogue=EPI_BF16, tile=-1):
    """dW_i = dY_i^T . X for the column segments dY_i of dY (widths = outs[i].shape[0]); one launch.
    dY / X may be KPair (two micro-batches in one K = 2 T launch)."""
    if isinstance(dy2d, KPair):
        linear_wgrad_grouped([(dy2d, x2d, outs)], epilogue)
        return outs
    _bf16_rowmajor(dy2d, "dy")
    _bf16_rowmajor(x2d, "x")
    T, N = dy2d.shape
    Kin = x2d.shape[1]
    ns = [o.shape[0] for o in outs]
    _req(sum(ns) == N, "wgrad: output rows must cover dY's width")
    form = wgrad_form([(dy2d, x2d, outs)], epilogue, tile)
    if form is None:
        return _linear_wgrad_padded(dy2d, x2d, outs, epilogue)
    tile, s = form
    if s > 1:
        _wgrad_ksplit_run([(dy2d, x2d, outs)], epilogue, s, tile)
    else:
        _gemm(dy2d, dy2d.stride(0), 0, [x2d], [x2d.stride(0)], [0, Kin], 0, 0, outs, [o.stride(0) for o in outs],
              _bounds(ns), N, Kin, T, epilogue, tile)
    return outs


# ------------------------------------------------------------------------------- LSE merge
def lse_merge(out, block_out, lse, block_lse):
    """(out_new f32, lse_new) = update_out_and_lse's non-first step (context_parallel.py:157-187) over
    contiguous out / block_out [..., D] and lse / block_lse [...] (lse in bf16 or f32)."""
    _req(out.dtype == torch.float32 and out.is_cuda, "lse_merge: out must be an f32 device tensor")
    _req(block_out.shape == out.shape and block_out.dtype in (BF16, torch.float32), "lse_merge: block_out")
    _req(lse.dtype == block_lse.dtype and lse.dtype in (BF16, torch.float32), "lse_merge: lse dtypes")
    D = out.shape[-1]
    rows = out.numel() // D
    _req(lse.numel() == rows and block_lse.numel() == rows, "lse_merge: one lse per output row")
    out, block_out, lse, block_lse = (t.contiguous() for t in (out, block_out, lse, block_lse))
    out_new = torch.empty_like(out)
    lse_new = torch.empty_like(lse)
    rc = _C.lib().pt_lse_merge(_ptr(out), _ptr(block_out), 0 if block_out.dtype == BF16 else 1, _ptr(lse),
                               _ptr(block_lse), 0 if lse.dtype == BF16 else 1, _ptr(out_new), _ptr(lse_new), rows, D,
                               _C.stream_ptr(out.device))
    _C.check(rc, "pt_lse_merge")
    return out_new, lse_new


# ------------------------------------------------------------------------------- attention
def _str3(t):
    _req(t.dim() == 4 and t.stride(3) == 1, "attention tensors are [B, S, H, D] views with d contiguous")
    return _C.i64arr([t.stride(0), t.stride(1), t.stride(2)])


def _lse_ld(t, B, H, Sq, name="lse"):
    """Row stride of an f32 [B, H, Sq] LSE / delta tensor: dense, or the Sq-column slice of a longer
    [B, H, S] one (the zig-zag ring's half blocks); the kernels index (b, h) rows lse_ld apart."""
    _req(t.dtype == torch.float32 and tuple(t.shape) == (B, H, Sq) and t.stride(2) == 1
         and t.stride(1) >= Sq and (B == 1 or t.stride(0) == H * t.stride(1)) and (H == 1 or t.stride(1) > 0),
         f"{name} must be f32 [B, H, Sq] with unit column stride and (b, h) rows evenly spaced")
    return t.stride(1) if H > 1 else (t.stride(0) if B > 1 else Sq)


# causal attention over a sequence length off the kernels' 128-row query blocks (attention.hip
# check_common: Sq % 128): q / k / v zero-padded to the next multiple.  Causality keeps the padded
# keys out of every real query's softmax, and the padded queries' rows are sliced off (forward) or
# carry dO = 0 and LSE = +inf, so P = 0 and they add nothing to dK / dV (backward): the real rows'
# results are the kernels' own on the real data.
ATTN_Q_BLOCK = 128


def _attn_padded_len(S):
    return -(-int(S) // ATTN_Q_BLOCK) * ATTN_Q_BLOCK


def _pad_seq(t, Sp, fill=0.0):
    """[B, S, ...] -> a contiguous [B, Sp, ...] copy whose rows past S are `fill`."""
    out = torch.full((t.shape[0], Sp) + tuple(t.shape[2:]), fill, dtype=t.dtype, device=t.device)
    out[:, :t.shape[1]] = t
    return out


def _attn_off_block(causal, Sq, Sk, lse, B, H):
    return causal and Sq == Sk and Sq % ATTN_Q_BLOCK != 0 and (lse is None or _lse_ld(lse, B, H, Sq) == Sq)


# Band attention (document masking and sliding windows; include/picotron_hip.h pt_attn_fwd_band): key j
# is visible to query i of batch row b iff kv_lo[b, i] <= j <= i.
_BAND_KEY = object()


class AttnBand:
    """The two bound arrays of a band, int32 [B, S] on the device: kv_lo[b, i] = the first key query i
    sees, q_hi[b, j] = one past the last query that sees key j.  Built only by attn_band(), so the
    kernels never see an invalid bound and nothing has to be read back to validate one."""

    def __init__(self, key, kv_lo, q_hi):
        if key is not _BAND_KEY:
            raise TypeError("AttnBand is built by attn_band()")
        self.kv_lo, self.q_hi = kv_lo, q_hi
        self.B, self.S = kv_lo.shape
        self._padded = {}

    @property
    def device(self):
        return self.kv_lo.device

    def padded(self, Sp):
        """The band over Sp >= S rows: every row past S is a one-token document of its own."""
        if Sp == self.S:
            return self
        _req(Sp > self.S, "AttnBand.padded: a shorter sequence")
        if Sp not in self._padded:
            tail = torch.arange(self.S, Sp, dtype=torch.int32, device=self.device).expand(self.B, -1)
            self._padded[Sp] = AttnBand(_BAND_KEY, torch.cat([self.kv_lo, tail], 1).contiguous(),
                                        torch.cat([self.q_hi, tail + 1], 1).contiguous())
        return self._padded[Sp]

    def mask(self):
        """The boolean [B, 1, S, S] mask (query on dim 2), from kv_lo; for tests and references."""
        i = torch.arange(self.S, device=self.device)
        return ((i[None, None, :] >= self.kv_lo[:, :, None]) & (i[None, None, :] <= i[None, :, None]))[:, None]


def attn_band(B, S, device, document_ids=None, window=None):
    """The AttnBand of B rows of S tokens.  document_ids: integer [B, S]; a document boundary falls
    wherever the value changes along a row, and a token sees only its own document's earlier tokens.
    window: W >= 1, a token sees the last W keys (itself included).  Both: the intersection.  Neither:
    plain causal attention.  Runs on `device` without a host synchronisation."""
    B, S = int(B), int(S)
    _req(B > 0 and S > 0, "attn_band: B and S must be positive")
    device = torch.device(device)
    idx = torch.arange(S, dtype=torch.int32, device=device)
    kv_lo = torch.zeros(B, S, dtype=torch.int32, device=device)
    if document_ids is not None:
        _req(isinstance(document_ids, torch.Tensor) and tuple(document_ids.shape) == (B, S),
             f"attn_band: document_ids must be a [B, S] = [{B}, {S}] tensor")
        _req(not document_ids.dtype.is_floating_point and not document_ids.dtype.is_complex
             and document_ids.dtype != torch.bool, "attn_band: document_ids must be an integer tensor")
        ids = document_ids.to(device)
        first = torch.ones(B, S, dtype=torch.bool, device=device)
        first[:, 1:] = ids[:, 1:] != ids[:, :-1]
        kv_lo = torch.cummax(torch.where(first, idx, torch.zeros_like(idx)), dim=1).values.to(torch.int32)
    if window is not None:
        _req(isinstance(window, int) and not isinstance(window, bool) and window >= 1,
             "attn_band: window must be an integer >= 1")
        if window < S:
            kv_lo = torch.maximum(kv_lo, (idx - (window - 1)).clamp_(min=0))
    kv_lo = kv_lo.contiguous()
    # the first i with kv_lo[b, i] > j (kv_lo is non-decreasing along a row), S when there is none
    q_hi = torch.searchsorted(kv_lo, idx.expand(B, S).contiguous(), right=True).to(torch.int32).contiguous()
    return AttnBand(_BAND_KEY, kv_lo, q_hi)


# Block bands (include/picotron_hip.h pt_attn_fwd_block_band): the band of one block of a
# context-parallel schedule -- a rank's queries (global positions qpos) against one owner's keys
# (kpos).  Key j of the block is visible to query i iff kv_lo[b, i] <= j, and j <= i on the diagonal
# block.
class AttnBlockBand:
    """The bounds of one block, int32 on the device: kv_lo [B, Sq] = the first key of the block query i
    sees (Sk: none), q_hi [B, Sk] = one past the last query of the block that sees key j (0: none);
    causal: the diagonal block (qpos == kpos).  Built only by attn_block_band()."""

    def __init__(self, key, kv_lo, q_hi, causal):
        if key is not _BAND_KEY:
            raise TypeError("AttnBlockBand is built by attn_block_band()")
        self.kv_lo, self.q_hi, self.causal = kv_lo, q_hi, bool(causal)
        (self.B, self.Sq), self.Sk = kv_lo.shape, q_hi.shape[1]

    @property
    def device(self):
        return self.kv_lo.device

    def mask(self):
        """The boolean [B, 1, Sq, Sk] mask (query on dim 2), from kv_lo; for tests and references."""
        j = torch.arange(self.Sk, device=self.device)
        m = j[None, None, :] >= self.kv_lo[:, :, None]
        if self.causal:
            m = m & (j[None, None, :] <= torch.arange(self.Sq, device=self.device)[None, :, None])
        return m[:, None]


def attn_block_band(lo, qpos, kpos, causal):
    """The AttnBlockBand of the queries at global positions qpos [Sq] against the keys at kpos [Sk]
    (both increasing), under the whole row's lower bounds lo [B, S] (lo[b, g] = the first global key
    token g sees: attn_band(...).kv_lo).  causal: the diagonal block (qpos == kpos, j <= i in local
    index); otherwise every key must lie before every query.  Runs on lo's device, nothing read back."""
    _req(isinstance(lo, torch.Tensor) and lo.dim() == 2 and not lo.dtype.is_floating_point,
         "attn_block_band: lo must be an integer [B, S] tensor")
    dev = lo.device
    qpos = torch.as_tensor(qpos, dtype=torch.int64, device=dev)
    kpos = torch.as_tensor(kpos, dtype=torch.int64, device=dev)
    _req(qpos.dim() == 1 and kpos.dim() == 1 and qpos.numel() > 0 and kpos.numel() > 0,
         "attn_block_band: qpos / kpos are non-empty 1-D position lists")
    _req(not causal or qpos.numel() == kpos.numel(), "attn_block_band: the diagonal block has qpos == kpos")
    B, Sk = lo.shape[0], kpos.numel()
    kv_lo = torch.searchsorted(kpos, lo[:, qpos].to(torch.int64).contiguous()).to(torch.int32).contiguous()
    # the first i with kv_lo[b, i] > j (kv_lo is non-decreasing along a row), Sq when there is none
    keys = torch.arange(Sk, dtype=torch.int32, device=dev).expand(B, Sk).contiguous()
    q_hi = torch.searchsorted(kv_lo, keys, right=True).to(torch.int32).contiguous()
    return AttnBlockBand(_BAND_KEY, kv_lo, q_hi, causal)


def _block_band_for(band, q, k, causal, what):
    """The checks every block-band call shares."""
    B, Sq, Sk = q.shape[0], q.shape[1], k.shape[1]
    _req(bool(causal) == band.causal, f"{what}: causal={bool(causal)} but the block band was built causal={band.causal}")
    _req((band.B, band.Sq, band.Sk) == (B, Sq, Sk) and band.device == q.device,
         f"{what}: the block band is [{band.B}, {band.Sq} x {band.Sk}] on {band.device}, the block "
         f"[{B}, {Sq} x {Sk}] on {q.device}")
    _req(Sq % ATTN_Q_BLOCK == 0 and Sk % ATTN_Q_BLOCK == 0,
         f"{what}: a block band needs Sq and Sk on the kernels' {ATTN_Q_BLOCK}-row blocks (no padded path)")


def _band_for(band, q, k, causal, what):
    """The checks every band call shares; returns the band padded to the kernels' 128-row blocks."""
    B, Sq = q.shape[0], q.shape[1]
    _req(isinstance(band, AttnBand), f"{what}: band must be an AttnBand (attn_band())")
    _req(bool(causal), f"{what}: a band is a causal mask (causal=False given)")
    _req(Sq == k.shape[1], f"{what}: a band needs Sq == Sk")
    _req((band.B, band.S) == (B, Sq) and band.device == q.device,
         f"{what}: the band is [{band.B}, {band.S}] on {band.device}, the queries [{B}, {Sq}] on {q.device}")
    return band.padded(_attn_padded_len(Sq))


def attn_fwd(q, k, v, scale, causal, out=None, lse=None, merge=False, band=None):
    """q [B,Sq,H,D], k/v [B,Sk,Hkv,D] (token-major views).  Returns (out, lse[B,H,Sq] f32).
    merge=True: `out` is an f32 accumulator and `lse` the running LSE; this block is merged in.
    lse may be the Sq-column slice of a longer [B, H, S] LSE (rows evenly spaced).
    band (an AttnBand): document-masked / sliding-window causal attention; causal only, no merge,
    dense lse; the few-head split forms are not taken.
    band (an AttnBlockBand): one block of a context-parallel schedule; causal or not, merge, a strided
    lse; Sq and Sk on the 128-row blocks."""
    B, Sq, H, D = q.shape
    Sk, HKV = k.shape[1], k.shape[2]
    if isinstance(band, AttnBlockBand):
        _block_band_for(band, q, k, causal, "attn_fwd")
        _req(not merge or (out is not None and lse is not None), "attn_fwd: merge=True needs out and lse")
        if out is None:
            out = torch.empty(B, Sq, H, D, dtype=BF16, device=q.device)
        if lse is None:
            lse = torch.empty(B, H, Sq, dtype=torch.float32, device=q.device)
        rc = _C.lib().pt_attn_fwd_block_band(_ptr(q), _str3(q), _ptr(k), _str3(k), _ptr(v), _str3(v), _ptr(out),
                                             _str3(out), _ptr(lse), B, H, HKV, Sq, Sk, D, float(scale),
                                             int(bool(causal)), int(bool(merge)), _lse_ld(lse, B, H, Sq),
                                             _ptr(band.kv_lo), _ptr(band.q_hi), _C.stream_ptr(q.device))
        _C.check(rc, "pt_attn_fwd_block_band")
        return out, lse
    if band is not None:
        _req(not merge, "attn_fwd: a band does not combine with merge=True")
        bp = _band_for(band, q, k, causal, "attn_fwd")
        _req(lse is None or _lse_ld(lse, B, H, Sq) == Sq, "attn_fwd: a band takes a dense lse")
        if bp is not band:   # S off the 128-row blocks: the padded path below, pad rows their own documents
            op, lp = attn_fwd(_pad_seq(q, bp.S), _pad_seq(k, bp.S), _pad_seq(v, bp.S), scale, True, band=bp)
            if out is None:
                out = op[:, :Sq].contiguous()
            else:
                out.copy_(op[:, :Sq])
            if lse is None:
                lse = lp[:, :, :Sq].contiguous()
            else:
                lse.copy_(lp[:, :, :Sq])
            return out, lse
        if out is None:
            out = torch.empty(B, Sq, H, D, dtype=BF16, device=q.device)
        if lse is None:
            lse = torch.empty(B, H, Sq, dtype=torch.float32, device=q.device)
        rc = _C.lib().pt_attn_fwd_band(_ptr(q), _str3(q), _ptr(k), _str3(k), _ptr(v), _str3(v), _ptr(out), _str3(out),
                                       _ptr(lse), B, H, HKV, Sq, Sk, D, float(scale), _ptr(band.kv_lo),
                                       _ptr(band.q_hi), _C.stream_ptr(q.device))
        _C.check(rc, "pt_attn_fwd_band")
        return out, lse
    if not merge and _attn_off_block(causal, Sq, Sk, lse, B, H):
        Sp = _attn_padded_len(Sq)
        op, lp = attn_fwd(_pad_seq(q, Sp), _pad_seq(k, Sp), _pad_seq(v, Sp), scale, True)
        if out is None:
            out = op[:, :Sq].contiguous()
        else:
            out.copy_(op[:, :Sq])
        if lse is None:
            lse = lp[:, :, :Sq].contiguous()
        else:
            lse.copy_(lp[:, :, :Sq])
        return out, lse
    if out is None:
        out = torch.empty(B, Sq, H, D, dtype=BF16, device=q.device)
    if lse is None:
        lse = torch.empty(B, H, Sq, dtype=torch.float32, device=q.device)
    ld = _lse_ld(lse, B, H, Sq)
    ws = _attn_split_ws(B, H, HKV, Sq, Sk, D, causal, 0, q.device) if (not merge and ld == Sq) else None
    if ws is not None:   # few heads (a TP shard): split work items + merge (pt_attn_split_plan)
        rc = _C.lib().pt_attn_fwd_split(_ptr(q), _str3(q), _ptr(k), _str3(k), _ptr(v), _str3(v), _ptr(out),
                                        _str3(out), _ptr(lse), B, H, HKV, Sq, Sk, D, float(scale), int(bool(causal)),
                                        _ptr(ws), ws.numel(), _C.stream_ptr(q.device))
        _C.check(rc, "pt_attn_fwd_split")
        return out, lse
    rc = _C.lib().pt_attn_fwd(_ptr(q), _str3(q), _ptr(k), _str3(k), _ptr(v), _str3(v), _ptr(out), _str3(out),
                              _ptr(lse), B, H, HKV, Sq, Sk, D, float(scale), int(bool(causal)), int(bool(merge)),
                              ld, _C.stream_ptr(q.device))
    _C.check(rc, "pt_attn_fwd")
    return out, lse


def _attn_split_ws(B, H, HKV, Sq, Sk, D, causal, backward, device):
    """The workspace (uint8) of the few-head split forms when they apply to this shape, else None."""
    nb = ctypes.c_int64(0)
    rc = _C.lib().pt_attn_split_plan(B, H, HKV, Sq, Sk, D, int(bool(causal)), int(backward), ctypes.byref(nb))
    _C.check(min(rc, 0), "pt_attn_split_plan")
    return torch.empty(nb.value, dtype=torch.uint8, device=device) if rc == 1 else None


def attn_delta(dout, out, delta=None):
    """delta[b, h, q] = sum_d dO * O  (f32 [B, H, Sq]) for the backward (FA2 'D'); into `delta` (a
    dense or row-strided [B, H, Sq] f32 tensor) when given."""
    B, Sq, H, D = out.shape
    if delta is None:
        delta = torch.empty(B, H, Sq, dtype=torch.float32, device=out.device)
    ld = _lse_ld(delta, B, H, Sq, "delta")
    rc = _C.lib().pt_attn_bwd_delta(_ptr(dout), _str3(dout), _ptr(out), _str3(out), _ptr(delta), B, H, Sq, D, ld,
                                    _C.stream_ptr(out.device))
    _C.check(rc, "pt_attn_bwd_delta")
    return delta


def attn_bwd_part(dout, q, k, v, lse, delta, scale, causal, dq=None, dk=None, dv=None, grad_f32=True, band=None):
    """Only dQ (dk = dv = None) or only dK / dV (dq = None) of one attention block, accumulated into the
    given f32 (grad_f32) or stored into bf16 tensors (pt_attn_bwd_part); lse / delta: the queries'
    rows (f32 [B, H, Sq], any row stride shared by both).  band: the block's AttnBlockBand."""
    B, Sq, H, D = q.shape
    Sk, HKV = k.shape[1], k.shape[2]
    parts = (1 if dq is not None else 0) | (2 if dk is not None else 0)
    _req(parts in (1, 2) and (dk is None) == (dv is None), "attn_bwd_part: dq alone, or dk and dv")
    if band is not None:
        _req(isinstance(band, AttnBlockBand), "attn_bwd_part: band must be an AttnBlockBand (attn_block_band())")
        return _attn_bwd_block_band(dout, q, k, v, lse, delta, scale, causal, dq, dk, dv, grad_f32, parts, band,
                                    "attn_bwd_part")
    ld = _lse_ld(lse, B, H, Sq)
    _req(_lse_ld(delta, B, H, Sq, "delta") == ld, "attn_bwd_part: delta and lse rows must share a stride")
    z = _C.i64arr([0, 0, 0])
    rc = _C.lib().pt_attn_bwd_part(_ptr(q), _str3(q), _ptr(k), _str3(k), _ptr(v), _str3(v), _ptr(dout), _str3(dout),
                                   _ptr(lse), _ptr(delta), _ptr(dq), _str3(dq) if dq is not None else z, _ptr(dk),
                                   _str3(dk) if dk is not None else z, _ptr(dv), _str3(dv) if dv is not None else z,
                                   B, H, HKV, Sq, Sk, D, float(scale), int(bool(causal)), int(bool(grad_f32)), ld,
                                   parts, _C.stream_ptr(q.device))
    _C.check(rc, "pt_attn_bwd_part")


def attn_bwd(dout, q, k, v, out, lse, scale, causal, dq=None, dk=None, dv=None, grad_f32=False, delta=None,
             rope=None, band=None):
    """rope = (cos, sin) [S, d] bf16 tables: dq / dk are stored rotated back by -theta (the RoPE
    backward fused into the attention backward; positions = sequence index).
    band (an AttnBand): the backward of attn_fwd(band=); bf16 gradients, dense lse, D = rowsum(dO * O)
    always formed inside the dQ kernel (no `delta` argument).
    band (an AttnBlockBand): one block of a context-parallel schedule; bf16 stores or f32 accumulation,
    a given (or separately formed) delta, a strided lse; no fused RoPE inverse."""
    B, Sq, H, D = q.shape
    Sk, HKV = k.shape[1], k.shape[2]
    if isinstance(band, AttnBlockBand):
        _req(rope is None, "attn_bwd: a block band has no fused RoPE inverse")
        if delta is None:
            ld0 = _lse_ld(lse, B, H, Sq)
            delta = attn_delta(dout, out, torch.empty(B, H, ld0, dtype=torch.float32, device=q.device)[:, :, :Sq]
                               if ld0 != Sq else None)
        gdt = torch.float32 if grad_f32 else BF16
        new = torch.zeros if grad_f32 else torch.empty
        dq = new(B, Sq, H, D, dtype=gdt, device=q.device) if dq is None else dq
        dk = new(B, Sk, HKV, D, dtype=gdt, device=q.device) if dk is None else dk
        dv = new(B, Sk, HKV, D, dtype=gdt, device=q.device) if dv is None else dv
        _attn_bwd_block_band(dout, q, k, v, lse, delta, scale, causal, dq, dk, dv, grad_f32, 3, band, "attn_bwd")
        return dq, dk, dv, delta
    if band is not None:
        return _attn_bwd_band(dout, q, k, v, out, lse, scale, causal, dq, dk, dv, grad_f32, delta, rope, band)
    if not grad_f32 and _attn_off_block(causal, Sq, Sk, lse, B, H) and \
            (delta is None or _lse_ld(delta, B, H, Sq, "delta") == Sq):
        Sp = _attn_padded_len(Sq)
        lsep = torch.full((B, H, Sp), float("inf"), dtype=torch.float32, device=q.device)
        lsep[:, :, :Sq] = lse
        dlp = None
        if delta is not None:
            dlp = torch.zeros(B, H, Sp, dtype=torch.float32, device=q.device)
            dlp[:, :, :Sq] = delta
        rp = None
        if rope is not None:   # tables long enough for the padded rows (their values are never used)
            rp = tuple(t if t.shape[0] >= Sp else _pad_seq(t.unsqueeze(0), Sp)[0] for t in rope)
        dqp, dkp, dvp, dlt = attn_bwd(_pad_seq(dout, Sp), _pad_seq(q, Sp), _pad_seq(k, Sp), _pad_seq(v, Sp),
                                      _pad_seq(out, Sp), lsep, scale, True, delta=dlp, rope=rp)
        res = []
        for given, got in ((dq, dqp), (dk, dkp), (dv, dvp)):
            if given is None:
                res.append(got[:, :Sq].contiguous())
            else:
                given.copy_(got[:, :Sq])
                res.append(given)
        return res[0], res[1], res[2], dlt[:, :, :Sq]
    lib = _C.lib()
    fuse_delta = delta is None and not grad_f32 and out.dtype == BF16 and SW.fuse_delta != 0
    if delta is None and not fuse_delta:
        ld0 = _lse_ld(lse, B, H, Sq)
        delta = attn_delta(dout, out, torch.empty(B, H, ld0, dtype=torch.float32, device=q.device)[:, :, :Sq]
                           if ld0 != Sq else None)
    if delta is not None:
        _req(_lse_ld(delta, B, H, Sq, "delta") == _lse_ld(lse, B, H, Sq), "attn_bwd: delta and lse rows must share a stride")
    gdt = torch.float32 if grad_f32 else BF16
    if dq is None:
        dq = (torch.zeros if grad_f32 else torch.empty)(B, Sq, H, D, dtype=gdt, device=q.device)
    if dk is None:
        dk = (torch.zeros if grad_f32 else torch.empty)(B, Sk, HKV, D, dtype=gdt, device=q.device)
    if dv is None:
        dv = (torch.zeros if grad_f32 else torch.empty)(B, Sk, HKV, D, dtype=gdt, device=q.device)
    rc_cos = rc_sin = None
    rstride = 0
    if rope is not None:
        rc_cos, rc_sin = rope
        _req(rc_cos.dtype == BF16 and rc_sin.dtype == BF16 and rc_cos.stride(-1) == 1 and rc_cos.shape[0] >= Sq,
             "attn_bwd rope tables: bf16 [S, d]")
        _req(rc_sin.stride(0) == rc_cos.stride(0), "attn_bwd rope tables share a stride")
        rstride = rc_cos.stride(0)
    ld = _lse_ld(lse, B, H, Sq)
    if fuse_delta:   # D = rowsum(dO * O) inside the dQ kernel (no separate pass)
        _req(out.shape == q.shape, "attn_bwd: out must be [B, Sq, H, D]")
        _req(ld == Sq, "attn_bwd: the fused-delta form takes a dense lse")
        delta = torch.empty(B, H, Sq, dtype=torch.float32, device=q.device)
        ws = _attn_split_ws(B, H, HKV, Sq, Sk, D, causal, 1, q.device)
        if ws is not None:   # few heads (a TP shard): split work items + reduce passes
            rc = lib.pt_attn_bwd_split(_ptr(q), _str3(q), _ptr(k), _str3(k), _ptr(v), _str3(v), _ptr(out), _str3(out),
                                       _ptr(dout), _str3(dout), _ptr(lse), _ptr(delta), _ptr(dq), _str3(dq), _ptr(dk),
                                       _str3(dk), _ptr(dv), _str3(dv), B, H, HKV, Sq, Sk, D, float(scale),
                                       int(bool(causal)), _ptr(rc_cos), _ptr(rc_sin), rstride, _ptr(ws), ws.numel(),
                                       _C.stream_ptr(q.device))
            _C.check(rc, "pt_attn_bwd_split")
            return dq, dk, dv, delta
        rc = lib.pt_attn_bwd_fused_delta(_ptr(q), _str3(q), _ptr(k), _str3(k), _ptr(v), _str3(v), _ptr(out), _str3(out),
                                         _ptr(dout), _str3(dout), _ptr(lse), _ptr(delta), _ptr(dq), _str3(dq), _ptr(dk),
                                         _str3(dk), _ptr(dv), _str3(dv), B, H, HKV, Sq, Sk, D, float(scale),
                                         int(bool(causal)), _ptr(rc_cos), _ptr(rc_sin), rstride, ld,
                                         _C.stream_ptr(q.device))
        _C.check(rc, "pt_attn_bwd_fused_delta")
        return dq, dk, dv, delta
    rc = lib.pt_attn_bwd(_ptr(q), _str3(q), _ptr(k), _str3(k), _ptr(v), _str3(v), _ptr(dout), _str3(dout),
                         _ptr(lse), _ptr(delta), _ptr(dq), _str3(dq), _ptr(dk), _str3(dk), _ptr(dv), _str3(dv),
                         B, H, HKV, Sq, Sk, D, float(scale), int(bool(causal)), int(bool(grad_f32)),
                         _ptr(rc_cos), _ptr(rc_sin), rstride, ld, _C.stream_ptr(q.device))
    _C.check(rc, "pt_attn_bwd")
    return dq, dk, dv, delta


def _attn_bwd_block_band(dout, q, k, v, lse, delta, scale, causal, dq, dk, dv, grad_f32, parts, band, what):
    B, Sq, H, D = q.shape
    Sk, HKV = k.shape[1], k.shape[2]
    _block_band_for(band, q, k, causal, what)
    ld = _lse_ld(lse, B, H, Sq)
    _req(_lse_ld(delta, B, H, Sq, "delta") == ld, f"{what}: delta and lse rows must share a stride")
    z = _C.i64arr([0, 0, 0])
    rc = _C.lib().pt_attn_bwd_block_band(_ptr(q), _str3(q), _ptr(k), _str3(k), _ptr(v), _str3(v), _ptr(dout),
                                         _str3(dout), _ptr(lse), _ptr(delta), _ptr(dq),
                                         _str3(dq) if dq is not None else z, _ptr(dk),
                                         _str3(dk) if dk is not None else z, _ptr(dv),
                                         _str3(dv) if dv is not None else z, B, H, HKV, Sq, Sk, D, float(scale),
                                         int(bool(causal)), int(bool(grad_f32)), ld, parts, _ptr(band.kv_lo),
                                         _ptr(band.q_hi), _C.stream_ptr(q.device))
    _C.check(rc, "pt_attn_bwd_block_band")


def _attn_bwd_band(dout, q, k, v, out, lse, scale, causal, dq, dk, dv, grad_f32, delta, rope, band):
    B, Sq, H, D = q.shape
    Sk, HKV = k.shape[1], k.shape[2]
    _req(not grad_f32, "attn_bwd: a band writes bf16 gradients (grad_f32=True given)")
    _req(delta is None, "attn_bwd: under a band D is formed inside the dQ kernel (no delta argument)")
    bp = _band_for(band, q, k, causal, "attn_bwd")
    _req(_lse_ld(lse, B, H, Sq) == Sq, "attn_bwd: a band takes a dense lse")
    _req(out.dtype == BF16 and out.shape == q.shape, "attn_bwd: out must be bf16 [B, Sq, H, D]")
    if bp is not band:   # S off the 128-row blocks: as the causal padded path, pad rows their own documents
        Sp = bp.S
        lsep = torch.full((B, H, Sp), float("inf"), dtype=torch.float32, device=q.device)
        lsep[:, :, :Sq] = lse
        rp = None
        if rope is not None:
            rp = tuple(t if t.shape[0] >= Sp else _pad_seq(t.unsqueeze(0), Sp)[0] for t in rope)
        dqp, dkp, dvp, dlt = attn_bwd(_pad_seq(dout, Sp), _pad_seq(q, Sp), _pad_seq(k, Sp), _pad_seq(v, Sp),
                                      _pad_seq(out, Sp), lsep, scale, True, rope=rp, band=bp)
        res = []
        for given, got in ((dq, dqp), (dk, dkp), (dv, dvp)):
            if given is None:
                res.append(got[:, :Sq].contiguous())
            else:
                given.copy_(got[:, :Sq])
                res.append(given)
        return res[0], res[1], res[2], dlt[:, :, :Sq]
    if dq is None:
        dq = torch.empty(B, Sq, H, D, dtype=BF16, device=q.device)
    if dk is None:
        dk = torch.empty(B, Sk, HKV, D, dtype=BF16, device=q.device)
    if dv is None:
        dv = torch.empty(B, Sk, HKV, D, dtype=BF16, device=q.device)
    rc_cos = rc_sin = None
    rstride = 0
    if rope is not None:
        rc_cos, rc_sin = rope
        _req(rc_cos.dtype == BF16 and rc_sin.dtype == BF16 and rc_cos.stride(-1) == 1 and rc_cos.shape[0] >= Sq,
             "attn_bwd rope tables: bf16 [S, d]")
        _req(rc_sin.stride(0) == rc_cos.stride(0), "attn_bwd rope tables share a stride")
        rstride = rc_cos.stride(0)
    delta = torch.empty(B, H, Sq, dtype=torch.float32, device=q.device)
    rc = _C.lib().pt_attn_bwd_band(_ptr(q), _str3(q), _ptr(k), _str3(k), _ptr(v), _str3(v), _ptr(out), _str3(out),
                                   _ptr(dout), _str3(dout), _ptr(lse), _ptr(delta), _ptr(dq), _str3(dq), _ptr(dk),
                                   _str3(dk), _ptr(dv), _str3(dv), B, H, HKV, Sq, Sk, D, float(scale),
                                   _ptr(rc_cos), _ptr(rc_sin), rstride, _ptr(band.kv_lo), _ptr(band.q_hi),
                                   _C.stream_ptr(q.device))
    _C.check(rc, "pt_attn_bwd_band")
    return dq, dk, dv, delta
