"""csrc/qk_norm.hip (per-head QK-norm fused with RoPE) through the C ABI and kernels.py against the
float64 reference of tests/_qk_norm_ref.py, per element, on the adversarial families of tests/_row_ref.py
(self-tested without a GPU in tests/test_qk_norm_checker_cpu.py).

Every tensor the kernels write sits in a buffer filled with a NaN-payload sentinel, with a guard row
above and below; x and dy are q|k|v rows whose v columns hold the sentinel, so a kernel that read v
would produce NaN and one that wrote it would change its bits.  The norm-only forward and the backward
are held to the derived per-element bounds on all five families and to the bit condition (at most 0.5 %
of the elements one rounding flip from the float64-sequenced expectation) on randn, rowscale, tiny and
cancel; `spike` is judged by the bound alone (tests/_qk_norm_ref.py says why).  The fused forward is
compared by bits with pt_rope applied to the kernel's own norm-only output.

Cases (rows, nq, nk, d): the smallest; a head count below a wave with rows off every grid; a head group
crossing a wave; heads past one wave and more than one partial row; GQA with several workgroups.
"""
import ctypes
import functools

import pytest
import torch

from tests import _qk_norm_ref as Q
from tests import _row_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS = 1e-5
CASES = ((3, 1, 1, 64), (130, 3, 1, 64), (257, 5, 5, 128), (520, 17, 1, 128), (1024, 8, 2, 64))
SINKS = (0, R.PT_DW_ACC_BF16, R.PT_DW_ACC_F32)


def C_():
    from picotron_amd import _C
    return _C


def call(name, *args):
    _C = C_()
    rc = getattr(_C.lib(), name)(*args, _C.stream_ptr())
    assert rc == 0, f"{name} returned {rc}"


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def sentinel(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.int16 if dtype == BF else torch.int32).fill_(R.NAN16 if dtype == BF else R.NAN32)
    return t


def guarded(rows, cols, dtype):
    """(full, view): a sentinel buffer [rows + 2, cols]; view = its rows 1 .. rows."""
    full = sentinel((rows + 2, cols), dtype)
    return full, full[1:rows + 1]


def in_guarded(t):
    full, view = guarded(t.shape[0], t.shape[1], t.dtype)
    view.copy_(t)
    return full, view


def only_written(full, rows, cols):
    """Everything of full outside rows 1 .. rows x columns < cols still holds the sentinel."""
    ib = full.view(torch.int16 if full.dtype == BF else torch.int32).clone()
    pat = R.NAN16 if full.dtype == BF else R.NAN32
    ib[1:rows + 1, :cols] = pat
    return bool((ib == pat).all())


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(R.ibits(a.cpu()), R.ibits(b.cpu()))


@functools.lru_cache(maxsize=8)
def qk_case(family, case):
    return Q.make_qk_case(family, *case)


@functools.lru_cache(maxsize=4)
def tables(seq_len, d):
    cos, sin = Q.make_tables(seq_len, d)
    return cos.to(DEV), sin.to(DEV)


def seq_of(rows):
    return 128 if rows > 128 else 2   # below the row count: positions wrap


def run_fwd(c, mode, rope, inplace):
    """(y view [rows, q|k|v width], rstd [rows, nq + nk]) through the C ABI; the sentinels checked."""
    rows, nq, nk, d = c["rows"], c["nq"], c["nk"], c["d"]
    width, qk = c["x"].shape[1], (nq + nk) * d
    xf, x = in_guarded(c["x"].to(DEV))
    yf, y = (xf, x) if inplace else guarded(rows, width, BF)
    rf, rstd = guarded(rows, nq + nk, F32)
    seq = seq_of(rows)
    cos, sin = tables(seq, d) if rope else (None, None)
    wq, wk = c["wq"].to(DEV), c["wk"].to(DEV)
    call("pt_qk_norm_rope_fwd", p(x), width, p(y), width, p(wq), p(wk), p(rstd), rows, nq, nk, d,
         EPS, mode, p(cos), p(sin), seq, d if rope else 0)
    torch.cuda.synchronize()
    assert only_written(yf, rows, qk), "y: v columns or guard rows written"
    assert only_written(rf, rows, nq + nk)
    if not inplace:
        assert same_bits(x, c["x"].to(DEV)), "x modified by an out-of-place call"
    Q.check_untouched("y", y, qk)
    return y, rstd


def rope_(t, nheads, d, rows):
    seq = seq_of(rows)
    cos, sin = tables(seq, d)
    call("pt_rope", p(t), rows, t.stride(0), nheads, d, p(cos), p(sin), seq, d, 0)
    return t


def run_bwd(c, rstd, mode, alias, need=(True, True)):
    """(dx view, partial_q, partial_k, their sentinel buffers) through the C ABI."""
    rows, nq, nk, d = c["rows"], c["nq"], c["nk"], c["d"]
    width, qk = c["x"].shape[1], (nq + nk) * d
    dyf, dy = in_guarded(c["dy"].to(DEV))
    xf, x = in_guarded(c["x"].to(DEV))
    dxf, dx = (dyf, dy) if alias else guarded(rows, width, BF)
    nparts = C_().lib().pt_qk_norm_bwd_partials(rows, nq, nk, d)
    assert nparts > 0
    pqf, pq = guarded(nparts, d, F32)
    pkf, pk = guarded(nparts, d, F32)
    wq, wk, rstd = c["wq"].to(DEV), c["wk"].to(DEV), rstd.contiguous()
    call("pt_qk_norm_bwd", p(dy), width, p(x), width, p(wq), p(wk), p(rstd), p(dx), width,
         p(pq) if need[0] else None, p(pk) if need[1] else None, rows, nq, nk, d, mode)
    torch.cuda.synchronize()
    assert only_written(dxf, rows, qk), "dx: v columns or guard rows written"
    assert only_written(pqf, nparts, d if need[0] else 0), "q partial: a NULL buffer's stand-in or a guard written"
    assert only_written(pkf, nparts, d if need[1] else 0), "k partial: a NULL buffer's stand-in or a guard written"
    assert same_bits(x, c["x"].to(DEV))
    for need_, part in zip(need, (pq, pk)):   # every row of a non-NULL partial buffer is written
        assert not need_ or bool(torch.isfinite(part).all())
    return dx, pq, pk


def colsum(parts_sinks, d):
    """[(partial, sink, old or None)] through ONE pt_rmsnorm_colsum_batch(cols = d): the dweight views."""
    _C = C_()
    bufs = []
    for part, sink, old in parts_sinks:
        full, view = guarded(1, d, F32 if sink == R.PT_DW_ACC_F32 else BF)
        if old is not None:
            view.copy_(old.to(DEV)[None, :])
        bufs.append((full, view))
    call("pt_rmsnorm_colsum_batch", ctypes.cast(_C.ptrarr([t.data_ptr() for t, _, _ in parts_sinks]), ctypes.c_void_p),
         ctypes.cast(_C.i32arr([t.shape[0] for t, _, _ in parts_sinks]), ctypes.c_void_p),
         ctypes.cast(_C.ptrarr([v.data_ptr() for _, v in bufs]), ctypes.c_void_p),
         ctypes.cast(_C.i32arr([s for _, s, _ in parts_sinks]), ctypes.c_void_p), len(parts_sinks), d)
    torch.cuda.synchronize()
    for full, _ in bufs:
        assert only_written(full, 1, d)
    return [v[0] for _, v in bufs]


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("case", CASES)
def test_forward(case, mode):
    """Norm only against the reference; in place; fused = pt_rope of the norm-only output, bit for bit."""
    rows, nq, nk, d = case
    for family in Q.FAMILIES:
        c = qk_case(family, case)
        tag = f"fwd {family} {case}"
        y, rstd = run_fwd(c, mode, rope=False, inplace=False)
        Q.check_forward(c, y, rstd, EPS, mode, tag)
        y2, rstd2 = run_fwd(c, mode, rope=False, inplace=True)
        assert same_bits(y, y2) and same_bits(rstd, rstd2), "in place differs from out of place"
        want = rope_(y.clone(), nq + nk, d, rows)
        torch.cuda.synchronize()
        for inplace in (False, True):
            f, rstd3 = run_fwd(c, mode, rope=True, inplace=inplace)
            assert same_bits(f, want), f"fused output differs from pt_rope of the norm-only output (in place {inplace})"
            assert same_bits(rstd3, rstd)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("case", CASES)
def test_backward(case, mode):
    """dx against the reference (also aliasing dy), dw through pt_rmsnorm_colsum_batch into the three sinks,
    a NULL partial, run-to-run identity."""
    rows, nq, nk, d = case
    for family in Q.FAMILIES:
        c = qk_case(family, case)
        tag = f"bwd {family} {case}"
        _, rstd = run_fwd(c, mode, rope=False, inplace=False)
        dx, pq, pk = run_bwd(c, rstd, mode, alias=False)
        refs = Q.check_backward(c, dx, rstd, mode, tag)
        dx2, pq2, pk2 = run_bwd(c, rstd, mode, alias=True)
        assert same_bits(dx, dx2), "dx aliasing dy differs"
        assert same_bits(pq, pq2) and same_bits(pk, pk2), "partials differ between two runs"
        jobs, olds = [], []
        for part, nm in ((pq, "q"), (pk, "k")):
            for sink in SINKS:
                old = None if sink == 0 else torch.randn(d, generator=R._gen("old", sink, d, nm)).to(BF if sink == 4 else F32)
                jobs.append((part, sink, old))
        outs = colsum(jobs, d)
        for (part, sink, old), got, ref, nm in zip(jobs, outs, [refs[0]] * 3 + [refs[1]] * 3, "qqqkkk"):
            t, b = R.dw_target_bound(ref["dw"], ref["dw_err"], sink, old)   # rows * heads terms
            R.check(f"{nm} dw sink {sink}", got, t, b, tag)
        if family == "randn":   # a frozen weight: its partial buffer is not touched, the other is unchanged
            for need in ((False, True), (True, False), (False, False)):
                dx3, pq3, pk3 = run_bwd(c, rstd, mode, alias=False, need=need)
                assert same_bits(dx3, dx)
                assert not need[0] or same_bits(pq3, pq)
                assert not need[1] or same_bits(pk3, pk)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("case", CASES)
def test_cross_check_against_the_row_kernels(case, mode):
    """The q heads and the k heads copied into contiguous [rows * heads, d] matrices, through pt_rmsnorm_fwd /
    pt_rmsnorm_bwd and pt_rope: only rstd's summation order differs between the two paths, so y and dx are
    within one rounding flip of those results, and the rotation adds no difference of its own."""
    rows, nq, nk, d = case
    qk = (nq + nk) * d
    for family in Q.CAPPED:
        c = qk_case(family, case)
        tag = f"cross {family} {case}"
        y, rstd = run_fwd(c, mode, rope=False, inplace=False)
        fused, _ = run_fwd(c, mode, rope=True, inplace=False)
        dx, _, _ = run_bwd(c, rstd, mode, alias=False)
        refs_f = Q.ref_case_fwd(c, EPS, mode)
        old_y, old_dx = [], []
        for nm, xm, dym, w, ref in zip("qk", (c["xq"], c["xk"]), (c["dyq"], c["dyk"]), (c["wq"], c["wk"]), refs_f):
            n = xm.shape[0]
            xd, dyd, wd = xm.to(DEV), dym.to(DEV), w.to(DEV)
            yo, dxo = torch.empty_like(xd), torch.empty_like(xd)
            ro = torch.empty(n, dtype=F32, device=DEV)
            call("pt_rmsnorm_fwd", p(xd), None, p(wd), p(yo), None, p(ro), n, d, EPS, mode)
            part = torch.empty(C_().lib().pt_rmsnorm_bwd_partials(n, d), d, dtype=F32, device=DEV)
            call("pt_rmsnorm_bwd", p(dyd), p(xd), p(wd), p(ro), None, p(dxo), None, p(part), n, d, mode)
            torch.cuda.synchronize()
            old_y.append(yo)
            old_dx.append(dxo)
            mine_y, mine_dx = (Q.split_heads(t.cpu(), nq, nk, d)[0 if nm == "q" else 1] for t in (y, dx))
            R.check_bits(f"{nm} y vs pt_rmsnorm_fwd", mine_y, yo.cpu(), ref["y_alts"] + (ref["y_want"],), tag=tag)
            rb = Q.ref_bwd(dym, xm, w, ro.cpu(), mode)
            R.check_bits(f"{nm} dx vs pt_rmsnorm_bwd", mine_dx, dxo.cpu(), tag=tag, flip=rb["dx_flip"])
        # ... then pt_rope on the row kernels' y: it differs from the fused output only where y did
        oy = Q.join_heads(old_y[0], old_y[1], rows, nq, nk, d).contiguous()
        orot = rope_(oy.clone(), nq + nk, d, rows)
        torch.cuda.synchronize()
        ydiff = (R.ibits(y[:, :qk].cpu()) != R.ibits(oy.cpu())).view(rows, nq + nk, 2, d // 2).any(2, keepdim=True)
        rdiff = (R.ibits(fused[:, :qk].cpu()) != R.ibits(orot.cpu())).view(rows, nq + nk, 2, d // 2)
        assert not bool((rdiff & ~ydiff).any()), "rotated outputs differ where the normed pairs were bit-equal"
        share = float(rdiff.double().mean())
        print(f"row-check {tag} rotated bit-mismatch share {share:.2e}")
        assert share <= R.BIT_CAP


def test_kernels_py_wrappers_equal_the_abi():
    """kernels.qk_norm_rope_fwd / qk_norm_bwd: the same bits as the C calls, v untouched, y / dx in place."""
    from picotron_amd import kernels as K
    case = (257, 5, 5, 128)
    rows, nq, nk, d = case
    qk = (nq + nk) * d
    c = qk_case("randn", case)
    wq, wk = c["wq"].to(DEV), c["wk"].to(DEV)
    seq = seq_of(rows)
    cos, sin = tables(seq, d)
    for mode in (0, 1):
        f, rstd = run_fwd(c, mode, rope=True, inplace=False)
        x = c["x"].to(DEV)
        y, r = K.qk_norm_rope_fwd(x, nq, nk, d, wq, wk, EPS, mode, cos, sin, seq)
        assert tuple(y.shape) == (rows, qk) and same_bits(y, f[:, :qk].contiguous()) and same_bits(r, rstd.contiguous())
        y2, r2 = K.qk_norm_rope_fwd(x, nq, nk, d, wq, wk, EPS, mode, cos, sin, seq, out=x)
        assert y2 is x and same_bits(x[:, :qk].contiguous(), y) and same_bits(r2, r)
        Q.check_untouched("in-place qkv", x, qk)
        n_only, _ = K.qk_norm_rope_fwd(c["x"].to(DEV), nq, nk, d, wq, wk, EPS, mode, None, None, seq)
        assert same_bits(K.rope_(n_only, nq + nk, d, cos, sin, seq), y)
        dx, pq, pk = run_bwd(c, rstd, mode, alias=False)
        dy = c["dy"].to(DEV)
        kdx, kpq, kpk = K.qk_norm_bwd(dy, c["x"].to(DEV), wq, wk, r, nq, nk, d, mode, dx=dy)
        assert kdx is dy and same_bits(dy[:, :qk].contiguous(), dx[:, :qk].contiguous())
        assert same_bits(kpq, pq.contiguous()) and same_bits(kpk, pk.contiguous())
        Q.check_untouched("in-place dqkv", dy, qk)
        _, nq_part, nk_part = K.qk_norm_bwd(c["dy"].to(DEV), c["x"].to(DEV), wq, wk, r, nq, nk, d, mode, need_dw=(False, True))
        assert nq_part is None and same_bits(nk_part, kpk)
    with pytest.raises(ValueError):
        K.qk_norm_rope_fwd(c["x"].to(DEV)[:, :qk - 8], nq, nk, d, wq, wk, EPS, 0, cos, sin, seq)


def test_refused_shapes_launch_nothing():
    _C = C_()
    x = sentinel((4, 384), BF)
    w = torch.ones(64, dtype=BF, device=DEV)
    rstd = sentinel((4, 6), F32)
    rc = _C.lib().pt_qk_norm_rope_fwd(p(x), 384, p(x), 384, p(w), p(w), p(rstd), 4, 4, 2, 60, EPS, 0, None, None, 4, 0,
                                      _C.stream_ptr())
    assert rc == -3
    assert _C.lib().pt_qk_norm_bwd_partials(4, 4, 2, 96) == -3
    torch.cuda.synchronize()
    assert only_written(x, 0, 0) and only_written(rstd, 0, 0)
