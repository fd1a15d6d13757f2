"""Bit identity of the row kernels (csrc/rmsnorm.hip, csrc/cross_entropy.hip) with a pinned build.

Every case feeds one family of tests/_row_ref.py's seeded CPU generators through the C ABI, as
tests/test_row_conformance_gpu.py does, and takes the SHA-256 of every output buffer's bytes.
tests/golden/row_bits.json holds those digests from a build of the commit it names ("parent"), with the
`hipcc --version` line of that build; it was written once by

    python tests/test_row_bits_gpu.py LIBRARY [COMMIT]

(LIBRARY: `python -m picotron_amd.build --out LIBRARY` from a checkout of COMMIT) and is never
regenerated to make a change pass: a refactor of these kernels must reproduce it bit for bit.

Shapes: the smallest that reach every instantiation.  RMSNorm register-resident NCH 1 / 2 / 4 / 8 (cols
64, 520, 1032, 2056) at rows 25, 1025, 4097 (the wave-per-block tiers and the first grid-strided row), the
wide kernels with 4 waves (cols 4104, rows 25 / 1025) and 2 waves (cols 8200, rows 25 / 513); each with
modes 0 / 1, with and without the residual / dres, plain and split-K dy, the three dW sinks and the
partial rows alone.  Fused CE at NC 4 / 8 / 16 / 24 / 32 and the 2-pass kernel, z = 0 and z > 0, loss
only, into a strided sink and in place, with an ignored and a bad target; the streaming pair, a shard,
the statistics forward, the vocab-parallel pair and the mean.

The file's 32 cases run in 4.8 s on an MI355X (the largest, 4097 x 2056, in 0.74 s, most of it the CPU
generators and the digests).
"""
import ctypes
import hashlib
import json
import math
import os
import subprocess
import sys

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pytest
import torch

from tests import _row_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_bits.json")
DEV = "cuda"
BF, F32, I64 = torch.bfloat16, torch.float32, torch.int64
EPS, IGN, Z = 1e-5, R.IGNORE, 0.25
CE_ROWS = 8


def _C():
    from picotron_amd import _C
    return _C


def call(lib, name, *args):
    rc = getattr(lib, name)(*args, _C().stream_ptr())
    assert rc == 0, f"{name} returned {rc}"


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def dev(t):
    return t.to(DEV).contiguous()


def zeros(*shape, dtype=BF):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def padded(rows, cols, gap=16):
    """(full, view): a zeroed [rows, cols + gap] bf16 buffer and its first cols columns."""
    full = zeros(rows, cols + gap)
    return full, full[:, :cols]


# ============================================================================== RMSNorm
NORM_SHAPES = [(r, c) for c in (64, 520, 1032, 2056) for r in (25, 1025, 4097)] + \
              [(25, 4104), (1025, 4104), (25, 8200), (513, 8200)]
# (mode, split-K dy, dres, dW sink or None for the partial rows alone)
NORM_BWD = ((0, False, True, 0), (0, False, False, R.PT_DW_ACC_BF16), (0, True, True, R.PT_DW_ACC_F32),
            (0, True, False, None), (1, False, True, R.PT_DW_ACC_F32), (1, True, False, 0), (1, False, False, None))


def norm_digests(lib, rows, cols):
    family = R.NORM_FAMILIES[NORM_SHAPES.index((rows, cols)) % len(R.NORM_FAMILIES)]
    c = R.make_norm_case(family, rows, cols)
    x, r, w, dy, dres = (dev(c[k]) for k in ("x", "r", "w", "dy", "dres"))
    p0 = torch.randn(rows, cols, generator=R._gen("bits split", rows, cols))
    p0, p1 = dev(p0), dev(c["dy"].float() - p0)
    out, saved = {"family": family}, {}
    for mode in (0, 1):
        for res in (False, True):
            y, z, rstd = zeros(rows, cols), zeros(rows, cols), zeros(rows, dtype=F32)
            call(lib, "pt_rmsnorm_fwd", p(x), p(r) if res else None, p(w), p(y), p(z) if res else None, p(rstd), rows,
                 cols, EPS, mode)
            tag = f"fwd mode {mode} res {int(res)}"
            out.update({f"{tag} y": sha(y), f"{tag} z": sha(z), f"{tag} rstd": sha(rstd)})
            saved[mode, res] = (z if res else x), rstd
    nparts = lib.pt_rmsnorm_bwd_partials(rows, cols)
    assert nparts > 0
    out["nparts"] = nparts
    for mode, split, with_dres, sink in NORM_BWD:
        z, rstd = saved[mode, True]
        dx, part = zeros(rows, cols), zeros(nparts, cols, dtype=F32)
        dw = None
        if sink is not None:
            old = torch.randn(cols, generator=R._gen("bits old", sink, cols))
            dw = dev(old.to(F32 if sink == R.PT_DW_ACC_F32 else BF))
        tail = (p(z), p(w), p(rstd), p(dres) if with_dres else None, p(dx), p(dw), p(part), rows, cols, mode | (sink or 0))
        if split:
            call(lib, "pt_rmsnorm_bwd_splitk", p(p0), p(p1), *tail)
        else:
            call(lib, "pt_rmsnorm_bwd", p(dy), *tail)
        tag = f"bwd mode {mode} split {int(split)} dres {int(with_dres)} sink {sink}"
        out.update({f"{tag} dx": sha(dx), f"{tag} partial": sha(part)})
        if dw is not None:
            out[f"{tag} dw"] = sha(dw)
    return out


def colsum_digests(lib):
    cols, jobs = 40, ((1, 0), (129, R.PT_DW_ACC_BF16), (129, R.PT_DW_ACC_F32), (1, R.PT_DW_ACC_F32), (129, 0))
    g = R._gen("bits colsum", cols)
    parts = [dev(torch.randn(n, cols, generator=g) * 2.0 ** (i - 2)) for i, (n, _) in enumerate(jobs)]
    outs = [dev(torch.randn(cols, generator=g).to(F32 if s == R.PT_DW_ACC_F32 else BF)) for _, s in jobs]
    C = _C()
    call(lib, "pt_rmsnorm_colsum_batch", ctypes.cast(C.ptrarr([t.data_ptr() for t in parts]), ctypes.c_void_p),
         ctypes.cast(C.i32arr([n for n, _ in jobs]), ctypes.c_void_p),
         ctypes.cast(C.ptrarr([t.data_ptr() for t in outs]), ctypes.c_void_p),
         ctypes.cast(C.i32arr([s for _, s in jobs]), ctypes.c_void_p), len(jobs), cols)
    return {f"job {i} nparts {n} sink {s}": sha(o) for i, ((n, s), o) in enumerate(zip(jobs, outs))}


# ============================================================================== cross-entropy
V_FUSED = (8, 2040, 8200, 16392, 32776, 49160, 65544)


def ce_inputs(key, V, rows=CE_ROWS):
    """(family, logits on the device, targets with row 4 ignored and row 6 bad (= V))."""
    family = R.CE_FAMILIES[key % len(R.CE_FAMILIES)]
    tgt = R.make_targets(rows, V)
    assert int(tgt[4]) == IGN
    tgt[6] = V
    return family, dev(R.make_ce_case(family, rows, V)), dev(tgt)


def zs():
    """(tag, the entry point's suffix, the arguments the _z form adds before the stream) per z."""
    return (("z 0", "", lambda rows: ()), (f"z {Z}", "_z", lambda rows: (Z, p(keep(zeros(rows, dtype=F32))))))


_KEPT = []


def keep(t):
    _KEPT.append(t)
    return t


def fused_digests(lib, V):
    family, x, t = ce_inputs(V_FUSED.index(V), V)
    inv = dev(torch.tensor([1.0 / 7]))
    out = {"family": family}
    for ztag, suffix, zargs in zs():
        for form in ("loss", "sink", "inplace"):
            logits = x.clone()
            full, d = (None, None) if form == "loss" else padded(CE_ROWS, V) if form == "sink" else (logits, logits)
            rl, status = zeros(CE_ROWS, dtype=F32), zeros(1, dtype=torch.int32)
            del _KEPT[:]
            call(lib, "pt_cross_entropy_fwd_bwd" + suffix, p(logits), V, p(t), p(d), d.stride(0) if d is not None else 0,
                 p(rl), CE_ROWS, V, 0.5, p(inv), IGN, p(status), *zargs(CE_ROWS))
            tag = f"{ztag} {form}"
            out.update({f"{tag} row_loss": sha(rl), f"{tag} status": sha(status), f"{tag} logits": sha(logits)})
            if full is not None:
                out[f"{tag} dlogits"] = sha(full)
            if _KEPT:
                out[f"{tag} row_z"] = sha(_KEPT[0])
    return out


def stream_digests(lib, V):
    family, x, t = ce_inputs(V, V)
    out = {"family": family}
    for ztag, suffix, zargs in zs():
        rl, lse, status = zeros(CE_ROWS, dtype=F32), zeros(CE_ROWS, dtype=F32), zeros(1, dtype=torch.int32)
        del _KEPT[:]
        call(lib, "pt_cross_entropy_fwd_lse" + suffix, p(x), V, p(t), p(rl), p(lse), CE_ROWS, V, IGN, p(status),
             *zargs(CE_ROWS))
        out.update({f"{ztag} row_loss": sha(rl), f"{ztag} row_lse": sha(lse), f"{ztag} status": sha(status)})
        if _KEPT:
            out[f"{ztag} row_z"] = sha(_KEPT[0])
        for stride in (0, 1):
            scale = dev(torch.tensor([0.25]) if stride == 0 else (0.125 * (1 + torch.arange(CE_ROWS) % 3)).float())
            full, d = padded(CE_ROWS, V)
            call(lib, "pt_cross_entropy_bwd_lse" + suffix, p(x), V, p(t), p(lse), p(d), d.stride(0), CE_ROWS, V, p(scale),
                 stride, IGN, *((Z,) if suffix else ()))
            out[f"{ztag} dlogits stride {stride}"] = sha(full)
    return out


def shard_digests(lib):
    V, lo, width = 4104, 2056, 2048
    family, x, _ = ce_inputs(1, V)
    t = dev(torch.tensor([lo, lo + width - 1, lo - 1, lo + width, IGN, lo + 7, 0, V - 1]))
    lse = dev((8.0 + torch.randn(CE_ROWS, generator=R._gen("bits shard lse"))).float())
    scale = dev((0.125 * (1 + torch.arange(CE_ROWS) % 3)).float())
    out = {"family": family}
    for ztag, suffix, _ in zs():
        full, d = padded(CE_ROWS, width)
        call(lib, "pt_cross_entropy_bwd_lse_shard" + suffix, p(x[:, lo:]), V, p(t), p(lse), p(d), d.stride(0), CE_ROWS,
             width, lo, p(scale), 1, IGN, *((Z,) if suffix else ()))
        out[f"{ztag} dlogits"] = sha(full)
    return out


def synthetic_stats(key, nblk, rows):
    """f32 [nblk, rows, 2] (m_b, s_b) from a seeded generator, one (-inf, 0) tile per row when nblk > 1."""
    g = R._gen("bits stats", key, nblk, rows)
    st = torch.stack([torch.randn(nblk, rows, generator=g) * 3, 1 + 15 * torch.rand(nblk, rows, generator=g)], 2)
    if nblk > 1:
        rr = torch.arange(rows)
        st[(rr * 5) % nblk, rr] = torch.tensor([-math.inf, 0.0])
    return st.float().contiguous()


def stats_digests(lib, nblk):
    rows, V = 33, nblk * 16
    g = R._gen("bits stats x", nblk)
    x = dev((torch.randn(rows, V, generator=g) * 3).to(BF))
    tgt = torch.randint(0, V, (rows,), generator=g)
    tgt[16], tgt[20] = IGN, V
    t, st = dev(tgt), dev(synthetic_stats(0, nblk, rows))
    out = {}
    for ztag, suffix, zargs in zs():
        rl, lse, status = zeros(rows, dtype=F32), zeros(rows, dtype=F32), zeros(1, dtype=torch.int32)
        del _KEPT[:]
        call(lib, "pt_cross_entropy_fwd_stats" + suffix, p(x), V, p(t), p(st), nblk, p(rl), p(lse), rows, V, IGN,
             p(status), *zargs(rows))
        out.update({f"{ztag} row_loss": sha(rl), f"{ztag} row_lse": sha(lse), f"{ztag} status": sha(status)})
        if _KEPT:
            out[f"{ztag} row_z"] = sha(_KEPT[0])
    return out


def vp_digests(lib, tp):
    rows, Vs, nblk = 33, 256, 2
    V = tp * Vs
    family = "neg_inf" if tp > 1 else "offset"
    x = dev(R.make_ce_case(family, rows, V))
    tgt = R.make_targets(rows, V)
    tgt[6] = V
    t = dev(tgt)
    parts = zeros(tp, rows, 4, dtype=F32)
    for q in range(tp):
        st = dev(synthetic_stats(1 + q, nblk, rows))
        call(lib, "pt_cross_entropy_vp_partial", p(x[:, q * Vs:]), V, p(t), p(st), nblk, p(parts[q]), rows, Vs, q * Vs)
    out = {"family": family, "parts": sha(parts)}
    for ztag, suffix, zargs in zs():
        rl, lse, status = zeros(rows, dtype=F32), zeros(rows, dtype=F32), zeros(1, dtype=torch.int32)
        del _KEPT[:]
        call(lib, "pt_cross_entropy_vp_combine" + suffix, p(parts), tp, p(t), p(rl), p(lse), rows, V, IGN, p(status),
             *zargs(rows))
        out.update({f"{ztag} row_loss": sha(rl), f"{ztag} row_lse": sha(lse), f"{ztag} status": sha(status)})
        if _KEPT:
            out[f"{ztag} row_z"] = sha(_KEPT[0])
    return out


def mean_digests(lib):
    rows = 1025
    g = R._gen("bits mean", rows)
    rl = (torch.rand(rows, generator=g) * 10).float()
    tgt = torch.randint(0, 100, (rows,), generator=g)
    tgt[::3] = IGN
    rd, td = dev(torch.where(tgt != IGN, rl, torch.zeros_like(rl))), dev(tgt)
    out = {}
    for reduce_sum in (0, 1):
        for out_bf16 in (0, 1):
            o, l32, inv = zeros(1, dtype=BF if out_bf16 else F32), zeros(1, dtype=F32), zeros(1, dtype=F32)
            call(lib, "pt_cross_entropy_mean", p(rd), p(td), rows, IGN, p(l32), p(inv), p(o), out_bf16, reduce_sum)
            tag = f"sum {reduce_sum} bf16 {out_bf16}"
            out.update({f"{tag} out": sha(o), f"{tag} loss_f32": sha(l32), f"{tag} inv_count": sha(inv)})
    return out


CASES = {f"rmsnorm {r}x{c}": (norm_digests, r, c) for r, c in NORM_SHAPES}
CASES["rmsnorm colsum_batch"] = (colsum_digests,)
CASES.update({f"ce fused V {v}": (fused_digests, v) for v in V_FUSED})
CASES.update({f"ce stream V {v}": (stream_digests, v) for v in (8, 10232)})
CASES["ce shard"] = (shard_digests,)
CASES.update({f"ce stats nblk {n}": (stats_digests, n) for n in (1, 9)})
CASES.update({f"ce vocab-parallel tp {n}": (vp_digests, n) for n in (1, 8)})
CASES["ce mean"] = (mean_digests,)


def hipcc_version():
    for c in ("/opt/rocm/bin/hipcc", "hipcc"):
        try:
            text = subprocess.run([c, "--version"], capture_output=True, text=True).stdout
        except OSError:
            continue
        return next((line.strip() for line in text.splitlines() if "HIP version" in line), "unknown")
    return "unknown"


def _load():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_holds_exactly_the_cases():
    assert sorted(_load()["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_row_bits(name):
    golden = _load()
    fn, *args = CASES[name]
    got, want = fn(_C().lib(), *args), golden["cases"][name]
    differ = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
    assert not differ, (f"{name}: {len(differ)} of {len(want)} outputs differ by bits from commit {golden['parent']}: "
                        f"{', '.join(differ)}\n  the pinned build's compiler: {golden['hipcc']}\n  this machine's:"
                        f"              {hipcc_version()}")


if __name__ == "__main__":
    lib = _C().load_library(os.path.abspath(sys.argv[1]), strict=False)
    commit = sys.argv[2] if len(sys.argv) > 2 else "unknown"
    cases = {}
    for name in sorted(CASES):
        fn, *args = CASES[name]
        cases[name] = fn(lib, *args)
    with open(GOLDEN, "w") as f:
        json.dump({"parent": commit, "hipcc": hipcc_version(), "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN}: {len(cases)} cases from {sys.argv[1]}")
