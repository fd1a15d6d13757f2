"""The QK-norm kernels (csrc/qk_norm.hip) at the layer's shapes: us per call from a HIP graph of `reps`
back-to-back calls (no host gaps) and the achieved HBM rate on the bytes each kernel must move.

    python tools/qk_norm_bench.py [--rows 4096] [--mode 0]

Shapes: T 4096 with 32 + 32 heads of 64 (SmolLM-1.7B's layer) and with 32 + 8 heads of 128, on q|k|v rows
(v is skipped, as in the layer).  Bytes, E = T (nq + nk) d elements:
    forward   read q|k once, write it once, rstd:       4 E + 4 T (nq + nk)
    backward  read dy and x, write dx (+ rstd, partials): 6 E + 4 T (nq + nk)
Baseline of the forward: what the library offered before these kernels -- pt_rmsnorm_fwd on the contiguous
[T heads, d] head rows of q and of k (one wave per 64- or 128-wide row) and then pt_rope on the rows --
WITHOUT the copies that would pack the heads into those matrices and back, i.e. in its favour.  Both are
timed in the same process, alternating, three rounds; the ratio printed is baseline / fused.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from picotron_amd import kernels as K  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from norm_bench import graph_us  # noqa: E402

SHAPES = ((32, 32, 64), (32, 8, 128))   # (q heads, k heads, head_dim)
SEQ = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--mode", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qk_norm_bench: needs a HIP device; a CPU run measures nothing")
    bf = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    ratios = []
    for nq, nk, d in SHAPES:
        T = a.rows
        nh, width = nq + nk, (nq + 2 * nk) * d
        E = T * nh * d
        qkv, dqkv = (torch.randn(T, width, device="cuda", generator=g).to(bf) for _ in range(2))
        wq, wk = ((1 + 0.1 * torch.randn(d, device="cuda", generator=g)).to(bf) for _ in range(2))
        ang = torch.rand(SEQ, d // 2, device="cuda", generator=g) * 6.283
        cos, sin = torch.cos(ang).repeat(1, 2).to(bf), torch.sin(ang).repeat(1, 2).to(bf)
        out = torch.empty(T, nh * d, dtype=bf, device="cuda")
        dx = torch.empty_like(dqkv)
        # the baseline's inputs, already packed: its copies are not timed
        xq, xk = qkv[:, :nq * d].reshape(T * nq, d).contiguous(), qkv[:, nq * d:nh * d].reshape(T * nk, d).contiguous()

        def fused():
            return K.qk_norm_rope_fwd(qkv, nq, nk, d, wq, wk, 1e-5, a.mode, cos, sin, SEQ, out=out)

        def norm_only():
            return K.qk_norm_rope_fwd(qkv, nq, nk, d, wq, wk, 1e-5, a.mode, None, None, SEQ, out=out)

        def baseline():
            yq, _, _ = K.rmsnorm_fwd(xq, wq, 1e-5, a.mode)
            yk, _, _ = K.rmsnorm_fwd(xk, wk, 1e-5, a.mode)
            K.rope_(yq.view(T, nq * d), nq, d, cos, sin, SEQ)
            K.rope_(yk.view(T, nk * d), nk, d, cos, sin, SEQ)
            return yq, yk

        _, rstd = fused()

        def backward():
            return K.qk_norm_bwd(dqkv, qkv, wq, wk, rstd, nq, nk, d, a.mode, dx=dx)

        # same results first (faster and different is not faster): the fused output against the baseline's
        yq, yk = baseline()
        fused()
        torch.cuda.synchronize()
        same = (torch.cat([yq.view(T, nq * d), yk.view(T, nk * d)], 1).view(torch.int16) != out.view(torch.int16))
        fb, bb = 4 * E + 4 * T * nh, 6 * E + 4 * T * nh
        for rnd in range(3):
            order = (("fused", fused), ("baseline", baseline)) if rnd % 2 == 0 else (("baseline", baseline), ("fused", fused))
            t = {name: graph_us(fn) for name, fn in order}
            t_n, t_b = graph_us(norm_only), graph_us(backward)
            print(json.dumps({
                "shape": f"T{T} {nq}+{nk}x{d}", "round": rnd, "mode": a.mode,
                "fwd_us": round(t["fused"], 2), "fwd_GBps": round(fb / t["fused"] / 1e3, 1),
                "fwd_norm_only_us": round(t_n, 2),
                "baseline_rmsnorm_plus_rope_us": round(t["baseline"], 2),
                "baseline_over_fused": round(t["baseline"] / t["fused"], 2),
                "bwd_us": round(t_b, 2), "bwd_GBps": round(bb / t_b / 1e3, 1),
                "fwd_MiB": round(fb / 2 ** 20, 1), "bwd_MiB": round(bb / 2 ** 20, 1),
                "bit_mismatch_share_vs_baseline": round(float(same.double().mean()), 6)}), flush=True)
            ratios.append(t["baseline"] / t["fused"])
    if min(ratios) <= 1.0:
        raise SystemExit(f"qk_norm_bench: the fused forward is not faster than pt_rmsnorm_fwd + pt_rope ({min(ratios):.2f}x)")


if __name__ == "__main__":
    main()
