"""GeGLU MLP microbenchmark: the dense MLP block forward + backward (functional.mlp_block_fwd / mlp_block_bwd:
gate|up GEMM, activation, down_proj; down_proj dX + dW, activation backward, gate|up dX + dW) at T 4096, H 2048,
I 8192, three arms alternating in one process:

    swiglu   act="silu", the fused epilogues (EPI 5 / 6): the yardstick, the path bench.py takes
    geglu    act="gelu_tanh", the fused epilogues (EPI 10 / 11)
    rows     act="gelu_tanh" with the fusion switch off (switches.fuse = 0): plain GEMMs + the row kernels

ms per step from HIP events around `reps` eager steps; the sorted windows and the median of `rounds` windows per
arm, the arms' order rotating between rounds.  The three arms' outputs are compared once (geglu == rows bit for bit).

    python tools/geglu_bench.py [--reps 200] [--rounds 7] [--shape T H I] [--arms swiglu ...]

--arms swiglu alone also runs on a checkout from before the act keyword (the parent's time of the shared code).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from picotron_amd import functional as FN  # noqa: E402
from picotron_amd import switches  # noqa: E402

ARMS = {"swiglu": ("silu", 1), "geglu": ("gelu_tanh", 1), "rows": ("gelu_tanh", 0)}   # arm -> (act, switches.fuse)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)   # ~1 ms steps: 0.2 s windows
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shape", type=int, nargs=3, default=(4096, 2048, 8192), metavar=("T", "H", "I"))
    ap.add_argument("--arms", nargs="+", default=list(ARMS), choices=list(ARMS))
    a = ap.parse_args()
    arms = a.arms
    prop = torch.cuda.get_device_properties(0)
    print(json.dumps({"device": prop.name, "arch": getattr(prop, "gcnArchName", ""), "cus": prop.multi_processor_count,
                      "uuid": str(getattr(prop, "uuid", ""))}), flush=True)
    T, H, I = a.shape
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    x, dm = rnd(T, H).to(torch.bfloat16), rnd(T, H).to(torch.bfloat16)
    ws = [(rnd(o, i) / i ** 0.5).to(torch.bfloat16).requires_grad_(True) for o, i in ((I, H), (I, H), (H, I))]
    tp = FN.TPContext()

    def step(arm):
        act, fuse = ARMS[arm]
        kw = {} if act == "silu" else {"act": act}   # the SiLU arm makes the calls the parent commit makes
        with switches.override(fuse=fuse):
            for w in ws:
                w.grad = None
            m, saved = FN.mlp_block_fwd(x, *ws, tp, **kw)
            dx = FN.mlp_block_bwd(dm, x, saved, *ws, tp, **kw)
        return m, dx

    outs = {}
    for arm in arms:   # warm-up: allocations, the kernels' first launches
        step(arm)
        m, dx = step(arm)
        torch.cuda.synchronize()
        outs[arm] = [m.clone(), dx.clone()] + [w.grad.clone() for w in ws]
    t = {arm: [] for arm in arms}
    for r in range(a.rounds):
        for arm in arms[r % len(arms):] + arms[:r % len(arms)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                step(arm)
            e1.record()
            torch.cuda.synchronize()
            t[arm].append(e0.elapsed_time(e1) / a.reps)
    row = {"T": T, "H": H, "I": I, "reps": a.reps}
    med = {arm: statistics.median(t[arm]) for arm in arms}
    for arm in arms:
        row[f"{arm}_ms"] = [round(v, 4) for v in sorted(t[arm])]
        row[f"{arm}_median_ms"] = round(med[arm], 4)
    if len(arms) == 3:
        row["geglu_fused_equals_rows"] = all(torch.equal(p, q) for p, q in zip(outs["geglu"], outs["rows"]))
        row["geglu_over_swiglu"] = round(med["geglu"] / med["swiglu"], 4)
        row["rows_over_geglu"] = round(med["rows"] / med["geglu"], 4)
        row["geglu_median_inside_swiglu_windows"] = min(t["swiglu"]) <= med["geglu"] <= max(t["swiglu"])
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
