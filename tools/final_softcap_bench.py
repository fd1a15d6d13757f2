"""Final-logit soft-capping microbenchmark: lm_head forward, cross-entropy forward and backward, lm_head backward
(dX and dW) at T 4096, H 2048, V 49152, three arms alternating in one process:

    fused    lm_head_linear(softcap=c): the cap in the GEMM epilogue, its derivative in the CE backward's store
    plain    no cap (the path bench.py takes)
    torch    the cap as torch ops between lm_head_linear and F.cross_entropy (divide, tanh, multiply)

ms per step from HIP events around `reps` eager steps; medians of `rounds` windows per arm, the arms' order
rotating between rounds.

    python tools/final_softcap_bench.py [--reps 10] [--rounds 5] [--softcap 30]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from picotron_amd import functional as FN  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--softcap", type=float, default=30.0)
    ap.add_argument("--shape", type=int, nargs=3, default=(4096, 2048, 49152), metavar=("T", "H", "V"))
    a = ap.parse_args()
    prop = torch.cuda.get_device_properties(0)
    print(json.dumps({"device": prop.name, "arch": getattr(prop, "gcnArchName", ""), "cus": prop.multi_processor_count,
                      "uuid": str(getattr(prop, "uuid", ""))}), flush=True)
    T, H, V = a.shape
    c = a.softcap
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(T, H, device="cuda", generator=g).to(torch.bfloat16).requires_grad_(True)
    w = (torch.randn(V, H, device="cuda", generator=g) * (c / H ** 0.5)).to(torch.bfloat16).requires_grad_(True)
    tgt = torch.randint(0, V, (T,), device="cuda", generator=g)

    def step(arm):
        x.grad = None
        if arm == "torch":
            y = FN.lm_head_linear(x, w)
            y = torch.tanh(y / c) * c
        else:
            y = FN.lm_head_linear(x, w, softcap=c if arm == "fused" else None)
        FN.cross_entropy(y, tgt).backward()

    arms = ["fused", "plain", "torch"]
    for arm in arms:   # warm-up: allocations, the kernels' first launches, w.grad
        step(arm)
        step(arm)
    torch.cuda.synchronize()
    t = {arm: [] for arm in arms}
    for rnd in range(a.rounds):
        for arm in arms[rnd % 3:] + arms[:rnd % 3]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                step(arm)
            e1.record()
            torch.cuda.synchronize()
            t[arm].append(e0.elapsed_time(e1) / a.reps)
    row = {"T": T, "H": H, "V": V, "softcap": c, "reps": a.reps}
    for arm in arms:
        row[f"{arm}_ms"] = [round(v, 3) for v in sorted(t[arm])]
    med = {arm: statistics.median(t[arm]) for arm in arms}
    row["fused_over_plain"] = round(med["fused"] / med["plain"], 3)
    row["torch_over_plain"] = round(med["torch"] / med["plain"], 3)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
