"""Soft-capping microbenchmark: the soft-capped forward and backward beside the plain ones, alternating in one
process.  B 4, H 32 / HKV 32, d 64 and 128, S 1024 and 4096, causal, softcap 50.  us per call from a HIP graph of
`reps` back-to-back calls (tools/attn_bench.py's timer); medians of `rounds` windows per arm.

    python tools/attn_softcap_bench.py [--reps 20] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from attn_bench import graph_us  # noqa: E402
from picotron_amd import kernels as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--softcap", type=float, default=50.0)
    a = ap.parse_args()
    prop = torch.cuda.get_device_properties(0)
    print(json.dumps({"device": prop.name, "arch": getattr(prop, "gcnArchName", ""), "cus": prop.multi_processor_count,
                      "uuid": str(getattr(prop, "uuid", ""))}), flush=True)
    B, H = 4, 32
    for D in (64, 128):
        for S in (1024, 4096):
            g = torch.Generator(device="cuda").manual_seed(0)
            qkv = torch.randn(B, S, 3, H, D, device="cuda", generator=g).to(torch.bfloat16)
            q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
            do = torch.randn(B, S, H, D, device="cuda", generator=g).to(torch.bfloat16)
            scale = D ** -0.5
            buf = {}
            for name, c in (("plain", None), ("cap", a.softcap)):   # each arm's own o / lse, so its backward matches
                o, lse = K.attn_fwd(q, k, v, scale, True, softcap=c)
                buf[name] = (c, o, lse) + K.attn_bwd(do, q, k, v, o, lse, scale, True, softcap=c)[:3]

            def fwd(n):
                c, o, lse = buf[n][:3]
                return lambda: K.attn_fwd(q, k, v, scale, True, out=o, lse=lse, softcap=c)

            def bwd(n):
                c, o, lse, dq, dk, dv = buf[n]
                return lambda: K.attn_bwd(do, q, k, v, o, lse, scale, True, dq=dq, dk=dk, dv=dv, softcap=c)

            row = {"D": D, "S": S, "softcap": a.softcap}
            for what, mk in (("fwd", fwd), ("bwd", bwd)):
                t = {n: [] for n in buf}
                for rnd in range(a.rounds):   # alternate, and rotate who goes first
                    for n in (list(buf) if rnd % 2 == 0 else list(buf)[::-1]):
                        t[n].append(graph_us(mk(n), a.reps, rounds=1))
                for n in buf:
                    row[f"{what}_{n}_us"] = [round(x, 1) for x in sorted(t[n])]
                row[f"{what}_cap_over_plain"] = round(statistics.median(t["cap"]) / statistics.median(t["plain"]), 3)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
