"""Attention-sink microbenchmark: the sink forward beside the plain forward, alternating in one process, and
kernels.attn_sink_bwd beside the whole backward.  B 4, H 32 / HKV 32, d 64 and 128, S 1024 and 4096, causal
and a 128-key window.  us per call from a HIP graph of `reps` back-to-back calls (tools/attn_bench.py's timer).

    python tools/attn_sinks_bench.py [--reps 20] [--rounds 5]
"""
import argparse
import json
import os
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
    a = ap.parse_args()
    prop = torch.cuda.get_device_properties(0)
    print(json.dumps({"device": prop.name, "arch": getattr(prop, "gcnArchName", ""), "cus": prop.multi_processor_count,
                      "uuid": str(getattr(prop, "uuid", ""))}), flush=True)
    B, H = 4, 32
    for D in (64, 128):
        for S in (1024, 4096):
            for window in (None, 128):
                g = torch.Generator(device="cuda").manual_seed(0)
                qkv = torch.randn(B, S, 3, H, D, device="cuda", generator=g).to(torch.bfloat16)
                q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
                do = torch.randn(B, S, H, D, device="cuda", generator=g).to(torch.bfloat16)
                sinks = torch.randn(H, device="cuda", generator=g).to(torch.bfloat16)
                band = K.attn_band(B, S, "cuda", window=window) if window else None
                scale = D ** -0.5
                o, lse = K.attn_fwd(q, k, v, scale, True, band=band, sinks=sinks)
                arms = {"plain": lambda: K.attn_fwd(q, k, v, scale, True, out=o, lse=lse, band=band),
                        "sink": lambda: K.attn_fwd(q, k, v, scale, True, out=o, lse=lse, band=band, sinks=sinks)}
                t = {n: [] for n in arms}
                for rnd in range(a.rounds):   # alternate, and rotate who goes first
                    for n in (list(arms) if rnd % 2 == 0 else list(arms)[::-1]):
                        t[n].append(graph_us(arms[n], a.reps, rounds=1))
                arms["sink"]()
                dq, dk, dv, delta = K.attn_bwd(do, q, k, v, o, lse, scale, True, band=band)
                gs = torch.empty(H, dtype=torch.bfloat16, device="cuda")
                t_bwd = graph_us(lambda: K.attn_bwd(do, q, k, v, o, lse, scale, True, dq=dq, dk=dk, dv=dv, band=band), a.reps)
                t_sb = graph_us(lambda: K.attn_sink_bwd(lse, delta, sinks, out=gs), a.reps)
                print(json.dumps({"D": D, "S": S, "window": window,
                                  "fwd_plain_us": [round(x, 1) for x in sorted(t["plain"])],
                                  "fwd_sink_us": [round(x, 1) for x in sorted(t["sink"])],
                                  "bwd_us": round(t_bwd, 1), "sink_bwd_us": round(t_sb, 1), "sink_bwd_bytes": B * H * S * 8,
                                  "sink_bwd_GBps": round(B * H * S * 8 / t_sb / 1e3, 1),
                                  "sink_bwd_over_bwd": round(t_sb / t_bwd, 4)}), flush=True)


if __name__ == "__main__":
    main()
