"""Head dim 256 attention kernels (csrc/attention_d256.hip) timed, forward and backward, B 4, S 1024 / 4096,
in one process: d256 at H 8 / HKV 8 and H 8 / HKV 4 against (a) this project's d128 causal kernels at H 16
-- the same causal FLOP -- and (b) torch scaled_dot_product_attention on the d256 tensors of each head
layout.  The variants alternate round by round; each figure is the median over rounds of a device-event
window of `--iters` calls, and every shape is warmed first.  Causal FLOP from the shapes: forward
2 B H S^2/2 (2 D), backward 2.5 times that.  Each d256 line ends with its FLOP rate relative to the d128
kernels of the same run.  Writes the table and the device's id to --out; needs a GPU (no fallback).

  python tools/attn_d256_bench.py [--rounds 5] [--iters 100] [--out profiles/attn_d256_bench.log]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from picotron_amd import kernels as K   # noqa: E402

BF = torch.bfloat16
B = 4


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def ours(S, H, HKV, D, g):
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32).to(BF)
    q, k, v, do = rn(B, S, H, D), rn(B, S, HKV, D), rn(B, S, HKV, D), rn(B, S, H, D)
    scale = D ** -0.5
    o, lse = K.attn_fwd(q, k, v, scale, True)
    gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    return (q, k, v, do), (lambda: K.attn_fwd(q, k, v, scale, True, out=o, lse=lse),
                           lambda: K.attn_bwd(do, q, k, v, o, lse, scale, True, dq=gq, dk=gk, dv=gv))


def sdpa(q, k, v, do):
    qt, kt, vt = (t.transpose(1, 2).contiguous().requires_grad_(True) for t in (q, k, v))
    dot = do.transpose(1, 2).contiguous()
    gqa = q.shape[2] != k.shape[2]
    fwd = lambda: torch.nn.functional.scaled_dot_product_attention(qt, kt, vt, is_causal=True, enable_gqa=gqa)
    ot = fwd()
    return fwd, lambda: torch.autograd.grad(ot, (qt, kt, vt), dot, retain_graph=True)


def cases(S, notes):
    """name -> (forward, backward); all of the same causal FLOP.  A torch SDPA form this torch build does
    not run is noted as not measured; ours must run."""
    g = torch.Generator(device="cuda").manual_seed(S)
    out = {}
    for name, hkv in (("d256 h8/kv8", 8), ("d256 h8/kv4", 4)):
        tensors, out[name] = ours(S, 8, hkv, 256, g)
        try:
            out["sdpa" + name[4:]] = sdpa(*tensors)
        except RuntimeError as e:
            notes.append(f"S {S:5d} sdpa{name[4:]}: not measured ({str(e).splitlines()[0][:100]})")
    out["d128 h16"] = ours(S, 16, 16, 128, g)[1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    lines = [f"device: {props.name} {getattr(props, 'gcnArchName', '')} uuid {getattr(props, 'uuid', '?')} host {os.uname().nodename}",
             f"B {B}; median of {a.rounds} alternating rounds of {a.iters} calls; TFLOP/s = causal FLOP from shapes / time; "
             "x d128 = FLOP rate relative to the d128 kernels of this run"]
    for S in (1024, 4096):
        cs = cases(S, lines)
        flop = 2.0 * B * 8 * S * S / 2 * (2 * 256)
        times = {(n, d): [] for n in cs for d in (0, 1)}
        for c in cs.values():   # warm every shape
            c[0](), c[1]()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for n, c in cs.items():
                for d in (0, 1):
                    times[n, d].append(window(c[d], a.iters))
        for n in cs:
            for d, what in ((0, "fwd"), (1, "bwd")):
                t, base = times[n, d], statistics.median(times["d128 h16", d])
                med, fl = statistics.median(t), flop * (1.0 if d == 0 else 2.5)
                lines.append(f"S {S:5d} {n:12s} {what}: {med * 1e6:9.1f} us  (min {min(t) * 1e6:.1f} max {max(t) * 1e6:.1f})  "
                             f"{fl / med * 1e-12:7.1f} TFLOP/s  {base / med:5.2f} x d128")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
