"""Muon over the hidden matrices of SmolLM-1.7B (15 layers, H 2048, I 8192: 105 matrices, 1.01 B bf16
parameters): us per step, graph-timed, medians of alternating rounds in one call, of

    (a) the plain bf16 AdamW step on the same parameters (kernels.adamw_step_multi: the baseline),
    (b) optim.Muon.step(),
    (c) torch.optim.Muon.step() on copies of the same tensors,

then (b) split into its parts (momentum + norms, scale, Newton-Schulz, apply), and the Newton-Schulz GEMMs
per launch label under a GemmProbe (HIP events around every launch): achieved TF/s of the Gram (X X^T or
X^T X), the square (A A, f32 sink) and the update (P' X or X P') per shape, to set beside DESIGN section 4's
forward / dX / dW rates of the same shapes.
python tools/muon_bench.py [--layers 15] [--rounds 3] [--reps 2]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from picotron_amd import kernels as K  # noqa: E402
from picotron_amd import optim  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attn_bench import graph_us  # noqa: E402


def out(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    H, I = 2048, 8192
    shapes = [s for _ in range(a.layers) for s in ((H, H), (H, H), (H, H), (H, H), (I, H), (I, H), (H, I))]
    gen = torch.Generator(device="cuda").manual_seed(0)
    params = [torch.nn.Parameter((torch.randn(*s, device="cuda", generator=gen) * 0.02).to(torch.bfloat16)) for s in shapes]
    for p in params:
        p.grad = (torch.randn(p.shape, device="cuda", generator=gen) * 1e-3).to(torch.bfloat16)
    n = sum(p.numel() for p in params)
    ns_flop = sum(5 * 2 * (2 * min(s) ** 2 * max(s) + min(s) ** 3) for s in shapes)
    out(what="parameters", matrices=len(params), params=n, ns_tflop_per_step=round(ns_flop / 1e12, 2))

    adam_items = [(p.detach(), p.grad, torch.zeros_like(p), torch.zeros_like(p)) for p in params]
    adam_args = (0.999 * 3e-4, 0.1, 0.999, 0.001, 0.03, 1e-8, 3e-4)
    muon = optim.Muon(params, lr=0.02)
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    for t, p in zip(twins, params):
        t.grad = p.grad.clone()
    tmuon = torch.optim.Muon(twins, lr=0.02)
    variants = [("a: adamw_step_multi (bf16 state), same parameters", lambda: K.adamw_step_multi(adam_items, *adam_args)),
                ("b: optim.Muon.step()", muon.step),
                ("c: torch.optim.Muon.step()", tmuon.step)]
    times = {name: [] for name, _ in variants}
    for rnd in range(a.rounds):
        for name, fn in (variants if rnd % 2 == 0 else variants[::-1]):
            try:
                us = graph_us(fn, a.reps)
                how = "graph"
            except RuntimeError as e:   # a stream-capture error (an op the graph cannot hold): events around eager calls
                print(f"# {name}: not captured ({e}); timed eagerly", flush=True)
                torch.cuda.synchronize()
                how = f"eager ({type(e).__name__})"
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                fn()
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) / a.reps * 1e3
            times[name].append(us)
            out(variant=name, round=rnd, us=round(us, 1), timed=how)
    for name, ts in times.items():
        out(variant=name, median_us=round(statistics.median(ts), 1), spread_us=round(max(ts) - min(ts), 1),
            ns_tflops=round(ns_flop / statistics.median(ts) / 1e6, 1) if name.startswith("b") else None)

    # (b) in parts
    work = muon._work()
    (group, items, _), = work
    mu, nes = group["momentum"], group["nesterov"]
    sq = K.muon_momentum(items, mu, nes)
    xs = [it[3] for it in items]
    parts = [("momentum + squared norms (4 B/param read, 2 written)", lambda: K.muon_momentum(items, mu, nes), 6),
             ("scale (4 B/param read, 2 written)", lambda: K.muon_scale(items, sq, mu, nes, group["eps"]), 6),
             ("newton_schulz, 5 iterations", lambda: K.muon_newton_schulz(xs, group["ns_coefficients"], 5), None),
             ("apply (4 B/param read, 2 written)", lambda: K.muon_apply(items, 0.02, 0.1), 6)]
    for rnd in range(a.rounds):
        for name, fn, nbytes in parts:
            K.muon_scale(items, sq, mu, nes, group["eps"])   # a sane X0 for the iteration
            us = graph_us(fn, a.reps)
            out(part=name, round=rnd, us=round(us, 1), TBps=round(nbytes * n / us / 1e6, 2) if nbytes else None,
                tflops=None if nbytes else round(ns_flop / us / 1e6, 1))

    # the GEMMs by launch label
    K.muon_scale(items, sq, mu, nes, group["eps"])
    for _ in range(2):
        with K.GemmProbe() as probe:
            K.muon_newton_schulz(xs, group["ns_coefficients"], 5)
            labels = probe.by_label()
    for label, (launches, ms, tf) in labels.items():
        out(gemm=label, launches=launches, total_ms=ms, tflops=tf)
    out(what="status", value=K.device_status(torch.device("cuda")))


if __name__ == "__main__":
    main()
