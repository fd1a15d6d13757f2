"""The mixture-of-experts block at SmolLM-1.7B's width (H 2048, T 4096 tokens) for E = 8, k = 2 and
E = 64, k = 8 at capacity_factor 1.25: us per call, graph-timed (events around eager calls where a
capture is refused), the best of three replays per round, of

    each routing kernel of csrc/moe.hip with its algorithmic bytes and achieved GB/s,
    the whole block forward (functional.moe_block_fwd) and backward (moe_block_bwd),
    the dense block (mlp_block_fwd / mlp_block_bwd) at the same active FLOPs, I_dense = k * I_moe,

then the expert GEMMs per launch label under a GemmProbe.  No threshold: the log is the record.
python tools/moe_bench.py [--tokens 4096] [--hidden 2048] [--dense-inter 8192] [--rounds 3] [--reps 4]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from picotron_amd import functional as FN  # noqa: E402
from picotron_amd import kernels as K  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attn_bench import graph_us  # noqa: E402

BF = torch.bfloat16


def out(**kw):
    print(json.dumps(kw), flush=True)


def time_us(fn, reps):
    try:
        return graph_us(fn, reps), "graph"
    except RuntimeError as e:   # a stream-capture error: events around eager calls
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3, f"eager ({type(e).__name__})"


def weights(n, rows, cols, gen):
    ws = [torch.nn.Parameter(((torch.rand(rows, cols, device="cuda", generator=gen) * 2 - 1) / cols ** 0.5).to(BF))
          for _ in range(n)]
    for w in ws:
        w.grad = torch.zeros_like(w)   # the accumulating epilogue, as in every micro-batch but the first
    return ws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--dense-inter", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=4)
    a = ap.parse_args()
    T, H = a.tokens, a.hidden
    gen = torch.Generator(device="cuda").manual_seed(0)
    h2 = torch.randn(T, H, device="cuda", generator=gen).to(BF)
    res = torch.randn(T, H, device="cuda", generator=gen).to(BF)
    dout = torch.randn(T, H, device="cuda", generator=gen).to(BF)
    tp = FN.TPContext.current()

    for E, k in ((8, 2), (64, 8)):
        I = a.dense_inter // k
        C = K.moe_capacity(T, E, k, 1.25)
        R = E * C
        out(what="case", E=E, k=k, T=T, H=H, I_moe=I, I_dense=k * I, C=C, rows=R)
        rw = weights(1, E, H, gen)[0]
        wgs, wus, wds = weights(E, I, H, gen), weights(E, I, H, gen), weights(E, H, I, gen)
        logits = K.linear_fwd(h2, [rw])
        idx, gate, probs, counts, aux = K.moe_route(logits, k)
        slot, src = K.moe_plan(idx, E, C)
        kept = int((slot >= 0).sum())
        out(what="routing", items=T * k, kept=kept, dropped=T * k - kept, counts_max=int(counts.max()), aux=round(aux.item(), 4))
        xe = K.moe_dispatch(h2, src, k)
        ye = torch.randn(R, H, device="cuda", generator=gen).to(BF)
        dye, dgate = K.moe_combine_bwd(dout, ye, slot, src, gate)
        d_aux = torch.full((1,), 0.01, device="cuda")
        parts = [
            ("route", lambda: K.moe_route(logits, k), T * E * 6 + T * k * 8),
            ("plan", lambda: K.moe_plan(idx, E, C), T * k * 16 + R * 4),
            ("dispatch", lambda: K.moe_dispatch(h2, src, k), kept * H * 2 + R * H * 2 + R * 4),
            ("combine (gate, residual)", lambda: K.moe_combine(ye, slot, gate, res), kept * H * 2 + 2 * T * H * 2 + T * k * 8),
            ("combine (dispatch backward)", lambda: K.moe_combine(ye, slot), kept * H * 2 + T * H * 2 + T * k * 4),
            ("combine_bwd", lambda: K.moe_combine_bwd(dout, ye, slot, src, gate), 2 * kept * H * 2 + R * H * 2 + T * k * 12 + R * 4),
            ("route_bwd", lambda: K.moe_route_bwd(dgate, probs, idx, counts, d_aux), T * E * 6 + T * k * 8),
        ]
        for rnd in range(a.rounds):
            for name, fn, nbytes in (parts if rnd % 2 == 0 else parts[::-1]):
                us, how = time_us(fn, a.reps)
                out(kernel=name, E=E, k=k, round=rnd, us=round(us, 2), bytes=nbytes, GBps=round(nbytes / us / 1e3, 1), timed=how)

        saved = FN.moe_block_fwd(h2, res, rw, wgs, wus, wds, k, 1.25)[2]
        moe_flop = 6 * kept * H * I   # gate, up, down: 2 flop each per kept item, forward
        dI = k * I
        dg, du, dd = weights(1, dI, H, gen)[0], weights(1, dI, H, gen)[0], weights(1, H, dI, gen)[0]
        dsaved = FN.mlp_block_fwd(h2, dg, du, dd, tp, residual=res)[1]
        blocks = [
            ("moe block forward", lambda: FN.moe_block_fwd(h2, res, rw, wgs, wus, wds, k, 1.25), moe_flop),
            ("moe block backward", lambda: FN.moe_block_bwd(dout, d_aux, h2, saved, rw, wgs, wus, wds, k), 2 * moe_flop),
            ("dense block forward", lambda: FN.mlp_block_fwd(h2, dg, du, dd, tp, residual=res), 6 * T * H * dI),
            ("dense block backward", lambda: FN.mlp_block_bwd(dout, h2, dsaved, dg, du, dd, tp), 12 * T * H * dI),
        ]
        for rnd in range(a.rounds):
            for name, fn, flop in (blocks if rnd % 2 == 0 else blocks[::-1]):
                us, how = time_us(fn, a.reps)
                out(block=name, E=E, k=k, round=rnd, us=round(us, 1), tflops=round(flop / us / 1e6, 1), timed=how)
        for _ in range(2):
            with K.GemmProbe() as probe:
                s2 = FN.moe_block_fwd(h2, res, rw, wgs, wus, wds, k, 1.25)[2]
                FN.moe_block_bwd(dout, d_aux, h2, s2, rw, wgs, wus, wds, k)
                labels = probe.by_label()
        for label, (launches, ms, tf) in labels.items():
            out(gemm=label, E=E, k=k, launches=launches, total_ms=ms, tflops=tf)
        del wgs, wus, wds, dg, du, dd, saved, dsaved, s2
        torch.cuda.empty_cache()
    out(what="status", value=K.device_status(torch.device("cuda")))


if __name__ == "__main__":
    main()
