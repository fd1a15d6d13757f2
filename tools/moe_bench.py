"""The mixture-of-experts block at SmolLM-1.7B's width (H 2048, T 4096 tokens) for E = 8, k = 2 and
E = 64, k = 8 at capacity_factor 1.25: us per call, graph-timed (events around eager calls where a
capture is refused), the best of three replays per round, of

    each routing kernel of csrc/moe.hip with its algorithmic bytes and achieved GB/s,
    the whole block forward (functional.moe_block_fwd) and backward (moe_block_bwd),
    the dense block (mlp_block_fwd / mlp_block_bwd) at the same active FLOPs, I_dense = k * I_moe,

then the expert GEMMs per launch label under a GemmProbe.  No threshold: the log is the record.
--router sigmoid adds the sigmoid router (kernels.moe_route_sigmoid: no groups at E = 8, 4 of 8 groups at
E = 64, a selection bias, scale 2.5) beside the softmax one in the same interleaved rounds: its route and
route_bwd kernels, and the whole block forward and backward.
python tools/moe_bench.py [--tokens 4096] [--hidden 2048] [--dense-inter 8192] [--rounds 3] [--reps 4] [--router sigmoid]"""
import argparse
import hashlib
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


def dropless_rounds(a, h2, res, dout, rw, wgs, wus, wds, E, k, I):
    """Forward and backward of the block dropless, at factor 1.25 and at E / k, alternating in every round;
    tflops counts the items each setting keeps (dropless and E / k: all T k)."""
    T, H = h2.shape
    d_aux = torch.full((1,), 0.01, device="cuda")
    runs = []
    for name, cf in (("dropless", None), ("cf 1.25", 1.25), ("cf E/k", E / k)):
        saved = FN.moe_block_fwd(h2, res, rw, wgs, wus, wds, k, cf)[2]
        kept = int((saved[4] >= 0).sum())
        out(what="setting", E=E, k=k, setting=name, rows=saved[6].shape[0], kept=kept, dropped=T * k - kept)
        runs.append((name + " forward", lambda cf=cf: FN.moe_block_fwd(h2, res, rw, wgs, wus, wds, k, cf), 6 * kept * H * I))
        runs.append((name + " backward", lambda saved=saved, cf=cf: FN.moe_block_bwd(dout, d_aux, h2, saved, rw, wgs, wus, wds, k,
                                                                                     dropless=cf is None), 12 * kept * H * I))
    for rnd in range(a.rounds):
        for name, fn, flop in (runs if rnd % 2 == 0 else runs[::-1]):
            us, how = time_us(fn, a.reps)
            out(block=name, E=E, k=k, round=rnd, us=round(us, 1), tflops=round(flop / us / 1e6, 1), timed=how)
    for _ in range(2):   # the second pass is the warm one
        with K.GemmProbe() as probe:
            s2 = FN.moe_block_fwd(h2, res, rw, wgs, wus, wds, k, None)[2]
            FN.moe_block_bwd(dout, d_aux, h2, s2, rw, wgs, wus, wds, k, dropless=True)
            labels = probe.by_label()
    for label, (launches, ms, tf) in labels.items():
        out(gemm=label, E=E, k=k, launches=launches, total_ms=ms, tflops=tf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--dense-inter", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--dropless", action="store_true",
                    help="the block at capacity_factor None (segment GEMMs), 1.25 and E / k (never drops), interleaved")
    ap.add_argument("--router", choices=("softmax", "sigmoid"), default="softmax",
                    help="sigmoid: also time the sigmoid router's kernels and the block with it, interleaved")
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
        if a.dropless:
            dropless_rounds(a, h2, res, dout, rw, wgs, wus, wds, E, k, I)
            del wgs, wus, wds
            torch.cuda.empty_cache()
            continue
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
        router = None
        if a.router == "sigmoid":
            G, Kg = (1, 1) if E < 64 else (8, 4)
            router = FN.MoERouter(torch.randn(E, device="cuda", generator=gen) * 0.1, G, Kg, 2.5, None)
            sg = K.moe_route_sigmoid(logits, k, True, router.bias, G, Kg, 2.5)
            out(what="sigmoid routing", n_group=G, topk_group=Kg, counts_max=int(sg[3].max()), aux=round(sg[4].item(), 4))
            parts += [
                ("route (sigmoid)", lambda: K.moe_route_sigmoid(logits, k, True, router.bias, G, Kg, 2.5), T * E * 6 + T * k * 8),
                ("route_bwd (sigmoid)", lambda: K.moe_route_sigmoid_bwd(dgate, sg[2], sg[0], sg[1], sg[3], d_aux, True, 2.5),
                 T * E * 6 + T * k * 12),
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
        if router is not None:   # (its own routing: the kept items differ, so the tflops column is the softmax block's only)
            ssaved = FN.moe_block_fwd(h2, res, rw, wgs, wus, wds, k, 1.25, router=router)[2]
            skept = int((ssaved[4] >= 0).sum())
            blocks += [
                ("moe block forward (sigmoid)", lambda: FN.moe_block_fwd(h2, res, rw, wgs, wus, wds, k, 1.25, router=router),
                 6 * skept * H * I),
                ("moe block backward (sigmoid)", lambda: FN.moe_block_bwd(dout, d_aux, h2, ssaved, rw, wgs, wus, wds, k,
                                                                          router=router), 12 * skept * H * I),
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
    import socket
    out(what="box", id=hashlib.sha1(socket.gethostname().encode()).hexdigest()[:8])
    out(what="status", value=K.device_status(torch.device("cuda")))


if __name__ == "__main__":
    main()
