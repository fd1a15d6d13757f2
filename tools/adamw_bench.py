"""Multi-tensor AdamW over the SmolLM-1.7B parameter set (1.21 B bf16 parameters, the model's tensor
sizes): us per step (graph-timed) and HBM rate on 14 B per parameter; --old: another build's library in
the same process -- every variant that calls into the library is then timed once per library per round,
alternating, and its record names the library; --calib: beside it torch's fused AdamW on the same tensors and
the HBM rate of torch's copy (1 read : 1 write) and add (2 : 1) over the same bytes, which bracket
AdamW's 8 : 6 mix; --clip: global gradient-norm clipping -- (a) the plain step, (b) the norm pass alone
(rate on 2 B per parameter, beside torch's x.sum() over the same bytes), (c) norm pass + clipped step,
(c') the clipped step alone, (d) torch.nn.utils.clip_grad_norm_(foreach=True) + (a), alternating over three rounds in one call;
--master: fp32 master weights -- (a), the master step on bf16 / f32 gradients (28 / 30 B per parameter), the f32
norm pass, and torch's fused f32 AdamW + a copy into the bf16 weights, alternating over three rounds in one call;
--sr: stochastic rounding in bf16 state -- (a), (m16) the master step on bf16 gradients, and the SR list step on
bf16 / f32 gradients (14 / 16 B per parameter), clipped and not, alternating over three rounds in one call.
python tools/adamw_bench.py [--old lib.so] [--calib] [--clip] [--master] [--sr]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from picotron_amd import _C  # noqa: E402
from picotron_amd import kernels as K  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attn_bench import graph_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default="")
    ap.add_argument("--calib", action="store_true")
    ap.add_argument("--clip", action="store_true")
    ap.add_argument("--master", action="store_true")
    ap.add_argument("--sr", action="store_true")
    a = ap.parse_args()
    H, I, V, L = 2048, 8192, 49152, 15
    shapes = [(V, H)] + [s for _ in range(L) for s in ((H,), (H, H), (H, H), (H, H), (H, H), (I, H), (I, H), (H, I), (H,))] + [(H,)]
    items = []
    n = 0
    for sh in shapes:
        p = torch.randn(*sh, device="cuda").to(torch.bfloat16)
        items.append((p, torch.randn_like(p) * 1e-3, torch.zeros_like(p), torch.zeros_like(p)))
        n += p.numel()
    args = (0.999 * 3e-4, 0.1, 0.999, 0.001, 0.03, 1e-8, 3e-4)
    libs = {"new": _C.load_library()}
    if a.old:
        libs["old"] = _C.load_library(os.path.abspath(a.old), strict=False)
    for rnd in range(2):
        for name, lib in libs.items():
            use(lib)
            us = graph_us(lambda: K.adamw_step_multi(items, *args), 3)
            print(json.dumps({"lib": f"{name}:r{rnd}", "params": n, "us": round(us, 1), "TBps": round(14 * n / us / 1e6, 2)}),
                  flush=True)
    use(libs["new"])
    if a.calib:
        calib(items, n, args)
    if a.clip:
        clip(items, n, args, libs)
    if a.master:
        master(items, n, args, libs)
    if a.sr:
        sr(items, n, args, libs)


def use(lib):
    """The library the ops call from here on; its descriptor tables are built anew."""
    _C._lib = lib
    K._ADAM_DESC.clear()


def rounds(tag, variants, n, libs):
    """variants: [(name, fn, bytes per parameter or None, calls the library)].  Three rounds; in each,
    a variant that calls the library is timed once per library, a torch-only probe once."""
    for rnd in range(3):
        for name, fn, bpp, in_lib in variants:
            order = list(libs.items())[::-1 if rnd % 2 else 1] if in_lib else [(None, None)]   # who goes first alternates
            for lib_name, lib in order:
                if lib is not None:
                    use(lib)
                us = graph_us(fn, 3)
                rec = {tag: name, "round": rnd, "params": n, "us": round(us, 1)}
                if lib_name:
                    rec["lib"] = lib_name
                if bpp:
                    rec["TBps"] = round(bpp * n / us / 1e6, 2)
                print(json.dumps(rec), flush=True)
    use(libs["new"])


def clip(items, n, args, libs):
    dev = items[0][0].device
    sq = torch.zeros(1, dtype=torch.float32, device=dev)
    status = K.status_word(dev)
    params = []
    for p, g, _, _ in items:   # torch's clip wants parameters with .grad: the same gradient tensors
        q = torch.nn.Parameter(p, requires_grad=True)
        q.grad = g
        params.append(q)
    max_norm = 1.0   # the gradients' norm is ~35: clipping is active
    x = torch.empty(n, dtype=torch.bfloat16, device=dev).normal_()

    def torch_clip_then_step():
        torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=True)
        K.adamw_step_multi(items, *args)

    def fused():
        K.grad_sqnorm(items=items, out=sq)
        K.adamw_step_multi_clip(items, sq, max_norm, *args, status=status)
    variants = [("a: adamw_step_multi", lambda: K.adamw_step_multi(items, *args), 14, True),
                ("b: grad_sqnorm", lambda: K.grad_sqnorm(items=items, out=sq), 2, True),
                ("probe: sum 1r", lambda: x.sum(), 2, False),
                ("c: grad_sqnorm + adamw_step_multi_clip", fused, 16, True),
                ("c': adamw_step_multi_clip alone", lambda: K.adamw_step_multi_clip(items, sq, max_norm, *args, status=status), 14, True),
                ("d: torch clip_grad_norm_ + adamw_step_multi", torch_clip_then_step, None, True)]
    rounds("clip", variants, n, libs)
    torch.cuda.synchronize()
    print(json.dumps({"clip": "grad norm", "value": round(float(sq.sqrt()), 4),
                      "status": K.device_status(dev)}), flush=True)


def master(items, n, args, libs):
    """fp32 master weights: (a) today's bf16 step, (m16) / (m32) the master step on bf16 / f32 gradients
    (28 / 30 B per parameter), (n32) the f32 norm pass alone (4 B), (t) what a user would do without the
    kernel: torch._fused_adamw_ on f32 param / grad / moments, then _foreach_copy_ into the bf16 weights;
    beside them torch's copy over the master step's bytes (1 read : 1 write, the step's own mix)."""
    ps = [p for p, _, _, _ in items]
    g16 = [g for _, g, _, _ in items]
    ws = [p.float() for p in ps]
    g32 = [g.float() for g in g16]
    ms = [torch.zeros_like(w) for w in ws]
    vs = [torch.zeros_like(w) for w in ws]
    m16 = list(zip(ws, ps, g16, ms, vs))
    m32 = list(zip(ws, ps, g32, ms, vs))
    sq = torch.zeros(1, dtype=torch.float32, device=ps[0].device)
    lr, wd, b1, b2, eps = args[6], 0.1, 0.9, args[2], args[5]
    step = torch.tensor(3.0, device="cuda")

    def torch_master():
        torch._fused_adamw_(ws, g32, ms, vs, [], [step] * len(ws), lr=lr, beta1=b1, beta2=b2, weight_decay=wd, eps=eps,
                            amsgrad=False, maximize=False)
        torch._foreach_copy_(ps, ws)
    x = torch.empty(7 * n, dtype=torch.bfloat16, device=ps[0].device).normal_()   # the master step's 14 B read,
    y = torch.empty_like(x)                                                        # 14 B written, as one copy
    variants = [("a: adamw_step_multi (bf16 state)", lambda: K.adamw_step_multi(items, *args), 14, True),
                ("probe: torch copy 1r:1w over 28 B/param", lambda: y.copy_(x), 28, False),
                ("m16: adamw_master_step_multi, bf16 grads", lambda: K.adamw_master_step_multi(m16, *args), 28, True),
                ("m32: adamw_master_step_multi, f32 grads", lambda: K.adamw_master_step_multi(m32, *args), 30, True),
                ("n32: grad_sqnorm, f32 grads", lambda: K.grad_sqnorm(items=m32, out=sq), 4, True),
                ("t: torch._fused_adamw_ f32 + _foreach_copy_ to bf16", torch_master, None, False)]
    rounds("master", variants, n, libs)
    torch.cuda.synchronize()
    print(json.dumps({"master": "status", "value": K.device_status(ps[0].device)}), flush=True)


def sr(items, n, args, libs):
    """Stochastic rounding: (a) the plain bf16 step and (m16) the master step on bf16 gradients, the two recipes it
    sits between; (sr16) / (sr32) the SR list step on bf16 / f32 gradients (14 / 16 B per parameter, the plain
    step's traffic; the state is 8 B per parameter smaller than the master recipe's); (sr16c) / (sr32c) the same with
    the clip coefficient applied to the loaded gradient (the norm pass is timed by --clip and --master)."""
    ps = [p for p, _, _, _ in items]
    g16 = [g for _, g, _, _ in items]
    g32 = [g.float() for g in g16]
    m16 = list(zip([p.float() for p in ps], ps, g16, [torch.zeros_like(g) for g in g32], [torch.zeros_like(g) for g in g32]))
    s16 = [(p, g, m, v, i) for i, (p, g, m, v) in enumerate(items)]
    s32 = [(p, g, m, v, i) for i, ((p, _, m, v), g) in enumerate(zip(items, g32))]
    dev = ps[0].device
    sq = K.grad_sqnorm(items=s16)
    status = K.status_word(dev)
    key = dict(seed=0x123456789ABCDEF0, step=3)
    max_norm = 1.0   # the gradients' norm is ~35: clipping is active
    variants = [("a: adamw_step_multi (bf16 state)", lambda: K.adamw_step_multi(items, *args), 14, True),
                ("m16: adamw_master_step_multi, bf16 grads", lambda: K.adamw_master_step_multi(m16, *args), 28, True),
                ("sr16: adamw_sr_step_multi, bf16 grads", lambda: K.adamw_sr_step_multi(s16, *args, **key), 14, True),
                ("sr32: adamw_sr_step_multi, f32 grads", lambda: K.adamw_sr_step_multi(s32, *args, **key), 16, True),
                ("sr16c: adamw_sr_step_multi_clip, bf16 grads",
                 lambda: K.adamw_sr_step_multi_clip(s16, sq, max_norm, *args, status=status, **key), 14, True),
                ("sr32c: adamw_sr_step_multi_clip, f32 grads",
                 lambda: K.adamw_sr_step_multi_clip(s32, sq, max_norm, *args, status=status, **key), 16, True)]
    rounds("sr", variants, n, libs)
    torch.cuda.synchronize()
    print(json.dumps({"sr": "status", "value": K.device_status(dev), "grad norm": round(float(sq.sqrt()), 4)}), flush=True)


def calib(items, n, args):
    ps, gs, ms, vs = (list(t) for t in zip(*items))
    lr, wd, b1, b2, eps = args[6], 0.1, 0.9, args[2], args[5]
    step = torch.tensor(3.0, device="cuda")
    us = graph_us(lambda: torch._fused_adamw_(ps, gs, ms, vs, [], [step] * len(ps), lr=lr, beta1=b1, beta2=b2,
                                              weight_decay=wd, eps=eps, amsgrad=False, maximize=False), 3)
    print(json.dumps({"lib": "torch._fused_adamw_", "params": n, "us": round(us, 1), "TBps": round(14 * n / us / 1e6, 2)}),
          flush=True)
    hot_cold(items, args)
    x = torch.empty(n, dtype=torch.bfloat16, device="cuda").normal_()
    y, z = torch.empty_like(x), torch.empty_like(x)
    us = graph_us(lambda: y.copy_(x), 3)
    print(json.dumps({"probe": "copy 1r:1w", "bytes": 4 * n, "us": round(us, 1), "TBps": round(4 * n / us / 1e6, 2)}), flush=True)
    us = graph_us(lambda: torch.add(x, y, out=z), 3)
    print(json.dumps({"probe": "add 2r:1w", "bytes": 6 * n, "us": round(us, 1), "TBps": round(6 * n / us / 1e6, 2)}), flush=True)
    us = graph_us(lambda: x.sum(), 3)
    print(json.dumps({"probe": "sum 1r", "bytes": 2 * n, "us": round(us, 1), "TBps": round(2 * n / us / 1e6, 2)}), flush=True)


def hot_cold(items, args):
    """One AdamW launch right after ~0.8 s of back-to-back bf16 GEMMs (the chip as the training step
    leaves it) vs after 0.5 s idle: the in-situ kernel table's launch is ~25 % slower than the graph loop."""
    import time
    fn = lambda: K.adamw_step_multi(items, *args)  # noqa: E731
    fn()
    torch.cuda.synchronize()
    A = torch.randn(8192, 8192, device="cuda", dtype=torch.bfloat16)
    C = torch.empty_like(A)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(3):
        for mode in ("idle", "hot"):
            torch.cuda.synchronize()
            if mode == "idle":
                time.sleep(0.5)
            else:
                for _ in range(900):
                    torch.mm(A, A, out=C)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            print(json.dumps({"adamw_after": mode, "round": rnd, "us": round(e0.elapsed_time(e1) * 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
