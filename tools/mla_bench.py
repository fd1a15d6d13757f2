"""MLA attention kernels (csrc/attention_mla.hip) timed, forward and backward, H 16, B 4, S 1024 / 4096,
in one process against (a) torch scaled_dot_product_attention on the materialised 192 / 128 tensors and
(b) this project's d128 causal kernels at the same B, S, H (256 / 320 of MLA's forward FLOP: compare the
FLOP rates, not the times).  The three alternate round by round; each figure is the median over rounds
of a device-event window of `--iters` calls.  Causal FLOP from the shapes: forward 2 B H S^2/2 (dqk + dv),
backward 2.5 times that.  Writes the table and the device's id to --out.

  python tools/mla_bench.py [--rounds 7] [--iters 20] [--out profiles/mla_bench.log]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from picotron_amd import kernels as K   # noqa: E402

BF = torch.bfloat16
B, H, DN, DR, DV = 4, 16, 128, 64, 128


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def cases(S):
    """name -> (forward, backward, forward FLOP)."""
    g = torch.Generator(device="cuda").manual_seed(S)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32).to(BF)
    q, kvb, kva, do = rn(B, S, H, DN + DR), rn(B, S, H, DN + DV), rn(B, S, 512 + DR), rn(B, S, H, DV)
    k_nope, v, k_pe = kvb[..., :DN], kvb[..., DN:], kva[..., 512:]
    scale = (DN + DR) ** -0.5
    cos, sin = torch.ones(S, DR, dtype=BF, device="cuda"), torch.zeros(S, DR, dtype=BF, device="cuda")
    o, lse = K.mla_attn_fwd(q, k_nope, k_pe, v, scale)
    ws = K.mla_workspace(B, S, H, "cuda")
    sinks = dict(dq=torch.empty_like(q), dk_nope=torch.empty_like(kvb)[..., :DN], dv=torch.empty_like(kvb)[..., DN:],
                 dk_pe=torch.empty_like(kva)[..., 512:], ws=ws)
    flop = lambda dqk, dv: 2.0 * B * H * S * S / 2 * (dqk + dv)
    out = {"mla": (lambda: K.mla_attn_fwd(q, k_nope, k_pe, v, scale, out=o, lse=lse),
                   lambda: K.mla_attn_bwd(do, q, k_nope, k_pe, v, o, lse, scale, cos, sin, **sinks), flop(DN + DR, DV))}
    # (a) torch SDPA on the materialised k [B, H, S, 192] (the broadcast built outside the timed window)
    qt = q.transpose(1, 2).contiguous().requires_grad_(True)
    kt = torch.cat([k_nope, k_pe[:, :, None, :].expand(B, S, H, DR)], -1).transpose(1, 2).contiguous().requires_grad_(True)
    vt = v.transpose(1, 2).contiguous().requires_grad_(True)
    dot = do.transpose(1, 2).contiguous()
    sdpa = lambda: torch.nn.functional.scaled_dot_product_attention(qt, kt, vt, is_causal=True, scale=scale)
    ot = sdpa()
    out["sdpa"] = (lambda: sdpa(), lambda: torch.autograd.grad(ot, (qt, kt, vt), dot, retain_graph=True), flop(DN + DR, DV))
    # (b) the d128 kernels
    q1, k1, v1, do1 = rn(B, S, H, 128), rn(B, S, H, 128), rn(B, S, H, 128), rn(B, S, H, 128)
    o1, lse1 = K.attn_fwd(q1, k1, v1, 128 ** -0.5, True)
    g1 = [torch.empty_like(q1) for _ in range(3)]
    out["d128"] = (lambda: K.attn_fwd(q1, k1, v1, 128 ** -0.5, True, out=o1, lse=lse1),
                   lambda: K.attn_bwd(do1, q1, k1, v1, o1, lse1, 128 ** -0.5, True, dq=g1[0], dk=g1[1], dv=g1[2]), flop(128, 128))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    props = torch.cuda.get_device_properties(0)
    lines = [f"device: {props.name} {getattr(props, 'gcnArchName', '')} uuid {getattr(props, 'uuid', '?')} host {os.uname().nodename}",
             f"B {B} H {H} dims {DN}/{DR}/{DV}; median of {a.rounds} alternating rounds of {a.iters} calls; TFLOP/s = causal FLOP from shapes / time"]
    for S in (1024, 4096):
        cs = cases(S)
        times = {(n, d): [] for n in cs for d in (0, 1)}
        for n, c in cs.items():   # warm every shape
            c[0](), c[1]()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for n, c in cs.items():
                for d in (0, 1):
                    times[n, d].append(window(c[d], a.iters))
        for n, c in cs.items():
            for d, what in ((0, "fwd"), (1, "bwd")):
                t = times[n, d]
                med, fl = statistics.median(t), c[2] * (1.0 if d == 0 else 2.5)
                lines.append(f"S {S:5d} {n:5s} {what}: {med * 1e6:9.1f} us  (min {min(t) * 1e6:.1f} max {max(t) * 1e6:.1f})  "
                             f"{fl / med * 1e-12:7.1f} TFLOP/s")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
