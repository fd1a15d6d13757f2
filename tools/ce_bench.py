"""Cross-entropy forms at the lm_head's shape (T 4096, V 49152): us per call from a HIP graph of `reps`
back-to-back calls (no host gaps), as tools/norm_bench.py times the norms.

    python tools/ce_bench.py [--rows 4096 --vocab 49152] [--old lib.so] [--rounds 5]

fwd_lse: the streaming forward (pt_cross_entropy_fwd_lse); bwd_lse: the elementwise backward from the
saved LSE; fwd_stats: the forward from the lm_head GEMM's tile statistics (synthetic statistics of the
same logits, 256-column tiles); fwd_bwd: the one-read fused form, in place.
--old: a library holding another build of the pt_cross_entropy_* entry points, timed in the same process,
the two libraries alternating per round.  The last lines give, per form, each library's median over the
rounds, the old library's max - min, and whether new <= old's median + that spread.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from picotron_amd import _C  # noqa: E402
from picotron_amd import kernels as K  # noqa: E402  (ce_stats_block)
from tools.norm_bench import graph_us  # noqa: E402

FORMS = ("fwd_lse", "bwd_lse", "fwd_stats", "fwd_bwd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--vocab", type=int, default=49152)
    ap.add_argument("--old", default="")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    T, V = a.rows, a.vocab
    g = torch.Generator(device="cuda").manual_seed(0)
    x = (torch.randn(T, V, device="cuda", generator=g) * 3).to(torch.bfloat16)
    tgt = torch.randint(0, V, (T,), device="cuda", generator=g)
    tgt[::17] = -100
    scale = torch.full((1,), 1.0 / T, device="cuda")
    nblk = V // K.ce_stats_block(T, V)
    tiles = x.float().view(T, nblk, V // nblk)
    m = tiles.amax(2)
    stats = torch.stack([m, torch.exp(tiles - m[..., None]).sum(2)], 2).permute(1, 0, 2).contiguous()
    del tiles
    work, dl = x.clone(), torch.empty_like(x)
    rl, rl2, lse, lse2 = (torch.empty(T, dtype=torch.float32, device="cuda") for _ in range(4))
    inv = torch.full((1,), 1.0 / T, device="cuda")
    p = lambda t: t.data_ptr()   # noqa: E731

    def measure(tag, lib):
        """The native entry points themselves, on preallocated outputs: nothing but the kernels is timed."""
        def call(name, *args):
            rc = getattr(lib, name)(*args, _C.stream_ptr())
            assert rc == 0, f"{name} returned {rc}"
        forms = {
            "fwd_lse": lambda: call("pt_cross_entropy_fwd_lse", p(x), V, p(tgt), p(rl), p(lse), T, V, -100, None),
            "bwd_lse": lambda: call("pt_cross_entropy_bwd_lse", p(x), V, p(tgt), p(lse), p(dl), V, T, V, p(scale), 0, -100),
            "fwd_stats": lambda: call("pt_cross_entropy_fwd_stats", p(x), V, p(tgt), p(stats), nblk, p(rl), p(lse2), T, V,
                                      -100, None),
            # in place on a scratch copy: the values drift from call to call, the time does not
            "fwd_bwd": lambda: call("pt_cross_entropy_fwd_bwd", p(work), V, p(tgt), p(work), V, p(rl2), T, V, 1.0, p(inv),
                                    -100, None)}
        t = {f: graph_us(fn) for f, fn in forms.items()}
        print(json.dumps({"cfg": tag, **{f + "_us": round(v, 2) for f, v in t.items()}}), flush=True)
        return t, (rl.clone(), lse.clone(), dl.clone(), lse2.clone())

    libs = {"new": _C.load_library()}
    if a.old:
        libs["old"] = _C.load_library(os.path.abspath(a.old), strict=False)
    times, refs = {n: {f: [] for f in FORMS} for n in libs}, {}
    for rnd in range(a.rounds):
        for name, lib in (list(libs.items())[::-1] if rnd % 2 else libs.items()):
            t, refs[name] = measure(f"{name}:r{rnd}", lib)
            for f in FORMS:
                times[name][f].append(t[f])
    if "old" in libs:
        def bits(t):
            return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
        same = [torch.equal(bits(n), bits(o)) for n, o in zip(refs["new"], refs["old"])]
        print(json.dumps({"bit_identical_rowloss_lse_grad_statslse": same}), flush=True)
        for f in FORMS:
            new, old = statistics.median(times["new"][f]), statistics.median(times["old"][f])
            spread = max(times["old"][f]) - min(times["old"][f])
            print(json.dumps({"form": f, "new_median_us": round(new, 2), "old_median_us": round(old, 2),
                              "old_spread_us": round(spread, 2), "accept": new <= old + spread}), flush=True)


if __name__ == "__main__":
    main()
