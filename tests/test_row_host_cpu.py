"""The native host code of the row entry points (csrc/rmsnorm.hip, cross_entropy.hip, swiglu.hip,
rope.hip, and pt_embedding_sort's length limit), pinned without a GPU.

The real library loads on a machine with no device, and its argument checks return before any HIP
call.  Every row of REFUSALS is a call that must be refused, with its return code, replayed against
tests/golden/row_host.json and compared exactly.  Pointers are fake, non-null, 16-byte-aligned
integers (never dereferenced: the call refuses); the pointer tables of pt_rmsnorm_colsum_batch, which
the host code does read, are real host arrays of such integers.  Rows marked (2) hold two violations
and pin which check answers first.

`python tests/test_row_host_cpu.py [library]` writes the golden file.  It was generated once, from the
library of the commit before this file was added, and is never regenerated to make a change pass.
The generator asserts that every recorded code is negative: a call the library accepts has no place in
the table (it would launch a kernel on fake pointers).

ADDED_REFUSALS (tests/golden/row_host_added.json) are the rows that commit did not refuse:
pt_cross_entropy_fwd_bwd cast rows and vocab to int / unsigned without the `> INT32_MAX` check its
four siblings make.
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "row_host.json")
ADDED_GOLDEN = os.path.join(ROOT, "tests", "golden", "row_host_added.json")

P = [0x10000000 + i * 0x100000 for i in range(12)]   # fake device pointers
BIG = 2 ** 31                                         # INT32_MAX + 1, a multiple of 8
DW_BF16, DW_F32 = 4, 8

# entry -> its arguments in ABI order (the stream, always NULL, is appended by call())
DEFAULTS = {
    "pt_rmsnorm_fwd": dict(x=P[0], residual=None, weight=P[1], y=P[2], z_out=None, rstd=P[3], rows=4, cols=64,
                           eps=1e-5, mode=0),
    "pt_rmsnorm_bwd_partials": dict(rows=4, cols=64),
    "pt_rmsnorm_bwd": dict(dy=P[0], z=P[1], weight=P[2], rstd=P[3], dres=None, dx=P[4], dweight=None, dw_partial=P[5],
                           rows=4, cols=64, mode=0),
    "pt_rmsnorm_bwd_splitk": dict(dy_p0=P[0], dy_p1=P[6], z=P[1], weight=P[2], rstd=P[3], dres=None, dx=P[4],
                                  dweight=None, dw_partial=P[5], rows=4, cols=64, mode=0),
    "pt_rmsnorm_colsum_batch": dict(partials=[P[0], P[1]], nparts=[2, 2], dweights=[P[2], P[3]], sinks=[0, DW_F32],
                                    n=2, cols=64),
    "pt_rope": dict(x=P[0], rows=4, row_stride=64, nheads=1, head_dim=64, cos=P[1], sin=P[2], seq_len=4,
                    table_stride=64, inverse=0),
    "pt_swiglu_fwd": dict(g=P[0], g_stride=64, u=P[1], u_stride=64, h=P[2], h_stride=64, rows=4, cols=64),
    "pt_swiglu_bwd": dict(dh=P[0], dh_stride=64, g=P[1], g_stride=64, u=P[2], u_stride=64, dg=P[3], dg_stride=64,
                          du=P[4], du_stride=64, rows=4, cols=64),
    "pt_residual_add": dict(x=P[0], r=P[1], out=P[2], n=64),
    "pt_cross_entropy_fwd_bwd": dict(logits=P[0], logits_stride=64, targets=P[1], dlogits=P[2], dlogits_stride=64,
                                     row_loss=P[3], rows=4, vocab=64, scale=1.0, inv_count=None, ignore_index=-100,
                                     status=None),
    "pt_cross_entropy_fwd_lse": dict(logits=P[0], logits_stride=64, targets=P[1], row_loss=P[3], row_lse=P[4], rows=4,
                                     vocab=64, ignore_index=-100, status=None),
    "pt_cross_entropy_bwd_lse": dict(logits=P[0], logits_stride=64, targets=P[1], row_lse=P[4], dlogits=P[2],
                                     dlogits_stride=64, rows=4, vocab=64, scale=P[5], scale_stride=0, ignore_index=-100),
    "pt_cross_entropy_bwd_lse_shard": dict(logits=P[0], logits_stride=64, targets=P[1], row_lse=P[4], dlogits=P[2],
                                           dlogits_stride=64, rows=4, vocab_shard=64, vocab_lo=64, scale=P[5],
                                           scale_stride=0, ignore_index=-100),
    "pt_cross_entropy_fwd_stats": dict(logits=P[0], logits_stride=64, targets=P[1], stats=P[6], nblk=2, row_loss=P[3],
                                       row_lse=P[4], rows=4, vocab=64, ignore_index=-100, status=None),
    "pt_cross_entropy_vp_partial": dict(logits=P[0], logits_stride=64, targets=P[1], stats=P[6], nblk=2, part=P[7],
                                        rows=4, vocab_shard=64, vocab_lo=0),
    "pt_cross_entropy_vp_combine": dict(parts=P[7], tp=2, targets=P[1], row_loss=P[3], row_lse=P[4], rows=4, vocab=128,
                                        ignore_index=-100, status=None),
    "pt_cross_entropy_mean": dict(row_loss=P[3], targets=P[1], rows=4, ignore_index=-100, loss_f32=None, inv_count=P[5],
                                  out=None, out_bf16=0, reduce_sum=0),
    "pt_embedding_sort": dict(ids=P[0], T=64, vocab_lo=0, vocab_hi=1024, has_padding=0, padding_idx=0, sorted_ids=P[1],
                              perm=P[2]),
}
(NF, NP, NB, NS, NC, RO, SF, SB, RA, CF, CL, CB, CS, CT, VP, VC, CM, ES) = DEFAULTS
RES = dict(residual=P[8], z_out=P[9])

# (entry point, case name, overrides)                                      # the statement reached
REFUSALS = [
    (NF, "null_x", dict(x=None)),                                            # null / counts / cols & 7
    (NF, "null_weight", dict(weight=None)),
    (NF, "null_y", dict(y=None)),
    (NF, "null_rstd", dict(rstd=None)),
    (NF, "rows0", dict(rows=0)),
    (NF, "cols0", dict(cols=0)),
    (NF, "cols_mod", dict(cols=68)),
    (NF, "cols_mod+x_unaligned", dict(cols=68, x=P[0] + 8)),                 # (2) PT_EINVAL first
    (NF, "residual_without_z", dict(residual=P[8])),                         # residual && !z_out
    (NF, "x_unaligned", dict(x=P[0] + 8)),                                   # alignment
    (NF, "weight_unaligned", dict(weight=P[1] + 2)),
    (NF, "y_unaligned", dict(y=P[2] + 8)),
    (NF, "residual_unaligned", dict(RES, residual=P[8] + 8)),
    (NF, "z_unaligned", dict(RES, z_out=P[9] + 8)),
    (NF, "cols_16392", dict(cols=16392)),                                    # above the wide kernels
    (NF, "cols_16392+y_unaligned", dict(cols=16392, y=P[2] + 8)),            # (2) PT_EALIGN first
    (NP, "cols_16392", dict(cols=16392)),
    (NP, "cols_8196", dict(cols=8196)),                                      # wide and off the 8 grid
    (NB, "null_dy", dict(dy=None)),
    (NB, "null_z", dict(z=None)),
    (NB, "null_weight", dict(weight=None)),
    (NB, "null_rstd", dict(rstd=None)),
    (NB, "null_dx", dict(dx=None)),
    (NB, "null_dw_partial", dict(dw_partial=None)),
    (NB, "rows0", dict(rows=0)),
    (NB, "cols_mod", dict(cols=68)),
    (NB, "dy_unaligned", dict(dy=P[0] + 8)),
    (NB, "z_unaligned", dict(z=P[1] + 8)),
    (NB, "dx_unaligned", dict(dx=P[4] + 8)),
    (NB, "dres_unaligned", dict(dres=P[8] + 8)),
    (NB, "cols_16392", dict(cols=16392)),
    (NB, "mode2", dict(mode=2)),                                             # norm mode above 1
    (NB, "mode3_acc", dict(mode=3 | DW_BF16)),
    (NB, "both_acc_bits", dict(mode=DW_BF16 | DW_F32)),                      # both PT_DW_ACC bits
    (NB, "both_acc_bits_mode1", dict(mode=1 | DW_BF16 | DW_F32)),
    (NB, "cols_16392+both_acc_bits", dict(cols=16392, mode=DW_BF16 | DW_F32)),   # (2) PT_EUNSUPPORTED first
    (NS, "null_p0", dict(dy_p0=None)),
    (NS, "null_p1", dict(dy_p1=None)),
    (NS, "null_dw_partial", dict(dw_partial=None)),
    (NS, "cols_mod", dict(cols=68)),
    (NS, "p0_unaligned", dict(dy_p0=P[0] + 8)),
    (NS, "p1_unaligned", dict(dy_p1=P[6] + 4)),
    (NS, "z_unaligned", dict(z=P[1] + 8)),
    (NS, "dres_unaligned", dict(dres=P[8] + 8)),
    (NS, "cols_16392", dict(cols=16392)),
    (NS, "mode2", dict(mode=2)),
    (NS, "both_acc_bits", dict(mode=DW_BF16 | DW_F32)),
    (NC, "null_partials", dict(partials=None)),
    (NC, "null_nparts", dict(nparts=None)),
    (NC, "null_dweights", dict(dweights=None)),
    (NC, "null_sinks", dict(sinks=None)),
    (NC, "n0", dict(n=0)),
    (NC, "n33", dict(partials=[P[0]] * 33, nparts=[1] * 33, dweights=[P[2]] * 33, sinks=[0] * 33, n=33)),
    (NC, "cols0", dict(cols=0)),
    (NC, "cols_mod", dict(cols=68)),
    (NC, "null_partial_1", dict(partials=[P[0], None])),
    (NC, "null_dweight_0", dict(dweights=[None, P[3]])),
    (NC, "nparts0", dict(nparts=[2, 0])),
    (NC, "sink1", dict(sinks=[0, 1])),                                       # an unknown sink
    (NC, "sink2", dict(sinks=[2, 0])),
    (NC, "sink_both_bits", dict(sinks=[0, DW_BF16 | DW_F32])),
    (RO, "null_x", dict(x=None)),
    (RO, "null_cos", dict(cos=None)),
    (RO, "null_sin", dict(sin=None)),
    (RO, "rows0", dict(rows=0)),
    (RO, "nheads0", dict(nheads=0)),
    (RO, "seq0", dict(seq_len=0)),
    (RO, "head_dim8", dict(head_dim=8)),
    (RO, "head_dim24", dict(head_dim=24)),
    (RO, "row_stride_mod", dict(row_stride=68)),
    (RO, "table_stride_mod", dict(table_stride=68)),
    (RO, "x_unaligned", dict(x=P[0] + 8)),
    (RO, "cos_unaligned", dict(cos=P[1] + 8)),
    (RO, "sin_unaligned", dict(sin=P[2] + 2)),
    (RO, "rows0+head_dim24", dict(rows=0, head_dim=24)),                     # (2) PT_EINVAL first
    (SF, "null_g", dict(g=None)),
    (SF, "null_u", dict(u=None)),
    (SF, "null_h", dict(h=None)),
    (SF, "rows0", dict(rows=0)),
    (SF, "cols0", dict(cols=0)),
    (SF, "cols_mod", dict(cols=68)),
    (SF, "g_stride_mod", dict(g_stride=68)),
    (SF, "u_stride_mod", dict(u_stride=132)),
    (SF, "h_stride_mod", dict(h_stride=66)),
    (SF, "g_unaligned", dict(g=P[0] + 8)),
    (SF, "u_unaligned", dict(u=P[1] + 8)),
    (SF, "h_unaligned", dict(h=P[2] + 8)),
    (SB, "null_dh", dict(dh=None)),
    (SB, "null_dg", dict(dg=None)),
    (SB, "null_du", dict(du=None)),
    (SB, "cols_mod", dict(cols=68)),
    (SB, "dh_stride_mod", dict(dh_stride=68)),
    (SB, "dg_stride_mod", dict(dg_stride=68)),
    (SB, "du_stride_mod", dict(du_stride=68)),
    (SB, "dh_unaligned", dict(dh=P[0] + 8)),
    (SB, "dg_unaligned", dict(dg=P[3] + 8)),
    (SB, "du_unaligned", dict(du=P[4] + 8)),
    (SB, "null_dh+cols_mod", dict(dh=None, cols=68)),                        # (2) PT_EINVAL first
    (RA, "null_x", dict(x=None)),
    (RA, "null_out", dict(out=None)),
    (RA, "n0", dict(n=0)),
    (RA, "n_mod", dict(n=68)),
    (RA, "r_unaligned", dict(r=P[1] + 8)),
    (RA, "out_unaligned", dict(out=P[2] + 8)),
    (CF, "null_logits", dict(logits=None)),
    (CF, "null_targets", dict(targets=None)),
    (CF, "null_row_loss", dict(row_loss=None)),
    (CF, "rows0", dict(rows=0)),
    (CF, "vocab0", dict(vocab=0)),
    (CF, "vocab_mod", dict(vocab=68)),
    (CF, "logits_stride_mod", dict(logits_stride=68)),
    (CF, "dlogits_stride_mod", dict(dlogits_stride=68)),
    (CF, "logits_unaligned", dict(logits=P[0] + 8)),
    (CF, "dlogits_unaligned", dict(dlogits=P[2] + 8)),
    (CL, "null_logits", dict(logits=None)),
    (CL, "null_row_lse", dict(row_lse=None)),
    (CL, "vocab_mod", dict(vocab=68)),
    (CL, "logits_stride_mod", dict(logits_stride=68)),
    (CL, "logits_unaligned", dict(logits=P[0] + 8)),
    (CL, "rows_2_31", dict(rows=BIG)),
    (CL, "vocab_2_31", dict(vocab=BIG, logits_stride=BIG)),
    (CL, "vocab_mod+rows_2_31", dict(vocab=68, rows=BIG)),                   # (2) PT_EALIGN first
    (CB, "null_row_lse", dict(row_lse=None)),
    (CB, "null_scale", dict(scale=None)),
    (CB, "null_dlogits", dict(dlogits=None)),
    (CB, "scale_stride2", dict(scale_stride=2)),
    (CB, "scale_stride_negative", dict(scale_stride=-1)),
    (CB, "vocab_mod", dict(vocab=68)),
    (CB, "dlogits_stride_mod", dict(dlogits_stride=68)),
    (CB, "dlogits_unaligned", dict(dlogits=P[2] + 8)),
    (CB, "rows_2_31", dict(rows=BIG)),
    (CB, "scale_stride2+vocab_mod", dict(scale_stride=2, vocab=68)),         # (2) PT_EINVAL first
    (CS, "null_scale", dict(scale=None)),
    (CS, "scale_stride2", dict(scale_stride=2)),
    (CS, "vocab_shard_mod", dict(vocab_shard=68)),
    (CS, "logits_stride_mod", dict(logits_stride=68)),
    (CS, "logits_unaligned", dict(logits=P[0] + 8)),
    (CS, "vocab_shard_2_31", dict(vocab_shard=BIG)),
    (CT, "null_stats", dict(stats=None)),
    (CT, "null_row_lse", dict(row_lse=None)),
    (CT, "nblk0", dict(nblk=0)),
    (CT, "nblk_not_dividing", dict(nblk=3)),                                 # vocab % nblk
    (CT, "stats_unaligned", dict(stats=P[6] + 8)),
    (VP, "null_part", dict(part=None)),
    (VP, "nblk0", dict(nblk=0)),
    (VP, "nblk_not_dividing", dict(nblk=3)),
    (VP, "stats_unaligned", dict(stats=P[6] + 8)),
    (VP, "part_unaligned", dict(part=P[7] + 8)),
    (VP, "rows_2_31", dict(rows=BIG)),
    (VC, "null_parts", dict(parts=None)),
    (VC, "tp0", dict(tp=0)),
    (VC, "vocab0", dict(vocab=0)),
    (VC, "parts_unaligned", dict(parts=P[7] + 8)),
    (CM, "null_row_loss", dict(row_loss=None)),
    (CM, "null_targets", dict(targets=None)),
    (CM, "null_inv_count", dict(inv_count=None)),
    (CM, "rows0", dict(rows=0)),
    (ES, "T_16385", dict(T=16385)),                                          # T > 16384
    (ES, "null_perm", dict(perm=None)),
    (ES, "vocab_hi_below_lo", dict(vocab_lo=8, vocab_hi=0)),
]

ADDED_REFUSALS = [
    (CF, "rows_2_31", dict(rows=BIG)),                                       # rows > INT32_MAX
    (CF, "vocab_2_31", dict(vocab=BIG, logits_stride=BIG, dlogits_stride=BIG)),
    (CF, "vocab_2_31_loss_only", dict(vocab=BIG, logits_stride=BIG, dlogits=None)),
]


def library(path=None):
    from picotron_amd import _C
    if path:
        return _C.load_library(path, strict=False)
    if not os.path.exists(_C.LIB_PATH):
        from picotron_amd import build
        build.build(verbose=False)
    return _C.load_library()


def call(lib, entry, over, keep):
    a = dict(DEFAULTS[entry])
    unknown = set(over) - set(a)
    assert not unknown, (entry, unknown)
    a.update(over)
    if entry == NC:   # the host reads these tables: real arrays
        from picotron_amd import _C
        for name, make in (("partials", _C.ptrarr), ("dweights", _C.ptrarr), ("nparts", _C.i32arr), ("sinks", _C.i32arr)):
            if a[name] is not None:
                arr = make([v or 0 for v in a[name]])
                keep.append(arr)
                a[name] = ctypes.cast(arr, ctypes.c_void_p)
    args = list(a.values())
    if entry != NP:
        args.append(None)   # the stream
    return getattr(lib, entry)(*args)


def refusal_codes(lib, rows):
    out, keep = {}, []
    for entry, case, over in rows:
        key = f"{entry}/{case}"
        assert key not in out, key
        out[key] = call(lib, entry, over, keep)
    return out


def test_rows_cover_every_row_entry_point():
    assert {e for e, _, _ in REFUSALS} == set(DEFAULTS)
    cases = {f"{e}/{c}" for e, c, _ in REFUSALS}
    # what the table was written to pin: the 8 grid, alignment, the width limit, scale_stride 2, both
    # PT_DW_ACC bits, an unknown sink, nblk not dividing the vocabulary, the sort's length limit
    assert {f"{NF}/cols_mod", f"{NF}/x_unaligned", f"{NF}/cols_16392", f"{NB}/cols_16392", f"{NS}/cols_16392",
            f"{CB}/scale_stride2", f"{CS}/scale_stride2", f"{NB}/both_acc_bits", f"{NS}/both_acc_bits", f"{NC}/sink1",
            f"{CT}/nblk_not_dividing", f"{VP}/nblk_not_dividing", f"{ES}/T_16385", f"{CF}/vocab_mod",
            f"{RO}/row_stride_mod", f"{SF}/g_stride_mod"} <= cases
    assert sum("+" in c for _, c, _ in REFUSALS) >= 7


def test_refusals_match_golden():
    want, got = json.load(open(GOLDEN))["refusals"], refusal_codes(library(), REFUSALS)
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    assert all(rc < 0 for rc in got.values())
    assert set(got.values()) == {-1, -2, -3}


def test_added_refusals_match_their_golden():
    want, got = json.load(open(ADDED_GOLDEN))["refusals"], refusal_codes(library(), ADDED_REFUSALS)
    assert got == want and all(rc == -3 for rc in got.values())
    assert not set(got) & set(json.load(open(GOLDEN))["refusals"])


def _write(path, codes):
    accepted = {k: rc for k, rc in codes.items() if rc >= 0}
    assert not accepted, f"rows the library accepts have no place in the table: {accepted}"
    with open(path, "w") as f:
        f.write('{\n "refusals": {\n' + ",\n".join(f"  {json.dumps(k)}: {rc}" for k, rc in codes.items()) + "\n }\n}\n")
    print(f"wrote {path}: {len(codes)} refusals")


if __name__ == "__main__":
    # `library` = the build to record: the golden from the commit before, the added rows from this one
    which, path = (sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else None) if len(sys.argv) > 1 else ("golden", None)
    if which == "added":
        _write(ADDED_GOLDEN, refusal_codes(library(path), ADDED_REFUSALS))
    else:
        _write(GOLDEN, refusal_codes(library(path), REFUSALS))
