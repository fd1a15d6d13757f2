"""The native host code of csrc/attention.hip, pinned without a GPU.

The real library loads on a machine with no device, and its argument checks return before any HIP
call.  Two tables are replayed against tests/golden/attn_host.json and compared exactly:

  * pt_attn_split_plan: the return value and ws_bytes over a grid of shapes (PLAN_GRID) and for the
    inputs it refuses (PLAN_REFUSED);
  * refusals: for each of the seven pt_attn_* launch entry points, calls that must be refused, with
    the return code (REFUSALS).  Pointers are fake, non-null, 16-byte-aligned integers: they are
    never dereferenced because the call refuses (the stride arrays are real).  Every row holds at
    least one violation; the rows with two pin which check comes first.

`python tests/test_attn_host_cpu.py` writes the golden file.  It was generated once, from the
commit before the host code was first refactored, and is never regenerated to make a refactor
pass: a refactor of the host code keeps every code in it.  The generator asserts that every
recorded refusal is negative -- a call the library accepts has no place in the table (it would
launch a kernel on fake pointers).

The comment beside each row names the `return PT_E...` statement of that commit's host code it
reaches, by function and condition.  One statement there cannot be reached through the ABI and has
no row: attn_bwd_impl's `delta_w && parts != 3` (only pt_attn_bwd_part passes parts, and it passes
no delta_w)."""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_host.json")

PLAN_GRID = {
    "B": (1, 2, 4),
    "H_HKV": ((4, 4), (4, 2), (8, 2), (32, 32)),
    "Sq_Sk": ((128, 128), (256, 256), (1024, 1024), (512, 1024), (1024, 512), (192, 192)),
    "D": (64, 128),
    "causal": (0, 1),
    "backward": (0, 1),
}
# (B, H, HKV, Sq, Sk, D, causal, backward, ws_bytes given?)
PLAN_REFUSED = [
    (1, 4, 4, 256, 256, 64, 1, 0, False),   # pt_attn_split_plan: !ws_bytes
    (1, 4, 3, 256, 256, 64, 1, 0, True),    # pt_attn_split_plan: H % HKV
    (0, 4, 4, 256, 256, 64, 1, 0, True),    # pt_attn_split_plan: B <= 0
    (0, 4, 3, 256, 256, 64, 1, 1, False),   # pt_attn_split_plan: all three at once
]

PARAMS = {
    "pt_attn_fwd": "q q_str k k_str v v_str o o_str lse B H HKV Sq Sk D scale causal merge lse_ld stream",
    "pt_attn_bwd_delta": "dout do_str o o_str delta B H Sq D lse_ld stream",
    "pt_attn_bwd": "q q_str k k_str v v_str dout do_str lse delta dq dq_str dk dk_str dv dv_str B H HKV Sq Sk D "
                   "scale causal grad_f32 rope_cos rope_sin rope_stride lse_ld stream",
    "pt_attn_bwd_part": "q q_str k k_str v v_str dout do_str lse delta dq dq_str dk dk_str dv dv_str B H HKV Sq Sk "
                        "D scale causal grad_f32 lse_ld parts stream",
    "pt_attn_bwd_fused_delta": "q q_str k k_str v v_str o o_str dout do_str lse delta_out dq dq_str dk dk_str dv "
                               "dv_str B H HKV Sq Sk D scale causal rope_cos rope_sin rope_stride lse_ld stream",
    "pt_attn_fwd_split": "q q_str k k_str v v_str o o_str lse B H HKV Sq Sk D scale causal ws ws_bytes stream",
    "pt_attn_bwd_split": "q q_str k k_str v v_str o o_str dout do_str lse delta_out dq dq_str dk dk_str dv dv_str "
                         "B H HKV Sq Sk D scale causal rope_cos rope_sin rope_stride ws ws_bytes stream",
}
POINTERS = "q k v o lse dout delta delta_out dq dk dv ws".split()   # fake: 1 MiB apart, 16-byte aligned
FAKE = {n: 0x10000000 + i * 0x100000 for i, n in enumerate(POINTERS)}
ROPE = {"rope_cos": 0x20000000, "rope_sin": 0x20100000, "rope_stride": 64}
BAD_ROPE = {"rope_cos": 0x20000000, "rope_sin": None}
BIG = 1 << 40   # workspace bytes no plan exceeds


def default_args(entry):
    """A call the entry point accepts (never made): one (batch, 4 heads) causal d64 problem, which
    is also a shape the split forms take."""
    a = dict(FAKE)
    a.update(B=1, H=4, HKV=4, Sq=256, Sk=256, D=64, scale=0.125, causal=1, merge=0, grad_f32=0, lse_ld=0, parts=3,
             rope_cos=None, rope_sin=None, rope_stride=0, ws_bytes=BIG, stream=None)
    for n in ("q", "k", "v", "o", "do", "dq", "dk", "dv"):
        a[n + "_str"] = [256 * 4 * 64, 4 * 64, 64]
    return a


def S(a, b, c):   # a stride triple
    return [a, b, c]


E = "pt_attn_"
# (entry point, case name, overrides of default_args)   # the statement reached
REFUSALS = [
    (E + "fwd", "null_q", dict(q=None)),                                   # pt_attn_fwd: null pointer
    (E + "fwd", "null_lse", dict(lse=None)),                               # pt_attn_fwd: null pointer
    (E + "fwd", "null_o+d96", dict(o=None, D=96)),                         # pt_attn_fwd: null pointer (2)
    (E + "fwd", "lse_ld_short", dict(lse_ld=128)),                         # pt_attn_fwd: lse_ld < Sq
    (E + "fwd", "lse_ld_short+causal_sq_ne_sk", dict(lse_ld=128, Sk=512)),  # pt_attn_fwd: lse_ld < Sq (2)
    (E + "fwd", "d96", dict(D=96)),                                        # check_common: D
    (E + "fwd", "d96+h_mod_hkv", dict(D=96, HKV=3)),                       # check_common: D (2)
    (E + "fwd", "h_mod_hkv", dict(HKV=3)),                                 # check_common: B/H/HKV
    (E + "fwd", "b0", dict(B=0)),                                          # check_common: B/H/HKV
    (E + "fwd", "hkv0", dict(HKV=0)),                                      # check_common: B/H/HKV
    (E + "fwd", "h_mod_hkv+sq192", dict(HKV=3, Sq=192, Sk=192)),           # check_common: B/H/HKV (2)
    (E + "fwd", "sq192", dict(Sq=192, Sk=192)),                            # check_common: Sq % 128 / Sk % 64
    (E + "fwd", "sk96", dict(Sk=96, causal=0)),                            # check_common: Sq % 128 / Sk % 64
    (E + "fwd", "sq192+causal_sq_ne_sk", dict(Sq=192, Sk=256)),            # check_common: Sq % 128 (2)
    (E + "fwd", "causal_sq_ne_sk", dict(Sk=512)),                          # check_common: causal Sq != Sk

    (E + "bwd_delta", "null_dout", dict(dout=None)),                       # pt_attn_bwd_delta: null / D % 8
    (E + "bwd_delta", "null_delta", dict(delta=None)),                     # pt_attn_bwd_delta: null / D % 8
    (E + "bwd_delta", "d60", dict(D=60)),                                  # pt_attn_bwd_delta: null / D % 8
    (E + "bwd_delta", "d60+lse_ld_short", dict(D=60, lse_ld=8)),           # pt_attn_bwd_delta: null / D % 8 (2)
    (E + "bwd_delta", "lse_ld_short", dict(lse_ld=255)),                   # pt_attn_bwd_delta: lse_ld < Sq
    (E + "bwd_delta", "lse_ld_short+d96", dict(lse_ld=255, D=96)),         # pt_attn_bwd_delta: lse_ld < Sq (2)
    (E + "bwd_delta", "d96", dict(D=96)),                                  # pt_attn_bwd_delta: D not 64 / 128
    (E + "bwd_delta", "d256", dict(D=256)),                                # pt_attn_bwd_delta: D not 64 / 128

    (E + "bwd", "null_delta", dict(delta=None)),                           # pt_attn_bwd: !delta
    (E + "bwd", "null_delta+d96", dict(delta=None, D=96)),                 # pt_attn_bwd: !delta (2)
    (E + "bwd", "null_q", dict(q=None)),                                   # attn_bwd_impl: null / parts range
    (E + "bwd", "null_dout", dict(dout=None)),                             # attn_bwd_impl: null / parts range
    (E + "bwd", "null_lse+null_dq", dict(lse=None, dq=None)),              # attn_bwd_impl: null / parts range (2)
    (E + "bwd", "null_dq", dict(dq=None)),                                 # attn_bwd_impl: a part's pointers
    (E + "bwd", "null_dk_str", dict(dk_str=None)),                         # attn_bwd_impl: a part's pointers
    (E + "bwd", "null_dv+lse_ld_short", dict(dv=None, lse_ld=1)),          # attn_bwd_impl: a part's pointers (2)
    (E + "bwd", "lse_ld_short", dict(lse_ld=128)),                         # attn_bwd_impl: lse_ld < Sq
    (E + "bwd", "lse_ld_short+causal_sq_ne_sk", dict(lse_ld=128, Sk=512)),  # attn_bwd_impl: lse_ld < Sq (2)
    (E + "bwd", "lse_ld_short+rope_no_sin", dict(lse_ld=128, **BAD_ROPE)),  # attn_bwd_impl: lse_ld < Sq (2)
    (E + "bwd", "rope_no_sin", dict(BAD_ROPE)),                            # attn_bwd_impl: rope
    (E + "bwd", "rope+grad_f32", dict(ROPE, grad_f32=1)),                  # attn_bwd_impl: rope
    (E + "bwd", "rope+grad_f32+d96", dict(ROPE, grad_f32=1, D=96)),        # attn_bwd_impl: rope (2)
    (E + "bwd", "rope+sq_ne_sk", dict(ROPE, causal=0, Sk=512)),            # attn_bwd_impl: rope
    (E + "bwd", "rope_stride6", dict(ROPE, rope_stride=6)),                # attn_bwd_impl: rope
    (E + "bwd", "rope_cos_unaligned", dict(ROPE, rope_cos=0x20000008)),    # attn_bwd_impl: rope
    (E + "bwd", "rope_sin_unaligned", dict(ROPE, rope_sin=0x20100002)),    # attn_bwd_impl: rope
    (E + "bwd", "d96", dict(D=96)),                                        # check_common: D
    (E + "bwd", "d96+h_mod_hkv", dict(D=96, HKV=3)),                       # check_common: D (2)
    (E + "bwd", "h_mod_hkv", dict(HKV=3)),                                 # check_common: B/H/HKV
    (E + "bwd", "sq192", dict(Sq=192, Sk=192)),                            # check_common: Sq % 128 / Sk % 64
    (E + "bwd", "causal_sq_ne_sk", dict(Sk=512)),                          # check_common: causal Sq != Sk
    (E + "bwd", "sk192", dict(Sk=192, causal=0)),                          # attn_bwd_impl: Sk % 128
    (E + "bwd", "rope+sk192", dict(ROPE, Sk=192, causal=0)),      # attn_bwd_impl: rope (2)

    (E + "bwd_part", "null_delta", dict(delta=None)),                      # pt_attn_bwd_part: !delta
    (E + "bwd_part", "null_delta+parts0", dict(delta=None, parts=0)),      # pt_attn_bwd_part: !delta (2)
    (E + "bwd_part", "parts0", dict(parts=0)),                             # attn_bwd_impl: null / parts range
    (E + "bwd_part", "parts4", dict(parts=4)),                             # attn_bwd_impl: null / parts range
    (E + "bwd_part", "parts1_null_dq", dict(parts=1, dq=None)),            # attn_bwd_impl: a part's pointers
    (E + "bwd_part", "parts1_null_dq+d96", dict(parts=1, dq=None, D=96)),  # attn_bwd_impl: a part's pointers (2)
    (E + "bwd_part", "parts1_null_dq_str", dict(parts=1, dq_str=None)),    # attn_bwd_impl: a part's pointers
    (E + "bwd_part", "parts2_null_dk", dict(parts=2, dk=None)),            # attn_bwd_impl: a part's pointers
    (E + "bwd_part", "parts2_null_dv_str", dict(parts=2, dv_str=None)),    # attn_bwd_impl: a part's pointers
    (E + "bwd_part", "parts3_null_dv", dict(dv=None)),                     # attn_bwd_impl: a part's pointers
    (E + "bwd_part", "lse_ld_short", dict(lse_ld=255)),                    # attn_bwd_impl: lse_ld < Sq
    # the other part's pointers are not looked at: these reach the shape checks
    (E + "bwd_part", "parts1_no_dkdv_d96", dict(parts=1, dk=None, dv=None, dk_str=None, dv_str=None, D=96)),  # check_common: D
    (E + "bwd_part", "parts2_no_dq_h_mod_hkv", dict(parts=2, dq=None, dq_str=None, HKV=3)),  # check_common: B/H/HKV
    (E + "bwd_part", "parts2_sk192", dict(parts=2, Sk=192, causal=0)),     # attn_bwd_impl: Sk % 128
    (E + "bwd_part", "parts1_sk192", dict(parts=1, Sk=192, causal=0)),     # attn_bwd_impl: Sk % 128
    (E + "bwd_part", "causal_sq_ne_sk", dict(Sq=512)),                     # check_common: causal Sq != Sk

    (E + "bwd_fused_delta", "null_o", dict(o=None)),                       # pt_attn_bwd_fused_delta: null
    (E + "bwd_fused_delta", "null_delta_out", dict(delta_out=None)),       # pt_attn_bwd_fused_delta: null
    (E + "bwd_fused_delta", "null_o_str", dict(o_str=None)),               # pt_attn_bwd_fused_delta: null
    (E + "bwd_fused_delta", "o_unaligned+null_delta_out", dict(o=FAKE["o"] + 8, delta_out=None)),  # pt_attn_bwd_fused_delta: null (2)
    (E + "bwd_fused_delta", "o_unaligned", dict(o=FAKE["o"] + 8)),         # pt_attn_bwd_fused_delta: o alignment
    (E + "bwd_fused_delta", "o_str_b", dict(o_str=S(65540, 256, 64))),     # pt_attn_bwd_fused_delta: o alignment
    (E + "bwd_fused_delta", "o_str_s", dict(o_str=S(65536, 260, 64))),     # pt_attn_bwd_fused_delta: o alignment
    (E + "bwd_fused_delta", "o_str_h", dict(o_str=S(65536, 256, 68))),     # pt_attn_bwd_fused_delta: o alignment
    (E + "bwd_fused_delta", "o_unaligned+null_q", dict(o=FAKE["o"] + 2, q=None)),  # pt_attn_bwd_fused_delta: o alignment (2)
    (E + "bwd_fused_delta", "null_q", dict(q=None)),                       # attn_bwd_impl: null / parts range
    (E + "bwd_fused_delta", "null_dq", dict(dq=None)),                     # attn_bwd_impl: a part's pointers
    (E + "bwd_fused_delta", "lse_ld_short", dict(lse_ld=128)),             # attn_bwd_impl: lse_ld < Sq
    (E + "bwd_fused_delta", "rope_no_sin", dict(BAD_ROPE)),                # attn_bwd_impl: rope
    (E + "bwd_fused_delta", "rope_stride2+d96", dict(ROPE, rope_stride=2, D=96)),  # attn_bwd_impl: rope (2)
    (E + "bwd_fused_delta", "d96", dict(D=96)),                            # check_common: D
    (E + "bwd_fused_delta", "sq64", dict(Sq=64, Sk=64)),                   # check_common: Sq % 128 / Sk % 64
    (E + "bwd_fused_delta", "sk192", dict(Sk=192, causal=0)),              # attn_bwd_impl: Sk % 128

    (E + "fwd_split", "null_ws", dict(ws=None)),                           # pt_attn_fwd_split: null
    (E + "fwd_split", "null_q+d128", dict(q=None, D=128)),                 # pt_attn_fwd_split: null (2)
    (E + "fwd_split", "d128", dict(D=128)),                                # pt_attn_fwd_split: plan != 1
    (E + "fwd_split", "many_heads", dict(B=4, H=32, HKV=32, Sq=1024, Sk=1024)),  # pt_attn_fwd_split: plan != 1
    (E + "fwd_split", "h_mod_hkv", dict(HKV=3)),                           # pt_attn_fwd_split: plan != 1
    (E + "fwd_split", "sq192", dict(Sq=192, Sk=192)),                      # pt_attn_fwd_split: plan != 1
    (E + "fwd_split", "d128+ws_small", dict(D=128, ws_bytes=0)),           # pt_attn_fwd_split: plan != 1 (2)
    (E + "fwd_split", "ws_small", dict(ws_bytes=1024)),                    # pt_attn_fwd_split: ws
    (E + "fwd_split", "ws_unaligned", dict(ws=FAKE["ws"] + 8)),            # pt_attn_fwd_split: ws
    (E + "fwd_split", "ws_unaligned+ws_small", dict(ws=FAKE["ws"] + 4, ws_bytes=0)),  # pt_attn_fwd_split: ws (2)
    (E + "fwd_split", "ws_small+o_unaligned", dict(ws_bytes=0, o=FAKE["o"] + 8)),  # pt_attn_fwd_split: ws (2)
    (E + "fwd_split", "o_unaligned", dict(o=FAKE["o"] + 8)),               # pt_attn_fwd_split: o alignment
    (E + "fwd_split", "o_str_h", dict(o_str=S(65536, 256, 4))),            # pt_attn_fwd_split: o alignment
    (E + "fwd_split", "o_str_b", dict(o_str=S(65537, 256, 64))),           # pt_attn_fwd_split: o alignment

    (E + "bwd_split", "null_delta_out", dict(delta_out=None)),             # pt_attn_bwd_split: null
    (E + "bwd_split", "null_ws", dict(ws=None)),                           # pt_attn_bwd_split: null
    (E + "bwd_split", "null_dk+d128", dict(dk=None, D=128)),               # pt_attn_bwd_split: null (2)
    (E + "bwd_split", "d128", dict(D=128)),                                # pt_attn_bwd_split: plan != 1
    (E + "bwd_split", "sq_ne_sk_causal", dict(Sk=512)),                    # pt_attn_bwd_split: plan != 1
    (E + "bwd_split", "ws_small", dict(ws_bytes=4096)),                    # pt_attn_bwd_split: ws
    (E + "bwd_split", "ws_unaligned", dict(ws=FAKE["ws"] + 8)),            # pt_attn_bwd_split: ws
    (E + "bwd_split", "ws_unaligned+ws_small", dict(ws=FAKE["ws"] + 8, ws_bytes=0)),  # pt_attn_bwd_split: ws (2)
    (E + "bwd_split", "ws_small+rope_no_sin", dict(BAD_ROPE, ws_bytes=0)),  # pt_attn_bwd_split: ws (2)
    (E + "bwd_split", "o_unaligned", dict(o=FAKE["o"] + 8)),               # pt_attn_bwd_split: o alignment
    (E + "bwd_split", "o_str_s", dict(o_str=S(65536, 257, 64))),           # pt_attn_bwd_split: o alignment
    (E + "bwd_split", "o_unaligned+dq_str", dict(o=FAKE["o"] + 8, dq_str=S(65536, 256, 65))),  # pt_attn_bwd_split: o alignment (2)
    (E + "bwd_split", "dq_str_h", dict(dq_str=S(65536, 256, 65))),         # pt_attn_bwd_split: dq/dk/dv strides
    (E + "bwd_split", "dk_str_b", dict(dk_str=S(65532, 256, 64))),         # pt_attn_bwd_split: dq/dk/dv strides
    (E + "bwd_split", "dv_str_s", dict(dv_str=S(65536, 258, 64))),         # pt_attn_bwd_split: dq/dk/dv strides
    (E + "bwd_split", "dv_str_s+rope_no_sin", dict(BAD_ROPE, dv_str=S(65536, 258, 64))),  # pt_attn_bwd_split: dq/dk/dv strides (2)
    (E + "bwd_split", "dq_unaligned", dict(dq=FAKE["dq"] + 8)),            # pt_attn_bwd_split: dq/dk/dv pointers
    (E + "bwd_split", "dk_unaligned", dict(dk=FAKE["dk"] + 4)),            # pt_attn_bwd_split: dq/dk/dv pointers
    (E + "bwd_split", "dv_unaligned", dict(dv=FAKE["dv"] + 2)),            # pt_attn_bwd_split: dq/dk/dv pointers
    (E + "bwd_split", "dv_unaligned+rope_stride4", dict(ROPE, rope_stride=4, dv=FAKE["dv"] + 2)),  # pt_attn_bwd_split: dq/dk/dv pointers (2)
    (E + "bwd_split", "rope_no_sin", dict(BAD_ROPE)),                      # pt_attn_bwd_split: rope
    (E + "bwd_split", "rope_stride4", dict(ROPE, rope_stride=4)),          # pt_attn_bwd_split: rope
    (E + "bwd_split", "rope_cos_unaligned", dict(ROPE, rope_cos=0x20000008)),  # pt_attn_bwd_split: rope
    (E + "bwd_split", "rope_sin_unaligned", dict(ROPE, rope_sin=0x20100008)),  # pt_attn_bwd_split: rope
]


def library():
    from picotron_amd import _C
    if not os.path.exists(_C.LIB_PATH):
        from picotron_amd import build
        build.build(verbose=False)
    return _C.load_library()


class kv_chunk_default:
    """The plan depends on the attn_kv_chunk variant: both tables are taken at its default, 4."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.saved = self.lib.pt_get_variant(b"attn_kv_chunk")
        assert self.lib.pt_set_variant(b"attn_kv_chunk", 4) == 0

    def __exit__(self, *exc):
        self.lib.pt_set_variant(b"attn_kv_chunk", self.saved)


def plan_rows(lib):
    g = PLAN_GRID
    rows = []
    for B, (H, HKV), (Sq, Sk), D, causal, backward in itertools.product(
            g["B"], g["H_HKV"], g["Sq_Sk"], g["D"], g["causal"], g["backward"]):
        ws = ctypes.c_int64(-7)
        rc = lib.pt_attn_split_plan(B, H, HKV, Sq, Sk, D, causal, backward, ctypes.byref(ws))
        rows.append([B, H, HKV, Sq, Sk, D, causal, backward, rc, ws.value])
    return rows


def plan_refused(lib):
    out = []
    for *shape, given in PLAN_REFUSED:
        ws = ctypes.c_int64(-7)
        rc = lib.pt_attn_split_plan(*shape, ctypes.byref(ws) if given else None)
        out.append([*shape, int(given), rc, ws.value])
    return out


def refusal_codes(lib):
    from picotron_amd import _C
    out, keep = {}, []
    for entry, case, over in REFUSALS:
        a = default_args(entry)
        unknown = set(over) - set(a)
        assert not unknown, (entry, case, unknown)
        a.update(over)
        args = []
        for name in PARAMS[entry].split():
            val = a[name]
            if name.endswith("_str") and val is not None:
                val = _C.i64arr(val)
                keep.append(val)
            args.append(val)
        key = f"{entry}/{case}"
        assert key not in out, key
        out[key] = getattr(lib, entry)(*args)
    return out


def tables():
    lib = library()
    with kv_chunk_default(lib):
        return {"plan": plan_rows(lib), "plan_refused": plan_refused(lib), "refusals": refusal_codes(lib)}


def test_rows_cover_every_entry_point_and_pin_check_order():
    assert {e for e, _, _ in REFUSALS} == set(PARAMS)
    assert sum(case.count("+") > 0 for _, case, _ in REFUSALS) >= 6


def test_split_plan_matches_golden():
    want, got = json.load(open(GOLDEN)), tables()
    assert len(got["plan"]) == 3 * 4 * 6 * 2 * 2 * 2
    assert got["plan"] == want["plan"]
    assert got["plan_refused"] == want["plan_refused"]
    assert any(r[8] == 1 for r in got["plan"]) and any(r[8] == 0 for r in got["plan"])


def test_refusals_match_golden():
    want, got = json.load(open(GOLDEN))["refusals"], tables()["refusals"]
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    assert all(rc < 0 for rc in got.values())


if __name__ == "__main__":
    t = tables()
    accepted = {k: rc for k, rc in t["refusals"].items() if rc >= 0}
    assert not accepted, f"rows the library accepts have no place in the table: {accepted}"
    assert all(r[-2] < 0 for r in t["plan_refused"]), t["plan_refused"]
    with open(GOLDEN, "w") as f:
        f.write("{\n")
        for name in ("plan", "plan_refused"):
            f.write(f' "{name}": [\n' + ",\n".join("  " + json.dumps(r) for r in t[name]) + "\n ],\n")
        f.write(' "refusals": {\n' + ",\n".join(f"  {json.dumps(k)}: {rc}" for k, rc in t["refusals"].items()))
        f.write("\n }\n}\n")
    print(f"wrote {GOLDEN}: {len(t['plan'])} plan rows, {len(t['plan_refused'])} refused plans, "
          f"{len(t['refusals'])} refusals")
