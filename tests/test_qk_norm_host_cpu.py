"""The native host code of the QK-norm entry points (csrc/qk_norm.hip), pinned without a GPU.

As tests/test_row_host_cpu.py: the real library loads on a machine with no device and its argument
checks return before any HIP call.  Every row of REFUSALS is a call that must be refused, on fake,
non-null, 16-byte-aligned pointers (never dereferenced), with its return code replayed against
tests/golden/qk_norm_host.json and compared exactly.  Rows marked (2) hold two violations and pin
the order of the checks the header documents: head_dim; null pointers, counts, mode, the cos / sin
pair; sizes past 32 bits; rows narrower than their heads; alignment.

`python tests/test_qk_norm_host_cpu.py` writes the golden file.  It was generated once, from the
library of the commit that added the entries, and is never regenerated to make a change pass.  The
generator asserts that every recorded code is negative: a call the library accepts has no place in
the table (it would launch a kernel on fake pointers).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "qk_norm_host.json")

P = [0x10000000 + i * 0x100000 for i in range(10)]   # fake device pointers
BIG = 2 ** 31                                         # INT32_MAX + 1, a multiple of 8
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3

FWD, PARTS, BWD = "pt_qk_norm_rope_fwd", "pt_qk_norm_bwd_partials", "pt_qk_norm_bwd"
# entry -> its arguments in ABI order (the stream, always NULL, is appended by call())
DEFAULTS = {
    FWD: dict(x=P[0], x_stride=384, y=P[1], y_stride=384, wq=P[2], wk=P[3], rstd=P[4], rows=4, nq=4, nk=2, d=64,
              eps=1e-5, mode=0, cos=P[5], sin=P[6], seq_len=4, table_stride=64),
    PARTS: dict(rows=4, nq=4, nk=2, d=64),
    BWD: dict(dy=P[0], dy_stride=384, x=P[1], x_stride=384, wq=P[2], wk=P[3], rstd=P[4], dx=P[7], dx_stride=384,
              dwq=P[8], dwk=P[9], rows=4, nq=4, nk=2, d=64, mode=0),
}
NOROPE = dict(cos=None, sin=None)

# (entry point, case name, overrides)                                        # the check that answers
REFUSALS = [
    (FWD, "head_dim32", dict(d=32)),                                           # head_dim
    (FWD, "head_dim96", dict(d=96)),
    (FWD, "head_dim256", dict(d=256)),
    (FWD, "head_dim0", dict(d=0)),
    (FWD, "head_dim60+null_x", dict(d=60, x=None)),                            # (2) PT_EUNSUPPORTED first
    (FWD, "head_dim60+rows0", dict(d=60, rows=0)),                             # (2) PT_EUNSUPPORTED first
    (FWD, "null_x", dict(x=None)),                                             # null / counts / mode / pair
    (FWD, "null_y", dict(y=None)),
    (FWD, "null_wq", dict(wq=None)),
    (FWD, "null_wk", dict(wk=None)),
    (FWD, "null_rstd", dict(rstd=None)),
    (FWD, "rows0", dict(rows=0)),
    (FWD, "rows_negative", dict(rows=-4)),
    (FWD, "nq0", dict(nq=0)),
    (FWD, "nk0", dict(nk=0)),
    (FWD, "mode2", dict(mode=2)),
    (FWD, "mode_negative", dict(mode=-1)),
    (FWD, "cos_without_sin", dict(sin=None)),
    (FWD, "sin_without_cos", dict(cos=None)),
    (FWD, "seq0", dict(seq_len=0)),
    (FWD, "table_stride0", dict(table_stride=0)),
    (FWD, "null_x+x_stride_mod", dict(x=None, x_stride=388)),                  # (2) PT_EINVAL first
    (FWD, "cos_without_sin+y_unaligned", dict(sin=None, y=P[1] + 8)),          # (2) PT_EINVAL first
    (FWD, "mode2+rows_2_31", dict(mode=2, rows=BIG)),                          # (2) PT_EINVAL first
    (FWD, "rows_2_31", dict(rows=BIG)),                                        # past 32 bits
    (FWD, "nq_2_31", dict(nq=BIG)),
    (FWD, "nk_2_25", dict(nk=2 ** 25)),
    (FWD, "x_stride_2_31", dict(x_stride=BIG)),
    (FWD, "y_stride_2_31", dict(y_stride=BIG)),
    (FWD, "seq_2_31", dict(seq_len=BIG)),
    (FWD, "table_stride_2_31", dict(table_stride=BIG)),
    (FWD, "rows_2_31+x_unaligned", dict(rows=BIG, x=P[0] + 8)),                # (2) PT_EUNSUPPORTED first
    (FWD, "x_stride_2_31+y_stride_short", dict(x_stride=BIG, y_stride=320)),   # (2) PT_EUNSUPPORTED first
    (FWD, "x_stride_short", dict(x_stride=320)),                               # rows narrower than q|k
    (FWD, "y_stride_short", dict(y_stride=376)),
    (FWD, "table_stride_short", dict(table_stride=24)),
    (FWD, "x_stride_short+wq_unaligned", dict(x_stride=320, wq=P[2] + 2)),     # (2) PT_EINVAL first
    (FWD, "x_stride_mod", dict(x_stride=388)),                                 # alignment
    (FWD, "y_stride_mod", dict(y_stride=388)),
    (FWD, "table_stride_mod", dict(table_stride=68)),
    (FWD, "x_unaligned", dict(x=P[0] + 8)),
    (FWD, "y_unaligned", dict(y=P[1] + 8)),
    (FWD, "wq_unaligned", dict(wq=P[2] + 2)),
    (FWD, "wk_unaligned", dict(wk=P[3] + 4)),
    (FWD, "cos_unaligned", dict(cos=P[5] + 8)),
    (FWD, "sin_unaligned", dict(sin=P[6] + 8)),
    (FWD, "norm_only_x_unaligned", dict(NOROPE, x=P[0] + 8)),
    (FWD, "norm_only_y_stride_mod", dict(NOROPE, y_stride=388)),
    (FWD, "norm_only_head_dim60", dict(NOROPE, d=60)),
    (PARTS, "head_dim60", dict(d=60)),
    (PARTS, "rows0", dict(rows=0)),
    (PARTS, "nq0", dict(nq=0)),
    (PARTS, "nk_negative", dict(nk=-1)),
    (PARTS, "rows_2_31", dict(rows=BIG)),
    (PARTS, "nq_2_31", dict(nq=BIG)),
    (PARTS, "head_dim60+rows0", dict(d=60, rows=0)),                           # (2) PT_EUNSUPPORTED first
    (PARTS, "rows0+nq_2_31", dict(rows=0, nq=BIG)),                            # (2) PT_EINVAL first
    (BWD, "head_dim32", dict(d=32)),
    (BWD, "head_dim60+null_dy", dict(d=60, dy=None)),                          # (2) PT_EUNSUPPORTED first
    (BWD, "null_dy", dict(dy=None)),
    (BWD, "null_x", dict(x=None)),
    (BWD, "null_wq", dict(wq=None)),
    (BWD, "null_wk", dict(wk=None)),
    (BWD, "null_rstd", dict(rstd=None)),
    (BWD, "null_dx", dict(dx=None)),
    (BWD, "rows0", dict(rows=0)),
    (BWD, "nq0", dict(nq=0)),
    (BWD, "nk0", dict(nk=0)),
    (BWD, "mode2", dict(mode=2)),
    (BWD, "mode_with_sink_bit", dict(mode=4)),                                 # no sink bits here: partials only
    (BWD, "null_dx+dx_stride_mod", dict(dx=None, dx_stride=388)),              # (2) PT_EINVAL first
    (BWD, "rows_2_31", dict(rows=BIG)),
    (BWD, "dy_stride_2_31", dict(dy_stride=BIG)),
    (BWD, "x_stride_2_31", dict(x_stride=BIG)),
    (BWD, "dx_stride_2_31", dict(dx_stride=BIG)),
    (BWD, "rows_2_31+dy_unaligned", dict(rows=BIG, dy=P[0] + 8)),              # (2) PT_EUNSUPPORTED first
    (BWD, "dy_stride_short", dict(dy_stride=320)),
    (BWD, "x_stride_short", dict(x_stride=376)),
    (BWD, "dx_stride_short", dict(dx_stride=8)),
    (BWD, "dx_stride_short+x_unaligned", dict(dx_stride=8, x=P[1] + 8)),       # (2) PT_EINVAL first
    (BWD, "dy_stride_mod", dict(dy_stride=388)),
    (BWD, "x_stride_mod", dict(x_stride=388)),
    (BWD, "dx_stride_mod", dict(dx_stride=388)),
    (BWD, "dy_unaligned", dict(dy=P[0] + 8)),
    (BWD, "x_unaligned", dict(x=P[1] + 8)),
    (BWD, "dx_unaligned", dict(dx=P[7] + 8)),
    (BWD, "wq_unaligned", dict(wq=P[2] + 8)),
    (BWD, "wk_unaligned", dict(wk=P[3] + 8)),
    (BWD, "null_partials_dy_unaligned", dict(dwq=None, dwk=None, dy=P[0] + 8)),
]

# the codes the issue fixes, whatever the golden file says
REQUIRED = {
    f"{FWD}/head_dim96": EUNSUPPORTED, f"{BWD}/head_dim32": EUNSUPPORTED, f"{PARTS}/head_dim60": EUNSUPPORTED,
    f"{FWD}/null_x": EINVAL, f"{FWD}/rows0": EINVAL, f"{FWD}/cos_without_sin": EINVAL, f"{FWD}/sin_without_cos": EINVAL,
    f"{BWD}/null_dx": EINVAL, f"{BWD}/nk0": EINVAL,
    f"{FWD}/x_stride_mod": EALIGN, f"{FWD}/y_unaligned": EALIGN, f"{BWD}/dx_stride_mod": EALIGN,
    f"{BWD}/wk_unaligned": EALIGN,
}


def library():
    from picotron_amd import _C
    if not os.path.exists(_C.LIB_PATH):
        from picotron_amd import build
        build.build(verbose=False)
    return _C.load_library()


def call(lib, entry, over):
    a = dict(DEFAULTS[entry])
    unknown = set(over) - set(a)
    assert not unknown, (entry, unknown)
    a.update(over)
    args = list(a.values())
    if entry != PARTS:
        args.append(None)   # the stream
    return getattr(lib, entry)(*args)


def refusal_codes(lib):
    out = {}
    for entry, case, over in REFUSALS:
        key = f"{entry}/{case}"
        assert key not in out, key
        out[key] = call(lib, entry, over)
    return out


def test_library_exports_the_entries():
    lib = library()
    from picotron_amd import _C
    for name in (FWD, PARTS, BWD):
        assert name in _C.SIGNATURES
        assert getattr(lib, name).argtypes == _C.SIGNATURES[name][1]


def test_rows_cover_every_check():
    assert {e for e, _, _ in REFUSALS} == set(DEFAULTS)
    assert sum("+" in c for _, c, _ in REFUSALS) >= 12   # rows with two violations: the order of the checks
    assert set(REQUIRED) <= {f"{e}/{c}" for e, c, _ in REFUSALS}


def test_refusals_match_golden():
    want, got = json.load(open(GOLDEN))["refusals"], refusal_codes(library())
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    assert all(rc < 0 for rc in got.values())
    assert set(got.values()) == {EINVAL, EALIGN, EUNSUPPORTED}
    assert not {k: (got[k], rc) for k, rc in REQUIRED.items() if got[k] != rc}


def test_bwd_partials_positive_for_valid_shapes():
    lib = library()
    for rows, nq, nk, d in ((3, 1, 1, 64), (130, 3, 1, 64), (257, 5, 5, 128), (520, 17, 1, 128), (1024, 8, 2, 64),
                            (4096, 32, 32, 64), (4096, 32, 8, 128), (1 << 20, 32, 32, 64)):
        n = lib.pt_qk_norm_bwd_partials(rows, nq, nk, d)
        # one row per workgroup of 256 threads, each owning 16 columns of one head, capped
        assert 0 < n <= 1024 and n <= -(-rows * (nq + nk) * (d // 16) // 256), (rows, nq, nk, d, n)
    assert lib.pt_qk_norm_bwd_partials(520, 17, 1, 128) > 1
    assert lib.pt_qk_norm_bwd_partials(1024, 8, 2, 64) >= 2


def _write(path, codes):
    accepted = {k: rc for k, rc in codes.items() if rc >= 0}
    assert not accepted, f"rows the library accepts have no place in the table: {accepted}"
    with open(path, "w") as f:
        f.write('{\n "refusals": {\n' + ",\n".join(f"  {json.dumps(k)}: {rc}" for k, rc in codes.items()) + "\n }\n}\n")
    print(f"wrote {path}: {len(codes)} refusals")


if __name__ == "__main__":
    _write(GOLDEN, refusal_codes(library()))
