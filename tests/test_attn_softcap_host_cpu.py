"""Host side of pt_attn_fwd_softcap / pt_attn_bwd_softcap (CPU): the codes of include/picotron_hip.h's section --
a refused call launches nothing, so the fake pointers are never read."""
import ctypes

import pytest

PTR = 1 << 20   # a non-null, 16-byte aligned address no refused call dereferences
EINVAL, EUNSUPPORTED = -1, -3
B, H, HKV = 2, 4, 2


def call(lib, bwd, first=PTR, S=128, D=64, softcap=50.0, kv_lo=None, q_hi=None):
    """The entry with its first checked pointer (forward: q; backward: o) at `first`, every view regular."""
    row = (H + 2 * HKV) * D
    ok = (ctypes.c_int64 * 3)(S * row, row, D)
    dims = (B, H, HKV, S, S, D, 0.125, softcap)
    if not bwd:
        return lib.pt_attn_fwd_softcap(first, ok, PTR, ok, PTR, ok, PTR, ok, PTR, *dims, kv_lo, q_hi, None)
    return lib.pt_attn_bwd_softcap(PTR, ok, PTR, ok, PTR, ok, first, ok, PTR, ok, PTR, PTR, PTR, ok, PTR, ok, PTR, ok,
                                   *dims, None, None, 0, kv_lo, q_hi, None)


CASES = [
    (dict(first=None), EINVAL),
    (dict(softcap=0.0), EINVAL), (dict(softcap=-2.0), EINVAL),
    (dict(softcap=float("inf")), EINVAL), (dict(softcap=float("nan")), EINVAL),
    (dict(kv_lo=PTR), EINVAL), (dict(q_hi=PTR), EINVAL),            # exactly one bound NULL
    (dict(D=96), EUNSUPPORTED), (dict(D=256), EUNSUPPORTED), (dict(S=192), EUNSUPPORTED),
    (dict(kv_lo=PTR, q_hi=PTR, S=192), EUNSUPPORTED),               # both bounds: on to the shape checks
    (dict(softcap=0.0, D=256), EINVAL),                             # precedence: the cap before the shape
]


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("args,code", CASES, ids=[",".join(f"{k}={v}" for k, v in c[0].items()) for c in CASES])
def test_entries_refuse_before_launch(bwd, args, code):
    from picotron_amd import _C
    assert call(_C.load_library(), bwd, **args) == code
