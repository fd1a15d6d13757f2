"""Host side of the head dim 256 attention entries (CPU): every check of include/picotron_hip.h's section,
in its order, with its code -- a refused call launches nothing, so fake pointers are never read."""
import ctypes

import pytest

PTR = 1 << 20   # a non-null, 16-byte aligned address no refused call dereferences
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
B, H, HKV, S, D = 2, 4, 2, 128, 256


def call(lib, bwd, ptr=PTR, seq=None, head=D, batch=None, **dims):
    """The entry with view 0 (q) at `ptr` and strides (batch, seq, head), every other view regular."""
    d = dict(dict(B=B, H=H, HKV=HKV, S=S, scale=0.07), **dims)
    row = (H + 2 * HKV) * D
    st = lambda *s: (ctypes.c_int64 * 3)(*s)
    ok = st(S * row, row, D)
    first = st(S * row if batch is None else batch, row if seq is None else seq, head)
    views = [ptr, first] + [PTR, ok] * (4 if bwd else 3)                  # q, k, v, o (, dout)
    tail = [PTR, PTR] + [PTR, ok] * 3 if bwd else [PTR]                   # lse (, delta, dq, dk, dv)
    fn = lib.pt_attn_d256_bwd if bwd else lib.pt_attn_d256_fwd
    return fn(*views, *tail, d["B"], d["H"], d["HKV"], d["S"], d["scale"], None)


CASES = [
    (dict(ptr=None), EINVAL),                       # 1. a NULL pointer
    (dict(B=0), EINVAL),                            #    a size < 1
    (dict(S=192), EUNSUPPORTED),                    # 2. S off the 128-row blocks
    (dict(H=3), EUNSUPPORTED),                      #    H % HKV
    (dict(B=65536), EUNSUPPORTED),                  #    a count past 32 bits
    (dict(seq=128), EINVAL),                        # 3. a seq stride below the row
    (dict(head=128), EINVAL),                       #    a head stride below the row
    (dict(ptr=PTR + 8), EALIGN),                    # 4. a pointer off 16 bytes
    (dict(seq=(H + 2 * HKV) * D + 4), EALIGN),      #    a stride off 8 elements
    (dict(ptr=None, S=192), EINVAL),                # precedence: 1 before 2
    (dict(S=192, seq=128), EUNSUPPORTED),           #             2 before 3
    (dict(seq=132), EINVAL),                        #             3 before 4 (below the row and off 8)
]


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("args,code", CASES, ids=[",".join(c[0]) for c in CASES])
def test_entries_refuse_before_launch(bwd, args, code):
    from picotron_amd import _C
    assert call(_C.load_library(), bwd, **args) == code
