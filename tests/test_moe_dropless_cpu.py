"""Dropless mixture-of-experts, host side: the static row bound and the refusals of the segment-GEMM entry
points, which answer before any launch (no device needed)."""
import ctypes

import pytest

A = 128


@pytest.mark.parametrize("T,E,k", [(1, 1, 1), (192, 8, 2), (1000, 60, 4), (4096, 8, 2), (4096, 64, 8), (7, 128, 8)])
def test_rows_bound_any_routing(T, E, k):
    from picotron_amd import _C
    from picotron_amd import kernels as K
    R = K.moe_dropless_rows(T, E, k)
    assert R % A == 0 and R == _C.load_library().pt_moe_dropless_rows(T, E, k) and K.MOE_SEG_ALIGN == A
    # the worst routing: as many experts as possible one item past a multiple of 128
    n, left, worst = T * k, min(E, T * k), 0
    for e in range(left):
        c = 1 if e < left - 1 else n - (left - 1)
        worst += -(-c // A) * A
    assert worst <= R
    assert R <= n + E * (A - 1)


def test_host_refusals():
    from picotron_amd import _C
    lib = _C.load_library()
    assert lib.pt_moe_seg_align() == A
    OK, EINVAL, EALIGN, EUNSUP = 0, -1, -2, -3   # include/picotron_hip.h
    out = (ctypes.c_int64 * (4 * 129))()
    ptrs = lambda v, n: (ctypes.c_void_p * n)(*([v] * n))
    assert lib.pt_moe_seg_table(ptrs(4096, 2), None, 128, 2, out) == OK and list(out[:8]) == [4096, 0, 128, 0] * 2
    assert lib.pt_moe_seg_table(ptrs(4096 + 8, 2), None, 128, 2, out) == EALIGN
    assert lib.pt_moe_seg_table(ptrs(4096, 2), ptrs(4096 + 2, 2), 128, 2, out) == EALIGN
    assert lib.pt_moe_seg_table(ptrs(4096, 2), None, 100, 2, out) == EALIGN
    assert lib.pt_moe_seg_table(ptrs(4096, 129), None, 128, 129, out) == EUNSUP
    assert lib.pt_moe_seg_table(ptrs(4096, 2), ptrs(None, 2), 128, 2, out) == EINVAL   # two pointers: none may be null
    P = 1 << 20   # a fake, aligned address: every case below is refused before anything is launched

    def seg(form=0, a=P, lda=256, b=None, ldb=0, c=P, ldc=256, R=256, N=256, K=256, split=256, E=4, epi=0, te=P):
        return lib.pt_moe_gemm_seg(form, a, lda, b, ldb, c, ldc, P, P, te, R, N, K, split, E, epi, None)
    assert seg(form=3) == EINVAL and seg(c=None) == EINVAL and seg(te=None) == EINVAL and seg(epi=1) == EINVAL
    assert seg(form=2, b=None) == EINVAL and seg(form=2, b=P, ldb=256, epi=4) == EINVAL and seg(split=0) == EINVAL
    assert seg(R=192) == EUNSUP and seg(N=192, ldc=192, split=192) == EUNSUP and seg(K=96) == EUNSUP
    assert seg(form=2, b=P, ldb=192, K=192) == EUNSUP   # form 2: Kin off the 128-grid
    assert seg(N=512, ldc=512, split=64) == EUNSUP and seg(form=1, split=32) == EUNSUP and seg(E=129) == EUNSUP
    assert seg(a=P + 8) == EALIGN and seg(c=P + 2) == EALIGN and seg(lda=260) == EALIGN and seg(ldc=128) == EALIGN
    assert seg(form=2, b=P + 4, ldb=256) == EALIGN and seg(form=2, b=P, ldb=250) == EALIGN
