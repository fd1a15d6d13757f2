// Final-logit soft-capping as row kernels (Gemma-2's final_logit_softcapping, also Grok-1):
//   fwd:  y  = bf16( c tanh(x / c) )                 (y may be x)
//   bwd:  dx = bf16( dy * (1 - (y / c)^2) )          (dx may be dy; y the forward's stored output)
//
// The lm_head GEMM applies the cap in its epilogue (gemm.hip EPI_CE_STATS_CAP) and the cross-entropy backward
// folds the derivative into its store (cross_entropy.hip CAP); these kernels serve what those two do not:
// an lm_head shape off the statistics' tile grid, the statistics switched off, and a gradient that is not
// the cross-entropy's own (a second consumer of the logits).  The tanh and its derivative are common.h's
// pt_softcap / pt_softcap_grad, the expressions of the fused forms.
//
// x, y, dy, dx are [rows, cols] bf16 views with independent row strides (elements).  A workgroup walks rows
// (grid-stride); its 256 threads take the row's 16-byte chunks two at a time per thread, both loads issued
// before the math, so a [4096, 49152] tensor keeps 2 x 16 B per lane in flight on every CU.  HBM-bound:
// fwd 4 bytes / element, bwd 6.
#include "common.h"

namespace {

constexpr int kThreads = 256, kUnroll = 2;

template <bool BWD>
__global__ __launch_bounds__(kThreads) void softcap_kernel(const uint16_t* a, int64_t as, const uint16_t* y, int64_t ys,
                                                           uint16_t* o, int64_t os, int64_t rows, int cols, PtCap cap) {
  const int nch = cols >> 3;
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const uint16_t* ar = a + r * as;
    const uint16_t* yr = BWD ? y + r * ys : nullptr;
    uint16_t* orow = o + r * os;
    for (int c0 = threadIdx.x; c0 < nch; c0 += kThreads * kUnroll) {
      bf16x8 va[kUnroll], vy[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int c = c0 + u * kThreads;
        if (c < nch) {
          va[u] = ld8(ar + c * 8);
          if (BWD) vy[u] = ld8(yr + c * 8);
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int c = c0 + u * kThreads;
        if (c >= nch) continue;
        float f[8], t[8];
        unpack8(va[u], f);
        if (BWD) unpack8(vy[u], t);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          f[j] = BWD ? f[j] * pt_softcap_grad(t[j], cap.c, cap.inv_c2) : pt_softcap(f[j], cap.k1, cap.c);
        st8(orow + c * 8, pack8(f));
      }
    }
  }
}

// the checks both entries make after their null pointers, sizes and the cap
int views_ok(const void* const* p, const int64_t* ld, int n, int64_t rows, int64_t cols) {
  if (cols & 7) return PT_EALIGN;
  for (int i = 0; i < n; ++i)
    if ((ld[i] & 7) || !pt_aligned16(p[i])) return PT_EALIGN;
  if (rows > INT32_MAX || cols > INT32_MAX) return PT_EUNSUPPORTED;
  return PT_OK;
}

unsigned grid_for(int64_t rows) { return (unsigned)(rows < PT_STREAM_GRID_CAP * 2 ? rows : PT_STREAM_GRID_CAP * 2); }

}  // namespace

extern "C" {

int pt_softcap_fwd(const void* x, int64_t ldx, void* y, int64_t ldy, int64_t rows, int64_t cols, float softcap,
                   hipStream_t stream) {
  if (!x || !y || rows <= 0 || cols <= 0) return PT_EINVAL;
  if (!pt_cap_valid(softcap)) return PT_EINVAL;
  const void* p[] = {x, y};
  const int64_t ld[] = {ldx, ldy};
  if (const int rc = views_ok(p, ld, 2, rows, cols)) return rc;
  softcap_kernel<false><<<grid_for(rows), kThreads, 0, stream>>>((const uint16_t*)x, ldx, nullptr, 0, (uint16_t*)y, ldy,
                                                                rows, (int)cols, pt_cap(softcap));
  PT_CHECK_LAUNCH();
  return PT_OK;
}

int pt_softcap_bwd(const void* dy, int64_t lddy, const void* y, int64_t ldy, void* dx, int64_t lddx, int64_t rows,
                   int64_t cols, float softcap, hipStream_t stream) {
  if (!dy || !y || !dx || rows <= 0 || cols <= 0) return PT_EINVAL;
  if (!pt_cap_valid(softcap)) return PT_EINVAL;
  const void* p[] = {dy, y, dx};
  const int64_t ld[] = {lddy, ldy, lddx};
  if (const int rc = views_ok(p, ld, 3, rows, cols)) return rc;
  softcap_kernel<true><<<grid_for(rows), kThreads, 0, stream>>>((const uint16_t*)dy, lddy, (const uint16_t*)y, ldy,
                                                               (uint16_t*)dx, lddx, rows, (int)cols, pt_cap(softcap));
  PT_CHECK_LAUNCH();
  return PT_OK;
}

}  // extern "C"
