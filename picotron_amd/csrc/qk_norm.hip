// Per-head QK-norm (RMSNorm over each q head's and each k head's head_dim values) fused with RoPE,
// forward and backward -- the OLMo-2 / Qwen3 / Gemma-3 / Chameleon stability recipe, applied between
// the q|k|v projection and the rotation (Qwen3 layout: one [d] weight for all q heads, one for all
// k heads).  Not in the reference (okoge-kaz/picotron has no QK-norm); the two norm modes are
// csrc/rmsnorm.hip's, the rotation is csrc/rope.hip's:
//
//   rstd = rsqrt(mean_d(x^2) + eps)                                   (f32, per row and head)
//   mode 0:  y = bf16(x * rstd * w)          mode 1:  y = bf16(w * bf16(x * rstd))
//   fwd :    o1 = y1*c - y2*s,  o2 = y2*c + y1*s  on the bf16 y   (one more bf16 rounding)
//            => bit-identical to the norm-only output (cos = sin = NULL) followed by pt_rope
//   bwd :    p = dy * w,  xh = x * rstd,  dx = bf16(rstd * (p - xh * mean_d(p * xh)))
//            dw[c] = sum over rows and heads of dy * xh   (mode 1: dy * bf16(xh))
//            dy is the gradient with respect to y (the attention backward's dq|dk after its RoPE
//            inverse), x the saved pre-norm projection output.
//
// Layout: token-major rows [rows, stride] bf16; the first nq + nk heads of a row are q|k, whatever
// follows (v) is neither read nor written.  rope.hip's unit of work: one thread owns 8 rotation
// pairs -- chunk c of the first half and chunk c of the second half of one head, two 16-byte loads
// -- so d / 16 lanes (4 at d = 64, 8 at d = 128) hold one head and a wave 16 or 8 heads.  The sum of
// squares (the backward's mean(p * xh)) is 16 terms added in the lane, first half then second half
// in column order, and 2 or 3 __shfl_xor levels (1, 2, 4) inside the lane group: no LDS.  Every
// input byte is read once, y may be x and dx may be dy (a thread reads its 32 bytes before it
// writes them).  HBM-bound: forward 4 B per q|k element + rstd, backward 6 B per element.
//
// Weight gradient: the grid stride is a multiple of d / 16, so a thread keeps its column chunk and
// accumulates dy * xh for its 16 columns in registers, q heads and k heads apart.  A workgroup sums
// its threads' accumulators through LDS in thread order and writes ONE f32 row of each partial
// buffer (zeros when it saw no head of that kind); pt_rmsnorm_colsum_batch(cols = d) finishes the
// sums into the sinks.  No float atomics: bit-reproducible.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBwdGridCap = 1024;   // 256 CUs x 4 resident 4-wave blocks: the partial rows' count

template <int CPH>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = 1; o < CPH; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// CPH = lanes per head = head_dim / 16
template <int CPH>
__global__ __launch_bounds__(kThreads) void qk_norm_rope_fwd_kernel(
    const uint16_t* x, int x_stride, uint16_t* y, int y_stride, const uint16_t* __restrict__ wq,
    const uint16_t* __restrict__ wk, float* __restrict__ rstd_out, int64_t rows, int nq, int nheads, float eps, int mode,
    const uint16_t* __restrict__ cos_t, const uint16_t* __restrict__ sin_t, int seq_len, int tab_stride) {
  constexpr int D = CPH * 16, HALF = D / 2;
  const int per_row = nheads * CPH;
  const int64_t total = rows * per_row;
  const int ch = threadIdx.x % CPH;   // the same for every unit of this thread (the stride is a multiple of CPH)
  const bf16x8 wq1 = ld8(wq + ch * 8), wq2 = ld8(wq + HALF + ch * 8);
  const bf16x8 wk1 = ld8(wk + ch * 8), wk2 = ld8(wk + HALF + ch * 8);
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t row = i / per_row;
    const int head = (int)(i - row * per_row) / CPH;
    const int64_t at = (int64_t)head * D + ch * 8;
    float a[8], b[8], w1[8], w2[8];
    unpack8(ld8(x + row * x_stride + at), a);
    unpack8(ld8(x + row * x_stride + at + HALF), b);
    const bool isq = head < nq;
    unpack8(isq ? wq1 : wk1, w1);
    unpack8(isq ? wq2 : wk2, w2);
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += a[j] * a[j];
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += b[j] * b[j];
    ss = group_sum<CPH>(ss);
    const float rstd = rsqrtf(ss * (1.0f / D) + eps);
    if (ch == 0) rstd_out[row * nheads + head] = rstd;
    float y1[8], y2[8];
    if (mode == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { y1[j] = a[j] * rstd * w1[j]; y2[j] = b[j] * rstd * w2[j]; }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) { y1[j] = w1[j] * round_bf(a[j] * rstd); y2[j] = w2[j] * round_bf(b[j] * rstd); }
    }
    if (cos_t) {   // rope.hip's rotation of the bf16 y
      const int pos = (int)(row % seq_len);
      float c[8], s[8];
      unpack8(ld8(cos_t + (int64_t)pos * tab_stride + ch * 8), c);
      unpack8(ld8(sin_t + (int64_t)pos * tab_stride + ch * 8), s);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float ya = round_bf(y1[j]), yb = round_bf(y2[j]);
        y1[j] = fmaf(ya, c[j], -(yb * s[j]));
        y2[j] = fmaf(yb, c[j], ya * s[j]);
      }
    }
    st8(y + row * y_stride + at, pack8(y1));
    st8(y + row * y_stride + at + HALF, pack8(y2));
  }
}

template <int CPH>
__global__ __launch_bounds__(kThreads) void qk_norm_bwd_kernel(
    const uint16_t* dy, int dy_stride, const uint16_t* __restrict__ x, int x_stride, const uint16_t* __restrict__ wq,
    const uint16_t* __restrict__ wk, const float* __restrict__ rstd_in, uint16_t* dx, int dx_stride,
    float* __restrict__ dwq_partial, float* __restrict__ dwk_partial, int64_t rows, int nq, int nheads, int mode) {
  constexpr int D = CPH * 16, HALF = D / 2;
  constexpr int kPad = 17;   // a thread's 16 accumulators, one word of padding: lane-stride 17 banks
  __shared__ float red[kThreads * kPad];
  const int per_row = nheads * CPH;
  const int64_t total = rows * per_row;
  const int ch = threadIdx.x % CPH;
  const bf16x8 wq1 = ld8(wq + ch * 8), wq2 = ld8(wq + HALF + ch * 8);
  const bf16x8 wk1 = ld8(wk + ch * 8), wk2 = ld8(wk + HALF + ch * 8);
  float accq[16], acck[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) accq[j] = acck[j] = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t row = i / per_row;
    const int head = (int)(i - row * per_row) / CPH;
    const int64_t at = (int64_t)head * D + ch * 8;
    float d[16], xh[16], w[16];
    unpack8(ld8(dy + row * dy_stride + at), d);
    unpack8(ld8(dy + row * dy_stride + at + HALF), d + 8);
    unpack8(ld8(x + row * x_stride + at), xh);
    unpack8(ld8(x + row * x_stride + at + HALF), xh + 8);
    const float rstd = rstd_in[row * nheads + head];
    const bool isq = head < nq;
    unpack8(isq ? wq1 : wk1, w);
    unpack8(isq ? wq2 : wk2, w + 8);
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      xh[j] *= rstd;
      dot += d[j] * w[j] * xh[j];
    }
    if (isq) {
#pragma unroll
      for (int j = 0; j < 16; ++j) accq[j] += d[j] * (mode == 0 ? xh[j] : round_bf(xh[j]));
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) acck[j] += d[j] * (mode == 0 ? xh[j] : round_bf(xh[j]));
    }
    dot = group_sum<CPH>(dot) * (1.0f / D);
    float o[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) o[j] = rstd * (d[j] * w[j] - xh[j] * dot);
    st8(dx + row * dx_stride + at, pack8(o));
    st8(dx + row * dx_stride + at + HALF, pack8(o + 8));
  }

  // the workgroup's threads of one column chunk summed in thread order: one partial row per buffer
  const int col = threadIdx.x;   // < D: the column this thread sums
  const int cch = (col % HALF) / 8, slot = (col / HALF) * 8 + (col & 7);
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    float* out = which == 0 ? dwq_partial : dwk_partial;
    if (!out) continue;   // a frozen weight: uniform over the grid
#pragma unroll
    for (int j = 0; j < 16; ++j) red[threadIdx.x * kPad + j] = which == 0 ? accq[j] : acck[j];
    __syncthreads();
    if (col < D) {
      float s = 0.f;
      for (int t = cch; t < kThreads; t += CPH) s += red[t * kPad + slot];
      out[(int64_t)blockIdx.x * D + col] = s;
    }
    __syncthreads();
  }
}

int64_t units(int64_t rows, int64_t nheads, int64_t head_dim) { return rows * nheads * (head_dim / 16); }

int bwd_grid(int64_t rows, int64_t nheads, int64_t head_dim) {
  const int64_t g = (units(rows, nheads, head_dim) + kThreads - 1) / kThreads;
  return (int)(g < kBwdGridCap ? g : kBwdGridCap);
}

// Argument checks, in this order (tests/golden/qk_norm_host.json pins it): head_dim; null pointers,
// counts, mode, the cos / sin pair; sizes past the kernels' 32-bit indices (a row's heads, strides,
// tables; rows themselves are indexed in 64 bits but capped the same); rows narrower than their
// heads; alignment.
int check_shape(int64_t rows, int64_t nq, int64_t nk, int64_t head_dim) {
  if (head_dim != 64 && head_dim != 128) return PT_EUNSUPPORTED;
  if (rows <= 0 || nq <= 0 || nk <= 0) return PT_EINVAL;
  return PT_OK;
}

bool fits32(int64_t rows, int64_t nq, int64_t nk) {
  return rows <= INT32_MAX && nq <= INT32_MAX / 128 && nk <= INT32_MAX / 128 && nq + nk <= INT32_MAX / 128;
}

}  // namespace

extern "C" {

int pt_qk_norm_bwd_partials(int64_t rows, int64_t nheads_q, int64_t nheads_k, int64_t head_dim) {
  const int rc = check_shape(rows, nheads_q, nheads_k, head_dim);
  if (rc != PT_OK) return rc;
  if (!fits32(rows, nheads_q, nheads_k)) return PT_EUNSUPPORTED;
  return bwd_grid(rows, nheads_q + nheads_k, head_dim);
}

int pt_qk_norm_rope_fwd(const void* x, int64_t x_stride, void* y, int64_t y_stride, const void* wq, const void* wk,
                        float* rstd, int64_t rows, int64_t nheads_q, int64_t nheads_k, int64_t head_dim, float eps,
                        int mode, const void* cos_table, const void* sin_table, int64_t seq_len, int64_t table_stride,
                        hipStream_t stream) {
  const int rc = check_shape(rows, nheads_q, nheads_k, head_dim);
  if (rc != PT_OK) return rc;
  const bool rope = cos_table != nullptr;
  if (!x || !y || !wq || !wk || !rstd || (mode != 0 && mode != 1) || rope != (sin_table != nullptr)) return PT_EINVAL;
  if (rope && (seq_len <= 0 || table_stride <= 0)) return PT_EINVAL;
  if (!fits32(rows, nheads_q, nheads_k) || x_stride > INT32_MAX || y_stride > INT32_MAX) return PT_EUNSUPPORTED;
  if (rope && (seq_len > INT32_MAX || table_stride > INT32_MAX)) return PT_EUNSUPPORTED;
  const int64_t nheads = nheads_q + nheads_k, width = nheads * head_dim;
  if (x_stride < width || y_stride < width || (rope && table_stride < head_dim / 2)) return PT_EINVAL;
  if (x_stride % 8 != 0 || y_stride % 8 != 0 || (rope && table_stride % 8 != 0)) return PT_EALIGN;
  if (!pt_aligned16(x) || !pt_aligned16(y) || !pt_aligned16(wq) || !pt_aligned16(wk)) return PT_EALIGN;
  if (rope && (!pt_aligned16(cos_table) || !pt_aligned16(sin_table))) return PT_EALIGN;
  int64_t g = (units(rows, nheads, head_dim) + kThreads - 1) / kThreads;
  if (g > PT_STREAM_GRID_CAP * 2) g = PT_STREAM_GRID_CAP * 2;
  const auto* X = (const uint16_t*)x;
  auto* Y = (uint16_t*)y;
  const auto* WQ = (const uint16_t*)wq;
  const auto* WK = (const uint16_t*)wk;
  const auto* C = (const uint16_t*)cos_table;
  const auto* S = (const uint16_t*)sin_table;
  if (head_dim == 64)
    qk_norm_rope_fwd_kernel<4><<<(int)g, kThreads, 0, stream>>>(X, (int)x_stride, Y, (int)y_stride, WQ, WK, rstd, rows,
                                                                 (int)nheads_q, (int)nheads, eps, mode, C, S,
                                                                 (int)seq_len, (int)table_stride);
  else
    qk_norm_rope_fwd_kernel<8><<<(int)g, kThreads, 0, stream>>>(X, (int)x_stride, Y, (int)y_stride, WQ, WK, rstd, rows,
                                                                 (int)nheads_q, (int)nheads, eps, mode, C, S,
                                                                 (int)seq_len, (int)table_stride);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

int pt_qk_norm_bwd(const void* dy, int64_t dy_stride, const void* x, int64_t x_stride, const void* wq, const void* wk,
                   const float* rstd, void* dx, int64_t dx_stride, float* dwq_partial, float* dwk_partial,
                   int64_t rows, int64_t nheads_q, int64_t nheads_k, int64_t head_dim, int mode, hipStream_t stream) {
  const int rc = check_shape(rows, nheads_q, nheads_k, head_dim);
  if (rc != PT_OK) return rc;
  if (!dy || !x || !wq || !wk || !rstd || !dx || (mode != 0 && mode != 1)) return PT_EINVAL;
  if (!fits32(rows, nheads_q, nheads_k) || dy_stride > INT32_MAX || x_stride > INT32_MAX || dx_stride > INT32_MAX)
    return PT_EUNSUPPORTED;
  const int64_t nheads = nheads_q + nheads_k, width = nheads * head_dim;
  if (dy_stride < width || x_stride < width || dx_stride < width) return PT_EINVAL;
  if (dy_stride % 8 != 0 || x_stride % 8 != 0 || dx_stride % 8 != 0) return PT_EALIGN;
  if (!pt_aligned16(dy) || !pt_aligned16(x) || !pt_aligned16(dx) || !pt_aligned16(wq) || !pt_aligned16(wk))
    return PT_EALIGN;
  const int g = bwd_grid(rows, nheads, head_dim);
  const auto* DY = (const uint16_t*)dy;
  const auto* X = (const uint16_t*)x;
  auto* DX = (uint16_t*)dx;
  const auto* WQ = (const uint16_t*)wq;
  const auto* WK = (const uint16_t*)wk;
  if (head_dim == 64)
    qk_norm_bwd_kernel<4><<<g, kThreads, 0, stream>>>(DY, (int)dy_stride, X, (int)x_stride, WQ, WK, rstd, DX,
                                                      (int)dx_stride, dwq_partial, dwk_partial, rows, (int)nheads_q,
                                                      (int)nheads, mode);
  else
    qk_norm_bwd_kernel<8><<<g, kThreads, 0, stream>>>(DY, (int)dy_stride, X, (int)x_stride, WQ, WK, rstd, DX,
                                                      (int)dx_stride, dwq_partial, dwk_partial, rows, (int)nheads_q,
                                                      (int)nheads, mode);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

}  // extern "C"
