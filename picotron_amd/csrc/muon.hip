// Muon's own device code for gfx950: everything of a Muon step that is not a GEMM.
//
// Replaces (torch 2.10, torch/optim/_muon.py) for a list of 2-D bf16 parameters:
//   buf.lerp_(grad, 1 - momentum); update = grad.lerp(buf, momentum) | buf          :310-311
//   ortho_grad.div_(ortho_grad.norm().clamp(min=eps))                                 :59
//   gram_update = addmm(gram, gram, gram, beta=b, alpha=c)  (+ the a of the next addmm) :63-66
//   param.mul_(1 - lr * wd); param.add_(update, alpha=-adjusted_lr)                   :317-318
// The matrix products of the Newton-Schulz iteration between them run on csrc/gemm.hip through the
// launch layer (kernels.muon_newton_schulz).
//
// The sequence per parameter p [R, C] with gradient g and state buf (the gradient's dtype):
//   g'   = CLIP ? r(g * clip_coef) : g                       as the AdamW kernels take the gradient
//   buf  = r(lerp(buf, g', 1 - mu))                           torch's lerp, both branches
//   u    = bf16(nesterov ? lerp(g', buf, mu) : buf)
//   sq   = sum u^2 in f32 over the bf16 u                     fixed order, no atomics
//   X0   = bf16(u / max(sqrt(sq), eps))                       into the zero-padded workspace
//   P'   = bf16(a I + b A + c S)                              A = bf16(X X^T), S = f32(A A)
//   p    = bf16(p * (1 - lr wd)); p = bf16(p - lr_adj O)      O = the iteration's result
//
// The table walk differs from the AdamW kernels' in one point, on purpose: a tensor's chunks are
// cut into BLOCKS of kBlockChunks chunks counted from the tensor's own first element, and a
// workgroup takes whole blocks (one f32 partial each).  So which thread adds which element, and in
// which order the partials are summed, depends on the tensor alone -- its squared norm has the same
// bits wherever it stands in the list, whatever its neighbours are, vector or scalar form.
//
// Top to bottom: element functions; the descriptor and the block walk; the kernels (momentum,
// final sum, scale, polynomial, apply); the host launch helpers; the extern "C" forwards.
#include "common.h"

namespace {

// ---- element functions ------------------------------------------------------------------------
// torch's lerp (ATen/native/Lerp.h): weight < 0.5 ? start + weight * (end - start)
//                                                 : end - (end - start) * (1 - weight),
// with the contraction spelled out, so every form computes the same bits
__device__ __forceinline__ float lerp_t(float start, float end, float w) {
#pragma clang fp contract(off)
  const float diff = end - start;
  return fabsf(w) < 0.5f ? fmaf(w, diff, start) : fmaf(-diff, 1.0f - w, end);
}

// the clip coefficient of csrc/adamw.hip (clip_coef / clip_grad there), restated: the same bits
// from the same device scalar, so one coefficient serves the AdamW and the Muon half of a model
template <bool CLIP>
struct ClipArgs {};
template <>
struct ClipArgs<true> {
  const float* sq;
  float max_norm;
  int* status;
};
__device__ __forceinline__ bool clip_coef(const ClipArgs<true>& c, float& coef, bool post) {
  const float sq = c.sq[0];
  if (!(sq <= 3.402823466e+38f)) {
    if (post && c.status && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
      atomicOr(c.status, PT_STATUS_NONFINITE_GRAD);
    return false;
  }
  coef = fminf(1.0f, c.max_norm / (sqrtf(sq) + 1e-6f));
  return true;
}
__device__ __forceinline__ float clip_grad(float g, float coef, bool bf) {
#pragma clang fp contract(off)
  const float x = g * coef;
  return bf ? round_bf(x) : x;
}

struct MomScalars {
  float w_buf;   // f32(1 - mu): the weight of buf.lerp_(grad, .)
  float w_nes;   // f32(mu): the weight of grad.lerp(buf, .)
  int nesterov;
};

// (new buf, u) of one element.  GT's storage rounding is applied to buf; u is rounded to bf16.
template <bool BF, bool CLIP>
__device__ __forceinline__ void mom_elem(float g, float& buf, float& u, const MomScalars& s, float coef) {
  if constexpr (CLIP) g = clip_grad(g, coef, BF);
  buf = lerp_t(buf, g, s.w_buf);
  if (BF) buf = round_bf(buf);
  u = round_bf(s.nesterov ? lerp_t(g, buf, s.w_nes) : buf);
}
// u alone, from the gradient and the ALREADY updated buffer (the scale kernel: cheaper than storing u)
template <bool BF, bool CLIP>
__device__ __forceinline__ float u_elem(float g, float buf, const MomScalars& s, float coef) {
  if constexpr (CLIP) g = clip_grad(g, coef, BF);
  return round_bf(s.nesterov ? lerp_t(g, buf, s.w_nes) : buf);
}

// 8 x f32 as two 16-byte vectors, non-temporal
typedef float pt_f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) pt_f32x4 pt_g_f32x4;
__device__ __forceinline__ void ld8_as_f(const uint16_t* p, float* f) { unpack8(ld8_nt(p), f); }
__device__ __forceinline__ void ld8_as_f(const float* p, float* f) {
  const pt_f32x4 lo = __builtin_nontemporal_load((const pt_g_f32x4*)(p));
  const pt_f32x4 hi = __builtin_nontemporal_load((const pt_g_f32x4*)(p + 4));
#pragma unroll
  for (int j = 0; j < 4; ++j) { f[j] = lo[j]; f[4 + j] = hi[j]; }
}
__device__ __forceinline__ void st8_from_f(uint16_t* p, const float* f) { st8_nt(p, pack8(f)); }
__device__ __forceinline__ void st8_from_f(float* p, const float* f) {
  __builtin_nontemporal_store(pt_f32x4{f[0], f[1], f[2], f[3]}, (pt_g_f32x4*)(p));
  __builtin_nontemporal_store(pt_f32x4{f[4], f[5], f[6], f[7]}, (pt_g_f32x4*)(p + 4));
}
__device__ __forceinline__ float ld_as_f(const uint16_t* p, int64_t i) { return bf2f(p[i]); }
__device__ __forceinline__ float ld_as_f(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ void st_from_f(uint16_t* p, int64_t i, float x) { p[i] = f2bf(x); }
__device__ __forceinline__ void st_from_f(float* p, int64_t i, float x) { p[i] = x; }

// ---- descriptor and block walk ----------------------------------------------------------------
struct MuonTensor {   // pt_muon_tensor (include/picotron_hip.h)
  uint16_t* p;        // [R, C] bf16, row stride ldp
  const void* g;      // [R, C] bf16 | f32, row stride ldg
  void* buf;          // [R, C] in the gradient's dtype, row stride ldb
  uint16_t* x;        // the workspace image: X0 is written there, O is read from there; row stride ldx
  int64_t n, cols;    // R * C, C
  int64_t ldp, ldg, ldb, ldx;
  float lr_ratio;     // _adjust_lr's ratio for the shape: lr_adj = lr * lr_ratio (apply)
  int32_t sq_slot;    // this tensor's entry of the squared-norm array
};

constexpr int kBlockChunks = 2048;   // chunks of 8 elements per block: 8 per thread

// The sum of a workgroup in a fixed order (wave butterfly, then the four waves in index order);
// every thread returns it.  Safe to call in a loop.
__device__ __forceinline__ float block_sum_256(float v) {
  __shared__ float part[4];
  v = wave_sum(v);
  __syncthreads();   // the previous call's readers are done
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((part[0] + part[1]) + part[2]) + part[3];
}

// offset of logical element i of a [R, C] view with row stride ld
__device__ __forceinline__ int64_t at(int64_t i, int64_t cols, int64_t ld) {
  return ld == cols ? i : (i / cols) * ld + (i % cols);
}

// 16-byte accesses need aligned bases and row strides and C on the 8-element grid
__device__ __forceinline__ bool mult8(int64_t v) { return (v & 7) == 0; }
__device__ __forceinline__ bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// fn(T, b): block b (counted inside tensor T) for every block of this workgroup, grid-strided over
// the table's blocks
template <typename F>
__device__ __forceinline__ void for_each_block(const MuonTensor* __restrict__ ts, const int64_t* __restrict__ block_start,
                                               int nt, F fn) {
  const int64_t total = block_start[nt];
  for (int64_t blk = blockIdx.x; blk < total; blk += gridDim.x) {
    int a = 0, b = nt - 1;   // the tensor holding block blk: largest t with block_start[t] <= blk
    while (a < b) {
      const int mid = (a + b + 1) >> 1;
      if (block_start[mid] <= blk) a = mid; else b = mid - 1;
    }
    fn(ts[a], blk - block_start[a], blk);
  }
}

// ---- momentum, u and the sum-of-squares partials ----------------------------------------------
// partial[global block] = sum of u^2 over the block: a thread adds its chunks' elements in index
// order into one accumulator, then block_sum_256.
template <typename GT, bool CLIP>
__global__ __launch_bounds__(256, 4) void muon_momentum_kernel(const MuonTensor* __restrict__ ts,
                                                               const int64_t* __restrict__ block_start, int nt,
                                                               MomScalars s, float* __restrict__ partial,
                                                               ClipArgs<CLIP> clip) {
  constexpr bool BF = sizeof(GT) == 2;
  float coef = 1.0f;
  if constexpr (CLIP) {
    if (!clip_coef(clip, coef, true)) return;
  }
  for_each_block(ts, block_start, nt, [&](const MuonTensor& T, int64_t b, int64_t blk) {
    const GT* G = (const GT*)T.g;
    GT* B = (GT*)T.buf;
    const bool vec = al16(G) && al16(B) && mult8(T.cols) && mult8(T.ldg) && mult8(T.ldb);
    const int64_t chunks = (T.n + 7) >> 3;
    const int64_t c1 = (b + 1) * kBlockChunks < chunks ? (b + 1) * kBlockChunks : chunks;
    float acc = 0.0f;
#pragma unroll 2
    for (int64_t c = b * kBlockChunks + threadIdx.x; c < c1; c += 256) {
      const int64_t i0 = c * 8;
      if (vec && i0 + 8 <= T.n) {
        const int64_t og = at(i0, T.cols, T.ldg), ob = at(i0, T.cols, T.ldb);
        float g[8], m[8];
        ld8_as_f(G + og, g);
        ld8_as_f(B + ob, m);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float u;
          mom_elem<BF, CLIP>(g[j], m[j], u, s, coef);
          acc = fmaf(u, u, acc);
        }
        st8_from_f(B + ob, m);
      } else {   // unaligned, a row stride off the 8-grid, or the ragged last chunk
        const int64_t i1 = i0 + 8 < T.n ? i0 + 8 : T.n;
        for (int64_t i = i0; i < i1; ++i) {
          const int64_t ob = at(i, T.cols, T.ldb);
          float m = ld_as_f(B, ob), u;
          mom_elem<BF, CLIP>(ld_as_f(G, at(i, T.cols, T.ldg)), m, u, s, coef);
          acc = fmaf(u, u, acc);
          st_from_f(B, ob, m);
        }
      }
    }
    const float sum = block_sum_256(acc);
    if (threadIdx.x == 0) partial[blk] = sum;
  });
}

// sq[T.sq_slot] = the sum of tensor T's block partials, one workgroup per tensor, fixed order
// (thread t takes partials t, t + 256, ... in index order).  CLIP with a non-finite global norm: the
// momentum kernel wrote no partials, and sq is left alone too.
template <bool CLIP>
__global__ __launch_bounds__(256) void muon_sq_final_kernel(const MuonTensor* __restrict__ ts,
                                                            const int64_t* __restrict__ block_start,
                                                            const float* __restrict__ partial,
                                                            float* __restrict__ sq, ClipArgs<CLIP> clip) {
  if constexpr (CLIP) {
    float coef;
    if (!clip_coef(clip, coef, false)) return;
  }
  const int t = blockIdx.x;
  const int64_t b0 = block_start[t], b1 = block_start[t + 1];
  float acc = 0.0f;
  for (int64_t i = b0 + threadIdx.x; i < b1; i += 256) acc += partial[i];
  const float sum = block_sum_256(acc);
  if (threadIdx.x == 0) sq[ts[t].sq_slot] = sum;
}

// ---- X0 = bf16(u / max(||u||, eps)) into the padded workspace ---------------------------------
template <typename GT, bool CLIP>
__global__ __launch_bounds__(256, 4) void muon_scale_kernel(const MuonTensor* __restrict__ ts,
                                                            const int64_t* __restrict__ block_start, int nt,
                                                            MomScalars s, const float* __restrict__ sq, float eps,
                                                            ClipArgs<CLIP> clip) {
  constexpr bool BF = sizeof(GT) == 2;
  float coef = 1.0f;
  if constexpr (CLIP) {
    if (!clip_coef(clip, coef, false)) return;
  }
  for_each_block(ts, block_start, nt, [&](const MuonTensor& T, int64_t b, int64_t) {
    const GT* G = (const GT*)T.g;
    const GT* B = (const GT*)T.buf;
    const float d = fmaxf(sqrtf(sq[T.sq_slot]), eps);
    const bool vec = al16(G) && al16(B) && al16(T.x) && mult8(T.cols) && mult8(T.ldg) && mult8(T.ldb) && mult8(T.ldx);
    const int64_t chunks = (T.n + 7) >> 3;
    const int64_t c1 = (b + 1) * kBlockChunks < chunks ? (b + 1) * kBlockChunks : chunks;
#pragma unroll 2
    for (int64_t c = b * kBlockChunks + threadIdx.x; c < c1; c += 256) {
      const int64_t i0 = c * 8;
      if (vec && i0 + 8 <= T.n) {
        float g[8], m[8], x[8];
        ld8_as_f(G + at(i0, T.cols, T.ldg), g);
        ld8_as_f(B + at(i0, T.cols, T.ldb), m);
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = u_elem<BF, CLIP>(g[j], m[j], s, coef) / d;
        st8(T.x + at(i0, T.cols, T.ldx), pack8(x));   // (read next by the GEMMs: the default cache policy)
      } else {
        const int64_t i1 = i0 + 8 < T.n ? i0 + 8 : T.n;
        for (int64_t i = i0; i < i1; ++i) {
          const float u = u_elem<BF, CLIP>(ld_as_f(G, at(i, T.cols, T.ldg)), ld_as_f(B, at(i, T.cols, T.ldb)), s, coef);
          T.x[at(i, T.cols, T.ldx)] = f2bf(u / d);
        }
      }
    }
  });
}

// ---- P' = bf16(a I + b A + c S) on [m, m], up to 4 matrices of one shape ----------------------
struct PolyArgs {
  const uint16_t* A[4];
  const float* S[4];
  uint16_t* P[4];
  int64_t m;   // rows = columns = leading dimension, a multiple of 8
  float a, b, c;
};
__device__ __forceinline__ float poly_elem(float A, float S, bool diag, const PolyArgs& q) {
#pragma clang fp contract(off)
  const float t = fmaf(q.c, S, q.b * A);
  return diag ? t + q.a : t;
}
__global__ __launch_bounds__(256) void muon_poly_kernel(PolyArgs q) {
  const int z = blockIdx.y;
  const uint16_t* __restrict__ A = q.A[z];
  const float* __restrict__ S = q.S[z];
  uint16_t* __restrict__ P = q.P[z];
  const int64_t chunks = q.m * q.m >> 3;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * 256) {
    const int64_t i0 = c * 8, row = i0 / q.m, col = i0 - row * q.m;   // a chunk lies inside one row
    float av[8], sv[8], p[8];
    unpack8(ld8(A + i0), av);
    ld8_as_f(S + i0, sv);
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = poly_elem(av[j], sv[j], col + j == row, q);
    st8(P + i0, pack8(p));
  }
}

// ---- p = bf16(p * decay); p = bf16(p - lr_adj * O) --------------------------------------------
// (lr_adj = f32(lr) * f32(ratio): one f32 rounding where torch rounds the double product once)
__device__ __forceinline__ float apply_elem(float p, float o, float decay, float lr_adj) {
#pragma clang fp contract(off)
  p = round_bf(p * decay);
  return fmaf(-lr_adj, o, p);
}
template <bool CLIP>
__global__ __launch_bounds__(256, 4) void muon_apply_kernel(const MuonTensor* __restrict__ ts,
                                                            const int64_t* __restrict__ block_start, int nt,
                                                            float decay, float lr, ClipArgs<CLIP> clip) {
  if constexpr (CLIP) {   // a non-finite global norm: the whole step is skipped
    float coef;
    if (!clip_coef(clip, coef, false)) return;
  }
  for_each_block(ts, block_start, nt, [&](const MuonTensor& T, int64_t b, int64_t) {
    const bool vec = al16(T.p) && al16(T.x) && mult8(T.cols) && mult8(T.ldp) && mult8(T.ldx);
    const float lr_adj = lr * T.lr_ratio;
    const int64_t chunks = (T.n + 7) >> 3;
    const int64_t c1 = (b + 1) * kBlockChunks < chunks ? (b + 1) * kBlockChunks : chunks;
#pragma unroll 2
    for (int64_t c = b * kBlockChunks + threadIdx.x; c < c1; c += 256) {
      const int64_t i0 = c * 8;
      if (vec && i0 + 8 <= T.n) {
        const int64_t op = at(i0, T.cols, T.ldp);
        float p[8], o[8];
        unpack8(ld8_nt(T.p + op), p);
        unpack8(ld8_nt(T.x + at(i0, T.cols, T.ldx)), o);
#pragma unroll
        for (int j = 0; j < 8; ++j) p[j] = apply_elem(p[j], o[j], decay, lr_adj);
        st8_nt(T.p + op, pack8(p));
      } else {
        const int64_t i1 = i0 + 8 < T.n ? i0 + 8 : T.n;
        for (int64_t i = i0; i < i1; ++i) {
          const int64_t op = at(i, T.cols, T.ldp);
          T.p[op] = f2bf(apply_elem(bf2f(T.p[op]), bf2f(T.x[at(i, T.cols, T.ldx)]), decay, lr_adj));
        }
      }
    }
  });
}

// ---- host launch helpers ----------------------------------------------------------------------
// one resident round: 4 blocks of 4 waves per CU at <= 128 VGPRs, as the AdamW list kernels
unsigned walk_grid(int64_t total_blocks) { return (unsigned)(total_blocks < 1024 ? total_blocks : 1024); }

bool list_ok(const void* tensors, const int64_t* block_start, int ntensors, int64_t total_blocks) {
  return tensors && block_start && ntensors > 0 && total_blocks >= 0;
}
bool dtype_ok(int dtype) { return dtype == 0 || dtype == 1; }   // bf16, f32
bool clip_ok(const ClipArgs<false>&) { return true; }
bool clip_ok(const ClipArgs<true>& c) { return c.sq && c.max_norm > 0.0f; }   // NaN is refused
bool weight_ok(float w) { return w - w == 0.0f; }   // finite

template <bool CLIP>
int momentum(const void* tensors, const int64_t* block_start, int ntensors, int64_t total_blocks, int grad_dtype,
             const MomScalars& s, float* partial, float* sq, const ClipArgs<CLIP>& clip, hipStream_t stream) {
  if (!list_ok(tensors, block_start, ntensors, total_blocks) || !dtype_ok(grad_dtype) || !partial || !sq ||
      !weight_ok(s.w_buf) || !weight_ok(s.w_nes) || !clip_ok(clip))
    return PT_EINVAL;
  const auto* ts = (const MuonTensor*)tensors;
  if (total_blocks) {
    const unsigned grid = walk_grid(total_blocks);
    if (grad_dtype == 0)
      muon_momentum_kernel<uint16_t, CLIP><<<grid, 256, 0, stream>>>(ts, block_start, ntensors, s, partial, clip);
    else
      muon_momentum_kernel<float, CLIP><<<grid, 256, 0, stream>>>(ts, block_start, ntensors, s, partial, clip);
    PT_CHECK_LAUNCH();
  }
  muon_sq_final_kernel<CLIP><<<ntensors, 256, 0, stream>>>(ts, block_start, partial, sq, clip);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

template <bool CLIP>
int scale(const void* tensors, const int64_t* block_start, int ntensors, int64_t total_blocks, int grad_dtype,
          const MomScalars& s, const float* sq, float eps, const ClipArgs<CLIP>& clip, hipStream_t stream) {
  if (!list_ok(tensors, block_start, ntensors, total_blocks) || !dtype_ok(grad_dtype) || !sq || !(eps >= 0.0f) ||
      !weight_ok(s.w_nes) || !clip_ok(clip))
    return PT_EINVAL;
  if (total_blocks == 0) return PT_OK;
  const auto* ts = (const MuonTensor*)tensors;
  const unsigned grid = walk_grid(total_blocks);
  if (grad_dtype == 0)
    muon_scale_kernel<uint16_t, CLIP><<<grid, 256, 0, stream>>>(ts, block_start, ntensors, s, sq, eps, clip);
  else
    muon_scale_kernel<float, CLIP><<<grid, 256, 0, stream>>>(ts, block_start, ntensors, s, sq, eps, clip);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

template <bool CLIP>
int apply(const void* tensors, const int64_t* block_start, int ntensors, int64_t total_blocks, float decay, float lr,
          const ClipArgs<CLIP>& clip, hipStream_t stream) {
  if (!list_ok(tensors, block_start, ntensors, total_blocks) || !weight_ok(decay) || !weight_ok(lr) || !clip_ok(clip))
    return PT_EINVAL;
  if (total_blocks == 0) return PT_OK;
  muon_apply_kernel<CLIP><<<walk_grid(total_blocks), 256, 0, stream>>>((const MuonTensor*)tensors, block_start, ntensors,
                                                                     decay, lr, clip);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

}  // namespace

extern "C" {

// ---- ABI forwards (include/picotron_hip.h) -----------------------------------------------------
int pt_muon_block_chunks(void) { return kBlockChunks; }

int pt_muon_momentum(const void* tensors, const int64_t* block_start, int ntensors, int64_t total_blocks,
                     int grad_dtype, float w_buf, float w_nes, int nesterov, float* partial, float* sq,
                     hipStream_t stream) {
  return momentum<false>(tensors, block_start, ntensors, total_blocks, grad_dtype, MomScalars{w_buf, w_nes, nesterov},
                         partial, sq, {}, stream);
}

int pt_muon_momentum_clip(const void* tensors, const int64_t* block_start, int ntensors, int64_t total_blocks,
                          int grad_dtype, float w_buf, float w_nes, int nesterov, float* partial, float* sq,
                          const float* grad_sq, float max_norm, int* status, hipStream_t stream) {
  return momentum<true>(tensors, block_start, ntensors, total_blocks, grad_dtype, MomScalars{w_buf, w_nes, nesterov},
                        partial, sq, ClipArgs<true>{grad_sq, max_norm, status}, stream);
}

int pt_muon_scale(const void* tensors, const int64_t* block_start, int ntensors, int64_t total_blocks, int grad_dtype,
                  float w_nes, int nesterov, const float* sq, float eps, hipStream_t stream) {
  return scale<false>(tensors, block_start, ntensors, total_blocks, grad_dtype, MomScalars{0.0f, w_nes, nesterov}, sq,
                      eps, {}, stream);
}

int pt_muon_scale_clip(const void* tensors, const int64_t* block_start, int ntensors, int64_t total_blocks,
                       int grad_dtype, float w_nes, int nesterov, const float* sq, float eps, const float* grad_sq,
                       float max_norm, int* status, hipStream_t stream) {
  return scale<true>(tensors, block_start, ntensors, total_blocks, grad_dtype, MomScalars{0.0f, w_nes, nesterov}, sq,
                     eps, ClipArgs<true>{grad_sq, max_norm, status}, stream);
}

int pt_muon_poly(const void* const* A, const float* const* S, void* const* P, int nmat, int64_t m, float a, float b,
                 float c, hipStream_t stream) {
  if (!A || !S || !P || nmat < 1 || nmat > 4 || m <= 0) return PT_EINVAL;
  if (m & 7) return PT_EALIGN;
  PolyArgs q{};
  for (int i = 0; i < nmat; ++i) {
    if (!A[i] || !S[i] || !P[i]) return PT_EINVAL;
    if (!pt_aligned16(A[i]) || !pt_aligned16(S[i]) || !pt_aligned16(P[i])) return PT_EALIGN;
    q.A[i] = (const uint16_t*)A[i];
    q.S[i] = S[i];
    q.P[i] = (uint16_t*)P[i];
  }
  q.m = m;
  q.a = a; q.b = b; q.c = c;
  const int64_t want = (m * m / 8 + 255) / 256;
  const dim3 grid((unsigned)(want < PT_STREAM_GRID_CAP ? want : PT_STREAM_GRID_CAP), (unsigned)nmat);
  muon_poly_kernel<<<grid, 256, 0, stream>>>(q);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

int pt_muon_apply(const void* tensors, const int64_t* block_start, int ntensors, int64_t total_blocks, float decay,
                  float lr, hipStream_t stream) {
  return apply<false>(tensors, block_start, ntensors, total_blocks, decay, lr, {}, stream);
}

int pt_muon_apply_clip(const void* tensors, const int64_t* block_start, int ntensors, int64_t total_blocks,
                       float decay, float lr, const float* grad_sq, float max_norm, int* status, hipStream_t stream) {
  return apply<true>(tensors, block_start, ntensors, total_blocks, decay, lr,
                     ClipArgs<true>{grad_sq, max_norm, status}, stream);
}

}  // extern "C"
