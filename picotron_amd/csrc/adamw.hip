// Fused AdamW step for gfx950: one pass over (param, grad, exp_avg, exp_avg_sq) per tensor.
//
// Replaces (reference): picotron/train.py:205-209 -- `torch.optim.AdamW(model.parameters(),
// lr=learning_rate)` (the reference's own fused switch at :205-207 is dead code), i.e. torch's
// multi-tensor Adam with decoupled weight decay, which on bf16 tensors runs eight foreach passes,
// each computing in f32 and rounding its result to the tensor dtype:
//   p  = r(p * decay)                       _foreach_mul_      decay = 1 - lr * wd
//   m  = r(m + w1 * (g - m))                _foreach_lerp_     w1 = 1 - beta1 (|w| < .5 form)
//   v  = r(v * beta2)                       _foreach_mul_
//   v  = r(v + c2 * (g * g))                _foreach_addcmul_  c2 = 1 - beta2
//   s  = r(sqrt(v)); s = r(s / bc2s); s = r(s + eps)   _foreach_sqrt / div_ / add_
//   p  = r(p + step * (m / s))              _foreach_addcdiv_  step = -lr / (1 - beta1^t)
// r() = round to the storage dtype.  The kernels perform exactly that sequence per element, with
// the roundings, so the result matches torch's bit for bit up to f32 contraction differences --
// but read each of the four tensors once and write three (14 bytes per bf16 parameter instead
// of ~44 over the eight passes).  Scalars arrive as f32, as torch's foreach kernels cast them.
//
// Also here, because they walk the same tensor tables: global gradient-norm clipping
// (torch.nn.utils.clip_grad_norm_ in front of the step) -- the f32 sum of squares of every
// gradient, and the clip coefficient applied where the AdamW kernels load the gradient (a
// compile-time variant of each) or in place.  And the two opt-in forms of the step that keep small
// updates: f32 master weights and moments behind the bf16 parameters, or bf16 state all the way with
// the three stores rounded stochastically (Philox4x32-10 bits, a pure function of seed, stream,
// step and element index).
//
// Top to bottom: element functions (adam_elem, adam_elem_master, the clip coefficient, the random
// bits and sr_bf16); the table walk (the three descriptor structs and for_each_run, a workgroup's
// run of 8-element chunks tensor by tensor); the kernels (step, master step, stochastic-rounding
// step and cast, sum of squares, in-place scale); the host launch helpers (geometry, the shared
// argument checks, one body per form with the clipping as a template argument: step_single /
// step_multi, master_single / master_multi, sr_single / sr_multi, grad_sq_sum); the extern "C"
// forwards.
#include "common.h"

namespace {

// ---- element functions ------------------------------------------------------------------------
struct AdamScalars {
  float decay, w1, beta2, c2, bc2s, eps, step;
};

template <typename T>
__device__ __forceinline__ float ld_as_f(const T* p, int64_t i);
template <>
__device__ __forceinline__ float ld_as_f<uint16_t>(const uint16_t* p, int64_t i) { return bf2f(p[i]); }
template <>
__device__ __forceinline__ float ld_as_f<float>(const float* p, int64_t i) { return p[i]; }

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamScalars& s, bool bf) {
  auto r = [bf](float x) { return bf ? round_bf(x) : x; };
  p = r(p * s.decay);
  m = r(m + s.w1 * (g - m));
  v = r(v * s.beta2);
  v = r(v + s.c2 * (g * g));
  float d = r(sqrtf(v));
  d = r(d / s.bc2s);
  d = r(d + s.eps);
  p = r(p + s.step * (m / d));
}

// Global gradient-norm clipping: torch.nn.utils.clip_grad_norm_'s coefficient, clip_coef =
// max_norm / (total_norm + 1e-6) clamped to 1, from the device scalar sq = sum g^2 (IEEE sqrt and
// division: every consumer computes the same bits).  false: sq is inf or NaN -- the consumer does
// nothing and posts the status bit.  The kernels take the scale as a compile-time variant: the
// unclipped instantiation's ClipArgs is empty and its code is what it was before there was a
// variant.
template <bool CLIP>
struct ClipArgs {};
template <>
struct ClipArgs<true> {
  const float* sq;
  float max_norm;
  int* status;
};

__device__ __forceinline__ bool clip_coef(const ClipArgs<true>& c, float& coef) {
  const float sq = c.sq[0];
  if (!(sq <= 3.402823466e+38f)) {
    if (c.status && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(c.status, PT_STATUS_NONFINITE_GRAD);
    return false;
  }
  coef = fminf(1.0f, c.max_norm / (sqrtf(sq) + 1e-6f));
  return true;
}
// the clipped gradient as torch's in-place _foreach_mul_ leaves it: one rounded f32 product (never
// contracted into adam_elem's g - m, which would differ from the stored-and-reloaded f32
// gradient), rounded to the storage dtype
__device__ __forceinline__ float clip_grad(float g, float coef, bool bf) {
#pragma clang fp contract(off)
  const float x = g * coef;
  return bf ? round_bf(x) : x;
}

// fp32 master weights and moments (optim.AdamW(master_weights=True)), the mixed-precision recipe
// on top of the bf16 one above: the optimizer owns an f32 copy of every bf16 weight and both
// moments in f32, updates them with torch's foreach *f32* AdamW sequence (no rounding between the
// ops) and publishes param = bf16(master), round to nearest even.  In bf16 state v * 0.999 rounds
// back to v (1 - beta2 is below half an ulp) and an update below half an ulp of the weight is
// lost; here neither happens.  The gradient is bf16 or f32 (a property of the launch); with
// clipping it is scaled in f32 as it is loaded and never rounded to bf16.
// Traffic per parameter: master, grad, m, v read (14 / 16 B), master, param, m, v written (14 B).
//
// The f32 sequence (adam_elem with bf = false) with its contraction spelled out: a fused
// multiply-add where torch's lerp / addcmul / addcdiv kernels have one, everything else rounded on
// its own.  Nothing is left to the compiler, so the bf16- and the f32-gradient instantiations,
// clipped or not, list or single tensor, are the same arithmetic on the same f32 inputs and give
// the same bits.
__device__ __forceinline__ void adam_elem_master(float& p, float g, float& m, float& v, const AdamScalars& s) {
#pragma clang fp contract(off)
  p = p * s.decay;
  m = fmaf(s.w1, g - m, m);
  v = v * s.beta2;
  v = fmaf(s.c2, g * g, v);
  float d = sqrtf(v);
  d = d / s.bc2s;
  d = d + s.eps;
  p = fmaf(s.step, m / d, p);
}

template <bool CLIP>
__device__ __forceinline__ void master_elem(float& w, float g, float& m, float& v, const AdamScalars& s, float coef) {
  if constexpr (CLIP) g = clip_grad(g, coef, false);
  adam_elem_master(w, g, m, v, s);
}

// 8 x f32 as two 16-byte vectors, non-temporal
typedef float pt_f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) pt_f32x4 pt_g_f32x4;
struct f32x8 { pt_f32x4 lo, hi; };
__device__ __forceinline__ f32x8 ld8f_nt(const float* p) {
  return f32x8{__builtin_nontemporal_load((const pt_g_f32x4*)(p)), __builtin_nontemporal_load((const pt_g_f32x4*)(p + 4))};
}
__device__ __forceinline__ void st8f_nt(float* p, const f32x8& x) {
  __builtin_nontemporal_store(x.lo, (pt_g_f32x4*)(p));
  __builtin_nontemporal_store(x.hi, (pt_g_f32x4*)(p + 4));
}
__device__ __forceinline__ void unpack8(const f32x8& x, float* f) {
#pragma unroll
  for (int j = 0; j < 4; ++j) { f[j] = x.lo[j]; f[4 + j] = x.hi[j]; }
}
__device__ __forceinline__ f32x8 pack8f(const float* f) {
  return f32x8{pt_f32x4{f[0], f[1], f[2], f[3]}, pt_f32x4{f[4], f[5], f[6], f[7]}};
}
// a chunk of the gradient stream in its storage type
template <typename GT> struct GradVec;
template <> struct GradVec<uint16_t> {
  typedef bf16x8 type;
  static __device__ __forceinline__ type ld(const uint16_t* p) { return ld8_nt(p); }
};
template <> struct GradVec<float> {
  typedef f32x8 type;
  static __device__ __forceinline__ type ld(const float* p) { return ld8f_nt(p); }
};

// Stochastic rounding (optim.AdamW(stochastic_rounding=True)): every tensor stays bf16, the update
// is adam_elem_master's f32 sequence on the widened values, and each of the three stores rounds up
// or down with probability equal to the discarded fraction, so E[stored] = the f32 value: updates
// below half an ulp accumulate in expectation and v * 0.999 no longer sticks, at the plain step's
// 14 / 16 B per parameter.
//
// The bits: Philox4x32-10 (Random123's constants), key = the 64-bit seed's halves, counter =
// (c lo, c hi, step, stream << 2 | which) with c = i >> 3 the 8-element chunk of element i INSIDE
// ITS TENSOR, step the parameter's step count (>= 1), stream < 2^30 the parameter's fixed id and
// which = 0 param, 1 exp_avg, 2 exp_avg_sq.  Element i takes the 16 bits
// r = (w[(i & 7) >> 1] >> (16 * (i & 1))) & 0xffff of the call's four words: the two halves of
// word j are the draws of the two elements packed into word j of the chunk's 16-byte store.
// Nothing of the launch (geometry, list order, neighbours, alignment, list or single form) enters.
struct SrArgs {
  uint32_t seed_lo, seed_hi, step;
};
constexpr int SR_PARAM = 0, SR_EXP_AVG = 1, SR_EXP_AVG_SQ = 2;

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&w)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {   // one 32 x 32 -> 64 product per half (v_mad_u64_u32)
    const uint64_t a = (uint64_t)0xD2511F53u * c0, b = (uint64_t)0xCD9E8D57u * c2;
    c0 = (uint32_t)(b >> 32) ^ c1 ^ k0;
    c2 = (uint32_t)(a >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)b;
    c3 = (uint32_t)a;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
// the three calls of chunk c (indexed by `which`)
__device__ __forceinline__ void sr_draw(const SrArgs& k, uint32_t rng_stream, int64_t c, uint32_t (&w)[3][4]) {
#pragma unroll
  for (int which = 0; which < 3; ++which)
    philox4x32_10((uint32_t)c, (uint32_t)((uint64_t)c >> 32), k.step, (rng_stream << 2) | which, k.seed_lo, k.seed_hi,
                  w[which]);
}
__device__ __forceinline__ uint32_t sr_pick(const uint32_t (&w)[4], int j) {   // element j of the chunk
  return (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
}
// sr_bf16(x, r), r in [0, 65536): the 16-bit value (u + r) >> 16 of x's bits u -- a bf16 value
// stays what it is, the magnitude goes up with probability low16 / 65536 exactly, -0 stays -0, and
// a value inside the last bf16 ulp below the largest finite one may become inf.  inf and NaN take
// the plain cast: the integer carry would turn some NaNs into a zero or an infinity.
__device__ __forceinline__ uint32_t sr_bf16(float x, uint32_t r) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x7f800000u) == 0x7f800000u ? (uint32_t)f2bf(x) : (u + r) >> 16;
}
__device__ __forceinline__ bf16x8 sr_pack8(const float* f, const uint32_t (&w)[4]) {
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v.w[j] = sr_bf16(f[2 * j], w[j] & 0xffffu) | (sr_bf16(f[2 * j + 1], w[j] >> 16) << 16);
  return v;
}

// ---- table walk -------------------------------------------------------------------------------
// Multi-tensor form: ONE launch per step over every listed parameter (torch's foreach AdamW works
// on the whole list too).  The tensors are a virtual concatenation of 8-element chunks; workgroup b
// owns a contiguous run of chunks, finds the tensor its run starts in by binary search over the
// chunk prefix sums (read from the caller's descriptor table), then walks forward.  A tensor whose
// length is not a multiple of 8 finishes its last chunk element by element.
struct AdamTensor {   // pt_adam_tensor (include/picotron_hip.h)
  uint16_t* p;
  const uint16_t* g;
  uint16_t* m;
  uint16_t* v;
  int64_t n;
};
struct AdamMasterTensor {   // pt_adam_master_tensor (include/picotron_hip.h)
  float* w;
  uint16_t* p;
  const void* g;
  float* m;
  float* v;
  int64_t n;
};

struct AdamSrTensor {   // pt_adam_sr_tensor (include/picotron_hip.h)
  uint16_t* p;
  const void* g;
  uint16_t* m;
  uint16_t* v;
  int64_t n;
  int64_t stream;   // the parameter's random stream, < 2^30 (the table's builder checks it)
};

// workgroup b's run of chunks, tensor by tensor; fn(T, from, to) gets the run's chunk range inside
// tensor T
template <typename TT, typename F>
__device__ __forceinline__ void for_each_run(const TT* __restrict__ ts, const int64_t* __restrict__ chunk_start,
                                             int nt, int64_t per_block, F fn) {
  const int64_t total = chunk_start[nt];
  const int64_t lo = (int64_t)blockIdx.x * per_block;
  const int64_t hi = lo + per_block < total ? lo + per_block : total;
  if (lo >= hi) return;
  // the tensor holding chunk lo: largest t with chunk_start[t] <= lo
  int a = 0, b = nt - 1;
  while (a < b) {
    const int mid = (a + b + 1) >> 1;
    if (chunk_start[mid] <= lo) a = mid; else b = mid - 1;
  }
  for (int t = a; t < nt && chunk_start[t] < hi; ++t) {
    const int64_t c0 = chunk_start[t], c1 = chunk_start[t + 1];
    fn(ts[t], (lo > c0 ? lo : c0) - c0, (hi < c1 ? hi : c1) - c0);
  }
}

// ---- the step: bf16 / f32 state ---------------------------------------------------------------
// bf16 tensors: 8 elements per thread (16-byte loads / stores on all four streams)
template <bool CLIP>
__global__ __launch_bounds__(256) void adamw_bf16_kernel(uint16_t* __restrict__ param, const uint16_t* __restrict__ grad,
                                                         uint16_t* __restrict__ m, uint16_t* __restrict__ v,
                                                         int64_t n8, AdamScalars s, ClipArgs<CLIP> clip) {
  float coef = 1.0f;
  if constexpr (CLIP) {
    if (!clip_coef(clip, coef)) return;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    float p[8], g[8], a[8], b[8];
    unpack8(ld8(param + i * 8), p);
    unpack8(ld8(grad + i * 8), g);
    unpack8(ld8(m + i * 8), a);
    unpack8(ld8(v + i * 8), b);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if constexpr (CLIP) g[j] = clip_grad(g[j], coef, true);
      adam_elem(p[j], g[j], a[j], b[j], s, true);
    }
    st8(param + i * 8, pack8(p));
    st8(m + i * 8, pack8(a));
    st8(v + i * 8, pack8(b));
  }
}

// scalar tail (n % 8) of a bf16 tensor, and f32 tensors
template <typename T, bool CLIP>
__global__ __launch_bounds__(256) void adamw_scalar_kernel(T* __restrict__ param, const T* __restrict__ grad,
                                                           T* __restrict__ m, T* __restrict__ v, int64_t n,
                                                           AdamScalars s, ClipArgs<CLIP> clip) {
  constexpr bool bf = sizeof(T) == 2;
  float coef = 1.0f;
  if constexpr (CLIP) {
    if (!clip_coef(clip, coef)) return;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float p = ld_as_f(param, i), g = ld_as_f(grad, i), a = ld_as_f(m, i), b = ld_as_f(v, i);
    if constexpr (CLIP) g = clip_grad(g, coef, bf);
    adam_elem(p, g, a, b, s, bf);
    if (bf) {
      ((uint16_t*)param)[i] = f2bf(p);
      ((uint16_t*)m)[i] = f2bf(a);
      ((uint16_t*)v)[i] = f2bf(b);
    } else {
      ((float*)param)[i] = p;
      ((float*)m)[i] = a;
      ((float*)v)[i] = b;
    }
  }
}

// The list of bf16 tensors, one launch.  CLIP: the gradient is scaled by the clip coefficient as it
// is loaded (g' = bf16(g * coef), what an in-place scale pass would have stored).
// The one list kernel that spells the walk of for_each_run out: with its body in for_each_run's
// callback the compiler puts the wait for the two-ahead loads in front of a chunk's arithmetic
// instead of behind it, and the step over 1.21 B parameters takes 2863 us instead of 2819.
template <bool CLIP>
__global__ __launch_bounds__(256) void adamw_multi_bf16_kernel(const AdamTensor* __restrict__ ts,
                                                               const int64_t* __restrict__ chunk_start, int nt,
                                                               int64_t per_block, AdamScalars s,
                                                               ClipArgs<CLIP> clip) {
  float coef = 1.0f;
  if constexpr (CLIP) {
    if (!clip_coef(clip, coef)) return;
  }
  const int64_t total = chunk_start[nt];
  const int64_t lo = (int64_t)blockIdx.x * per_block;
  const int64_t hi = lo + per_block < total ? lo + per_block : total;
  if (lo >= hi) return;
  // the tensor holding chunk lo: largest t with chunk_start[t] <= lo
  int a = 0, b = nt - 1;
  while (a < b) {
    const int mid = (a + b + 1) >> 1;
    if (chunk_start[mid] <= lo) a = mid; else b = mid - 1;
  }
  for (int t = a; t < nt && chunk_start[t] < hi; ++t) {
    const AdamTensor T = ts[t];
    const int64_t c0 = chunk_start[t], c1 = chunk_start[t + 1];
    const int64_t from = (lo > c0 ? lo : c0) - c0, to = (hi < c1 ? hi : c1) - c0;   // chunk range in t
    const int64_t full = T.n >> 3;
    const int64_t end = to < full ? to : full;   // this run's full chunks in tensor t
    // software-pipelined: the loads of a thread's next two chunks are issued before the current
    // chunk's stores, so every wait for a load sits behind loads only -- vmcnt counts stores too,
    // and loads issued after the previous chunk's stores waited out their write latency (5.0 TB/s)
    int64_t c = from + threadIdx.x;
    const int64_t bd = blockDim.x;
    bf16x8 cur[4], nx1[4], nx2[4];
    auto load4 = [&](int64_t cc, bf16x8 (&r)[4]) {
      r[0] = ld8_nt(T.p + cc * 8); r[1] = ld8_nt(T.g + cc * 8); r[2] = ld8_nt(T.m + cc * 8);
      r[3] = ld8_nt(T.v + cc * 8);
    };
    if (c < end) load4(c, cur);
    if (c + bd < end) load4(c + bd, nx1);
    for (; c < end; c += bd) {
      if (c + 2 * bd < end) load4(c + 2 * bd, nx2);
      float p[8], g[8], m[8], v[8];
      unpack8(cur[0], p); unpack8(cur[1], g); unpack8(cur[2], m); unpack8(cur[3], v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if constexpr (CLIP) g[j] = clip_grad(g[j], coef, true);
        adam_elem(p[j], g[j], m[j], v[j], s, true);
      }
      st8_nt(T.p + c * 8, pack8(p));
      st8_nt(T.m + c * 8, pack8(m));
      st8_nt(T.v + c * 8, pack8(v));
#pragma unroll
      for (int q = 0; q < 4; ++q) { cur[q] = nx1[q]; nx1[q] = nx2[q]; }
    }
    for (; c < to; c += blockDim.x) {
      if (c < full) {
        float p[8], g[8], m[8], v[8];
        unpack8(ld8(T.p + c * 8), p);
        unpack8(ld8(T.g + c * 8), g);
        unpack8(ld8(T.m + c * 8), m);
        unpack8(ld8(T.v + c * 8), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if constexpr (CLIP) g[j] = clip_grad(g[j], coef, true);
          adam_elem(p[j], g[j], m[j], v[j], s, true);
        }
        st8(T.p + c * 8, pack8(p));
        st8(T.m + c * 8, pack8(m));
        st8(T.v + c * 8, pack8(v));
      } else {   // the ragged last chunk
        for (int64_t i = c * 8; i < T.n; ++i) {
          float p = bf2f(T.p[i]), g = bf2f(T.g[i]), m = bf2f(T.m[i]), v = bf2f(T.v[i]);
          if constexpr (CLIP) g = clip_grad(g, coef, true);
          adam_elem(p, g, m, v, s, true);
          T.p[i] = f2bf(p);
          T.m[i] = f2bf(m);
          T.v[i] = f2bf(v);
        }
      }
    }
  }
}

// ---- the step: fp32 master weights and moments ------------------------------------------------
// One launch over the list.  Seven or eight 16-byte loads and seven stores per chunk: ONE chunk
// ahead (the bf16 kernel's two would need 3 x 32 data registers and drop the launch below four
// blocks per CU); the next chunk's loads are issued before the current chunk's stores, so a wait
// for a load never sits behind a store.  __launch_bounds__(256, 4): at most 128 VGPRs, the 1024
// blocks of multi_grid are one resident round.
template <typename GT, bool CLIP>
__global__ __launch_bounds__(256, 4) void adamw_master_multi_kernel(const AdamMasterTensor* __restrict__ ts,
                                                                    const int64_t* __restrict__ chunk_start, int nt,
                                                                    int64_t per_block, AdamScalars s,
                                                                    ClipArgs<CLIP> clip) {
  float coef = 1.0f;
  if constexpr (CLIP) {
    if (!clip_coef(clip, coef)) return;
  }
  for_each_run(ts, chunk_start, nt, per_block, [&](const AdamMasterTensor& T, int64_t from, int64_t to) {
    const GT* G = (const GT*)T.g;
    const int64_t full = T.n >> 3;
    const int64_t end = to < full ? to : full;   // this run's full chunks in tensor T
    const int64_t bd = blockDim.x;
    int64_t c = from + threadIdx.x;
    f32x8 cw, cm, cv, nw, nm, nv;
    typename GradVec<GT>::type cg, ng;
    if (c < end) {
      cw = ld8f_nt(T.w + c * 8); cg = GradVec<GT>::ld(G + c * 8); cm = ld8f_nt(T.m + c * 8); cv = ld8f_nt(T.v + c * 8);
    }
    for (; c < end; c += bd) {
      const int64_t n1 = c + bd;
      if (n1 < end) {
        nw = ld8f_nt(T.w + n1 * 8); ng = GradVec<GT>::ld(G + n1 * 8); nm = ld8f_nt(T.m + n1 * 8);
        nv = ld8f_nt(T.v + n1 * 8);
      }
      float w[8], g[8], m[8], v[8];
      unpack8(cw, w); unpack8(cg, g); unpack8(cm, m); unpack8(cv, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) master_elem<CLIP>(w[j], g[j], m[j], v[j], s, coef);
      st8f_nt(T.w + c * 8, pack8f(w));
      st8_nt(T.p + c * 8, pack8(w));
      st8f_nt(T.m + c * 8, pack8f(m));
      st8f_nt(T.v + c * 8, pack8f(v));
      cw = nw; cg = ng; cm = nm; cv = nv;
    }
    if (to > full && threadIdx.x == 0) {   // the ragged last chunk
      for (int64_t i = full * 8; i < T.n; ++i) {
        float w = T.w[i], m = T.m[i], v = T.v[i];
        master_elem<CLIP>(w, ld_as_f(G, i), m, v, s, coef);
        T.w[i] = w;
        T.p[i] = f2bf(w);
        T.m[i] = m;
        T.v[i] = v;
      }
    }
  });
}

// one tensor at any alignment (unaligned views, what the list form refuses): element by element
template <typename GT, bool CLIP>
__global__ __launch_bounds__(256) void adamw_master_scalar_kernel(float* __restrict__ master, uint16_t* __restrict__ param,
                                                                  const GT* __restrict__ grad, float* __restrict__ em,
                                                                  float* __restrict__ ev, int64_t n, AdamScalars s,
                                                                  ClipArgs<CLIP> clip) {
  float coef = 1.0f;
  if constexpr (CLIP) {
    if (!clip_coef(clip, coef)) return;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float w = master[i], m = em[i], v = ev[i];
    master_elem<CLIP>(w, ld_as_f(grad, i), m, v, s, coef);
    master[i] = w;
    param[i] = f2bf(w);
    em[i] = m;
    ev[i] = v;
  }
}

// ---- the step: bf16 state, stochastic rounding ------------------------------------------------
// One chunk of the step in registers: adam_elem_master on the widened values, then the three
// stochastically rounded 16-byte vectors.
template <bool CLIP>
__device__ __forceinline__ void sr_chunk(float* p, float* g, float* m, float* v, const AdamScalars& s, float coef) {
#pragma unroll
  for (int j = 0; j < 8; ++j) master_elem<CLIP>(p[j], g[j], m[j], v[j], s, coef);
}
// elements [i0, i1) of chunk c one by one (the ragged last chunk; a tensor at any alignment)
template <typename GT, bool CLIP>
__device__ __forceinline__ void sr_elems(uint16_t* P, const GT* G, uint16_t* M, uint16_t* V, int64_t c, int64_t i1,
                                         uint32_t rng_stream, const AdamScalars& s, const SrArgs& k, float coef) {
  uint32_t w[3][4];
  sr_draw(k, rng_stream, c, w);
  for (int64_t i = c * 8; i < i1; ++i) {
    const int j = (int)(i & 7);
    float p = bf2f(P[i]), m = bf2f(M[i]), v = bf2f(V[i]);
    master_elem<CLIP>(p, ld_as_f(G, i), m, v, s, coef);
    P[i] = (uint16_t)sr_bf16(p, sr_pick(w[SR_PARAM], j));
    M[i] = (uint16_t)sr_bf16(m, sr_pick(w[SR_EXP_AVG], j));
    V[i] = (uint16_t)sr_bf16(v, sr_pick(w[SR_EXP_AVG_SQ], j));
  }
}

// One launch over the list, bf16 or f32 gradients.  The loads of a thread's next two chunks are in
// flight while the current one is computed, as in the bf16 list kernel (three or four 16-byte loads
// and three stores per chunk); the chunk's three Philox calls depend on nothing that is loaded.
template <typename GT, bool CLIP>
__global__ __launch_bounds__(256, 4) void adamw_sr_multi_kernel(const AdamSrTensor* __restrict__ ts,
                                                                const int64_t* __restrict__ chunk_start, int nt,
                                                                int64_t per_block, AdamScalars s, SrArgs k,
                                                                ClipArgs<CLIP> clip) {
  float coef = 1.0f;
  if constexpr (CLIP) {
    if (!clip_coef(clip, coef)) return;
  }
  for_each_run(ts, chunk_start, nt, per_block, [&](const AdamSrTensor& T, int64_t from, int64_t to) {
    const GT* G = (const GT*)T.g;
    const uint32_t rs = (uint32_t)T.stream;
    const int64_t full = T.n >> 3;
    const int64_t end = to < full ? to : full;   // this run's full chunks in tensor T
    const int64_t bd = blockDim.x;
    int64_t c = from + threadIdx.x;
    struct In {
      bf16x8 p, m, v;
      typename GradVec<GT>::type g;
    } cur, nx1, nx2;
    auto load = [&](int64_t cc, In& r) {
      r.p = ld8_nt(T.p + cc * 8); r.g = GradVec<GT>::ld(G + cc * 8); r.m = ld8_nt(T.m + cc * 8);
      r.v = ld8_nt(T.v + cc * 8);
    };
    if (c < end) load(c, cur);
    if (c + bd < end) load(c + bd, nx1);
    for (; c < end; c += bd) {
      if (c + 2 * bd < end) load(c + 2 * bd, nx2);
      uint32_t w[3][4];
      sr_draw(k, rs, c, w);
      float p[8], g[8], m[8], v[8];
      unpack8(cur.p, p); unpack8(cur.g, g); unpack8(cur.m, m); unpack8(cur.v, v);
      sr_chunk<CLIP>(p, g, m, v, s, coef);
      st8_nt(T.p + c * 8, sr_pack8(p, w[SR_PARAM]));
      st8_nt(T.m + c * 8, sr_pack8(m, w[SR_EXP_AVG]));
      st8_nt(T.v + c * 8, sr_pack8(v, w[SR_EXP_AVG_SQ]));
      cur = nx1; nx1 = nx2;
    }
    if (to > full && threadIdx.x == 0)   // the ragged last chunk
      sr_elems<GT, CLIP>(T.p, G, T.m, T.v, full, T.n, rs, s, k, coef);
  });
}

// one tensor at any alignment: a thread takes a chunk element by element, the same bits as the list
template <typename GT, bool CLIP>
__global__ __launch_bounds__(256) void adamw_sr_scalar_kernel(uint16_t* __restrict__ param, const GT* __restrict__ grad,
                                                              uint16_t* __restrict__ em, uint16_t* __restrict__ ev,
                                                              int64_t n, uint32_t rng_stream, AdamScalars s, SrArgs k,
                                                              ClipArgs<CLIP> clip) {
  float coef = 1.0f;
  if constexpr (CLIP) {
    if (!clip_coef(clip, coef)) return;
  }
  const int64_t chunks = (n + 7) >> 3;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i1 = c * 8 + 8 < n ? c * 8 + 8 : n;
    sr_elems<GT, CLIP>(param, grad, em, ev, c, i1, rng_stream, s, k, coef);
  }
}

// the rounding alone: y[i] = sr_bf16(x[i], the draw of element i for output `which`)
__global__ __launch_bounds__(256) void sr_cast_kernel(const float* __restrict__ x, uint16_t* __restrict__ y, int64_t n,
                                                      uint32_t rng_stream, uint32_t which, SrArgs k) {
  const int64_t chunks = (n + 7) >> 3;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * blockDim.x) {
    uint32_t w[4];
    philox4x32_10((uint32_t)c, (uint32_t)((uint64_t)c >> 32), k.step, (rng_stream << 2) | which, k.seed_lo, k.seed_hi, w);
    const int64_t i1 = c * 8 + 8 < n ? c * 8 + 8 : n;
    for (int64_t i = c * 8; i < i1; ++i) y[i] = (uint16_t)sr_bf16(x[i], sr_pick(w, (int)(i & 7)));
  }
}

// ---- sum of squares of the gradients (the global norm) and the in-place scale ---------------
// Both walk a table the way the step does and touch only its grad field.
template <typename V>
__device__ __forceinline__ float sq8(const V& x, float acc) {
  float g[8];
  unpack8(x, g);
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = fmaf(g[j], g[j], acc);
  return acc;
}

// the workgroup's sum in a fixed order (wave butterfly, then the four waves in index order):
// thread 0 returns it
__device__ __forceinline__ float block_sum_256(float v) {
  __shared__ float part[4];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((part[0] + part[1]) + part[2]) + part[3];
}

// One f32 partial per workgroup: partial[b] = sum g^2 over workgroup b's run of table TT, whose
// gradients are stored as GT.  Nothing is stored on the way, so four chunks per thread are simply
// loaded together and summed into four independent accumulators (a thread's longest add chain:
// 8 * ceil(chunks per thread / 4)).
template <typename TT, typename GT>
__global__ __launch_bounds__(256) void grad_sq_list_kernel(const TT* __restrict__ ts,
                                                           const int64_t* __restrict__ chunk_start, int nt,
                                                           int64_t per_block, float* __restrict__ partial) {
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for_each_run(ts, chunk_start, nt, per_block, [&](const TT& T, int64_t from, int64_t to) {
    const GT* G = (const GT*)T.g;
    const int64_t full = T.n >> 3;
    const int64_t end = to < full ? to : full;
    const int64_t bd = blockDim.x;
    int64_t c = from + threadIdx.x;
    for (; c + 3 * bd < end; c += 4 * bd) {
      typename GradVec<GT>::type x[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) x[q] = GradVec<GT>::ld(G + (c + q * bd) * 8);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = sq8(x[q], acc[q]);
    }
    for (int q = 0; c < end; c += bd, ++q) acc[q & 3] = sq8(GradVec<GT>::ld(G + c * 8), acc[q & 3]);
    if (to > full && threadIdx.x == 0) {   // the ragged last chunk
      for (int64_t i = full * 8; i < T.n; ++i) {
        const float g = ld_as_f(G, i);
        acc[3] = fmaf(g, g, acc[3]);
      }
    }
  });
  const float sum = block_sum_256((acc[0] + acc[1]) + (acc[2] + acc[3]));
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// single tensor (f32, or bf16 at any alignment): element by element, grid-strided
template <typename T>
__global__ __launch_bounds__(256) void grad_sq_kernel(const T* __restrict__ grad, int64_t n,
                                                      float* __restrict__ partial) {
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {
    float g[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q] = ld_as_f(grad, i + q * stride);
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = fmaf(g[q], g[q], acc[q]);
  }
  for (int q = 0; i < n; i += stride, ++q) {
    const float g = ld_as_f(grad, i);
    acc[q & 3] = fmaf(g, g, acc[q & 3]);
  }
  const float sum = block_sum_256((acc[0] + acc[1]) + (acc[2] + acc[3]));
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// sq[0] = (accumulate ? sq[0] : 0) + weight * sum of the n partials, one workgroup, fixed order
// (thread t takes partials t, t + 256, ... in index order): bit-reproducible, no float atomics
__global__ __launch_bounds__(256) void grad_sq_final_kernel(const float* __restrict__ partial, int n, float weight,
                                                            int accumulate, float* __restrict__ sq) {
  float acc = 0.0f;
  for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
  const float sum = block_sum_256(acc);
  if (threadIdx.x == 0) sq[0] = accumulate ? sq[0] + weight * sum : weight * sum;
}

// grad = bf16(grad * coef) in place over the list (the stand-alone clip_grad_norm_); coef == 1
// (no clipping) stores nothing
__global__ __launch_bounds__(256) void grad_scale_multi_kernel(const AdamTensor* __restrict__ ts,
                                                               const int64_t* __restrict__ chunk_start, int nt,
                                                               int64_t per_block, ClipArgs<true> clip) {
  float coef;
  if (!clip_coef(clip, coef) || coef == 1.0f) return;
  for_each_run(ts, chunk_start, nt, per_block, [&](const AdamTensor& T, int64_t from, int64_t to) {
    uint16_t* G = const_cast<uint16_t*>(T.g);
    const int64_t full = T.n >> 3;
    const int64_t end = to < full ? to : full;
    for (int64_t c = from + threadIdx.x; c < end; c += blockDim.x) {
      float g[8];
      unpack8(ld8_nt(G + c * 8), g);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = clip_grad(g[j], coef, false);   // pack8 rounds
      st8_nt(G + c * 8, pack8(g));
    }
    if (to > full && threadIdx.x == 0) {
      for (int64_t i = full * 8; i < T.n; ++i) G[i] = f2bf(clip_grad(bf2f(G[i]), coef, false));
    }
  });
}

template <typename T>
__global__ __launch_bounds__(256) void grad_scale_kernel(T* __restrict__ grad, int64_t n, ClipArgs<true> clip) {
  float coef;
  if (!clip_coef(clip, coef) || coef == 1.0f) return;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float g = clip_grad(ld_as_f(grad, i), coef, false);
    if (sizeof(T) == 2) ((uint16_t*)grad)[i] = f2bf(g); else ((float*)grad)[i] = g;
  }
}

// ---- host launch helpers ----------------------------------------------------------------------
int grid_for(int64_t work) {
  int64_t g = (work + 255) / 256;
  return (int)(g < PT_STREAM_GRID_CAP ? (g < 1 ? 1 : g) : PT_STREAM_GRID_CAP);
}

// the multi-tensor launches' geometry: one resident round, 4 blocks of 4 waves per CU at <= 128
// VGPRs (2 chunks per thread in flight)
struct MultiGrid {
  unsigned blocks;
  int64_t per_block;
};
MultiGrid multi_grid(int64_t total_chunks, int64_t cap = 1024) {
  const int64_t want = (total_chunks + 511) / 512;
  const int64_t blocks = want < 1 ? 1 : (want < cap ? want : cap);
  return {(unsigned)blocks, (total_chunks + blocks - 1) / blocks};
}
// the norm pass and the scale only read / write 2 bytes per parameter at few VGPRs: 8 blocks per CU
constexpr int PT_GRAD_SQ_BLOCKS = PT_STREAM_GRID_CAP;

// The argument checks every entry shares.  An entry refuses (PT_EINVAL) before it looks at whether
// there is anything to do: total_chunks == 0 / n == 0 is PT_OK only with valid arguments.
bool list_ok(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks) {
  return tensors && chunk_start && ntensors > 0 && total_chunks >= 0;
}
bool dtype_ok(int dtype) { return dtype == 0 || dtype == 1; }   // bf16, f32
bool clip_ok(const ClipArgs<false>&) { return true; }
bool clip_ok(const ClipArgs<true>& c) { return c.sq && c.max_norm > 0.0f; }   // NaN is refused

// the bf16 / f32-state step, one body for the clipped and the unclipped entry point
template <bool CLIP>
int step_multi(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
               const AdamScalars& s, const ClipArgs<CLIP>& clip, hipStream_t stream) {
  if (!list_ok(tensors, chunk_start, ntensors, total_chunks) || !clip_ok(clip)) return PT_EINVAL;
  if (total_chunks == 0) return PT_OK;
  const MultiGrid g = multi_grid(total_chunks);
  adamw_multi_bf16_kernel<CLIP><<<g.blocks, 256, 0, stream>>>((const AdamTensor*)tensors, chunk_start, ntensors,
                                                              g.per_block, s, clip);
  PT_CHECK_LAUNCH();
  return PT_OK;
}
template <bool CLIP>
int step_single(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, int dtype,
                const AdamScalars& s, const ClipArgs<CLIP>& clip, hipStream_t stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || n < 0 || !dtype_ok(dtype) || !clip_ok(clip)) return PT_EINVAL;
  if (n == 0) return PT_OK;
  if (dtype == 1) {  // f32
    adamw_scalar_kernel<float, CLIP><<<grid_for(n), 256, 0, stream>>>((float*)param, (const float*)grad,
                                                                      (float*)exp_avg, (float*)exp_avg_sq, n, s, clip);
    PT_CHECK_LAUNCH();
    return PT_OK;
  }
  // bf16: the 16-byte vector kernel, then the scalar kernel on the n % 8 tail -- or on the whole
  // tensor when any pointer is unaligned
  auto* P = (uint16_t*)param;
  auto* G = (const uint16_t*)grad;
  auto* M = (uint16_t*)exp_avg;
  auto* V = (uint16_t*)exp_avg_sq;
  const bool vec = pt_aligned16(P) && pt_aligned16(G) && pt_aligned16(M) && pt_aligned16(V);
  const int64_t n8 = vec ? n / 8 : 0;
  if (n8) {
    adamw_bf16_kernel<CLIP><<<grid_for(n8), 256, 0, stream>>>(P, G, M, V, n8, s, clip);
    PT_CHECK_LAUNCH();
  }
  const int64_t done = n8 * 8;
  if (done < n) {
    adamw_scalar_kernel<uint16_t, CLIP><<<grid_for(n - done), 256, 0, stream>>>(P + done, G + done, M + done,
                                                                                V + done, n - done, s, clip);
    PT_CHECK_LAUNCH();
  }
  return PT_OK;
}

// the master-weight step, likewise
template <bool CLIP>
int master_multi(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks, int grad_dtype,
                 const AdamScalars& s, const ClipArgs<CLIP>& clip, hipStream_t stream) {
  if (!list_ok(tensors, chunk_start, ntensors, total_chunks) || !dtype_ok(grad_dtype) || !clip_ok(clip))
    return PT_EINVAL;
  if (total_chunks == 0) return PT_OK;
  const MultiGrid g = multi_grid(total_chunks);
  const auto* ts = (const AdamMasterTensor*)tensors;
  if (grad_dtype == 0)
    adamw_master_multi_kernel<uint16_t, CLIP><<<g.blocks, 256, 0, stream>>>(ts, chunk_start, ntensors, g.per_block, s, clip);
  else
    adamw_master_multi_kernel<float, CLIP><<<g.blocks, 256, 0, stream>>>(ts, chunk_start, ntensors, g.per_block, s, clip);
  PT_CHECK_LAUNCH();
  return PT_OK;
}
template <bool CLIP>
int master_single(float* master, void* param, const void* grad, float* m, float* v, int64_t n, int grad_dtype,
                  const AdamScalars& s, const ClipArgs<CLIP>& clip, hipStream_t stream) {
  if (!master || !param || !grad || !m || !v || n < 0 || !dtype_ok(grad_dtype) || !clip_ok(clip)) return PT_EINVAL;
  if (n == 0) return PT_OK;
  if (grad_dtype == 0)
    adamw_master_scalar_kernel<uint16_t, CLIP><<<grid_for(n), 256, 0, stream>>>(master, (uint16_t*)param,
                                                                                (const uint16_t*)grad, m, v, n, s, clip);
  else
    adamw_master_scalar_kernel<float, CLIP><<<grid_for(n), 256, 0, stream>>>(master, (uint16_t*)param,
                                                                             (const float*)grad, m, v, n, s, clip);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

// the stochastic-rounding step, likewise.  step >= 1; a stream id is below 2^30 (the list's ids sit
// in the caller's table and are checked where it is built)
bool sr_stream_ok(int64_t rng_stream) { return rng_stream >= 0 && rng_stream < ((int64_t)1 << 30); }
template <bool CLIP>
int sr_multi(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks, int grad_dtype,
             const AdamScalars& s, const SrArgs& k, const ClipArgs<CLIP>& clip, hipStream_t stream) {
  if (!list_ok(tensors, chunk_start, ntensors, total_chunks) || !dtype_ok(grad_dtype) || k.step == 0 || !clip_ok(clip))
    return PT_EINVAL;
  if (total_chunks == 0) return PT_OK;
  const MultiGrid g = multi_grid(total_chunks);
  const auto* ts = (const AdamSrTensor*)tensors;
  if (grad_dtype == 0)
    adamw_sr_multi_kernel<uint16_t, CLIP><<<g.blocks, 256, 0, stream>>>(ts, chunk_start, ntensors, g.per_block, s, k, clip);
  else
    adamw_sr_multi_kernel<float, CLIP><<<g.blocks, 256, 0, stream>>>(ts, chunk_start, ntensors, g.per_block, s, k, clip);
  PT_CHECK_LAUNCH();
  return PT_OK;
}
template <bool CLIP>
int sr_single(void* param, const void* grad, void* m, void* v, int64_t n, int grad_dtype, const AdamScalars& s,
              const SrArgs& k, int64_t rng_stream, const ClipArgs<CLIP>& clip, hipStream_t stream) {
  if (!param || !grad || !m || !v || n < 0 || !dtype_ok(grad_dtype) || k.step == 0 || !sr_stream_ok(rng_stream) ||
      !clip_ok(clip))
    return PT_EINVAL;
  if (n == 0) return PT_OK;
  const int grid = grid_for((n + 7) / 8);
  if (grad_dtype == 0)
    adamw_sr_scalar_kernel<uint16_t, CLIP><<<grid, 256, 0, stream>>>((uint16_t*)param, (const uint16_t*)grad, (uint16_t*)m,
                                                                     (uint16_t*)v, n, (uint32_t)rng_stream, s, k, clip);
  else
    adamw_sr_scalar_kernel<float, CLIP><<<grid, 256, 0, stream>>>((uint16_t*)param, (const float*)grad, (uint16_t*)m,
                                                                  (uint16_t*)v, n, (uint32_t)rng_stream, s, k, clip);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

// The sum of squares' two launches: `partials` puts one f32 per workgroup into workspace[0, blocks),
// then one workgroup sums them in a fixed order.  blocks == 0 (nothing to sum): no partials launch,
// and the final kernel still writes or keeps sq according to `accumulate`.
template <typename L>
int grad_sq_sum(unsigned blocks, L partials, float weight, int accumulate, float* workspace, float* sq,
                hipStream_t stream) {
  if (blocks) {
    partials();
    PT_CHECK_LAUNCH();
  }
  grad_sq_final_kernel<<<1, 256, 0, stream>>>(workspace, (int)blocks, weight, accumulate, sq);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

}  // namespace

extern "C" {

// ---- ABI forwards (include/picotron_hip.h) -----------------------------------------------------
// One tensor, dtype 0 bf16 / 1 f32, any alignment.  Any other dtype is PT_EINVAL, at n == 0 too.
int pt_adamw_step(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, int dtype,
                  float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps, float step_size,
                  hipStream_t stream) {
  return step_single<false>(param, grad, exp_avg, exp_avg_sq, n, dtype,
                            AdamScalars{decay, w1, beta2, c2, bc2_sqrt, eps, step_size}, {}, stream);
}

int pt_adamw_step_clip(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, int dtype,
                       float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps, float step_size,
                       const float* grad_sq, float max_norm, int* status, hipStream_t stream) {
  return step_single<true>(param, grad, exp_avg, exp_avg_sq, n, dtype,
                           AdamScalars{decay, w1, beta2, c2, bc2_sqrt, eps, step_size},
                           ClipArgs<true>{grad_sq, max_norm, status}, stream);
}

// bf16 tensors (every pointer 16-byte aligned), one launch.  tensors: device array of ntensors
// pt_adam_tensor; chunk_start: device int64 [ntensors + 1], chunk_start[i] = sum over j < i of
// ceil(n_j / 8) -- both built (and cached) by the caller.  total_chunks = chunk_start[ntensors].
int pt_adamw_step_multi(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                        float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps, float step_size,
                        hipStream_t stream) {
  return step_multi<false>(tensors, chunk_start, ntensors, total_chunks,
                           AdamScalars{decay, w1, beta2, c2, bc2_sqrt, eps, step_size}, {}, stream);
}

int pt_adamw_step_multi_clip(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                             float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps,
                             float step_size, const float* grad_sq, float max_norm, int* status,
                             hipStream_t stream) {
  return step_multi<true>(tensors, chunk_start, ntensors, total_chunks,
                          AdamScalars{decay, w1, beta2, c2, bc2_sqrt, eps, step_size},
                          ClipArgs<true>{grad_sq, max_norm, status}, stream);
}

int pt_adamw_master_step_multi(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                               int grad_dtype, float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps,
                               float step_size, hipStream_t stream) {
  return master_multi<false>(tensors, chunk_start, ntensors, total_chunks, grad_dtype,
                             AdamScalars{decay, w1, beta2, c2, bc2_sqrt, eps, step_size}, {}, stream);
}

int pt_adamw_master_step_multi_clip(const void* tensors, const int64_t* chunk_start, int ntensors,
                                    int64_t total_chunks, int grad_dtype, float decay, float w1, float beta2, float c2,
                                    float bc2_sqrt, float eps, float step_size, const float* grad_sq, float max_norm,
                                    int* status, hipStream_t stream) {
  return master_multi<true>(tensors, chunk_start, ntensors, total_chunks, grad_dtype,
                            AdamScalars{decay, w1, beta2, c2, bc2_sqrt, eps, step_size},
                            ClipArgs<true>{grad_sq, max_norm, status}, stream);
}

int pt_adamw_master_step(float* master, void* param, const void* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                         int grad_dtype, float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps,
                         float step_size, hipStream_t stream) {
  return master_single<false>(master, param, grad, exp_avg, exp_avg_sq, n, grad_dtype,
                              AdamScalars{decay, w1, beta2, c2, bc2_sqrt, eps, step_size}, {}, stream);
}

int pt_adamw_master_step_clip(float* master, void* param, const void* grad, float* exp_avg, float* exp_avg_sq,
                              int64_t n, int grad_dtype, float decay, float w1, float beta2, float c2, float bc2_sqrt,
                              float eps, float step_size, const float* grad_sq, float max_norm, int* status,
                              hipStream_t stream) {
  return master_single<true>(master, param, grad, exp_avg, exp_avg_sq, n, grad_dtype,
                             AdamScalars{decay, w1, beta2, c2, bc2_sqrt, eps, step_size},
                             ClipArgs<true>{grad_sq, max_norm, status}, stream);
}

// bf16 state with stochastic rounding.  tensors: device array of ntensors pt_adam_sr_tensor (every
// pointer 16-byte aligned, the gradients of one dtype: grad_dtype 0 bf16 / 1 f32).
int pt_adamw_sr_step_multi(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                           int grad_dtype, float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps,
                           float step_size, uint32_t seed_lo, uint32_t seed_hi, uint32_t step, hipStream_t stream) {
  return sr_multi<false>(tensors, chunk_start, ntensors, total_chunks, grad_dtype,
                         AdamScalars{decay, w1, beta2, c2, bc2_sqrt, eps, step_size}, SrArgs{seed_lo, seed_hi, step}, {},
                         stream);
}

int pt_adamw_sr_step_multi_clip(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                                int grad_dtype, float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps,
                                float step_size, uint32_t seed_lo, uint32_t seed_hi, uint32_t step, const float* grad_sq,
                                float max_norm, int* status, hipStream_t stream) {
  return sr_multi<true>(tensors, chunk_start, ntensors, total_chunks, grad_dtype,
                        AdamScalars{decay, w1, beta2, c2, bc2_sqrt, eps, step_size}, SrArgs{seed_lo, seed_hi, step},
                        ClipArgs<true>{grad_sq, max_norm, status}, stream);
}

int pt_adamw_sr_step(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, int grad_dtype,
                     float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps, float step_size,
                     uint32_t seed_lo, uint32_t seed_hi, uint32_t step, int64_t rng_stream, hipStream_t stream) {
  return sr_single<false>(param, grad, exp_avg, exp_avg_sq, n, grad_dtype,
                          AdamScalars{decay, w1, beta2, c2, bc2_sqrt, eps, step_size}, SrArgs{seed_lo, seed_hi, step},
                          rng_stream, {}, stream);
}

int pt_adamw_sr_step_clip(void* param, const void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, int grad_dtype,
                          float decay, float w1, float beta2, float c2, float bc2_sqrt, float eps, float step_size,
                          uint32_t seed_lo, uint32_t seed_hi, uint32_t step, int64_t rng_stream, const float* grad_sq,
                          float max_norm, int* status, hipStream_t stream) {
  return sr_single<true>(param, grad, exp_avg, exp_avg_sq, n, grad_dtype,
                         AdamScalars{decay, w1, beta2, c2, bc2_sqrt, eps, step_size}, SrArgs{seed_lo, seed_hi, step},
                         rng_stream, ClipArgs<true>{grad_sq, max_norm, status}, stream);
}

// y = sr_bf16(x) with the draws of (seed, rng_stream, step, which): the rounding on its own, any alignment
int pt_sr_cast_bf16(const float* x, void* y, int64_t n, uint32_t seed_lo, uint32_t seed_hi, uint32_t step,
                    int64_t rng_stream, int which, hipStream_t stream) {
  if (!x || !y || n < 0 || step == 0 || !sr_stream_ok(rng_stream) || which < 0 || which > 2) return PT_EINVAL;
  if (n == 0) return PT_OK;
  sr_cast_kernel<<<grid_for((n + 7) / 8), 256, 0, stream>>>(x, (uint16_t*)y, n, (uint32_t)rng_stream, (uint32_t)which,
                                                            SrArgs{seed_lo, seed_hi, step});
  PT_CHECK_LAUNCH();
  return PT_OK;
}

// global gradient-norm clipping: the sum of squares ...
int pt_grad_sq_workspace(void) { return PT_GRAD_SQ_BLOCKS; }

int pt_grad_sq_multi(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                     float weight, int accumulate, float* workspace, float* sq, hipStream_t stream) {
  if (!list_ok(tensors, chunk_start, ntensors, total_chunks) || !workspace || !sq) return PT_EINVAL;
  const MultiGrid g = multi_grid(total_chunks, PT_GRAD_SQ_BLOCKS);
  return grad_sq_sum(total_chunks ? g.blocks : 0, [&] {
    grad_sq_list_kernel<AdamTensor, uint16_t><<<g.blocks, 256, 0, stream>>>((const AdamTensor*)tensors, chunk_start,
                                                                            ntensors, g.per_block, workspace);
  }, weight, accumulate, workspace, sq, stream);
}

int pt_grad_sq_master_multi(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                            int grad_dtype, float weight, int accumulate, float* workspace, float* sq,
                            hipStream_t stream) {
  if (!list_ok(tensors, chunk_start, ntensors, total_chunks) || !workspace || !sq || !dtype_ok(grad_dtype))
    return PT_EINVAL;
  const MultiGrid g = multi_grid(total_chunks, PT_GRAD_SQ_BLOCKS);
  const auto* ts = (const AdamMasterTensor*)tensors;
  return grad_sq_sum(total_chunks ? g.blocks : 0, [&] {
    if (grad_dtype == 0)
      grad_sq_list_kernel<AdamMasterTensor, uint16_t><<<g.blocks, 256, 0, stream>>>(ts, chunk_start, ntensors, g.per_block, workspace);
    else
      grad_sq_list_kernel<AdamMasterTensor, float><<<g.blocks, 256, 0, stream>>>(ts, chunk_start, ntensors, g.per_block, workspace);
  }, weight, accumulate, workspace, sq, stream);
}

int pt_grad_sq_sr_multi(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                        int grad_dtype, float weight, int accumulate, float* workspace, float* sq, hipStream_t stream) {
  if (!list_ok(tensors, chunk_start, ntensors, total_chunks) || !workspace || !sq || !dtype_ok(grad_dtype))
    return PT_EINVAL;
  const MultiGrid g = multi_grid(total_chunks, PT_GRAD_SQ_BLOCKS);
  const auto* ts = (const AdamSrTensor*)tensors;
  return grad_sq_sum(total_chunks ? g.blocks : 0, [&] {
    if (grad_dtype == 0)
      grad_sq_list_kernel<AdamSrTensor, uint16_t><<<g.blocks, 256, 0, stream>>>(ts, chunk_start, ntensors, g.per_block, workspace);
    else
      grad_sq_list_kernel<AdamSrTensor, float><<<g.blocks, 256, 0, stream>>>(ts, chunk_start, ntensors, g.per_block, workspace);
  }, weight, accumulate, workspace, sq, stream);
}

int pt_grad_sq(const void* grad, int64_t n, int dtype, float weight, int accumulate, float* workspace, float* sq,
               hipStream_t stream) {
  if (!grad || n < 0 || !workspace || !sq || !dtype_ok(dtype)) return PT_EINVAL;
  const unsigned blocks = n ? grid_for(n) : 0;
  return grad_sq_sum(blocks, [&] {
    if (dtype == 0) grad_sq_kernel<uint16_t><<<blocks, 256, 0, stream>>>((const uint16_t*)grad, n, workspace);
    else grad_sq_kernel<float><<<blocks, 256, 0, stream>>>((const float*)grad, n, workspace);
  }, weight, accumulate, workspace, sq, stream);
}

// ... and the in-place scale
int pt_grad_scale_multi(const void* tensors, const int64_t* chunk_start, int ntensors, int64_t total_chunks,
                        const float* grad_sq, float max_norm, int* status, hipStream_t stream) {
  const ClipArgs<true> clip{grad_sq, max_norm, status};
  if (!list_ok(tensors, chunk_start, ntensors, total_chunks) || !clip_ok(clip)) return PT_EINVAL;
  if (total_chunks == 0) return PT_OK;
  const MultiGrid g = multi_grid(total_chunks, PT_GRAD_SQ_BLOCKS);
  grad_scale_multi_kernel<<<g.blocks, 256, 0, stream>>>((const AdamTensor*)tensors, chunk_start, ntensors,
                                                        g.per_block, clip);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

int pt_grad_scale(void* grad, int64_t n, int dtype, const float* grad_sq, float max_norm, int* status,
                  hipStream_t stream) {
  const ClipArgs<true> clip{grad_sq, max_norm, status};
  if (!grad || n < 0 || !dtype_ok(dtype) || !clip_ok(clip)) return PT_EINVAL;
  if (n == 0) return PT_OK;
  if (dtype == 0) grad_scale_kernel<uint16_t><<<grid_for(n), 256, 0, stream>>>((uint16_t*)grad, n, clip);
  else grad_scale_kernel<float><<<grid_for(n), 256, 0, stream>>>((float*)grad, n, clip);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

}  // extern "C"
