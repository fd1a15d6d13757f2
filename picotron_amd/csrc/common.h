// Shared device helpers for the picotron_amd gfx950 (CDNA4 / MI355X) kernels.
//
// Everything in csrc/ is plain HIP written for gfx950 only: 64-lane wavefronts,
// MFMA bf16 tiles, LDS staging.  Host entry points are `extern "C"` and take
// plain device pointers, sizes and a hipStream_t (see include/picotron_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PT_WAVE 64

// The C ABI (and the PT_* error codes: 0 ok, negative = argument error found before launch,
// positive = hipError_t of the launch).  Included here so every definition is checked against it.
#include "../../include/picotron_hip.h"

// measurement variants (pt_set_variant, csrc/variants.hip): read by the launchers, never the kernels
enum PtVariant { PT_VAR_ATTN_PAIR = 0, PT_VAR_ATTN_SPLIT, PT_VAR_GEMM_MIX, PT_VAR_GEMM_KH,
                 PT_VAR_ATTN_KV_CHUNK, PT_VAR_COUNT };
int pt_variant(PtVariant v);

#define PT_CHECK_LAUNCH()                          \
  do {                                             \
    hipError_t _e = hipGetLastError();             \
    if (_e != hipSuccess) return (int)_e;          \
  } while (0)

// ---- bf16 <-> f32 -----------------------------------------------------------
// bf16 is carried as raw uint16 bits.  f32->bf16 is round-to-nearest-even via
// the native __bf16 cast (hipcc emits v_cvt_pk_bf16_f32, NaN-preserving).
__device__ __forceinline__ float bf2f(uint16_t u) { return __uint_as_float((uint32_t)u << 16); }
__device__ __forceinline__ uint16_t f2bf(float f) {
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(uint16_t, b);
}
// round an f32 through bf16 and back (models a bf16 storage round trip)
__device__ __forceinline__ float round_bf(float f) { return bf2f(f2bf(f)); }
// sigmoid(x) = 1 / (1 + e^-x) with the hardware reciprocal (v_rcp_f32, 1 ulp) instead of the IEEE
// division sequence (v_div_scale / fmas / fixup, ~10 instructions): every SwiGLU kernel uses this
// one expression, so the fused epilogues and csrc/swiglu.hip stay bit-identical
__device__ __forceinline__ float pt_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

// The gate activation of a gated MLP and its derivative, one element: the ONE definition the row kernels
// (csrc/swiglu.hip) and the GEMM epilogues (csrc/gemm.hip) share, so fused and unfused give the same bits.
//   PT_ACT_SILU:       act = g s,  s = sigmoid(g),  act' = s (1 + g (1 - s))
//   PT_ACT_GELU_TANH:  gelu(g) = 0.5 g (1 + tanh(k (g + c g^3))), k = sqrt(2 / pi), c = 0.044715, written
//     with tanh(x) = 2 sigmoid(2 x) - 1 as  z = 2 k g (1 + c g^2),  s = sigmoid(z),  act = g s,
//     act' = s + g s (1 - s) z',  z' = 2 k (1 + 3 c g^2):  one pt_sigmoid (v_exp + v_rcp) as SiLU has,
//     no libm tanhf.
// g^2 is clamped at 2^100: a finite bf16 |g| > 1.8e19 overflows g g to inf, and z' = inf meets
// s (1 - s) = 0 as NaN (torch's gelu_backward has the same hole).  The sigmoid saturates to exactly 0 / 1
// from |z| ~ 104, i.e. |g| ~ 11, so where the clamp binds (|g| >= 2^50) g s (1 - s) is exactly +-0 and
// finite z' gives act' = s; below it the min returns g g itself, so no value on the common path changes.
// One v_min_f32 per element, no compare / select pair and no branch.
enum PtAct { PT_ACT_SILU = 0, PT_ACT_GELU_TANH = 1 };
template <int ACT>
struct PtGlu {
  float s, g2;   // the sigmoid the activation is written with; (clamped) g^2 of the GELU polynomial
  __device__ __forceinline__ explicit PtGlu(float g) {
    constexpr float k2 = 1.5957691216057308f, c = 0.044715f;   // 2 sqrt(2 / pi)
    if constexpr (ACT == PT_ACT_SILU) {
      s = pt_sigmoid(g);
    } else {
      g2 = fminf(g * g, 0x1p100f);
      s = pt_sigmoid(g * fmaf(k2 * c, g2, k2));
    }
  }
  __device__ __forceinline__ float act(float g) const { return g * s; }
  // a = act(g), the f32 value before any rounding
  __device__ __forceinline__ float dact(float g, float a) const {
    constexpr float k2 = 1.5957691216057308f, c = 0.044715f;
    if constexpr (ACT == PT_ACT_SILU) return s * (1.0f + g * (1.0f - s));
    else return fmaf(a * (1.0f - s), fmaf(3.0f * k2 * c, g2, k2), s);
  }
};
template <int ACT>
__device__ __forceinline__ float pt_glu_act(float g) { return PtGlu<ACT>(g).act(g); }
// one element of the gated MLP's backward with torch's bf16 rounding points: d = dh (already a bf16 value),
// g / u the forward's activations -> og = dg = bf16(dh u) act'(g), ou = du = dh bf16(act(g)) (stored as bf16)
template <int ACT>
__device__ __forceinline__ void pt_glu_bwd_elem(float d, float g, float u, float& og, float& ou) {
  const PtGlu<ACT> f(g);
  const float a = f.act(g);
  ou = d * round_bf(a);
  og = round_bf(d * u) * f.dact(g, a);
}

// Final-logit soft-capping (Gemma-2's final_logit_softcapping): t = c tanh(x / c), written as
// csrc/attention.hip's soft-cap stage writes it -- e = exp2(x k1) = exp(2 x / c), tanh = 1 - 2 rcp(1 + e):
// one v_mul, v_exp, v_add, v_rcp, v_fma, v_mul, no libm call.  e = +inf gives c, e = 0 gives -c.
struct PtCap {
  float c, k1, inv_c2;   // the cap, 2 log2(e) / c, 1 / c^2
};
// k1 as one IEEE f32 division: the host (pt_cap) and the GEMM epilogue, which is handed c alone, get the same bits
__host__ __device__ __forceinline__ float pt_cap_k1(float c) { return 2.8853900817779268f / c; }
static inline PtCap pt_cap(float softcap) {
  return {softcap, pt_cap_k1(softcap), (float)(1.0 / ((double)softcap * softcap))};
}
static inline bool pt_cap_valid(float softcap) { return softcap > 0.f && softcap < __builtin_inff(); }   // NaN fails
__device__ __forceinline__ float pt_softcap(float x, float k1, float c) {
  const float r = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * k1));
  return fmaf(-2.0f, r, 1.0f) * c;
}
// d t / d x = 1 - (t / c)^2 from the stored t, as (c - t)(c + t) / c^2: exactly 0 at t = +-c (1 - u u
// cancels there) and 0, not inf - inf, for the -inf padding columns of a vocabulary off the 8-column grid
__device__ __forceinline__ float pt_softcap_grad(float t, float c, float inv_c2) {
  return t == -INFINITY ? 0.f : (c - t) * (c + t) * inv_c2;
}

__device__ __forceinline__ uint32_t pack_bf2(float lo, float hi) {
  return (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
}
__device__ __forceinline__ float lo_bf(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float hi_bf(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// 8 x bf16 in one 16-byte vector
struct __attribute__((aligned(16))) bf16x8 { uint32_t w[4]; };

__device__ __forceinline__ void unpack8(const bf16x8& v, float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) { f[2 * i] = lo_bf(v.w[i]); f[2 * i + 1] = hi_bf(v.w[i]); }
}
__device__ __forceinline__ bf16x8 pack8(const float* f) {
  bf16x8 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) v.w[i] = pack_bf2(f[2 * i], f[2 * i + 1]);
  return v;
}
__device__ __forceinline__ bf16x8 ld8(const uint16_t* p) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ void st8(uint16_t* p, const bf16x8& v) { *reinterpret_cast<bf16x8*>(p) = v; }
// non-temporal forms for data touched once (streaming optimizer state, split-K partials): the guide's
// nt stream measured 6.5-6.8 TB/s against 6.4 with the default cache policy
// (global address space explicitly: pointers read from a device-side table would otherwise be flat)
typedef uint32_t pt_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) pt_u32x4 pt_g_u32x4;
__device__ __forceinline__ bf16x8 ld8_nt(const uint16_t* p) {
  const pt_u32x4 r = __builtin_nontemporal_load((const pt_g_u32x4*)(p));
  return bf16x8{{r.x, r.y, r.z, r.w}};
}
__device__ __forceinline__ void st8_nt(uint16_t* p, const bf16x8& v) {
  const pt_u32x4 r = {v.w[0], v.w[1], v.w[2], v.w[3]};
  __builtin_nontemporal_store(r, (pt_g_u32x4*)(p));
}

// ---- wave reductions (64 lanes) ---------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- LDS-DMA from inline asm ----------------------------------------------------
// global -> LDS copies (saddr form: wave-uniform base + per-lane byte offset; M0 = the LDS
// destination of lane 0).  Issued from asm so the compiler does not treat them as pending LDS
// writes: it otherwise cannot prove ds_read_b64_tr_b16 reads disjoint from an in-flight LDS-DMA
// and puts an `s_waitcnt vmcnt(0)` in front of them, draining every prefetch.  The kernels order
// the copies themselves (counted `s_waitcnt vmcnt(N)` + barrier before the first read).  M0 is
// written here and read by nothing else in those kernels.
__device__ __forceinline__ uint64_t pt_uniform_u64(uint64_t p) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)p);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(p >> 32));
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
__device__ __forceinline__ void pt_glds16(const void* base, uint32_t voff_bytes,
                                          __attribute__((address_space(3))) void* dst) {
  const uint64_t sb = pt_uniform_u64((uint64_t)(uintptr_t)base);
  const uint32_t m0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)dst);
  asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(m0), "v"(voff_bytes), "s"(sb) : "memory");
}
__device__ __forceinline__ void pt_glds4(const void* base, uint32_t voff_bytes,
                                         __attribute__((address_space(3))) void* dst) {
  const uint64_t sb = pt_uniform_u64((uint64_t)(uintptr_t)base);
  const uint32_t m0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)dst);
  asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dword %1, %2" ::"s"(m0), "v"(voff_bytes), "s"(sb) : "memory");
}

static inline bool pt_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// Grid cap for streaming (HBM-bound) kernels: 256 CUs x 8 blocks.
static constexpr int PT_STREAM_GRID_CAP = 2048;
