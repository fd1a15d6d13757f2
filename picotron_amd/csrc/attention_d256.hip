// Causal flash attention at head dim 256 for gfx950, forward and backward (Gemma 1 / 2 / 3, PaLM-style
// models, RecurrentGemma's local attention, Qwen3-Next).
//
// Layout: q / o / dO / dq [B, S, H, 256] and k / v / dk / dv [B, S, HKV, 256] token-major strided views
// (d contiguous; in the model column slices of one [T, (H + 2 HKV) * 256] buffer), lse / delta f32
// [B, H, S] dense.  Limits: bf16, f32 softmax and accumulation, causal, Sq == Sk = S, S % 128 == 0,
// H % HKV == 0 (query head h reads kv head h / (H / HKV)); the scale is the caller's.
//
// Fragment scheme: csrc/attention.hip's (all v_mfma_f32_32x32x16_bf16).  Scores "key on the row",
// S^T = K . Q^T as 16 k-steps into one accumulator; the S^T / dS^T accumulators are the B operand of
// O^T += V^T P^T and dQ^T += K^T dS^T (8 tiles each).  The dK/dV kernel mirrors it (S = Q . K^T).
// A 64-row x 256-column tile is staged as TWO 64 x 128 LDS images (columns 0..127 and 128..255, 16 KiB
// each) in the d128 XOR swizzle, which serves row reads and ds_read_b64_tr_b16 transposed reads alike,
// filled by global_load_lds_dwordx4.  A stage is a K|V (or Q|dO) pair of tiles = 4 images = 64 KiB, and
// the ring is 2 deep: 128 of the 160 KiB.  A workgroup is 4 waves, one per SIMD (512 VGPRs each).
//
// Forward: a wave owns 32 queries; Q fragments (64 VGPRs), O^T (8 tiles, 128) and the two S^T halves of
// a 64-key tile (32) stay in registers.
// dQ: a wave owns 32 queries; Q and dO fragments (64 + 64), dQ^T (128) and one S / dP pair (32) stay in
// registers; K and V come from the ring.  It also forms delta = rowsum(dO * O) and writes it.
// dK/dV: dK^T and dV^T of 32 keys are 128 VGPRs each, and with S, dP and the K and V fragments (64 + 64)
// that is past one wave, so 32 keys belong to a WAVE PAIR and a workgroup holds two pairs (64 keys).
// The choice: the pair splits the work by product, not by column half, so that no MFMA runs twice --
//   wave A (K fragments 64, dV^T 128, S 16):   S = Q K^T,  P = exp2(S c - lse),        dV^T += dO^T P
//   wave B (V fragments 64, dK^T 128, dP + P 32): dP = dO V^T, dS = P (dP - delta),    dK^T += Q^T dS
// each 2 of a step's 4 MFMA groups (the column-half split would run S and dP on both waves: 6 groups
// for 4).  A hands P to B as f32 in the accumulator's own lane layout (4 KiB a step, so dS is formed
// from the unrounded P exactly as a single wave would) through LDS, double-buffered by the step's
// parity: B's dP MFMAs run beside A's S and softmax, one workgroup barrier a step publishes P, and A's
// dV MFMAs run beside B's dK.  LDS: 2 x (64 KiB + 512 B of lse * log2(e) | delta) + 2 steps x 2 pairs x
// 4 KiB = 145 KiB.  The kernel walks the query heads of its kv head's group in head order.
// Causal load balance: block pairing (a workgroup runs block x, then block n - 1 - x) when the block
// count is even -- always for the dK/dV kernel's 64-key blocks.  Workgroup order: attention.hip's XCD
// remap.  No atomics anywhere: two runs give the same bits.
#include "common.h"

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) uint8_t lds_u8;
typedef __attribute__((address_space(3))) float lds_f32;
typedef __attribute__((address_space(3))) f32x4_t lds_f32x4;

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
constexpr float kRescaleLog2 = 8.0f;
constexpr int KT = 64;    // rows per staged tile
constexpr int NW = 4;     // waves per workgroup
constexpr int D = 256;    // head dim
constexpr int DI = 128;   // columns per LDS image
constexpr int KSI = DI / 16, TI = DI / 32;   // k-steps and 32-column tiles per image
constexpr int KS = D / 16, DT = D / 32;
constexpr int IMG = KT * DI * 2;             // 16 KiB
constexpr int TILE_B = 2 * IMG;              // a 64 x 256 tile
constexpr int STAGE_B = 2 * TILE_B;          // K | V or Q | dO: 64 KiB
constexpr int STAGE_Q = STAGE_B + 2 * KT * 4;   // dK/dV: + lse * log2(e) [64], delta [64]
constexpr int XCH_B = 32 * 32 * 4;           // one step's P of one wave pair, f32
constexpr int SMEM_RING = 2 * STAGE_B;
constexpr int SMEM_DKDV = 2 * STAGE_Q + 2 * 2 * XCH_B;
constexpr int KB = 2 * 32;                   // keys per dK/dV workgroup: two wave pairs

template <typename T>
struct View4 {
  T* p;
  int64_t sb, ss, sh;
  __device__ __forceinline__ T* row(int b, int64_t s, int h) const { return p + b * sb + s * ss + h * sh; }
};

struct Args {
  View4<const uint16_t> q, k, v, o, dout;
  View4<uint16_t> ow, dq, dk, dv;
  float* lse;     // [B, H, S]
  float* delta;   // [B, H, S]: written by the dQ kernel, read by the dK/dV kernel
  int B, H, HKV, S;
  float scale;
  int pair;
};

// ---- the LDS images and fragments of csrc/attention.hip at D = 128, one image per column half
__device__ __forceinline__ int aswz(int r) {
  return ((r & 1) << 2) | (((r >> 1) & 1) << 3) | ((r >> 3) & 1) | (((r >> 4) & 1) << 1);
}
// stage a [KT][128] bf16 block (rows `row_stride` elements apart) into a swizzled LDS image
__device__ __forceinline__ void stage_image(const uint16_t* __restrict__ g, int64_t row_stride, lds_u8* dst, int wave,
                                            int lane) {
  constexpr int RB = DI * 2, RC = RB / 16, RPI = 1024 / RB, NI = KT * RB / 1024;
  static_assert(NI % NW == 0, "image instructions split evenly over the waves");
#pragma unroll
  for (int it = 0; it < NI / NW; ++it) {
    const int i = it * NW + wave;
    const int r = i * RPI + lane / RC, c = lane % RC;
    pt_glds16(g, (uint32_t)((r * row_stride + 8 * (c ^ aswz(r))) * 2),
              (__attribute__((address_space(3))) void*)(dst + i * 1024));
  }
}
// a [KT][256] tile: its two images
__device__ __forceinline__ void stage_tile(const uint16_t* __restrict__ g, int64_t row_stride, lds_u8* dst, int wave,
                                           int lane) {
  stage_image(g, row_stride, dst, wave, lane);
  stage_image(g + DI, row_stride, dst + IMG, wave, lane);
}
// A operand (rows of the tile), k-step ks of 16: lane -> row row0 + (lane & 31), k = 16 ks + 8 (lane >> 5) + j
__device__ __forceinline__ bf16x8_t rd_row(const lds_u8* tile, int row0, int ks, int lane) {
  const lds_u8* t = tile + (ks / KSI) * IMG;
  const int r = row0 + (lane & 31), ch = 2 * (ks % KSI) + (lane >> 5);
  return *(const __attribute__((address_space(3))) bf16x8_t*)(t + r * (DI * 2) + 16 * (ch ^ aswz(r)));
}
// A operand X^T for 16-row step s and 32-column tile dt of 8: element j <-> tile row
// 16 s + 8 (j >> 2) + 4 (lane >> 5) + (j & 3), column 32 dt + (lane & 31)
__device__ __forceinline__ bf16x8_t rd_tr(const lds_u8* tile, int s, int dt, int lane) {
  const lds_u8* t = tile + (dt / TI) * IMG;
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int col = 32 * (dt % TI) + 16 * (g & 1) + 4 * p;
  bf16x4_t v[2];
#pragma unroll
  for (int sec = 0; sec < 2; ++sec) {
    const int r = 16 * s + 8 * sec + 4 * (g >> 1) + q;
    const int off = r * (DI * 2) + 16 * ((col >> 3) ^ aswz(r)) + 8 * ((col >> 2) & 1);
    v[sec] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4_t*)(t + off));
  }
  return __builtin_shufflevector(v[0], v[1], 0, 1, 2, 3, 4, 5, 6, 7);
}
// B operand from a C-layout 32x32 accumulator, k-step s (rows 16 s .. 16 s + 15)
__device__ __forceinline__ bf16x8_t acc_as_b(const f32x16_t& x, int s) {
  bf16x8_t out;
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = (__bf16)x[8 * s + j];
  return out;
}
// B operand straight from a global row: k = 16 ks + 8 (lane >> 5) + j
__device__ __forceinline__ bf16x8_t ld_row_frag(const uint16_t* row_ptr, int ks, int lane) {
  return *(const bf16x8_t*)(row_ptr + 16 * ks + 8 * (lane >> 5));
}
// C layout row index of register r for this lane
__device__ __forceinline__ int crow(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ int xcd_remap(int id, int nwg) {
  const int xcd = id & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
}
__device__ __forceinline__ void coords(int& x, int& y, int& z) {
  const int nx = gridDim.x, ny = gridDim.y, nwg = nx * ny * gridDim.z;
  const int pid = xcd_remap(blockIdx.x + nx * (blockIdx.y + ny * blockIdx.z), nwg);
  x = pid % nx;
  y = (pid / nx) % ny;
  z = pid / (nx * ny);
}
__device__ __forceinline__ float xor32_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float xor32_max(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ f32x16_t zero16() {
  f32x16_t z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
__device__ __forceinline__ f32x16_t mfma(const bf16x8_t& a, const bf16x8_t& b, const f32x16_t& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// store a 32(d) x 32(row) C-layout tile transposed into row-major memory: the lane's row, d = 32 dt +
// crow(r); lanes l and l ^ 32 trade 4-column chunks so each stores 8 consecutive columns (16 bytes)
__device__ __forceinline__ void store_T_bf16(uint16_t* row_ptr, int dt, const f32x16_t& x, float mul, int lane) {
#pragma unroll
  for (int gp = 0; gp < 4; gp += 2) {
    uint32_t a[2], b[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint32_t c0 = pack_bf2(x[4 * gp + 2 * u] * mul, x[4 * gp + 2 * u + 1] * mul);
      const uint32_t c1 = pack_bf2(x[4 * gp + 4 + 2 * u] * mul, x[4 * gp + 4 + 2 * u + 1] * mul);
      const auto r = __builtin_amdgcn_permlane32_swap(c0, c1, false, false);
      a[u] = r[0];
      b[u] = r[1];
    }
    *(uint4*)(row_ptr + 32 * dt + 8 * gp + (lane >= 32 ? 8 : 0)) = make_uint4(a[0], a[1], b[0], b[1]);
  }
}
// key (or query) rows crow(r) of a score tile: -inf where `hidden(row)` holds
template <typename F>
__device__ __forceinline__ void mask_rows(f32x16_t& s, F&& hidden) {
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (hidden((r & 3) + 8 * (r >> 2))) s[r] = -INFINITY;
}

// K-side stage of key tile kt of (b, hk): [K | V]
__device__ __forceinline__ void stage_kv(const Args& a, int b, int hk, int kt, lds_u8* st, int wave, int lane) {
  stage_tile(a.k.row(b, (int64_t)kt * KT, hk), a.k.ss, st, wave, lane);
  stage_tile(a.v.row(b, (int64_t)kt * KT, hk), a.v.ss, st + TILE_B, wave, lane);
}
// a 32 x 32 product tile: rows 32 half .. of the staged tile against the wave's own 32 rows (16 k-steps)
__device__ __forceinline__ f32x16_t dot_T(const lds_u8* tile, int half, const bf16x8_t (&f)[KS], int lane) {
  f32x16_t s = zero16();
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) s = mfma(rd_row(tile, 32 * half, ks, lane), f[ks], s);
  return s;
}
// acc^T[dt] += X^T (16-row step ks of the staged tile, every 32-column tile) . b
__device__ __forceinline__ void acc_T(f32x16_t (&acc)[DT], const lds_u8* tile, int ks, const bf16x8_t& b, int lane) {
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc[dt] = mfma(rd_tr(tile, ks, dt, lane), b, acc[dt]);
}

// ============================================================================ forward
__device__ __forceinline__ void fwd_block(const Args& a, int bx, int h, int b) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  lds_u8* smem = (lds_u8*)smem_raw;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nqb = a.S / (NW * 32);
  const int qb = nqb - 1 - bx;   // heavy blocks first
  const int q0 = qb * NW * 32 + wave * 32;
  const int myq = q0 + (lane & 31);
  const int hk = h / (a.H / a.HKV);

  bf16x8_t qf[KS];
  const uint16_t* qrow = a.q.row(b, myq, h);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = ld_row_frag(qrow, ks, lane);

  const int nkt = (qb + 1) * NW * 32 / KT;
  const float c2 = a.scale * kLog2e;
  f32x16_t o[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) o[i] = zero16();
  float m = -INFINITY, l = 0.f;

  stage_kv(a, b, hk, 0, smem, wave, lane);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), visible to the compiler: its own fragment loads are done
  __syncthreads();

  for (int kt = 0; kt < nkt; ++kt) {
    // into the stage tile kt - 1 used (every wave passed its barrier)
    if (kt + 1 < nkt) stage_kv(a, b, hk, kt + 1, smem + ((kt + 1) & 1) * STAGE_B, wave, lane);
    const lds_u8* st = smem + (kt & 1) * STAGE_B;
    const int kv0 = kt * KT;
    if (kv0 <= q0 + 31) {   // wave-uniform: else every key of the tile is after my queries
      f32x16_t s[2];
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) s[kh] = dot_T(st, kh, qf, lane);
      if (kv0 + KT - 1 > q0) {   // diagonal tile: key row visible iff <= thr
        const int thr = myq - kv0 - 4 * (lane >> 5);
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) mask_rows(s[kh], [&](int r) { return 32 * kh + r > thr; });
      }
      float mt = -INFINITY;
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int r = 0; r < 16; ++r) mt = fmaxf(mt, s[kh][r]);
      mt = xor32_max(mt) * c2;  // log2 units (c2 > 0)
      // lazy rescale: only when some query's max grew by > 2^8 (P <= 2^8: harmless in f32 and bf16)
      if (__any(mt > m + kRescaleLog2)) {
        const float mn = fmaxf(m, mt);
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        m = mn;
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
      }
      float lt[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[kh][r], c2, -m));
          s[kh][r] = p;
          lt[r & 3] += p;
        }
      l += (lt[0] + lt[1]) + (lt[2] + lt[3]);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) acc_T(o, st + TILE_B, ks, acc_as_b(s[ks >> 1], ks & 1), lane);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // tile kt + 1 has landed
    __syncthreads();
  }

  l = xor32_sum(l);
  const float inv_l = 1.0f / l;
  uint16_t* orow = a.ow.row(b, myq, h);
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) store_T_bf16(orow, dt, o[dt], inv_l, lane);
  if (lane < 32) a.lse[((int64_t)b * a.H + h) * a.S + myq] = m * kLn2 + __logf(l);
}

__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(1, 1))) void d256_fwd_kernel(Args a) {
  int bx, hh, b;
  coords(bx, hh, b);
  for (int pass = 0; pass <= a.pair; ++pass) {  // one inlined body: no register growth
    if (pass) __syncthreads();
    fwd_block(a, pass ? a.S / (NW * 32) - 1 - bx : bx, hh, b);
  }
}

// ============================================================================ dQ
// also forms D = rowsum(dO * O) of its rows and writes it for the dK/dV kernel (launched after it)
__device__ __forceinline__ void dq_block(const Args& a, int bx, int h, int b) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  lds_u8* smem = (lds_u8*)smem_raw;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nqb = a.S / (NW * 32);
  const int qb = nqb - 1 - bx;
  const int q0 = qb * NW * 32 + wave * 32;
  const int myq = q0 + (lane & 31);
  const int hk = h / (a.H / a.HKV);

  const uint16_t* qrow = a.q.row(b, myq, h);
  const uint16_t* dorow = a.dout.row(b, myq, h);
  const uint16_t* orow = a.o.row(b, myq, h);
  bf16x8_t qf[KS], dof[KS];
  float part = 0.f;   // this lane's half of the row's d; the other half is in lane ^ 32
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qf[ks] = ld_row_frag(qrow, ks, lane);
    dof[ks] = ld_row_frag(dorow, ks, lane);
    const bf16x8_t of = ld_row_frag(orow, ks, lane);
#pragma unroll
    for (int j = 0; j < 8; ++j) part += (float)dof[ks][j] * (float)of[j];
  }
  const int64_t ri = ((int64_t)b * a.H + h) * a.S + myq;
  const float nlse2 = -a.lse[ri] * kLog2e;
  const float del = xor32_sum(part);
  if (lane < 32) a.delta[ri] = del;
  const float c2 = a.scale * kLog2e;

  const int nkt = (qb + 1) * NW * 32 / KT;
  f32x16_t dq[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) dq[i] = zero16();

  stage_kv(a, b, hk, 0, smem, wave, lane);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), visible to the compiler
  __syncthreads();

  for (int kt = 0; kt < nkt; ++kt) {
    if (kt + 1 < nkt) stage_kv(a, b, hk, kt + 1, smem + ((kt + 1) & 1) * STAGE_B, wave, lane);
    const lds_u8* st = smem + (kt & 1) * STAGE_B;
    const int kv0 = kt * KT;
    if (kv0 <= q0 + 31) {   // wave-uniform
      // each 32-key half's dS feeds its two dQ k-steps right away: one S / dP pair live
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        f32x16_t s = dot_T(st, kh, qf, lane);
        const f32x16_t dp = dot_T(st + TILE_B, kh, dof, lane);
        if (kv0 + KT - 1 > q0) {
          const int thr = myq - kv0 - 32 * kh - 4 * (lane >> 5);
          mask_rows(s, [&](int r) { return r > thr; });
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], c2, nlse2)) * (dp[r] - del);
#pragma unroll
        for (int sh = 0; sh < 2; ++sh) acc_T(dq, st, 2 * kh + sh, acc_as_b(s, sh), lane);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  uint16_t* dqr = a.dq.row(b, myq, h);
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) store_T_bf16(dqr, dt, dq[dt], a.scale, lane);
}

__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(1, 1))) void d256_dq_kernel(Args a) {
  int bx, hh, b;
  coords(bx, hh, b);
  for (int pass = 0; pass <= a.pair; ++pass) {
    if (pass) __syncthreads();
    dq_block(a, pass ? a.S / (NW * 32) - 1 - bx : bx, hh, b);
  }
}

// ============================================================================ dK / dV
// 64 keys of kv head hk: waves (0, 1) are the pair of keys 0..31, waves (2, 3) of keys 32..63; the even
// wave of a pair is A (S, P, dV), the odd one B (dP, dS, dK) -- see the header.  Every wave meets every
// barrier: a step a pair skips (its queries all precede its keys) still ends in the step's barrier.
__device__ __forceinline__ void dkdv_block(const Args& a, int kb, int hk, int b) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  lds_u8* smem = (lds_u8*)smem_raw;
  lds_u8* xch = smem + 2 * STAGE_Q;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int pr = wave >> 1;
  const bool is_b = wave & 1;
  const int k0 = kb * KB + pr * 32;
  const int mykey = k0 + (lane & 31);
  const int group = a.H / a.HKV;

  // A keeps its keys' K rows, B their V rows
  const uint16_t* myrow = is_b ? a.v.row(b, mykey, hk) : a.k.row(b, mykey, hk);
  bf16x8_t mf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) mf[ks] = ld_row_frag(myrow, ks, lane);
  f32x16_t acc[DT];   // A: dV^T, B: dK^T
#pragma unroll
  for (int i = 0; i < DT; ++i) acc[i] = zero16();
  const float c2 = a.scale * kLog2e;

  // q tiles that can see this block's keys, for every query head of the group; Q-side stage:
  // [Q | dO | lse * log2(e) | delta]
  const int qt_begin = kb * KB / KT, nqt = a.S / KT;
  const int total = group * (nqt - qt_begin);
  float lse_next = 0.f;   // the LSE rows go through wave 0's registers, scaled on their way to LDS
  auto stage = [&](int h, int qt, int buf) {
    lds_u8* sq = smem + buf * STAGE_Q;
    stage_tile(a.q.row(b, (int64_t)qt * KT, h), a.q.ss, sq, wave, lane);
    stage_tile(a.dout.row(b, (int64_t)qt * KT, h), a.dout.ss, sq + TILE_B, wave, lane);
    if (wave == 0) {  // 64 delta floats = 256 B: one 4-byte DMA per lane
      const int64_t ro = ((int64_t)b * a.H + h) * a.S + qt * KT;
      lse_next = a.lse[ro + lane];
      pt_glds4(a.delta + ro, lane * 4u, (__attribute__((address_space(3))) void*)(sq + STAGE_B + KT * 4));
    }
  };
  auto put_lse = [&](int buf) {  // after the iteration's vmcnt(0), before its barrier
    if (wave == 0) ((lds_f32*)(smem + buf * STAGE_Q + STAGE_B))[lane] = lse_next * kLog2e;
  };

  int h = hk * group, qt = qt_begin;
  stage(h, qt, 0);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), visible to the compiler
  put_lse(0);
  __syncthreads();

  for (int it = 0; it < total; ++it) {
    const int buf = it & 1;
    int hn = h, qn = qt + 1;
    if (qn == nqt) { qn = qt_begin; ++hn; }
    if (it + 1 < total) stage(hn, qn, buf ^ 1);
    const lds_u8* sq = smem + buf * STAGE_Q;
    const lds_u8* t1 = is_b ? sq + TILE_B : sq;   // the score operand: A reads Q, B reads dO
    const lds_u8* t2 = is_b ? sq : sq + TILE_B;   // the gradient operand: A reads dO^T, B reads Q^T
    const lds_f32* sl2 = (const lds_f32*)(sq + STAGE_B);
    const lds_f32* sdel = sl2 + KT;
#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {
      const int qs = qt * KT + 32 * qh;
      const bool live = qs + 31 >= k0;   // pair-uniform: else all these queries precede the pair's keys
      lds_f32x4* x = (lds_f32x4*)(xch + (2 * qh + pr) * XCH_B) + lane;
      f32x16_t t = zero16();
      if (live) {
        // A: S = Q K^T, B: dP = dO V^T  (C layout: col = key = lane, row = query)
        t = dot_T(t1, qh, mf, lane);
        if (!is_b) {
          if (qs < k0 + 31) {  // diagonal: query row crow(r) sees my key iff >= thr
            const int thr = mykey - qs - 4 * (lane >> 5);
            mask_rows(t, [&](int r) { return r < thr; });
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) t[r] = __builtin_amdgcn_exp2f(fmaf(t[r], c2, -sl2[32 * qh + crow(r, lane)]));
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) x[64 * g4] = f32x4_t{t[4 * g4], t[4 * g4 + 1], t[4 * g4 + 2], t[4 * g4 + 3]};
        }
      }
      __syncthreads();   // P of this step is in LDS (the buffer of the other parity stays readable)
      if (live) {
        if (is_b) {
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4_t p = x[64 * g4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int r = 4 * g4 + u;
              t[r] = p[u] * (t[r] - sdel[32 * qh + crow(r, lane)]);   // dS
            }
          }
        }
#pragma unroll
        for (int sh = 0; sh < 2; ++sh) acc_T(acc, t2, 2 * qh + sh, acc_as_b(t, sh), lane);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (it + 1 < total) put_lse(buf ^ 1);
    __syncthreads();
    h = hn;
    qt = qn;
  }

  uint16_t* outr = is_b ? a.dk.row(b, mykey, hk) : a.dv.row(b, mykey, hk);
  const float mul = is_b ? a.scale : 1.0f;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) store_T_bf16(outr, dt, acc[dt], mul, lane);
}

__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(1, 1))) void d256_dkdv_kernel(Args a) {
  int bx, hh, b;
  coords(bx, hh, b);
  for (int pass = 0; pass < 2; ++pass) {   // S % 128 == 0: the 64-key block count is even, always paired
    if (pass) __syncthreads();
    dkdv_block(a, pass ? a.S / KB - 1 - bx : bx, hh, b);
  }
}

// ============================================================================ host
struct HostView {
  const void* p;
  const int64_t* st;
  int64_t heads;
};

// the checks of include/picotron_hip.h, in its order; `ptrs`: the dense f32 arrays
int check_call(const HostView* v, int nv, const void* const* ptrs, int np, int64_t B, int64_t H, int64_t HKV, int64_t S,
               float scale) {
  for (int i = 0; i < nv; ++i)
    if (!v[i].p || !v[i].st) return PT_EINVAL;
  for (int i = 0; i < np; ++i)
    if (!ptrs[i]) return PT_EINVAL;
  if (B < 1 || H < 1 || HKV < 1 || S < 1 || !(scale > 0.f)) return PT_EINVAL;
  if (S % (NW * 32) != 0 || H % HKV != 0 || B > 65535 || H > 65535 || S >= ((int64_t)1 << 31) ||
      B * H * S >= ((int64_t)1 << 31))
    return PT_EUNSUPPORTED;
  for (int i = 0; i < nv; ++i)   // (a 64-row tile's byte offsets stay within the DMA's 32-bit lane offset)
    if (v[i].st[1] >= ((int64_t)1 << 24)) return PT_EUNSUPPORTED;
  for (int i = 0; i < nv; ++i)
    if (v[i].st[0] < 0 || v[i].st[1] < D || (v[i].heads > 1 && v[i].st[2] < D)) return PT_EINVAL;
  for (int i = 0; i < nv; ++i)
    if (!pt_aligned16(v[i].p) || (v[i].st[0] & 7) || (v[i].st[1] & 7) || (v[i].st[2] & 7)) return PT_EALIGN;
  return PT_OK;
}
template <typename T>
View4<T> view(const void* p, const int64_t* st) { return {(T*)const_cast<void*>(p), st[0], st[1], st[2]}; }

template <typename K>
void launch(K kern, dim3 grid, int smem, hipStream_t stream, const Args& a) {
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
  kern<<<grid, NW * 64, smem, stream>>>(a);
}
dim3 query_grid(const Args& a) {
  const int nb = a.S / (NW * 32);
  return dim3((unsigned)(a.pair ? nb / 2 : nb), (unsigned)a.H, (unsigned)a.B);
}

}  // namespace

extern "C" {

int pt_attn_d256_fwd(const void* q, const int64_t* q_str, const void* k, const int64_t* k_str, const void* v,
                     const int64_t* v_str, void* o, const int64_t* o_str, float* lse, int64_t B, int64_t H, int64_t HKV,
                     int64_t S, float scale, hipStream_t stream) {
  const HostView views[] = {{q, q_str, H}, {k, k_str, HKV}, {v, v_str, HKV}, {o, o_str, H}};
  const void* ptrs[] = {lse};
  const int rc = check_call(views, 4, ptrs, 1, B, H, HKV, S, scale);
  if (rc) return rc;
  Args a{};
  a.q = view<const uint16_t>(q, q_str);
  a.k = view<const uint16_t>(k, k_str);
  a.v = view<const uint16_t>(v, v_str);
  a.ow = view<uint16_t>(o, o_str);
  a.lse = lse;
  a.B = (int)B; a.H = (int)H; a.HKV = (int)HKV; a.S = (int)S;
  a.scale = scale;
  a.pair = (S / (NW * 32)) % 2 == 0;
  launch(d256_fwd_kernel, query_grid(a), SMEM_RING, stream, a);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

int pt_attn_d256_bwd(const void* q, const int64_t* q_str, const void* k, const int64_t* k_str, const void* v,
                     const int64_t* v_str, const void* o, const int64_t* o_str, const void* dout, const int64_t* do_str,
                     const float* lse, float* delta_out, void* dq, const int64_t* dq_str, void* dk,
                     const int64_t* dk_str, void* dv, const int64_t* dv_str, int64_t B, int64_t H, int64_t HKV, int64_t S,
                     float scale, hipStream_t stream) {
  const HostView views[] = {{q, q_str, H},   {k, k_str, HKV},   {v, v_str, HKV},   {o, o_str, H},
                            {dout, do_str, H}, {dq, dq_str, H}, {dk, dk_str, HKV}, {dv, dv_str, HKV}};
  const void* ptrs[] = {lse, delta_out};
  const int rc = check_call(views, 8, ptrs, 2, B, H, HKV, S, scale);
  if (rc) return rc;
  Args a{};
  a.q = view<const uint16_t>(q, q_str);
  a.k = view<const uint16_t>(k, k_str);
  a.v = view<const uint16_t>(v, v_str);
  a.o = view<const uint16_t>(o, o_str);
  a.dout = view<const uint16_t>(dout, do_str);
  a.dq = view<uint16_t>(dq, dq_str);
  a.dk = view<uint16_t>(dk, dk_str);
  a.dv = view<uint16_t>(dv, dv_str);
  a.lse = const_cast<float*>(lse);
  a.delta = delta_out;
  a.B = (int)B; a.H = (int)H; a.HKV = (int)HKV; a.S = (int)S;
  a.scale = scale;
  a.pair = (S / (NW * 32)) % 2 == 0;
  launch(d256_dq_kernel, query_grid(a), SMEM_RING, stream, a);   // first: it writes the D the dK/dV kernel reads
  PT_CHECK_LAUNCH();
  launch(d256_dkdv_kernel, dim3((unsigned)(S / KB / 2), (unsigned)HKV, (unsigned)B), SMEM_DKDV, stream, a);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

}  // extern "C"
