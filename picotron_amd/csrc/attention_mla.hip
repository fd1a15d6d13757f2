// Multi-head latent attention (MLA, training form) for gfx950: causal flash attention whose q / k
// heads are 192 wide ([128 nope | 64 rope]) while v / o heads are 128 wide, and whose rotary key
// part is one 64-wide row per token shared by every head (DeepSeek-V2/V3, Moonlight, Kimi-K2).
//
// Layout: q [B, S, H, 192], k_nope / v [B, S, H, 128] and o / dO token-major strided views (d
// contiguous) -- the q projection's output and column slices of the kv_b projection's -- and k_pe
// [B, S, 64], a column slice of the kv_a projection's output.  The broadcast k [B, S, H, 192] is
// never formed: the kernels read the rope columns of every head's k from the one k_pe row.
// lse / delta f32 [B, H, S] dense.  Limits: bf16, f32 softmax, causal, Sq == Sk = S, S % 128 == 0,
// one k/v head per q head, dims 128 / 64 / 128.
//
// Fragment scheme: csrc/attention.hip's (all v_mfma_f32_32x32x16_bf16).  Scores "key on the row",
// S^T = K . Q^T as 8 nope + 4 rope k-steps into one accumulator; the S^T / dS^T accumulators are the B
// operand of O^T += V^T P^T (4 tiles) and dQ^T += K^T dS^T (4 nope + 2 rope tiles).  The dK/dV kernel
// mirrors it (S = Q . K^T): dV^T += dO^T P (4 tiles), dK^T += Q^T dS (4 nope + 2 rope tiles).
// A 64-row tile is staged as three LDS images -- nope 64 x 128 (16 KiB), rope 64 x 64 (8 KiB), V or dO
// 64 x 128 (16 KiB) -- each in the d128 / d64 XOR swizzle that serves row reads and ds_read_b64_tr_b16
// transposed reads alike, filled by global_load_lds_dwordx4 into a 2-deep ring (80 KiB; the dK/dV
// kernel adds 2 x 512 B of lse / delta).  A workgroup is 4 waves of 32 rows, one wave per SIMD.
// Causal load balance: block pairing (a workgroup runs block x, then block n - 1 - x) when the block
// count is even.  Workgroup order: attention.hip's XCD remap (a head's blocks share one L2; the k_pe
// rows of a batch, 128 B a token, stay resident in every L2 beside them).
// The rope columns of dK leave as one f32 row per (token, head) in a workspace; pt_mla_dkpe_reduce
// sums them over heads in head order and rotates back.  No atomics: two runs give the same bits.
#include "common.h"

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) uint8_t lds_u8;

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
constexpr float kRescaleLog2 = 8.0f;
constexpr int KT = 64;   // rows per staged tile
constexpr int NW = 4;    // waves per workgroup, 32 rows each
constexpr int DN = 128, DR = 64, DV = 128, DQ = DN + DR;
constexpr int KSN = DN / 16, KSR = DR / 16, KSV = DV / 16;   // k-steps
constexpr int TN = DN / 32, TR = DR / 32, TV = DV / 32;      // 32-column tiles
constexpr int IMG_N = KT * DN * 2, IMG_R = KT * DR * 2, IMG_V = KT * DV * 2;
constexpr int STAGE_B = IMG_N + IMG_R + IMG_V;               // 40 KiB
constexpr int STAGE_Q = STAGE_B + 2 * KT * 4;                // dK/dV: + lse * log2(e) [64], delta [64]

template <typename T>
struct View4 {
  T* p;
  int64_t sb, ss, sh;
  __device__ __forceinline__ T* row(int b, int64_t s, int h) const { return p + b * sb + s * ss + h * sh; }
};

struct MlaArgs {
  View4<const uint16_t> q, kn, v, o, dout;
  const uint16_t* kpe;          // [B, S, 64]
  int64_t kpe_sb, kpe_ss;
  View4<uint16_t> ow, dq, dkn, dv;
  float* lse;                   // [B, H, S]
  float* delta;                 // [B, H, S]: written by the dQ kernel, read by the dK/dV kernel
  float* dkpe_ws;               // [B, S, H, 64] f32
  int B, H, S;
  float scale;
  int pair;
};

// ---- the LDS images and fragments of csrc/attention.hip (D = the image's row width)
template <int D>
__device__ __forceinline__ int aswz(int r) {
  if (D == 64) return (((r >> 1) & 1) << 2) | ((r >> 3) & 1) | (((r >> 4) & 1) << 1);
  return ((r & 1) << 2) | (((r >> 1) & 1) << 3) | ((r >> 3) & 1) | (((r >> 4) & 1) << 1);
}
// stage a [KT][D] bf16 tile (rows `row_stride` elements apart) into a swizzled LDS image
template <int D>
__device__ __forceinline__ void stage_rows(const uint16_t* __restrict__ g, int64_t row_stride, lds_u8* dst,
                                           int wave, int lane) {
  constexpr int RB = D * 2, RC = RB / 16, RPI = 1024 / RB, NI = KT * RB / 1024;
  static_assert(NI % NW == 0, "tile instructions split evenly over the waves");
#pragma unroll
  for (int it = 0; it < NI / NW; ++it) {
    const int i = it * NW + wave;
    const int r = i * RPI + lane / RC, c = lane % RC;
    pt_glds16(g, (uint32_t)((r * row_stride + 8 * (c ^ aswz<D>(r))) * 2),
              (__attribute__((address_space(3))) void*)(dst + i * 1024));
  }
}
// A operand (rows of the tile): lane -> row row0 + (lane & 31), k = 16 ks + 8 (lane >> 5) + j
template <int D>
__device__ __forceinline__ bf16x8_t rd_row(const lds_u8* t, int row0, int ks, int lane) {
  const int r = row0 + (lane & 31), ch = 2 * ks + (lane >> 5);
  return *(const __attribute__((address_space(3))) bf16x8_t*)(t + r * (D * 2) + 16 * (ch ^ aswz<D>(r)));
}
// A operand X^T for 16-row step s and 32-column tile dt: element j <-> tile row
// 16 s + 8 (j >> 2) + 4 (lane >> 5) + (j & 3), column 32 dt + (lane & 31)
template <int D>
__device__ __forceinline__ bf16x8_t rd_tr(const lds_u8* t, int s, int dt, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int col = 32 * dt + 16 * (g & 1) + 4 * p;
  bf16x4_t v[2];
#pragma unroll
  for (int sec = 0; sec < 2; ++sec) {
    const int r = 16 * s + 8 * sec + 4 * (g >> 1) + q;
    const int off = r * (D * 2) + 16 * ((col >> 3) ^ aswz<D>(r)) + 8 * ((col >> 2) & 1);
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
__device__ __forceinline__ void mla_coords(int& x, int& y, int& z) {
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
// the same tile as f32: 4 consecutive d per 16-byte store
__device__ __forceinline__ void store_T_f32(float* row_ptr, int dt, const f32x16_t& x, float mul, int lane) {
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4)
    *(float4*)(row_ptr + 32 * dt + 8 * g4 + 4 * (lane >> 5)) =
        make_float4(x[4 * g4] * mul, x[4 * g4 + 1] * mul, x[4 * g4 + 2] * mul, x[4 * g4 + 3] * mul);
}
// key (or query) rows 32 half + crow(r) of a score tile: -inf where `hidden(row)` holds
template <typename F>
__device__ __forceinline__ void mask_rows(f32x16_t& s, F&& hidden) {
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (hidden((r & 3) + 8 * (r >> 2))) s[r] = -INFINITY;
}

// K-side stage of key tile kt of (b, h): [nope | rope | V]
__device__ __forceinline__ void stage_kv(const MlaArgs& a, int b, int h, int kt, lds_u8* st, int wave, int lane) {
  stage_rows<DN>(a.kn.row(b, (int64_t)kt * KT, h), a.kn.ss, st, wave, lane);
  stage_rows<DR>(a.kpe + b * a.kpe_sb + (int64_t)kt * KT * a.kpe_ss, a.kpe_ss, st + IMG_N, wave, lane);
  stage_rows<DV>(a.v.row(b, (int64_t)kt * KT, h), a.v.ss, st + IMG_N + IMG_R, wave, lane);
}
// S^T tile of 32 keys (rows 32 kh of the stage) against the wave's 32 queries: 8 nope + 4 rope k-steps
__device__ __forceinline__ f32x16_t score_T(const lds_u8* st, int kh, const bf16x8_t (&qf)[KSN + KSR], int lane) {
  f32x16_t s = zero16();
#pragma unroll
  for (int ks = 0; ks < KSN; ++ks) s = mfma(rd_row<DN>(st, 32 * kh, ks, lane), qf[ks], s);
#pragma unroll
  for (int ks = 0; ks < KSR; ++ks) s = mfma(rd_row<DR>(st + IMG_N, 32 * kh, ks, lane), qf[KSN + ks], s);
  return s;
}

// ============================================================================ forward
__device__ __forceinline__ void mla_fwd_block(const MlaArgs& a, int bx, int h, int b) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  lds_u8* smem = (lds_u8*)smem_raw;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nqb = a.S / (NW * 32);
  const int qb = nqb - 1 - bx;   // heavy blocks first
  const int q0 = qb * NW * 32 + wave * 32;
  const int myq = q0 + (lane & 31);

  bf16x8_t qf[KSN + KSR];
  const uint16_t* qrow = a.q.row(b, myq, h);
#pragma unroll
  for (int ks = 0; ks < KSN + KSR; ++ks) qf[ks] = ld_row_frag(qrow, ks, lane);

  const int nkt = (qb + 1) * NW * 32 / KT;
  const float c2 = a.scale * kLog2e;
  f32x16_t o[TV];
#pragma unroll
  for (int i = 0; i < TV; ++i) o[i] = zero16();
  float m = -INFINITY, l = 0.f;

  stage_kv(a, b, h, 0, smem, wave, lane);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), visible to the compiler: its own fragment loads are done
  __syncthreads();

  for (int kt = 0; kt < nkt; ++kt) {
    // into the stage tile kt - 1 used (every wave passed its barrier)
    if (kt + 1 < nkt) stage_kv(a, b, h, kt + 1, smem + ((kt + 1) & 1) * STAGE_B, wave, lane);
    const lds_u8* st = smem + (kt & 1) * STAGE_B;
    const int kv0 = kt * KT;
    if (kv0 <= q0 + 31) {   // wave-uniform: else every key of the tile is after my queries
      f32x16_t s[2];
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) s[kh] = score_T(st, kh, qf, lane);
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
        for (int dt = 0; dt < TV; ++dt)
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
      const lds_u8* sv = st + IMG_N + IMG_R;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8_t pb = acc_as_b(s[ks >> 1], ks & 1);
#pragma unroll
        for (int dt = 0; dt < TV; ++dt) o[dt] = mfma(rd_tr<DV>(sv, ks, dt, lane), pb, o[dt]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // tile kt + 1 has landed
    __syncthreads();
  }

  l = xor32_sum(l);
  const float inv_l = 1.0f / l;
  uint16_t* orow = a.ow.row(b, myq, h);
#pragma unroll
  for (int dt = 0; dt < TV; ++dt) store_T_bf16(orow, dt, o[dt], inv_l, lane);
  if (lane < 32) a.lse[((int64_t)b * a.H + h) * a.S + myq] = m * kLn2 + __logf(l);
}

__global__ __launch_bounds__(NW * 64) void mla_fwd_kernel(MlaArgs a) {
  int bx, hh, b;
  mla_coords(bx, hh, b);
  for (int pass = 0; pass <= a.pair; ++pass) {  // one inlined body: no register growth
    if (pass) __syncthreads();
    mla_fwd_block(a, pass ? a.S / (NW * 32) - 1 - bx : bx, hh, b);
  }
}

// ============================================================================ dQ
// also forms D = rowsum(dO * O) of its rows and writes it for the dK/dV kernel (launched after it)
__device__ __forceinline__ void mla_dq_block(const MlaArgs& a, int bx, int h, int b) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  lds_u8* smem = (lds_u8*)smem_raw;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nqb = a.S / (NW * 32);
  const int qb = nqb - 1 - bx;
  const int q0 = qb * NW * 32 + wave * 32;
  const int myq = q0 + (lane & 31);

  const uint16_t* qrow = a.q.row(b, myq, h);
  const uint16_t* dorow = a.dout.row(b, myq, h);
  const uint16_t* orow = a.o.row(b, myq, h);
  bf16x8_t qf[KSN + KSR], dof[KSV];
#pragma unroll
  for (int ks = 0; ks < KSN + KSR; ++ks) qf[ks] = ld_row_frag(qrow, ks, lane);
  float part = 0.f;   // this lane's half of the row's d; the other half is in lane ^ 32
#pragma unroll
  for (int ks = 0; ks < KSV; ++ks) {
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
  f32x16_t dq[TN + TR];
#pragma unroll
  for (int i = 0; i < TN + TR; ++i) dq[i] = zero16();

  stage_kv(a, b, h, 0, smem, wave, lane);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), visible to the compiler
  __syncthreads();

  for (int kt = 0; kt < nkt; ++kt) {
    if (kt + 1 < nkt) stage_kv(a, b, h, kt + 1, smem + ((kt + 1) & 1) * STAGE_B, wave, lane);
    const lds_u8* st = smem + (kt & 1) * STAGE_B;
    const lds_u8* sv = st + IMG_N + IMG_R;
    const int kv0 = kt * KT;
    if (kv0 <= q0 + 31) {   // wave-uniform
      // each 32-key half's dS feeds its two dQ k-steps right away: one S / dP pair live
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        f32x16_t s = score_T(st, kh, qf, lane), dp = zero16();
#pragma unroll
        for (int ks = 0; ks < KSV; ++ks) dp = mfma(rd_row<DV>(sv, 32 * kh, ks, lane), dof[ks], dp);
        if (kv0 + KT - 1 > q0) {
          const int thr = myq - kv0 - 32 * kh - 4 * (lane >> 5);
          mask_rows(s, [&](int r) { return r > thr; });
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], c2, nlse2)) * (dp[r] - del);
#pragma unroll
        for (int sh = 0; sh < 2; ++sh) {
          const int ks = 2 * kh + sh;
          const bf16x8_t db = acc_as_b(s, sh);
#pragma unroll
          for (int dt = 0; dt < TN; ++dt) dq[dt] = mfma(rd_tr<DN>(st, ks, dt, lane), db, dq[dt]);
#pragma unroll
          for (int dt = 0; dt < TR; ++dt) dq[TN + dt] = mfma(rd_tr<DR>(st + IMG_N, ks, dt, lane), db, dq[TN + dt]);
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  uint16_t* dqr = a.dq.row(b, myq, h);
#pragma unroll
  for (int dt = 0; dt < TN + TR; ++dt) store_T_bf16(dqr, dt, dq[dt], a.scale, lane);
}

__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(1, 1))) void mla_dq_kernel(MlaArgs a) {
  int bx, hh, b;
  mla_coords(bx, hh, b);
  for (int pass = 0; pass <= a.pair; ++pass) {
    if (pass) __syncthreads();
    mla_dq_block(a, pass ? a.S / (NW * 32) - 1 - bx : bx, hh, b);
  }
}

// ============================================================================ dK / dV
__device__ __forceinline__ void mla_dkdv_block(const MlaArgs& a, int kb, int h, int b) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_raw[];
  lds_u8* smem = (lds_u8*)smem_raw;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int k0 = kb * NW * 32 + wave * 32;
  const int mykey = k0 + (lane & 31);

  const uint16_t* knrow = a.kn.row(b, mykey, h);
  const uint16_t* perow = a.kpe + b * a.kpe_sb + (int64_t)mykey * a.kpe_ss;
  const uint16_t* vrow = a.v.row(b, mykey, h);
  bf16x8_t kf[KSN + KSR], vf[KSV];
#pragma unroll
  for (int ks = 0; ks < KSN; ++ks) kf[ks] = ld_row_frag(knrow, ks, lane);
#pragma unroll
  for (int ks = 0; ks < KSR; ++ks) kf[KSN + ks] = ld_row_frag(perow, ks, lane);
#pragma unroll
  for (int ks = 0; ks < KSV; ++ks) vf[ks] = ld_row_frag(vrow, ks, lane);
  f32x16_t dk[TN + TR], dv[TV];
#pragma unroll
  for (int i = 0; i < TN + TR; ++i) dk[i] = zero16();
#pragma unroll
  for (int i = 0; i < TV; ++i) dv[i] = zero16();
  const float c2 = a.scale * kLog2e;

  // q tiles that can see this block's keys; Q-side stage: [Q nope | Q rope | dO | lse * log2(e) | delta]
  const int qt_begin = kb * NW * 32 / KT, nqt = a.S / KT;
  float lse_next = 0.f;   // the LSE rows go through wave 0's registers, scaled on their way to LDS
  auto stage = [&](int qt, int buf) {
    lds_u8* sq = smem + buf * STAGE_Q;
    const uint16_t* qg = a.q.row(b, (int64_t)qt * KT, h);
    stage_rows<DN>(qg, a.q.ss, sq, wave, lane);
    stage_rows<DR>(qg + DN, a.q.ss, sq + IMG_N, wave, lane);
    stage_rows<DV>(a.dout.row(b, (int64_t)qt * KT, h), a.dout.ss, sq + IMG_N + IMG_R, wave, lane);
    if (wave == 0) {  // 64 delta floats = 256 B: one 4-byte DMA per lane
      const int64_t ro = ((int64_t)b * a.H + h) * a.S + qt * KT;
      lse_next = a.lse[ro + lane];
      pt_glds4(a.delta + ro, lane * 4u, (__attribute__((address_space(3))) void*)(sq + STAGE_B + KT * 4));
    }
  };
  auto put_lse = [&](int buf) {  // after the iteration's vmcnt(0), before its barrier
    if (wave == 0) ((__attribute__((address_space(3))) float*)(smem + buf * STAGE_Q + STAGE_B))[lane] = lse_next * kLog2e;
  };

  stage(qt_begin, 0);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), visible to the compiler
  put_lse(0);
  __syncthreads();

  for (int qt = qt_begin; qt < nqt; ++qt) {
    const int buf = (qt - qt_begin) & 1;
    if (qt + 1 < nqt) stage(qt + 1, buf ^ 1);
    const lds_u8* sq = smem + buf * STAGE_Q;
    const lds_u8* sdo = sq + IMG_N + IMG_R;
    const float* sl2 = (const float*)(sq + STAGE_B);
    const float* sdel = sl2 + KT;
#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {
      const int qs = qt * KT + 32 * qh;
      if (qs + 31 < k0) continue;  // wave-uniform: all these queries precede my keys
      // S = Q K^T and dP = dO V^T  (C layout: col = key = lane, row = query)
      f32x16_t s = zero16(), dp = zero16();
#pragma unroll
      for (int ks = 0; ks < KSN; ++ks) s = mfma(rd_row<DN>(sq, 32 * qh, ks, lane), kf[ks], s);
#pragma unroll
      for (int ks = 0; ks < KSR; ++ks) s = mfma(rd_row<DR>(sq + IMG_N, 32 * qh, ks, lane), kf[KSN + ks], s);
#pragma unroll
      for (int ks = 0; ks < KSV; ++ks) dp = mfma(rd_row<DV>(sdo, 32 * qh, ks, lane), vf[ks], dp);
      if (qs < k0 + 31) {  // diagonal: query row crow(r) sees my key iff >= thr
        const int thr = mykey - qs - 4 * (lane >> 5);
        mask_rows(s, [&](int r) { return r < thr; });
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qi = 32 * qh + crow(r, lane);
        const float p = __builtin_amdgcn_exp2f(fmaf(s[r], c2, -sl2[qi]));
        s[r] = p;                          // P
        dp[r] = p * (dp[r] - sdel[qi]);    // dS
      }
#pragma unroll
      for (int sh = 0; sh < 2; ++sh) {
        const int ks = 2 * qh + sh;
        const bf16x8_t pb = acc_as_b(s, sh), db = acc_as_b(dp, sh);
#pragma unroll
        for (int dt = 0; dt < TV; ++dt) dv[dt] = mfma(rd_tr<DV>(sdo, ks, dt, lane), pb, dv[dt]);
#pragma unroll
        for (int dt = 0; dt < TN; ++dt) dk[dt] = mfma(rd_tr<DN>(sq, ks, dt, lane), db, dk[dt]);
#pragma unroll
        for (int dt = 0; dt < TR; ++dt) dk[TN + dt] = mfma(rd_tr<DR>(sq + IMG_N, ks, dt, lane), db, dk[TN + dt]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (qt + 1 < nqt) put_lse(buf ^ 1);
    __syncthreads();
  }

  uint16_t* dknr = a.dkn.row(b, mykey, h);
  uint16_t* dvr = a.dv.row(b, mykey, h);
  float* wsr = a.dkpe_ws + (((int64_t)b * a.S + mykey) * a.H + h) * DR;
#pragma unroll
  for (int dt = 0; dt < TN; ++dt) store_T_bf16(dknr, dt, dk[dt], a.scale, lane);
#pragma unroll
  for (int dt = 0; dt < TR; ++dt) store_T_f32(wsr, dt, dk[TN + dt], a.scale, lane);
#pragma unroll
  for (int dt = 0; dt < TV; ++dt) store_T_bf16(dvr, dt, dv[dt], 1.0f, lane);
}

__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(1, 1))) void mla_dkdv_kernel(MlaArgs a) {
  int bx, hh, b;
  mla_coords(bx, hh, b);
  for (int pass = 0; pass <= a.pair; ++pass) {
    if (pass) __syncthreads();
    mla_dkdv_block(a, pass ? a.S / (NW * 32) - 1 - bx : bx, hh, b);
  }
}

// ============================================================================ row kernels
// csrc/rope.hip's arithmetic on one 8-pair chunk: (x1, x2) = columns (8 ch .. , 32 + 8 ch ..) of a
// 64-wide rotary vector; sign = -1 rotates back
__device__ __forceinline__ void rotate8(const float* x1, const float* x2, const uint16_t* cos_row,
                                        const uint16_t* sin_row, int ch, float sign, float* o1, float* o2) {
  float c[8], s[8];
  unpack8(ld8(cos_row + ch * 8), c);
  unpack8(ld8(sin_row + ch * 8), s);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float sj = sign * s[j];
    o1[j] = fmaf(x1[j], c[j], -(x2[j] * sj));
    o2[j] = fmaf(x2[j], c[j], x1[j] * sj);
  }
}

// in place: the rope columns of q's H heads (row r: q + r q_ld + 192 h + 128) and, when given, the
// k_pe row (item H of the row).  One thread = 8 rotation pairs.
__global__ __launch_bounds__(256) void mla_rope_kernel(uint16_t* __restrict__ q, int64_t q_ld, int H,
                                                       uint16_t* __restrict__ kpe, int64_t kpe_ld, int64_t rows,
                                                       const uint16_t* __restrict__ cos_t,
                                                       const uint16_t* __restrict__ sin_t, int seq_len,
                                                       int64_t tab_ld, float sign) {
  constexpr int CPH = DR / 16;   // chunks per rotary vector
  const int per_row = (H + (kpe ? 1 : 0)) * CPH;
  const int64_t total = rows * per_row;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / per_row;
    const int rem = (int)(i - row * per_row);
    const int head = rem / CPH, ch = rem - head * CPH;
    const int64_t pos = row % seq_len;
    uint16_t* p1 = (head < H ? q + row * q_ld + (int64_t)head * DQ + DN : kpe + row * kpe_ld) + ch * 8;
    uint16_t* p2 = p1 + DR / 2;
    float x1[8], x2[8], o1[8], o2[8];
    unpack8(ld8(p1), x1);
    unpack8(ld8(p2), x2);
    rotate8(x1, x2, cos_t + pos * tab_ld, sin_t + pos * tab_ld, ch, sign, o1, o2);
    st8(p1, pack8(o1));
    st8(p2, pack8(o2));
  }
}

// dk_pe[row] = rotate_back(sum over heads, in head order, of ws[row, h, :]): f32 sums, one bf16 rounding
__global__ __launch_bounds__(256) void mla_dkpe_reduce_kernel(const float* __restrict__ ws, int H,
                                                              uint16_t* __restrict__ dkpe, int64_t dkpe_ld,
                                                              int64_t rows, const uint16_t* __restrict__ cos_t,
                                                              const uint16_t* __restrict__ sin_t, int seq_len,
                                                              int64_t tab_ld) {
  constexpr int CPH = DR / 16;
  const int64_t total = rows * CPH;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / CPH;
    const int ch = (int)(i - row * CPH);
    const int64_t pos = row % seq_len;
    float g1[8], g2[8], o1[8], o2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) g1[j] = g2[j] = 0.f;
    for (int h = 0; h < H; ++h) {
      const float* w = ws + (row * H + h) * DR + ch * 8;
      const float4 a0 = *(const float4*)w, a1 = *(const float4*)(w + 4);
      const float4 b0 = *(const float4*)(w + DR / 2), b1 = *(const float4*)(w + DR / 2 + 4);
      g1[0] += a0.x; g1[1] += a0.y; g1[2] += a0.z; g1[3] += a0.w;
      g1[4] += a1.x; g1[5] += a1.y; g1[6] += a1.z; g1[7] += a1.w;
      g2[0] += b0.x; g2[1] += b0.y; g2[2] += b0.z; g2[3] += b0.w;
      g2[4] += b1.x; g2[5] += b1.y; g2[6] += b1.z; g2[7] += b1.w;
    }
    rotate8(g1, g2, cos_t + pos * tab_ld, sin_t + pos * tab_ld, ch, -1.0f, o1, o2);
    uint16_t* p = dkpe + row * dkpe_ld + ch * 8;
    st8(p, pack8(o1));
    st8(p + DR / 2, pack8(o2));
  }
}

// ============================================================================ host
// a [B, S, H, width] bf16 view the kernels may read or write with 16-byte accesses and LDS-DMA rows:
// non-null, 16-byte aligned, strides multiples of 8, rows that hold `width` columns and heads that do
// not overlap, and a 64-row tile's byte offsets within the DMA's 32-bit lane offset
bool view_ok(const void* p, const int64_t* st, int64_t H, int64_t width, int& rc) {
  if (!p || !st) { rc = PT_EINVAL; return false; }
  if (st[0] < 0 || st[1] < width || (H > 1 && st[2] < width) || st[1] >= ((int64_t)1 << 24)) { rc = PT_EINVAL; return false; }
  if (!pt_aligned16(p) || (st[0] & 7) || (st[1] & 7) || (st[2] & 7)) { rc = PT_EALIGN; return false; }
  return true;
}
bool dims_ok(int64_t B, int64_t H, int64_t S, int64_t d_nope, int64_t d_rope, int64_t d_v) {
  return d_nope == DN && d_rope == DR && d_v == DV && B > 0 && H > 0 && S > 0 && S % (NW * 32) == 0 &&
         B <= 65535 && H <= 65535 && B * H * S < ((int64_t)1 << 31);
}
template <typename T>
View4<T> view(const void* p, const int64_t* st) { return {(T*)const_cast<void*>(p), st[0], st[1], st[2]}; }

// fills the operands both directions read, and checks them
int fill_inputs(MlaArgs& a, const void* q, const int64_t* q_str, const void* kn, const int64_t* kn_str,
                const void* kpe, const int64_t* kpe_str, const void* v, const int64_t* v_str, int64_t B, int64_t H,
                int64_t S, int64_t d_nope, int64_t d_rope, int64_t d_v, float scale) {
  if (!dims_ok(B, H, S, d_nope, d_rope, d_v) || !(scale > 0.f)) return PT_EINVAL;
  int rc = PT_OK;
  if (!view_ok(q, q_str, H, DQ, rc) || !view_ok(kn, kn_str, H, DN, rc) || !view_ok(v, v_str, H, DV, rc)) return rc;
  if (!kpe || !kpe_str || kpe_str[0] < 0 || kpe_str[1] < DR || kpe_str[1] >= ((int64_t)1 << 24)) return PT_EINVAL;
  if (!pt_aligned16(kpe) || (kpe_str[0] & 7) || (kpe_str[1] & 7)) return PT_EALIGN;
  a.q = view<const uint16_t>(q, q_str);
  a.kn = view<const uint16_t>(kn, kn_str);
  a.v = view<const uint16_t>(v, v_str);
  a.kpe = (const uint16_t*)kpe; a.kpe_sb = kpe_str[0]; a.kpe_ss = kpe_str[1];
  a.B = (int)B; a.H = (int)H; a.S = (int)S;
  a.scale = scale;
  a.pair = (S / (NW * 32)) % 2 == 0;
  return PT_OK;
}
dim3 mla_grid(const MlaArgs& a) {
  const int nb = a.S / (NW * 32);
  return dim3((unsigned)(a.pair ? nb / 2 : nb), (unsigned)a.H, (unsigned)a.B);
}
template <typename K>
void launch(K kern, int smem, hipStream_t stream, const MlaArgs& a) {
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
  kern<<<mla_grid(a), NW * 64, smem, stream>>>(a);
}
int row_grid(int64_t total) {
  const int64_t g = (total + 255) / 256;
  return (int)(g > 2 * PT_STREAM_GRID_CAP ? 2 * PT_STREAM_GRID_CAP : g);
}
bool tables_ok(const void* c, const void* s, int64_t seq_len, int64_t tab_ld, int& rc) {
  if (!c || !s || seq_len <= 0 || tab_ld < DR / 2) { rc = PT_EINVAL; return false; }
  if (!pt_aligned16(c) || !pt_aligned16(s) || (tab_ld & 7)) { rc = PT_EALIGN; return false; }
  return true;
}

}  // namespace

extern "C" {

int pt_mla_attn_fwd(const void* q, const int64_t* q_str, const void* k_nope, const int64_t* kn_str, const void* k_pe,
                    const int64_t* kpe_str, const void* v, const int64_t* v_str, void* o, const int64_t* o_str,
                    float* lse, int64_t B, int64_t H, int64_t S, int64_t d_nope, int64_t d_rope, int64_t d_v,
                    float scale, hipStream_t stream) {
  MlaArgs a{};
  int rc = fill_inputs(a, q, q_str, k_nope, kn_str, k_pe, kpe_str, v, v_str, B, H, S, d_nope, d_rope, d_v, scale);
  if (rc) return rc;
  if (!lse) return PT_EINVAL;
  if (!view_ok(o, o_str, H, DV, rc)) return rc;
  a.ow = view<uint16_t>(o, o_str);
  a.lse = lse;
  launch(mla_fwd_kernel, 2 * STAGE_B, stream, a);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

int pt_mla_attn_bwd(const void* q, const int64_t* q_str, const void* k_nope, const int64_t* kn_str, const void* k_pe,
                    const int64_t* kpe_str, const void* v, const int64_t* v_str, const void* o, const int64_t* o_str,
                    const void* dout, const int64_t* do_str, const float* lse, float* delta_out, void* dq,
                    const int64_t* dq_str, void* dk_nope, const int64_t* dkn_str, void* dv, const int64_t* dv_str,
                    float* dkpe_ws, int64_t B, int64_t H, int64_t S, int64_t d_nope, int64_t d_rope, int64_t d_v,
                    float scale, hipStream_t stream) {
  MlaArgs a{};
  int rc = fill_inputs(a, q, q_str, k_nope, kn_str, k_pe, kpe_str, v, v_str, B, H, S, d_nope, d_rope, d_v, scale);
  if (rc) return rc;
  if (!lse || !delta_out || !dkpe_ws || !pt_aligned16(dkpe_ws)) return PT_EINVAL;
  if (!view_ok(o, o_str, H, DV, rc) || !view_ok(dout, do_str, H, DV, rc) || !view_ok(dq, dq_str, H, DQ, rc) ||
      !view_ok(dk_nope, dkn_str, H, DN, rc) || !view_ok(dv, dv_str, H, DV, rc))
    return rc;
  a.o = view<const uint16_t>(o, o_str);
  a.dout = view<const uint16_t>(dout, do_str);
  a.dq = view<uint16_t>(dq, dq_str);
  a.dkn = view<uint16_t>(dk_nope, dkn_str);
  a.dv = view<uint16_t>(dv, dv_str);
  a.lse = const_cast<float*>(lse);
  a.delta = delta_out;
  a.dkpe_ws = dkpe_ws;
  launch(mla_dq_kernel, 2 * STAGE_B, stream, a);   // first: it writes the D the dK/dV kernel reads
  PT_CHECK_LAUNCH();
  launch(mla_dkdv_kernel, 2 * STAGE_Q, stream, a);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

int pt_mla_rope(void* q, int64_t q_row_stride, int64_t H, void* k_pe, int64_t kpe_row_stride, int64_t rows,
                const void* cos_table, const void* sin_table, int64_t seq_len, int64_t table_stride, int64_t d_nope,
                int64_t d_rope, int inverse, hipStream_t stream) {
  if (!q || d_nope != DN || d_rope != DR || rows <= 0 || H <= 0 || H > 65535 || q_row_stride < H * DQ) return PT_EINVAL;
  if (k_pe && kpe_row_stride < DR) return PT_EINVAL;
  int rc = PT_OK;
  if (!tables_ok(cos_table, sin_table, seq_len, table_stride, rc)) return rc;
  if (!pt_aligned16(q) || (q_row_stride & 7) || (k_pe && (!pt_aligned16(k_pe) || (kpe_row_stride & 7)))) return PT_EALIGN;
  mla_rope_kernel<<<row_grid(rows * (H + 1) * (DR / 16)), 256, 0, stream>>>(
      (uint16_t*)q, q_row_stride, (int)H, (uint16_t*)k_pe, kpe_row_stride, rows, (const uint16_t*)cos_table,
      (const uint16_t*)sin_table, (int)seq_len, table_stride, inverse ? -1.0f : 1.0f);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

int pt_mla_dkpe_reduce(const float* ws, int64_t H, void* dk_pe, int64_t dkpe_row_stride, int64_t rows,
                       const void* cos_table, const void* sin_table, int64_t seq_len, int64_t table_stride,
                       int64_t d_rope, hipStream_t stream) {
  if (!ws || !dk_pe || d_rope != DR || rows <= 0 || H <= 0 || H > 65535 || dkpe_row_stride < DR) return PT_EINVAL;
  int rc = PT_OK;
  if (!tables_ok(cos_table, sin_table, seq_len, table_stride, rc)) return rc;
  if (!pt_aligned16(ws) || !pt_aligned16(dk_pe) || (dkpe_row_stride & 7)) return PT_EALIGN;
  mla_dkpe_reduce_kernel<<<row_grid(rows * (DR / 16)), 256, 0, stream>>>(
      ws, (int)H, (uint16_t*)dk_pe, dkpe_row_stride, rows, (const uint16_t*)cos_table, (const uint16_t*)sin_table,
      (int)seq_len, table_stride);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

}  // extern "C"
