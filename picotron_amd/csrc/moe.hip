// Mixture-of-experts routing for gfx950: everything of an MoE MLP that is not a GEMM.
//
// Not in the reference (its MLP is dense, picotron/model.py:184-186): the token routing of Mixtral /
// Qwen3-MoE / OLMoE with a GShard / Switch capacity, so every shape is static and nothing is read on
// the host.  T tokens pick k of E experts; expert e owns rows [e C, (e + 1) C) of an [E C, H] buffer.
//
//   route        logits bf16 [T, E] -> p = softmax (f32, all E), idx = top-k of the STORED bf16 values
//                (ties to the lower expert), gate = p[idx] (/ their sum), counts, and the Switch loss
//                aux = E sum_e (count_e / (T k)) (mean_t p[t, e])
//   plan         item i = t k + j (flat order); pos = the number of earlier items of the same expert;
//                slot[i] = e C + pos (pos < C) or -1 (dropped); src = its inverse, -1 for empty rows
//   dispatch     xe[r] = x[src[r] / k], zeros for empty rows
//   combine      y[t] = bf16(residual[t] + sum_j gate[t, j] ye[slot[t, j]]), f32, j order, one rounding
//   combine_bwd  dye[r] = bf16(gate[src[r]] dy[src[r] / k]);  dgate[i] = <dy[t], ye[slot[i]]> in f32
//   route_bwd    dlogits = the backward of softmax, selection and renormalisation, plus the aux term
//
// No atomics anywhere: sums over tokens go through per-workgroup partials added in index order, the
// prefix count of `plan` through a per-workgroup histogram scanned by one thread per expert -- two
// runs give the same bits, and no result depends on how workgroups are scheduled.  The row kernels
// move O(T k H) bytes in 16-byte accesses and do nothing else.
//
// Top to bottom: route (+ its final sum), plan (three passes), the row kernels, route_bwd, the
// extern "C" entries with their host-side validation.
#include "common.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int kMaxE = 128;        // two experts per lane of one wave
constexpr int kMaxK = 8;
constexpr int kRouteTokens = 16;  // tokens per workgroup of the route kernel: 4 per wave
constexpr int kPlanBlock = 1024;  // items per workgroup of the plan passes: 16 waves

// (value, expert) order of the selection: the larger stored value, ties to the lower index
__device__ __forceinline__ bool better(float v, int e, float bv, int be) { return v > bv || (v == bv && e < be); }

// ---- route ---------------------------------------------------------------------------------------
// One wave per token, lane l holds experts l and l + 64.  The wave's per-expert sums of p and of the
// selections stay in registers over its tokens; the workgroup's four waves add up through LDS in wave
// order into one partial row (part_p / part_c [workgroups, E]).
__global__ __launch_bounds__(256) void moe_route_kernel(const uint16_t* __restrict__ logits, int64_t ldl, int T, int E,
                                                        int k, int norm, int32_t* __restrict__ idx,
                                                        float* __restrict__ gate, float* __restrict__ probs,
                                                        float* __restrict__ part_p, int32_t* __restrict__ part_c) {
  __shared__ float sh_p[4][kMaxE];
  __shared__ int sh_c[4][kMaxE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int e0 = lane, e1 = lane + 64;
  const bool has0 = e0 < E, has1 = e1 < E;
  float ps0 = 0.0f, ps1 = 0.0f;
  int c0 = 0, c1 = 0;
  const int t0 = blockIdx.x * kRouteTokens + w * (kRouteTokens / 4);
  for (int i = 0; i < kRouteTokens / 4; ++i) {
    const int t = t0 + i;   // wave-uniform
    if (t >= T) break;
    const uint16_t* row = logits + (int64_t)t * ldl;
    const float v0 = has0 ? bf2f(row[e0]) : -INFINITY;
    const float v1 = has1 ? bf2f(row[e1]) : -INFINITY;
    // softmax over all E stored values, f32 (expf: the accurate one; a row is a few hundred bytes)
    const float m = wave_max(fmaxf(v0, v1));
    const float x0 = has0 ? expf(v0 - m) : 0.0f;
    const float x1 = has1 ? expf(v1 - m) : 0.0f;
    const float sum = wave_sum(x0 + x1);
    const float p0 = x0 / sum, p1 = x1 / sum;
    if (has0) probs[(int64_t)t * E + e0] = p0;
    if (has1) probs[(int64_t)t * E + e1] = p1;
    ps0 += p0;
    ps1 += p1;
    // top-k: k rounds of a wave argmax over the experts not yet taken (a NaN never wins a round
    // while another value is left)
    const float k0 = v0 == v0 ? v0 : -INFINITY, k1 = v1 == v1 ? v1 : -INFINITY;
    bool tk0 = !has0, tk1 = !has1;
    int my_e = 0;
    float my_p = 0.0f;   // lane j keeps the j-th choice
    for (int j = 0; j < k; ++j) {
      float bv = -INFINITY;
      int be = INT_MAX;
      if (!tk0) { bv = k0; be = e0; }
      if (!tk1 && better(k1, e1, bv, be)) { bv = k1; be = e1; }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oe = __shfl_xor(be, o, 64);
        if (better(ov, oe, bv, be)) { bv = ov; be = oe; }
      }
      be = __builtin_amdgcn_readfirstlane(be);   // the same in every lane: k <= E leaves a candidate
      if (be == e0) tk0 = true;
      if (be == e1) tk1 = true;
      const float pj = __shfl(be >= 64 ? p1 : p0, be & 63, 64);
      if (lane == j) { my_e = be; my_p = pj; }
    }
    const float s = wave_sum(lane < k ? my_p : 0.0f);
    if (lane < k) {
      idx[(int64_t)t * k + lane] = my_e;
      gate[(int64_t)t * k + lane] = norm ? my_p / s : my_p;
    }
    c0 += (has0 && tk0) ? 1 : 0;
    c1 += (has1 && tk1) ? 1 : 0;
  }
  sh_p[w][e0] = ps0; sh_p[w][e1] = ps1;
  sh_c[w][e0] = c0;  sh_c[w][e1] = c1;
  __syncthreads();
  if ((int)threadIdx.x < E) {
    const int e = threadIdx.x;
    part_p[(int64_t)blockIdx.x * E + e] = ((sh_p[0][e] + sh_p[1][e]) + sh_p[2][e]) + sh_p[3][e];
    part_c[(int64_t)blockIdx.x * E + e] = sh_c[0][e] + sh_c[1][e] + sh_c[2][e] + sh_c[3][e];
  }
}

// counts[e], and aux = E sum_e f_e P_e: thread e adds the partial rows in workgroup order, thread 0
// the E terms in expert order
__global__ __launch_bounds__(kMaxE) void moe_route_final_kernel(const float* __restrict__ part_p,
                                                                const int32_t* __restrict__ part_c, int nblk, int T,
                                                                int E, int k, int32_t* __restrict__ counts,
                                                                float* __restrict__ aux) {
  __shared__ float term[kMaxE];
  const int e = threadIdx.x;
  float P = 0.0f;
  int c = 0;
  if (e < E) {
    for (int b = 0; b < nblk; ++b) {
      P += part_p[(int64_t)b * E + e];
      c += part_c[(int64_t)b * E + e];
    }
    counts[e] = c;
  }
  term[e] = e < E ? ((float)c / ((float)T * (float)k)) * (P / (float)T) : 0.0f;
  __syncthreads();
  if (e == 0) {
    float s = 0.0f;
    for (int i = 0; i < E; ++i) s += term[i];
    aux[0] = (float)E * s;
  }
}

// ---- plan ----------------------------------------------------------------------------------------
// Pass 1, one workgroup per kPlanBlock items: an item's rank among the workgroup's earlier items of
// its expert (left in slot[]), and the workgroup's histogram hist[b, E].  Inside a wave the lanes of
// one expert find each other with 7 ballots over the expert's bits; across the 16 waves one thread
// per expert scans the wave totals in LDS.
// Pass 2, one thread per expert: the exclusive scan of hist over the workgroups, in place, and the
// totals in row nblk.
// Pass 3: pos = scanned base + rank -> slot and src; the rows past an expert's total get src = -1.
// An index outside [0, E) is an item nobody owns: slot -1, not counted.
__global__ __launch_bounds__(kPlanBlock) void moe_plan_rank_kernel(const int32_t* __restrict__ idx, int N, int E,
                                                                   int32_t* __restrict__ slot,
                                                                   int32_t* __restrict__ hist) {
  __shared__ int cnt[kPlanBlock / 64][kMaxE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < (kPlanBlock / 64) * kMaxE; i += kPlanBlock) (&cnt[0][0])[i] = 0;
  __syncthreads();
  const int i = blockIdx.x * kPlanBlock + threadIdx.x;
  const int e = i < N ? idx[i] : -1;
  const bool valid = (unsigned)e < (unsigned)E;
  unsigned long long same = __ballot(valid);
#pragma unroll
  for (int bit = 0; bit < 7; ++bit) {
    const bool on = (e >> bit) & 1;
    const unsigned long long b = __ballot(valid && on);
    same &= on ? b : ~b;
  }
  const int rank = __popcll(same & ((1ull << lane) - 1ull));
  if (valid && rank == __popcll(same) - 1) cnt[w][e] = rank + 1;   // the expert's last lane: its wave total
  __syncthreads();
  if ((int)threadIdx.x < E) {
    int run = 0;
    for (int j = 0; j < kPlanBlock / 64; ++j) {
      const int c = cnt[j][threadIdx.x];
      cnt[j][threadIdx.x] = run;
      run += c;
    }
    hist[(int64_t)blockIdx.x * E + threadIdx.x] = run;
  }
  __syncthreads();
  if (i < N) slot[i] = valid ? cnt[w][e] + rank : -1;
}

__global__ __launch_bounds__(kMaxE) void moe_plan_scan_kernel(int32_t* __restrict__ hist, int nblk, int E) {
  const int e = threadIdx.x;
  if (e >= E) return;
  int run = 0;
  for (int b = 0; b < nblk; ++b) {
    const int h = hist[(int64_t)b * E + e];
    hist[(int64_t)b * E + e] = run;
    run += h;
  }
  hist[(int64_t)nblk * E + e] = run;
}

__global__ __launch_bounds__(256) void moe_plan_place_kernel(const int32_t* __restrict__ idx,
                                                             const int32_t* __restrict__ hist, int N, int E, int C,
                                                             int nblk, int32_t* __restrict__ slot,
                                                             int32_t* __restrict__ src) {
  const int R = E * C;
  const int64_t n = N > R ? N : R;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    if (i < N) {
      const int e = idx[i];
      int s = -1;
      if ((unsigned)e < (unsigned)E) {
        const int pos = hist[(int64_t)(i / kPlanBlock) * E + e] + slot[i];
        if (pos < C) {
          s = e * C + pos;
          src[s] = (int)i;
        }
      }
      slot[i] = s;
    }
    if (i < R) {   // the rows no item fills (disjoint from the rows written above: those have pos < total)
      const int e = (int)(i / C);
      if ((int)i - e * C >= hist[(int64_t)nblk * E + e]) src[i] = -1;
    }
  }
}

// ---- the row kernels: one thread per 8 columns -----------------------------------------------------
__global__ __launch_bounds__(256) void moe_dispatch_kernel(const uint16_t* __restrict__ x, int64_t ldx,
                                                           const int32_t* __restrict__ src,
                                                           uint16_t* __restrict__ xe, int64_t ldxe, int N, int k,
                                                           int64_t R, int cpr) {
  const int64_t total = R * cpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cpr;
    const int c = (int)(i - r * cpr) * 8;
    const int s = src[r];
    bf16x8 v{{0u, 0u, 0u, 0u}};
    if ((unsigned)s < (unsigned)N) v = ld8(x + (int64_t)(s / k) * ldx + c);
    st8(xe + r * ldxe + c, v);
  }
}

__global__ __launch_bounds__(256) void moe_combine_kernel(const uint16_t* __restrict__ ye, int64_t ldye,
                                                          const int32_t* __restrict__ slot,
                                                          const float* __restrict__ gate,
                                                          const uint16_t* __restrict__ residual, int64_t ldr,
                                                          uint16_t* __restrict__ y, int64_t ldy, int64_t T, int k,
                                                          int R, int cpr) {
  const int64_t total = T * cpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = i / cpr;
    const int c = (int)(i - t * cpr) * 8;
    float acc[8];
    if (residual) {
      unpack8(ld8(residual + t * ldr + c), acc);
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] = 0.0f;
    }
    for (int j = 0; j < k; ++j) {
      const int s = slot[t * k + j];
      if ((unsigned)s >= (unsigned)R) continue;   // dropped
      const float g = gate ? gate[t * k + j] : 1.0f;
      float v[8];
      unpack8(ld8(ye + (int64_t)s * ldye + c), v);
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] = fmaf(g, v[q], acc[q]);
    }
    st8(y + t * ldy + c, pack8(acc));
  }
}

// One wave per expert row r: dye[r] and the row's dot product; every thread first zeroes the dgate of
// the dropped items it walks over (no row reaches those).
__global__ __launch_bounds__(256) void moe_combine_bwd_kernel(const uint16_t* __restrict__ dy, int64_t lddy,
                                                              const uint16_t* __restrict__ ye, int64_t ldye,
                                                              const int32_t* __restrict__ slot,
                                                              const int32_t* __restrict__ src,
                                                              const float* __restrict__ gate,
                                                              uint16_t* __restrict__ dye, int64_t lddye,
                                                              float* __restrict__ dgate, int N, int k, int R, int cpr) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256)
    if ((unsigned)slot[i] >= (unsigned)R) dgate[i] = 0.0f;
  const int lane = threadIdx.x & 63;
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < R; r += gridDim.x * 4) {
    const int s = src[r];   // wave-uniform
    uint16_t* out = dye + (int64_t)r * lddye;
    if ((unsigned)s >= (unsigned)N) {
      for (int c = lane; c < cpr; c += 64) st8(out + c * 8, bf16x8{{0u, 0u, 0u, 0u}});
      continue;
    }
    const float g = gate[s];
    const uint16_t* d = dy + (int64_t)(s / k) * lddy;
    const uint16_t* yr = ye + (int64_t)r * ldye;
    float acc = 0.0f;
    for (int c = lane; c < cpr; c += 64) {
      float dv[8], yv[8], o[8];
      unpack8(ld8(d + c * 8), dv);
      unpack8(ld8(yr + c * 8), yv);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        o[q] = g * dv[q];
        acc = fmaf(dv[q], yv[q], acc);
      }
      st8(out + c * 8, pack8(o));
    }
    acc = wave_sum(acc);
    if (lane == 0) dgate[s] = acc;
  }
}

// ---- route backward --------------------------------------------------------------------------------
// One wave per token.  With s = sum_j p[idx_j] and gate_j = p[idx_j] / s (norm) or p[idx_j]:
//   dp[idx_j] = (dgate_j - sum_i dgate_i gate_i) / s   |   dgate_j
//   dp[e]    += d_aux E f_e / T                          (aux = E sum_e f_e mean_t p[t, e]; f_e constant)
//   dlogit[e] = p[e] (dp[e] - sum_e' p[e'] dp[e'])
__global__ __launch_bounds__(256) void moe_route_bwd_kernel(const float* __restrict__ dgate,
                                                            const float* __restrict__ probs,
                                                            const int32_t* __restrict__ idx,
                                                            const int32_t* __restrict__ counts,
                                                            const float* __restrict__ d_aux, int norm,
                                                            uint16_t* __restrict__ dlogits, int64_t ldl, int T, int E,
                                                            int k) {
  const int lane = threadIdx.x & 63;
  const int e0 = lane, e1 = lane + 64;
  const bool has0 = e0 < E, has1 = e1 < E;
  const float da = d_aux ? d_aux[0] : 0.0f;
  const float fk = (float)T * (float)k;
  const float a0 = has0 ? da * (float)E * ((float)counts[e0] / fk) / (float)T : 0.0f;
  const float a1 = has1 ? da * (float)E * ((float)counts[e1] / fk) / (float)T : 0.0f;
  for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += gridDim.x * 4) {
    const float p0 = has0 ? probs[(int64_t)t * E + e0] : 0.0f;
    const float p1 = has1 ? probs[(int64_t)t * E + e1] : 0.0f;
    int my_e = -1;
    float my_d = 0.0f, my_p = 0.0f;   // lane j: the j-th choice
    if (lane < k) {
      my_e = idx[(int64_t)t * k + lane];
      my_d = dgate[(int64_t)t * k + lane];
      if ((unsigned)my_e < (unsigned)E) my_p = probs[(int64_t)t * E + my_e];
    }
    if (norm) {
      const float s = wave_sum(my_p);
      const float dot = wave_sum(my_d * (my_p / s));
      my_d = (my_d - dot) / s;
    }
    float dp0 = a0, dp1 = a1;
    for (int j = 0; j < k; ++j) {
      const int e = __shfl(my_e, j, 64);
      const float d = __shfl(my_d, j, 64);
      if (e == e0) dp0 += d;
      if (e == e1) dp1 += d;
    }
    const float inner = wave_sum(fmaf(p0, dp0, p1 * dp1));
    uint16_t* row = dlogits + (int64_t)t * ldl;
    if (has0) row[e0] = f2bf(p0 * (dp0 - inner));
    if (has1) row[e1] = f2bf(p1 * (dp1 - inner));
    for (int64_t c = E + lane; c < ldl; c += 64) row[c] = 0;   // the padded columns
  }
}

// ---- host side -------------------------------------------------------------------------------------
constexpr int64_t kI32 = 2147483647;

// the routing problem's sizes: PT_EINVAL, then what the kernels do not cover
int sizes_ok(int64_t T, int64_t E, int64_t k) {
  if (T < 1 || E < 1 || k < 1) return PT_EINVAL;
  if (E > kMaxE || k > kMaxK || k > E || T * k > kI32) return PT_EUNSUPPORTED;
  return PT_OK;
}
// a row kernel's: R expert rows of H columns besides the T k items
int rows_ok(int64_t T, int64_t k, int64_t R, int64_t H) {
  if (T < 1 || k < 1 || R < 1 || H < 1) return PT_EINVAL;
  if (k > kMaxK || (H & 63) || T * k > kI32 || R > kI32 || H > kI32) return PT_EUNSUPPORTED;
  return PT_OK;
}
bool row_aligned(const void* p, int64_t ld, int64_t H) { return pt_aligned16(p) && (ld & 7) == 0 && ld >= H; }

int stream_grid(int64_t threads) {
  const int64_t g = (threads + 255) / 256;
  return (int)(g < PT_STREAM_GRID_CAP * 2 ? g : PT_STREAM_GRID_CAP * 2);
}
int64_t route_blocks(int64_t T) { return (T + kRouteTokens - 1) / kRouteTokens; }
int64_t plan_blocks(int64_t N) { return (N + kPlanBlock - 1) / kPlanBlock; }

}  // namespace

extern "C" {

int pt_moe_route_workspace(int64_t T, int64_t E) {
  const int rc = sizes_ok(T, E, 1);
  if (rc != PT_OK) return rc;
  const int64_t words = 2 * route_blocks(T) * E;
  return words > kI32 ? PT_EUNSUPPORTED : (int)words;
}

int pt_moe_route(const void* logits, int64_t ldl, int64_t T, int64_t E, int64_t k, int norm_topk, int32_t* idx,
                 float* gate, float* probs, int32_t* counts, float* aux, void* workspace, hipStream_t stream) {
  if (!logits || !idx || !gate || !probs || !counts || !aux || !workspace) return PT_EINVAL;
  const int rc = sizes_ok(T, E, k);
  if (rc != PT_OK) return rc;
  if (ldl < E) return PT_EINVAL;
  if (T * ldl > kI32 * 2 || 2 * route_blocks(T) * E > kI32) return PT_EUNSUPPORTED;
  const int nblk = (int)route_blocks(T);
  float* part_p = (float*)workspace;
  int32_t* part_c = (int32_t*)workspace + (int64_t)nblk * E;
  moe_route_kernel<<<nblk, 256, 0, stream>>>((const uint16_t*)logits, ldl, (int)T, (int)E, (int)k, norm_topk ? 1 : 0,
                                             idx, gate, probs, part_p, part_c);
  PT_CHECK_LAUNCH();
  moe_route_final_kernel<<<1, kMaxE, 0, stream>>>(part_p, part_c, nblk, (int)T, (int)E, (int)k, counts, aux);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

int pt_moe_plan_block(void) { return kPlanBlock; }

int pt_moe_plan_workspace(int64_t T, int64_t E, int64_t k) {
  const int rc = sizes_ok(T, E, k);
  if (rc != PT_OK) return rc;
  const int64_t words = (plan_blocks(T * k) + 1) * E;
  return words > kI32 ? PT_EUNSUPPORTED : (int)words;
}

int pt_moe_plan(const int32_t* idx, int64_t T, int64_t E, int64_t k, int64_t C, int32_t* slot, int32_t* src,
                int32_t* workspace, hipStream_t stream) {
  if (!idx || !slot || !src || !workspace || C < 1) return PT_EINVAL;
  const int rc = sizes_ok(T, E, k);
  if (rc != PT_OK) return rc;
  if (E * C > kI32 || (plan_blocks(T * k) + 1) * E > kI32) return PT_EUNSUPPORTED;
  const int N = (int)(T * k), nblk = (int)plan_blocks(T * k);
  moe_plan_rank_kernel<<<nblk, kPlanBlock, 0, stream>>>(idx, N, (int)E, slot, workspace);
  PT_CHECK_LAUNCH();
  moe_plan_scan_kernel<<<1, kMaxE, 0, stream>>>(workspace, nblk, (int)E);
  PT_CHECK_LAUNCH();
  const int64_t n = N > E * C ? N : E * C;
  moe_plan_place_kernel<<<stream_grid(n), 256, 0, stream>>>(idx, workspace, N, (int)E, (int)C, nblk, slot, src);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

int pt_moe_dispatch(const void* x, int64_t ldx, const int32_t* src, void* xe, int64_t ldxe, int64_t T, int64_t k,
                    int64_t R, int64_t H, hipStream_t stream) {
  if (!x || !src || !xe) return PT_EINVAL;
  const int rc = rows_ok(T, k, R, H);
  if (rc != PT_OK) return rc;
  if (!row_aligned(x, ldx, H) || !row_aligned(xe, ldxe, H)) return PT_EALIGN;
  moe_dispatch_kernel<<<stream_grid(R * (H / 8)), 256, 0, stream>>>((const uint16_t*)x, ldx, src, (uint16_t*)xe, ldxe,
                                                                    (int)(T * k), (int)k, R, (int)(H / 8));
  PT_CHECK_LAUNCH();
  return PT_OK;
}

int pt_moe_combine(const void* ye, int64_t ldye, const int32_t* slot, const float* gate, const void* residual,
                   int64_t ldr, void* y, int64_t ldy, int64_t T, int64_t k, int64_t R, int64_t H, hipStream_t stream) {
  if (!ye || !slot || !y) return PT_EINVAL;
  const int rc = rows_ok(T, k, R, H);
  if (rc != PT_OK) return rc;
  if (!row_aligned(ye, ldye, H) || !row_aligned(y, ldy, H) || (residual && !row_aligned(residual, ldr, H)))
    return PT_EALIGN;
  moe_combine_kernel<<<stream_grid(T * (H / 8)), 256, 0, stream>>>((const uint16_t*)ye, ldye, slot, gate,
                                                                   (const uint16_t*)residual, ldr, (uint16_t*)y, ldy, T,
                                                                   (int)k, (int)R, (int)(H / 8));
  PT_CHECK_LAUNCH();
  return PT_OK;
}

int pt_moe_combine_bwd(const void* dy, int64_t lddy, const void* ye, int64_t ldye, const int32_t* slot,
                       const int32_t* src, const float* gate, void* dye, int64_t lddye, float* dgate, int64_t T,
                       int64_t k, int64_t R, int64_t H, hipStream_t stream) {
  if (!dy || !ye || !slot || !src || !gate || !dye || !dgate) return PT_EINVAL;
  const int rc = rows_ok(T, k, R, H);
  if (rc != PT_OK) return rc;
  if (!row_aligned(dy, lddy, H) || !row_aligned(ye, ldye, H) || !row_aligned(dye, lddye, H)) return PT_EALIGN;
  const int64_t want = (R + 3) / 4;
  const int grid = (int)(want < PT_STREAM_GRID_CAP * 2 ? want : PT_STREAM_GRID_CAP * 2);
  moe_combine_bwd_kernel<<<grid, 256, 0, stream>>>((const uint16_t*)dy, lddy, (const uint16_t*)ye, ldye, slot, src, gate,
                                                   (uint16_t*)dye, lddye, dgate, (int)(T * k), (int)k, (int)R,
                                                   (int)(H / 8));
  PT_CHECK_LAUNCH();
  return PT_OK;
}

int pt_moe_route_bwd(const float* dgate, const float* probs, const int32_t* idx, const int32_t* counts,
                     const float* d_aux, int norm_topk, void* dlogits, int64_t ldl, int64_t T, int64_t E, int64_t k,
                     hipStream_t stream) {
  if (!dgate || !probs || !idx || !counts || !dlogits) return PT_EINVAL;
  const int rc = sizes_ok(T, E, k);
  if (rc != PT_OK) return rc;
  if (ldl < E) return PT_EINVAL;
  if (T * ldl > kI32 * 2) return PT_EUNSUPPORTED;
  const int64_t want = (T + 3) / 4;
  const int grid = (int)(want < PT_STREAM_GRID_CAP * 2 ? want : PT_STREAM_GRID_CAP * 2);
  moe_route_bwd_kernel<<<grid, 256, 0, stream>>>(dgate, probs, idx, counts, d_aux, norm_topk ? 1 : 0,
                                                 (uint16_t*)dlogits, ldl, (int)T, (int)E, (int)k);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

}  // extern "C"
