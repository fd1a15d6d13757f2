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
// A second router, DeepSeek-V3 / Moonlight / GLM-4.5 / Kimi-K2 style (route_sigmoid, its backward and
// bias_update, below the softmax router's backward): sigmoid scores, a selection bias that moves the
// choice but not the gate, group-limited top-k, a routed scaling factor, and the auxiliary-loss-free
// bias step on the observed load.  Everything downstream of idx / gate is shared.
//
// No atomics anywhere: sums over tokens go through per-workgroup partials added in index order, the
// prefix count of `plan` through a per-workgroup histogram scanned by one thread per expert -- two
// runs give the same bits, and no result depends on how workgroups are scheduled.  The row kernels
// move O(T k H) bytes in 16-byte accesses and do nothing else.
//
// Top to bottom: route (+ its final sum), plan (three passes), the row kernels, route_bwd, the
// sigmoid router (route, backward, bias step), the extern "C" entries with their host-side validation.
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
// the E terms in expert order.  load (the sigmoid router's; NULL: none): load[e] += counts[e].
__global__ __launch_bounds__(kMaxE) void moe_route_final_kernel(const float* __restrict__ part_p,
                                                                const int32_t* __restrict__ part_c, int nblk, int T,
                                                                int E, int k, int32_t* __restrict__ counts,
                                                                float* __restrict__ aux, int32_t* __restrict__ load) {
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
    if (load) load[e] += c;
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

// ---- dropless plan ---------------------------------------------------------------------------------
// The same rank and scan passes, then segments instead of capacity slots: expert e's items take rows
// [seg[e], seg[e] + n_e) of one packed buffer in flat item order, every seg[e] a multiple of kSegAlign
// (the segment GEMMs' M-tile: csrc/gemm.hip), so a 128-row tile belongs to one expert.  R rows are
// allocated (the bound of kernels.moe_dropless_rows); seg[E] of them are in use.
constexpr int kSegAlign = 128;

// one workgroup: thread 0 adds the aligned totals in expert order, then every thread labels tiles
__global__ __launch_bounds__(kMaxE) void moe_plan_seg_kernel(const int32_t* __restrict__ hist, int nblk, int E,
                                                             int ntiles, int32_t* __restrict__ seg,
                                                             int32_t* __restrict__ tile_expert) {
  __shared__ int sh_seg[kMaxE + 1];
  if (threadIdx.x == 0) {
    int run = 0;
    for (int e = 0; e < E; ++e) {
      sh_seg[e] = run;
      run += (hist[(int64_t)nblk * E + e] + kSegAlign - 1) / kSegAlign * kSegAlign;
    }
    sh_seg[E] = run;
  }
  __syncthreads();
  for (int e = threadIdx.x; e <= E; e += kMaxE) seg[e] = sh_seg[e];
  for (int t = threadIdx.x; t < ntiles; t += kMaxE) {
    const int r = t * kSegAlign;
    int own = -1;   // the one expert with seg[e] <= r < seg[e + 1]; none past seg[E]
    for (int e = 0; e < E; ++e)
      if (r >= sh_seg[e] && r < sh_seg[e + 1]) own = e;
    tile_expert[t] = own;
  }
}

__global__ __launch_bounds__(256) void moe_plan_place_seg_kernel(const int32_t* __restrict__ idx,
                                                                 const int32_t* __restrict__ hist,
                                                                 const int32_t* __restrict__ seg,
                                                                 const int32_t* __restrict__ tile_expert, int N, int E,
                                                                 int R, int nblk, int32_t* __restrict__ slot,
                                                                 int32_t* __restrict__ src) {
  const int64_t n = N > R ? N : R;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    if (i < N) {
      const int e = idx[i];
      int s = -1;
      if ((unsigned)e < (unsigned)E) {
        s = seg[e] + hist[(int64_t)(i / kPlanBlock) * E + e] + slot[i];
        src[s] = (int)i;
      }
      slot[i] = s;
    }
    if (i < R) {   // padding rows and the unused tail (disjoint from the rows written above)
      const int e = tile_expert[i / kSegAlign];
      if (e < 0 || (int)i - seg[e] >= hist[(int64_t)nblk * E + e]) src[i] = -1;
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

// ---- sigmoid route ---------------------------------------------------------------------------------
// s = sigmoid(logit), key = s + bias[e]; the Kg of G contiguous expert groups with the largest sum of
// their two best keys stay, idx = the k best keys inside them, gate = scale s[idx] (/ their sum).
// One wave per token, lane l holds experts l and l + 64 as in the softmax router, but nothing here is
// a round of wave argmax.  Per token:
//   1. every group's two best keys at once: a segmented inclusive scan of (best, second) pairs along
//      the lanes, one per register slot, log2(E / G) steps of two lane shifts -- lane l merges lane
//      l - o only while that lane is still inside its group, so the groups need no alignment and no
//      power-of-two size; the last lane of a group ends up with its pair (a group across the 64-lane
//      seam: one pair per slot, merged on arrival)
//   2. lane g < G fetches group g's pair; its rank among the G scores is a count over G lane
//      broadcasts through scalar registers (v_readlane), and one ballot of rank < Kg is the kept mask
//   3. the top-k the same way: (key, expert) packed into one ordered integer per candidate, 0 for an
//      expert of a dropped group, and a candidate's rank is the number of larger integers among E
//      lane broadcasts.  The integers are distinct, so the ranks are, and rank r < k IS position r of
//      idx: every chosen lane stores its own entry, best first, with no selection rounds.
// The cost is E broadcasts and compares per token instead of k rounds of a 6-step argmax, and the
// group pass is 2 log2(E / G) + 4 lane moves.  A NaN key orders as -inf (it loses to every number and
// ties, by index, with other -inf keys), as in the softmax router.
constexpr int kMaxG = 16;

// the IEEE order of non-NaN floats as unsigned integers
__device__ __forceinline__ uint32_t ord_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// (ordered key, expert) -> the selection order in one integer: larger key first, then the lower expert
__device__ __forceinline__ uint64_t cand(uint32_t ok, int e) { return ((uint64_t)ok << 32) | (uint32_t)(kMaxE - 1 - e); }
__device__ __forceinline__ uint32_t lane_bcast(uint32_t v, int l) {   // l wave-uniform
  return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
// (a, b) = the two largest of {a, b, pa, pb}, a >= b; no NaNs reach here
__device__ __forceinline__ void top2_merge(float& a, float& b, float pa, float pb) {
  const float lo = fminf(a, pa);
  a = fmaxf(a, pa);
  b = fmaxf(lo, fmaxf(b, pb));
}
// the segmented scan of step 1 over one register slot; pos = the expert's position inside its group
__device__ __forceinline__ void group_top2_scan(float& a, float& b, int pos, int lane, int gs) {
  for (int o = 1; o < gs && o < 64; o <<= 1) {   // wave-uniform
    const float pa = __shfl_up(a, o, 64), pb = __shfl_up(b, o, 64);
    if (lane >= o && pos >= o) top2_merge(a, b, pa, pb);
  }
}

__global__ __launch_bounds__(256) void moe_route_sigmoid_kernel(
    const uint16_t* __restrict__ logits, int64_t ldl, const float* __restrict__ bias, int T, int E, int k, int G, int Kg,
    int norm, float scale, int32_t* __restrict__ idx, float* __restrict__ gate, float* __restrict__ probs,
    float* __restrict__ part_p, int32_t* __restrict__ part_c) {
  __shared__ float sh_p[4][kMaxE];
  __shared__ int sh_c[4][kMaxE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int e0 = lane, e1 = lane + 64;
  const bool has0 = e0 < E, has1 = e1 < E;
  const int gs = E / G;                      // experts per group
  const int g0 = e0 / gs, g1 = e1 / gs;      // (G == 1: 0 for every expert there is)
  const int pos0 = e0 - g0 * gs, pos1 = e1 - g1 * gs;
  // lane g < G: where group g's pair ends, per slot
  const int eF = lane * gs, eL = eF + gs - 1;
  const bool in0 = lane < G && eF < 64, in1 = lane < G && eL >= 64;
  const int l0 = (eL < 63 ? eL : 63) & 63, l1 = (eL - 64) & 63;
  const float b0 = (bias && has0) ? bias[e0] : 0.0f, b1 = (bias && has1) ? bias[e1] : 0.0f;
  const int n0 = E < 64 ? E : 64, n1 = E - n0;
  float qs0 = 0.0f, qs1 = 0.0f;
  int c0 = 0, c1 = 0;
  const int t0 = blockIdx.x * kRouteTokens + w * (kRouteTokens / 4);
  for (int i = 0; i < kRouteTokens / 4; ++i) {
    const int t = t0 + i;   // wave-uniform
    if (t >= T) break;
    const uint16_t* row = logits + (int64_t)t * ldl;
    // the accurate expf and an IEEE division: the scores are saved for the backward
    const float s0 = has0 ? 1.0f / (1.0f + expf(-bf2f(row[e0]))) : 0.0f;
    const float s1 = has1 ? 1.0f / (1.0f + expf(-bf2f(row[e1]))) : 0.0f;
    if (has0) probs[(int64_t)t * E + e0] = s0;
    if (has1) probs[(int64_t)t * E + e1] = s1;
    const float tot = wave_sum(s0 + s1);
    qs0 += s0 / tot;   // the aux loss runs on the normalised scores
    qs1 += s1 / tot;
    float k0 = (s0 + b0) + 0.0f, k1 = (s1 + b1) + 0.0f;   // (+ 0: no -0 in the integer order)
    k0 = (has0 && k0 == k0) ? k0 : -INFINITY;
    k1 = (has1 && k1 == k1) ? k1 : -INFINITY;
    uint32_t kept = 1u;
    if (G > 1) {
      float a0 = k0, m0 = -INFINITY, a1 = k1, m1 = -INFINITY;
      group_top2_scan(a0, m0, pos0, lane, gs);
      if (E > 64) group_top2_scan(a1, m1, pos1, lane, gs);
      float ga = -INFINITY, gb = -INFINITY;
      const float f0 = __shfl(a0, l0, 64), f1 = __shfl(m0, l0, 64);
      if (in0) top2_merge(ga, gb, f0, f1);
      if (E > 64) {
        const float h0 = __shfl(a1, l1, 64), h1 = __shfl(m1, l1, 64);
        if (in1) top2_merge(ga, gb, h0, h1);
      }
      float score = ga + gb;
      score = (lane < G && score == score) ? score : -INFINITY;
      int rank = 0;
      for (int j = 0; j < G; ++j) {
        const float sj = __uint_as_float(lane_bcast(__float_as_uint(score), j));
        rank += better(sj, j, score, lane) ? 1 : 0;
      }
      kept = (uint32_t)__ballot(lane < G && rank < Kg);
    }
    const bool v0 = has0 && ((kept >> g0) & 1u), v1 = has1 && ((kept >> g1) & 1u);
    const uint32_t o0 = v0 ? ord_key(k0) : 0u, o1 = v1 ? ord_key(k1) : 0u;   // an ordered -inf is > 0
    const uint64_t m0c = cand(o0, e0), m1c = cand(o1, e1);
    int r0 = 0, r1 = 0;
    for (int j = 0; j < n0; ++j) {
      const uint64_t c = cand(lane_bcast(o0, j), j);
      r0 += c > m0c ? 1 : 0;
      r1 += c > m1c ? 1 : 0;
    }
    for (int j = 0; j < n1; ++j) {
      const uint64_t c = cand(lane_bcast(o1, j), j + 64);
      r0 += c > m0c ? 1 : 0;
      r1 += c > m1c ? 1 : 0;
    }
    const bool sel0 = v0 && r0 < k, sel1 = v1 && r1 < k;   // k <= Kg E / G candidates: exactly k chosen
    float mul = scale;
    if (norm) mul = scale / (wave_sum((sel0 ? s0 : 0.0f) + (sel1 ? s1 : 0.0f)) + 1e-20f);
    if (sel0) {
      idx[(int64_t)t * k + r0] = e0;
      gate[(int64_t)t * k + r0] = s0 * mul;
    }
    if (sel1) {
      idx[(int64_t)t * k + r1] = e1;
      gate[(int64_t)t * k + r1] = s1 * mul;
    }
    c0 += sel0 ? 1 : 0;
    c1 += sel1 ? 1 : 0;
  }
  sh_p[w][e0] = qs0; sh_p[w][e1] = qs1;
  sh_c[w][e0] = c0;  sh_c[w][e1] = c1;
  __syncthreads();
  if ((int)threadIdx.x < E) {
    const int e = threadIdx.x;
    part_p[(int64_t)blockIdx.x * E + e] = ((sh_p[0][e] + sh_p[1][e]) + sh_p[2][e]) + sh_p[3][e];
    part_c[(int64_t)blockIdx.x * E + e] = sh_c[0][e] + sh_c[1][e] + sh_c[2][e] + sh_c[3][e];
  }
}

// One wave per token.  S = sum_i s[idx_i] + 1e-20, gate_j = scale s[idx_j] / S (norm) or scale s[idx_j]:
//   ds[idx_j] = (scale dgate_j - sum_i dgate_i gate_i) / S   |   scale dgate_j
//   ds[e]    += (dq_e - sum_e' q_e' dq_e') / sum_e' s_e',  dq_e = d_aux E f_e / T, q = s / sum s
//   dlogit[e] = ds[e] s[e] (1 - s[e])
__global__ __launch_bounds__(256) void moe_route_sigmoid_bwd_kernel(
    const float* __restrict__ dgate, const float* __restrict__ probs, const int32_t* __restrict__ idx,
    const float* __restrict__ gate, const int32_t* __restrict__ counts, const float* __restrict__ d_aux, int norm,
    float scale, uint16_t* __restrict__ dlogits, int64_t ldl, int T, int E, int k) {
  const int lane = threadIdx.x & 63;
  const int e0 = lane, e1 = lane + 64;
  const bool has0 = e0 < E, has1 = e1 < E;
  const float da = d_aux ? d_aux[0] : 0.0f;
  const float fk = (float)T * (float)k;
  const float a0 = has0 ? da * (float)E * ((float)counts[e0] / fk) / (float)T : 0.0f;
  const float a1 = has1 ? da * (float)E * ((float)counts[e1] / fk) / (float)T : 0.0f;
  for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += gridDim.x * 4) {
    const float s0 = has0 ? probs[(int64_t)t * E + e0] : 0.0f;
    const float s1 = has1 ? probs[(int64_t)t * E + e1] : 0.0f;
    int my_e = -1;
    float my_d = 0.0f, my_g = 0.0f, my_s = 0.0f;   // lane j: the j-th choice
    if (lane < k) {
      my_e = idx[(int64_t)t * k + lane];
      my_d = dgate[(int64_t)t * k + lane];
      my_g = gate[(int64_t)t * k + lane];
      if ((unsigned)my_e < (unsigned)E) my_s = probs[(int64_t)t * E + my_e];
    }
    if (norm) {
      const float S = wave_sum(my_s) + 1e-20f;
      const float dot = wave_sum(my_d * my_g);
      my_d = (scale * my_d - dot) / S;
    } else {
      my_d = scale * my_d;
    }
    float ds0 = 0.0f, ds1 = 0.0f;
    if (da != 0.0f) {   // wave-uniform
      const float tot = wave_sum(s0 + s1);
      const float inner = wave_sum(fmaf(s0 / tot, a0, (s1 / tot) * a1));
      ds0 = (a0 - inner) / tot;
      ds1 = (a1 - inner) / tot;
    }
    for (int j = 0; j < k; ++j) {
      const int e = (int)lane_bcast((uint32_t)my_e, j);
      const float d = __uint_as_float(lane_bcast(__float_as_uint(my_d), j));
      if (e == e0) ds0 += d;
      if (e == e1) ds1 += d;
    }
    uint16_t* row = dlogits + (int64_t)t * ldl;
    if (has0) row[e0] = f2bf(ds0 * (s0 * (1.0f - s0)));
    if (has1) row[e1] = f2bf(ds1 * (s1 * (1.0f - s1)));
    for (int64_t c = E + lane; c < ldl; c += 64) row[c] = 0;   // the padded columns
  }
}

// The auxiliary-loss-free balancing step, one workgroup: bias[e] += rate sign(sum load - E load[e])
// (int64: exact, a tie leaves the bias as it is), then load[e] = 0.
__global__ __launch_bounds__(kMaxE) void moe_bias_update_kernel(float* __restrict__ bias, int32_t* __restrict__ load,
                                                                int E, float rate) {
  __shared__ int sh_load[kMaxE];
  const int e = threadIdx.x;
  const int mine = e < E ? load[e] : 0;
  sh_load[e] = mine;
  __syncthreads();
  if (e >= E) return;
  int64_t total = 0;
  for (int i = 0; i < E; ++i) total += sh_load[i];
  const int64_t d = total - (int64_t)E * mine;
  if (d > 0) bias[e] += rate;
  if (d < 0) bias[e] -= rate;
  load[e] = 0;
}

// ---- host side -------------------------------------------------------------------------------------
constexpr int64_t kI32 = 2147483647;

// the routing problem's sizes: PT_EINVAL, then what the kernels do not cover
int sizes_ok(int64_t T, int64_t E, int64_t k) {
  if (T < 1 || E < 1 || k < 1) return PT_EINVAL;
  if (E > kMaxE || k > kMaxK || k > E || T * k > kI32) return PT_EUNSUPPORTED;
  return PT_OK;
}
// the sigmoid router's groups (sizes >= 1 checked by the caller): G | E, 1 <= Kg <= G <= 16, groups of
// two or more when there is more than one, and k candidates left inside the kept groups
int groups_ok(int64_t E, int64_t k, int64_t G, int64_t Kg) {
  if (G > kMaxG || Kg > G || E % G) return PT_EUNSUPPORTED;
  if ((G > 1 && E / G < 2) || k > Kg * (E / G)) return PT_EUNSUPPORTED;
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
  moe_route_final_kernel<<<1, kMaxE, 0, stream>>>(part_p, part_c, nblk, (int)T, (int)E, (int)k, counts, aux, nullptr);
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

int pt_moe_dropless_rows(int64_t T, int64_t E, int64_t k) {
  const int rc = sizes_ok(T, E, k);
  if (rc != PT_OK) return rc;
  const int64_t rows = (T * k + E * (kSegAlign - 1)) / kSegAlign * kSegAlign;
  return rows > kI32 ? PT_EUNSUPPORTED : (int)rows;
}

// slot [T, k], src [R], seg [E + 1], tile_expert [R / 128]; R >= pt_moe_dropless_rows, on the 128-grid
int pt_moe_plan_dropless(const int32_t* idx, int64_t T, int64_t E, int64_t k, int64_t R, int32_t* slot, int32_t* src,
                         int32_t* seg, int32_t* tile_expert, int32_t* workspace, hipStream_t stream) {
  if (!idx || !slot || !src || !seg || !tile_expert || !workspace) return PT_EINVAL;
  const int rc = sizes_ok(T, E, k);
  if (rc != PT_OK) return rc;
  if (R % kSegAlign || R < pt_moe_dropless_rows(T, E, k)) return PT_EINVAL;
  if (R > kI32 || (plan_blocks(T * k) + 1) * E > kI32) return PT_EUNSUPPORTED;
  const int N = (int)(T * k), nblk = (int)plan_blocks(T * k);
  moe_plan_rank_kernel<<<nblk, kPlanBlock, 0, stream>>>(idx, N, (int)E, slot, workspace);
  PT_CHECK_LAUNCH();
  moe_plan_scan_kernel<<<1, kMaxE, 0, stream>>>(workspace, nblk, (int)E);
  PT_CHECK_LAUNCH();
  moe_plan_seg_kernel<<<1, kMaxE, 0, stream>>>(workspace, nblk, (int)E, (int)(R / kSegAlign), seg, tile_expert);
  PT_CHECK_LAUNCH();
  const int64_t n = N > R ? N : R;
  moe_plan_place_seg_kernel<<<stream_grid(n), 256, 0, stream>>>(idx, workspace, seg, tile_expert, N, (int)E, (int)R, nblk,
                                                                slot, src);
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

int pt_moe_route_sigmoid(const void* logits, int64_t ldl, const float* bias, int64_t T, int64_t E, int64_t k,
                         int64_t n_group, int64_t topk_group, int norm_topk, float scale, int32_t* idx, float* gate,
                         float* probs, int32_t* counts, float* aux, int32_t* load, void* workspace,
                         hipStream_t stream) {
  if (!logits || !idx || !gate || !probs || !counts || !aux || !workspace || n_group < 1 || topk_group < 1)
    return PT_EINVAL;
  const int rc = sizes_ok(T, E, k);
  if (rc != PT_OK) return rc;
  const int gc = groups_ok(E, k, n_group, topk_group);
  if (gc != PT_OK) return gc;
  if (ldl < E) return PT_EINVAL;
  if (T * ldl > kI32 * 2 || 2 * route_blocks(T) * E > kI32) return PT_EUNSUPPORTED;
  const int nblk = (int)route_blocks(T);
  float* part_p = (float*)workspace;
  int32_t* part_c = (int32_t*)workspace + (int64_t)nblk * E;
  moe_route_sigmoid_kernel<<<nblk, 256, 0, stream>>>((const uint16_t*)logits, ldl, bias, (int)T, (int)E, (int)k,
                                                     (int)n_group, (int)topk_group, norm_topk ? 1 : 0, scale, idx, gate,
                                                     probs, part_p, part_c);
  PT_CHECK_LAUNCH();
  moe_route_final_kernel<<<1, kMaxE, 0, stream>>>(part_p, part_c, nblk, (int)T, (int)E, (int)k, counts, aux, load);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

int pt_moe_route_sigmoid_bwd(const float* dgate, const float* probs, const int32_t* idx, const float* gate,
                             const int32_t* counts, const float* d_aux, int norm_topk, float scale, void* dlogits,
                             int64_t ldl, int64_t T, int64_t E, int64_t k, hipStream_t stream) {
  if (!dgate || !probs || !idx || !gate || !counts || !dlogits) return PT_EINVAL;
  const int rc = sizes_ok(T, E, k);
  if (rc != PT_OK) return rc;
  if (ldl < E) return PT_EINVAL;
  if (T * ldl > kI32 * 2) return PT_EUNSUPPORTED;
  const int64_t want = (T + 3) / 4;
  const int grid = (int)(want < PT_STREAM_GRID_CAP * 2 ? want : PT_STREAM_GRID_CAP * 2);
  moe_route_sigmoid_bwd_kernel<<<grid, 256, 0, stream>>>(dgate, probs, idx, gate, counts, d_aux, norm_topk ? 1 : 0, scale,
                                                         (uint16_t*)dlogits, ldl, (int)T, (int)E, (int)k);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

int pt_moe_bias_update(float* bias, int32_t* load, int64_t E, float rate, hipStream_t stream) {
  if (!bias || !load || E < 1) return PT_EINVAL;
  if (E > kMaxE) return PT_EUNSUPPORTED;
  moe_bias_update_kernel<<<1, kMaxE, 0, stream>>>(bias, load, (int)E, rate);
  PT_CHECK_LAUNCH();
  return PT_OK;
}

}  // extern "C"
