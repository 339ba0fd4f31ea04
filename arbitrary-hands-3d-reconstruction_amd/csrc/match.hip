// Matching decoded hands to ground truth (acrmi_match_hands, acrmi_match_gather, acrmi_match_accumulate).
// The rule, the recurrence and the LDS carve-up: csrc/match_plan.h; tests/match_ref.py restates them in numpy float64.
// fp64 arithmetic, every operation rounded on its own (-ffp-contract=off).
//
//   match_kernel             one wave per problem (frame, side).  The K + G rows and the truths' valid bytes are read once from
//                            global memory and staged in LDS (under 50 KB at n = 256, D = 3); lane l < K * G owns pair (l / G,
//                            l % G) and computes its cost sequentially over the points (match_pair_cost).  Then K rounds of the
//                            subset recurrence over the 2^G states, at most four states per lane (match_step), two (cnt, sum)
//                            buffers and a K x 256 byte choice table in LDS, a barrier per round.  Lane 0 picks the final state,
//                            walks back (match_finish) and writes the problem's outputs.  The only indices are the kernel's own
//                            masks and loop counters: nothing read from memory becomes an address.
//   match_gather_kernel      one thread per 16 bytes of the destination when W % 4 == 0 and both pointers are 16-byte aligned
//                            (VEC = 4), else one thread per float (VEC = 1).  The row's index is range-checked
//                            (match_index_ok) before it becomes an address; a row without a source is written as +0.
//   match_accumulate_kernel  one block of 8 threads, thread e owns board element e and loops over the frames in ascending order.
// No atomics, one writer per element.
#include "kernels.h"
#include "match_plan.h"

namespace acrmi {

__global__ void __launch_bounds__(MATCH_WAVE) match_kernel(MatchArgs a) {
  extern __shared__ double s_match[];
  const int K = a.K, G = a.G, n = a.n, D = a.D, nD = n * D;
  const MatchLds L = match_lds(K, G, n, D);
  unsigned char* base = (unsigned char*)s_match;
  double* s_cost = (double*)(base + L.cost);
  double* s_sum[2] = {(double*)(base + L.sum0), (double*)(base + L.sum1)};
  float* s_pred = (float*)(base + L.pred);
  float* s_truth = (float*)(base + L.truth);
  unsigned char* s_valid = base + L.valid;
  signed char* s_cnt[2] = {(signed char*)(base + L.cnt0), (signed char*)(base + L.cnt1)};
  signed char* s_choice = (signed char*)(base + L.choice);
  unsigned char* s_allow = base + L.allow;
  unsigned char* s_flagged = base + L.flagged;
  const int b = (int)(blockIdx.x >> 1), s = (int)(blockIdx.x & 1), lane = threadIdx.x;

  // stage the rows of the problem
  for (int idx = lane; idx < K * nD; idx += MATCH_WAVE) {
    const int i = idx / nD, r = idx - i * nD;
    s_pred[idx] = a.pred[((size_t)(b * K + i) * 2 + s) * nD + r];
  }
  for (int idx = lane; idx < G * nD; idx += MATCH_WAVE) {
    const int g = idx / nD, r = idx - g * nD;
    s_truth[idx] = a.truth[((size_t)(b * G + g) * 2 + s) * nD + r];
  }
  for (int idx = lane; idx < G * n; idx += MATCH_WAVE) {
    const int g = idx / n, j = idx - g * n;
    s_valid[idx] = !a.valid || a.valid[((size_t)(b * G + g) * 2 + s) * n + j] != 0 ? 1 : 0;
  }
  for (int m = lane; m < (1 << G); m += MATCH_WAVE) {
    s_cnt[0][m] = m == 0 ? 0 : -1;
    s_sum[0][m] = 0.0;
  }
  __syncthreads();

  // the cost and the allowed byte of the lane's pair
  if (lane < K * G) {
    const int i = lane / G, g = lane - i * G;
    const size_t prow = (size_t)(b * K + i) * 2 + s, trow = (size_t)(b * G + g) * 2 + s;
    const bool flagged = !a.flags || match_flagged(a.flags[prow * a.flag_stride]);
    const bool tvalid = !a.truth_valid || a.truth_valid[trow] != 0;
    float t[3] = {0.f, 0.f, 0.f};
    if (a.trans) {
      t[0] = a.trans[prow * D];
      t[1] = a.trans[prow * D + 1];
      if (D == 3) t[2] = a.trans[prow * D + 2];
    }
    double cost = 0.0;
    const int count = match_pair_cost(s_pred + i * nD, s_truth + g * nD, s_valid + g * n, a.trans ? t : nullptr, n, D, &cost);
    s_cost[i * MATCH_MAX + g] = cost;
    s_allow[i * MATCH_MAX + g] = match_allowed(flagged, tvalid, count, a.min_points, cost, a.gate) ? 1 : 0;
    if (g == 0) s_flagged[i] = flagged ? 1 : 0;
  }
  __syncthreads();

  // K rounds over the 2^G states
  int cur = 0;
  for (int i = 0; i < K; ++i, cur ^= 1) {
    for (int m = lane; m < (1 << G); m += MATCH_WAVE) {
      int c;
      double sm;
      s_choice[i * MATCH_STATES + m] =
          (signed char)match_step(s_cnt[cur], s_sum[cur], s_cost + i * MATCH_MAX, s_allow + i * MATCH_MAX, G, m, &c, &sm);
      s_cnt[cur ^ 1][m] = (signed char)c;
      s_sum[cur ^ 1][m] = sm;
    }
    __syncthreads();
  }

  if (lane != 0) return;
  int match[MATCH_MAX], pred_of[MATCH_MAX];
  const int tp = match_finish(s_cnt[cur], s_sum[cur], s_choice, K, G, match);
#pragma unroll
  for (int g = 0; g < MATCH_MAX; ++g) pred_of[g] = -1;
  int n_flagged = 0, n_valid = 0;
  for (int i = 0; i < K; ++i) {
    const size_t prow = (size_t)(b * K + i) * 2 + s;
    const int g = match[i];
    a.match[prow] = g;
    a.cost[prow] = g >= 0 ? (float)s_cost[i * MATCH_MAX + g] : -1.f;
    n_flagged += s_flagged[i];
    // (g is one of the kernel's own loop counters, 0 <= g < G: match_step recorded it)
#pragma unroll
    for (int q = 0; q < MATCH_MAX; ++q)
      if (q == g) pred_of[q] = i;
  }
  for (int g = 0; g < G; ++g) {
    const size_t trow = (size_t)(b * G + g) * 2 + s;
    const bool tvalid = !a.truth_valid || a.truth_valid[trow] != 0;
    n_valid += tvalid ? 1 : 0;
    int p = -1;
#pragma unroll
    for (int q = 0; q < MATCH_MAX; ++q)
      if (q == g) p = pred_of[q];
    a.pred_of[trow] = p;
    a.group_out[trow] = tvalid ? (a.group ? a.group[trow] : s) : -1;
  }
  int32_t* cnt = a.counts + ((size_t)b * 2 + s) * 3;
  cnt[0] = tp;
  cnt[1] = n_flagged - tp;
  cnt[2] = n_valid - tp;
}

hipError_t launch_match(const MatchArgs& a, hipStream_t s) {
  if (a.B <= 0 || !match_sizes_ok(a.B, a.K, a.G, a.n, a.D) || !match_gate_ok(a.gate) || a.min_points < 1 || a.min_points > a.n)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(match_kernel, dim3(2u * (unsigned)a.B), dim3(MATCH_WAVE), match_lds(a.K, a.G, a.n, a.D).total, s, a);
  return hipGetLastError();
}

template <int VEC>
__global__ void __launch_bounds__(MATCH_GATHER_BLOCK) match_gather_kernel(MatchGatherArgs a) {
  const long long units = a.W / VEC;      // per row
  const long long at = (long long)blockIdx.x * MATCH_GATHER_BLOCK + threadIdx.x;
  if (at >= a.rows * units) return;
  const long long row = at / units, u = at - row * units;      // row = (b * Kd + q) * 2 + s
  const int s = (int)(row & 1);
  const long long b = (row >> 1) / a.Kd;
  const int32_t k = a.index[row];
  const bool ok = match_index_ok(k, a.Ks);
  if (VEC == 4) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) v = reinterpret_cast<const float4*>(a.src + ((size_t)(b * a.Ks + k) * 2 + s) * a.W)[u];
    reinterpret_cast<float4*>(a.dst + (size_t)row * a.W)[u] = v;
  } else {
    a.dst[(size_t)row * a.W + u] = ok ? a.src[((size_t)(b * a.Ks + k) * 2 + s) * a.W + u] : 0.f;
  }
}

hipError_t launch_match_gather(const MatchGatherArgs& a, hipStream_t s) {
  if (a.rows <= 0 || a.W < 1 || a.Ks < 1 || a.Kd < 1) return hipErrorInvalidValue;
  if (match_gather_vec4(a.src, a.dst, a.W))
    hipLaunchKernelGGL(match_gather_kernel<4>, dim3(match_gather_grid(a.rows, a.W / 4)), dim3(MATCH_GATHER_BLOCK), 0, s, a);
  else
    hipLaunchKernelGGL(match_gather_kernel<1>, dim3(match_gather_grid(a.rows, a.W)), dim3(MATCH_GATHER_BLOCK), 0, s, a);
  return hipGetLastError();
}

__global__ void __launch_bounds__(MATCH_WAVE) match_accumulate_kernel(MatchAccArgs a) {
  const int e = threadIdx.x;
  if (e >= MATCH_BOARD_WORDS) return;
  const int s = match_board_side(e), kind = match_board_kind(e);
  if (kind < 3) {
    int64_t v = a.board[e];
    for (int b = 0; b < a.B; ++b) v += (int64_t)a.counts[((size_t)b * 2 + s) * 3 + kind];
    a.board[e] = v;
  } else {
    double v = __longlong_as_double(a.board[e]);
    for (int b = 0; b < a.B; ++b)
      for (int i = 0; i < a.K; ++i) {
        const float c = a.cost[((size_t)b * a.K + i) * 2 + s];
        if (c >= 0.f) v = v + (double)c;
      }
    a.board[e] = __double_as_longlong(v);
  }
}

hipError_t launch_match_accumulate(const MatchAccArgs& a, hipStream_t s) {
  if (a.B <= 0 || a.K < 1 || a.K > MATCH_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(match_accumulate_kernel, dim3(1), dim3(MATCH_WAVE), 0, s, a);
  return hipGetLastError();
}

}  // namespace acrmi
