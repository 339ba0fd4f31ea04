// The rule and the host side of matching decoded hands to ground truth (acrmi_match_hands, acrmi_match_gather,
// acrmi_match_accumulate; the kernels are in csrc/match.hip): an exact assignment per (frame, side), the
// gather into truth order, detection counts and the board that keeps them on the device.  Plain C++, no HIP:
// tools/match_check.cpp compiles it alone; ACRMI_HD (csrc/roi_plan.h) is `__host__ __device__` when the translation unit is HIP.
//
// THE RULE.  A PROBLEM is one (frame b, side s): predictions i = 0..K-1 and truths g = 0..G-1, 1 <= K, G <= 8, independent of
// each other; point sets of n points (1 <= n <= 256) of D coordinates, D = 2 (pixels) or 3 (metres).  Inputs fp32, arithmetic
// fp64, every operation rounded on its own (no contraction).
//   cost of (i, g)  point j counts when valid[b,g,s,j] != 0 (or no valid array) and all 2D coordinates (prediction and truth)
//                   are finite.  P = prediction + trans[b,i,s] when trans is given, added in fp64.
//                   d_j = sqrt(dx*dx + dy*dy) for D = 2, sqrt((dx*dx + dy*dy) + dz*dz) for D = 3, dx = P_x - G_x.
//                   cost = (sum of d_j in ascending j, a point that does not count adds +0) / count.
//   allowed pairs   the prediction's flag > 0.5 (read with a stride; NaN is not flagged; no flags: every prediction is flagged);
//                   truth_valid[b,g,s] != 0 (or no such array); count >= min_points; the cost finite and cost <= (double)gate.
//                   gate is finite and >= 0, or +inf; min_points in 1..n.
//   objective       among one-to-one matchings of allowed pairs the most pairs, among those the smallest cost sum.
//   recurrence      state m = bitmask of used truths, value (cnt, sum); dp[0] = (0, +0.0), every other state unreachable.  For
//                   i = 0..K-1 in order, for every m: start from dp[m] (prediction i stays unmatched); then for g ascending
//                   with bit g set in m, (i, g) allowed and dp[m ^ (1 << g)] reachable, the candidate (cnt + 1, sum +
//                   cost[i][g]) replaces the current best only on a strict improvement: a larger cnt, or an equal cnt and a
//                   smaller sum (match_step).  The choice (-1 or g) is recorded per (i, m).  The final state is the best over
//                   m ascending, strict improvement again; backtrack from i = K-1 down (match_finish).
//   outputs         match int32 [B,K,2]: the truth of each prediction or -1; pred_of int32 [B,G,2]: the inverse; cost fp32
//                   [B,K,2]: the matched pair's cost rounded to fp32, -1 when unmatched; counts int32 [B,2,3]: TP = matched
//                   pairs, FP = flagged predictions left unmatched, FN = valid truths left unmatched; group int32 [B,G,2]: the
//                   caller's group (default the side) where the truth is valid, else -1.
//   gather          dst[b,q,s,:] = src[b, index[b,q,s], s, :] for fp32 rows of any width W; an index outside [0, Ks) gives a
//                   row of +0 bytes; every index is range-checked before it becomes an address (match_index_ok).
//   the board       8 words of 8 bytes, per side [TP, FP, FN int64 | matched-cost sum fp64]: every element continues from the
//                   board's value and adds, in ascending frame (then prediction) order, the counts and the fp32 costs >= 0
//                   converted to double; one writer per element, no atomics: 2B frames in one call equal two calls of B.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "roi_plan.h"      // ACRMI_HD

namespace acrmi {

constexpr int MATCH_MAX = 8;                // predictions, truths of a problem
constexpr int MATCH_MAX_POINTS = 256;
constexpr int MATCH_WAVE = 64;              // threads of a problem: lane l < K * G owns pair (l / G, l % G)
constexpr int MATCH_STATES = 1 << MATCH_MAX;
constexpr int MATCH_BOARD_WORDS = 8;        // per side TP, FP, FN, cost sum
constexpr int MATCH_GATHER_BLOCK = 256;

inline bool match_sizes_ok(long long B, int K, int G, int n, int D) {
  if (B < 0 || K < 1 || K > MATCH_MAX || G < 1 || G > MATCH_MAX || n < 1 || n > MATCH_MAX_POINTS || (D != 2 && D != 3)) return false;
  return B * (K > G ? K : G) * 2 * n * D <= 0x7fffffffll;
}
// finite and >= 0, or +inf; NaN and negative values fail
inline bool match_gate_ok(float gate) { return gate >= 0.f; }
inline bool match_gather_sizes_ok(long long B, int Ks, int Kd, long long W) {
  if (B < 0 || Ks < 1 || Ks > MATCH_MAX || Kd < 1 || Kd > MATCH_MAX || W < 1 || W > 0x7fffffffll) return false;
  return B * (Ks > Kd ? Ks : Kd) * 2 <= 0x7fffffffll / W;
}
inline size_t match_board_bytes() { return MATCH_BOARD_WORDS * 8; }

ACRMI_HD inline bool match_finite(float x) { return fabsf(x) <= 3.4028234e38f; }
ACRMI_HD inline bool match_flagged(float flag) { return flag > 0.5f; }
// the gather's check: an index becomes an address only through this
ACRMI_HD inline bool match_index_ok(int32_t k, int Ks) { return k >= 0 && k < Ks; }

// The dynamic LDS of a problem, byte offsets: the fp64 arrays first, then the staged rows, then the bytes.
struct MatchLds {
  size_t cost;        // double [MATCH_MAX * MATCH_MAX]: cost[i * 8 + g]
  size_t sum0, sum1;  // double [MATCH_STATES] each: the two value buffers
  size_t pred;        // float [K * n * D]
  size_t truth;       // float [G * n * D]
  size_t valid;       // bytes [G * n]
  size_t cnt0, cnt1;  // int8 [MATCH_STATES] each: -1 = unreachable
  size_t choice;      // int8 [K * MATCH_STATES]
  size_t allow;       // bytes [MATCH_MAX * MATCH_MAX]: allow[i * 8 + g]
  size_t flagged;     // bytes [MATCH_MAX]
  size_t total;
};
ACRMI_HD inline MatchLds match_lds(int K, int G, int n, int D) {
  MatchLds L;
  size_t at = 0;
  L.cost = at;    at += (size_t)MATCH_MAX * MATCH_MAX * 8;
  L.sum0 = at;    at += (size_t)MATCH_STATES * 8;
  L.sum1 = at;    at += (size_t)MATCH_STATES * 8;
  L.pred = at;    at += (size_t)K * n * D * 4;
  L.truth = at;   at += (size_t)G * n * D * 4;
  L.valid = at;   at += (size_t)G * n;
  L.cnt0 = at;    at += MATCH_STATES;
  L.cnt1 = at;    at += MATCH_STATES;
  L.choice = at;  at += (size_t)K * MATCH_STATES;
  L.allow = at;   at += (size_t)MATCH_MAX * MATCH_MAX;
  L.flagged = at; at += MATCH_MAX;
  L.total = (at + 7) & ~(size_t)7;
  return L;
}

// The cost of one pair over staged rows: p, g the n * D coordinates of the prediction and the truth, valid n bytes (non-zero =
// the point may count), t the D values of trans or null.  Returns the count; *cost is only written with a count >= 1.
ACRMI_HD inline int match_pair_cost(const float* p, const float* g, const unsigned char* valid, const float* t, int n, int D, double* cost) {
  double sum = 0.0;
  int count = 0;
  for (int j = 0; j < n; ++j) {
    if (!valid[j]) continue;
    const float px = p[j * D], py = p[j * D + 1], gx = g[j * D], gy = g[j * D + 1];
    if (!(match_finite(px) && match_finite(py) && match_finite(gx) && match_finite(gy))) continue;
    double dx = (double)px, dy = (double)py;
    if (t) { dx = dx + (double)t[0]; dy = dy + (double)t[1]; }
    dx = dx - (double)gx;
    dy = dy - (double)gy;
    double d2 = dx * dx + dy * dy;
    if (D == 3) {
      const float pz = p[j * D + 2], gz = g[j * D + 2];
      if (!(match_finite(pz) && match_finite(gz))) continue;
      double dz = (double)pz;
      if (t) dz = dz + (double)t[2];
      dz = dz - (double)gz;
      d2 = d2 + dz * dz;
    }
    sum = sum + sqrt(d2);
    ++count;
  }
  if (count >= 1) *cost = sum / (double)count;
  return count;
}

ACRMI_HD inline bool match_allowed(bool flagged, bool truth_valid, int count, int min_points, double cost, float gate) {
  return flagged && truth_valid && count >= 1 && count >= min_points && fabs(cost) <= 1.7976931348623157e308 && cost <= (double)gate;
}

ACRMI_HD inline bool match_better(int cnt, double sum, int best_cnt, double best_sum) {
  return cnt > best_cnt || (cnt == best_cnt && sum < best_sum);
}

// One state m of round i: cnt / sum are the values before the round (cnt -1 = unreachable), cost_i / allow_i the G entries of
// prediction i.  -> the state's value after the round and the recorded choice (-1: prediction i stays unmatched, else g).
ACRMI_HD inline int match_step(const signed char* cnt, const double* sum, const double* cost_i, const unsigned char* allow_i, int G,
                               int m, int* out_cnt, double* out_sum) {
  int best_cnt = cnt[m], choice = -1;
  double best_sum = sum[m];
  for (int g = 0; g < G; ++g) {
    const int bit = 1 << g;
    if (!(m & bit) || !allow_i[g]) continue;
    const int prev = cnt[m ^ bit];
    if (prev < 0) continue;
    const double cand = sum[m ^ bit] + cost_i[g];
    if (match_better(prev + 1, cand, best_cnt, best_sum)) {
      best_cnt = prev + 1;
      best_sum = cand;
      choice = g;
    }
  }
  *out_cnt = best_cnt;
  *out_sum = best_sum;
  return choice;
}

// The final state and the way back: cnt / sum after round K - 1, choice[i * MATCH_STATES + m].  match[i] = the truth of
// prediction i or -1; returns the number of pairs.
ACRMI_HD inline int match_finish(const signed char* cnt, const double* sum, const signed char* choice, int K, int G, int* match) {
  int best_m = 0, best_cnt = -1;
  double best_sum = 0.0;
  for (int m = 0; m < (1 << G); ++m) {
    if (cnt[m] >= 0 && match_better(cnt[m], sum[m], best_cnt, best_sum)) {
      best_m = m;
      best_cnt = cnt[m];
      best_sum = sum[m];
    }
  }
  int m = best_m;
  for (int i = K - 1; i >= 0; --i) {
    const int g = choice[i * MATCH_STATES + m];
    match[i] = g;
    if (g >= 0) m ^= 1 << g;
  }
  return best_cnt;
}

// The whole recurrence on the host, one state after the other (the kernel runs the states of a round side by side):
// cost[i * 8 + g], allow[i * 8 + g] -> match[K]; returns the number of pairs.
inline int match_solve(const double* cost, const unsigned char* allow, int K, int G, int* match) {
  signed char cnt[2][MATCH_STATES], choice[MATCH_MAX * MATCH_STATES];
  double sum[2][MATCH_STATES];
  const int S = 1 << G;
  for (int m = 0; m < S; ++m) {
    cnt[0][m] = m == 0 ? 0 : -1;
    sum[0][m] = 0.0;
  }
  int cur = 0;
  for (int i = 0; i < K; ++i, cur ^= 1) {
    for (int m = 0; m < S; ++m) {
      int c;
      double s;
      choice[i * MATCH_STATES + m] = (signed char)match_step(cnt[cur], sum[cur], cost + i * MATCH_MAX, allow + i * MATCH_MAX, G, m, &c, &s);
      cnt[cur ^ 1][m] = (signed char)c;
      sum[cur ^ 1][m] = s;
    }
  }
  return match_finish(cnt[cur], sum[cur], choice, K, G, match);
}

// The accumulate kernel: thread e < MATCH_BOARD_WORDS owns board element e = side * 4 + k (k = 0 TP, 1 FP, 2 FN, 3 the cost sum).
ACRMI_HD inline int match_board_side(int e) { return e >> 2; }
ACRMI_HD inline int match_board_kind(int e) { return e & 3; }

// The gather's geometry: 16-byte accesses when the row width and both pointers allow, else 4-byte ones.
inline bool match_gather_vec4(const void* src, const void* dst, long long W) {
  return W % 4 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0;
}
inline unsigned match_gather_grid(long long rows, long long row_units) {
  return (unsigned)((rows * row_units + MATCH_GATHER_BLOCK - 1) / MATCH_GATHER_BLOCK);
}

}  // namespace acrmi
