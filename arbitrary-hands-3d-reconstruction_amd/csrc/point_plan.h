// At which pixels the head towers run when the point heads serve several hands of each side (acrmi_point_heads_multi,
// ACRMI_OPT_POINT_HEADS_MULTI): the rule, once for the host and for the device.  Plain C++, no HIP:
// tools/point_plan_check.cpp compiles it alone; ACRMI_HD (csrc/roi_plan.h) is `__host__ __device__` when the translation unit
// is HIP.  Integers throughout, so host, device and the numpy restatement (tests/point_ref.py) agree exactly.
//
// Input, per frame: the K = max_hand picks of both sides as pick_centers_multi (csrc/heads.hip) leaves them - flag, flat index
// (0 for a rank without a detection: the placeholder samples pixel 0) and partner (the flat index of the other side's centre
// whose prior is added, -1 = none).  decode_multi_kernel reads, for row (side s, rank k), the params map of side s at
// flat[s][k] and, when partner[s][k] >= 0, the prior map of side s at partner[s][k].  So the towers of side s run at
//   own pixels    the distinct values of flat[s][0..K-1]: the params tower, the cam tower and the mix.  Pixel 0 appears once
//                 when any rank is a placeholder, and once when a flagged centre lies there as well
//   prior pixels  the distinct values of partner[s][k] >= 0: the prior tower of side s.  Two hands that share a partner give
//                 one point
// each list in the order of first appearance by rank, each of at most K entries.
//
// The picks workspace holds one PointPlan per frame (POINT_PLAN_INTS int32, written whole by the multi-pick kernel).
#pragma once
#include <stdint.h>

#include "roi_plan.h"      // ACRMI_HD

namespace acrmi {

constexpr int POINT_MAX_HAND = 8;            // = ACRMI_MAX_HAND

struct PointPlan {      // one frame
  int32_t n_own[2], n_prior[2];
  int32_t own[2][POINT_MAX_HAND];            // entries >= n_own[s] are -1
  int32_t prior[2][POINT_MAX_HAND];          // entries >= n_prior[s] are -1
};
constexpr int POINT_PLAN_INTS = 4 + 4 * POINT_MAX_HAND;
static_assert(sizeof(PointPlan) == POINT_PLAN_INTS * sizeof(int32_t), "PointPlan is plain int32");

// v[0..n-1] that are >= lo, each once, in the order of first appearance -> out[0..]; the rest of out[0..POINT_MAX_HAND-1] is
// -1.  Returns the count.  n <= POINT_MAX_HAND.
ACRMI_HD inline int32_t point_distinct(const int32_t* v, int n, int32_t lo, int32_t* out) {
  int32_t m = 0;
  for (int k = 0; k < n; ++k) {
    if (v[k] < lo) continue;
    bool seen = false;
    for (int j = 0; j < m; ++j) seen = seen || out[j] == v[k];
    if (!seen) out[m++] = v[k];
  }
  for (int j = m; j < POINT_MAX_HAND; ++j) out[j] = -1;
  return m;
}

// Side s of the plan from that side's K rows.  1 <= K <= POINT_MAX_HAND; flat entries are map pixels (0 .. 4095).
ACRMI_HD inline void point_plan_side(const int32_t* flat, const int32_t* partner, int K, int s, PointPlan* p) {
  p->n_own[s] = point_distinct(flat, K, 0, p->own[s]);
  p->n_prior[s] = point_distinct(partner, K, 0, p->prior[s]);
}

// Entry e of the fixed grid of 3 K entries per (frame, side): [0, K) the params tower at own pixel e, [K, 2K) the cam tower at
// own pixel e - K, [2K, 3K) the prior tower at prior pixel e - 2K.  Returns the pixel, -1 for an entry beyond its list;
// *tower = 0 params, 1 cam, 2 prior (the order of the packed towers, csrc/kernels.h).
ACRMI_HD inline int32_t point_plan_entry(const PointPlan& p, int s, int K, int e, int* tower) {
  const int t = e / K, i = e - t * K;
  *tower = t;
  if (t < 2) return i < p.n_own[s] ? p.own[s][i] : -1;
  return i < p.n_prior[s] ? p.prior[s][i] : -1;
}

}  // namespace acrmi
