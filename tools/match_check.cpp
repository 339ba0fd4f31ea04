// Stand-alone check of csrc/match_plan.h: the subset recurrence against exhaustive enumeration for all
// K, G <= 4 on integer costs with every allowed-mask density (count and cost equal exactly, and the matching it returns is a
// one-to-one matching of allowed pairs with that count and cost), the tie order, the pair cost (points that do not count, NaN /
// inf / 3e19 coordinates and trans), what is allowed, the LDS carve-up, one owner per board element, the gather's index check
// and geometry, and what is refused.  No GPU, no HIP:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/match_check.cpp -o match_check
//   (or: hipcc -x c++ -Xarch_host -fsanitize=address,undefined ...)  &&  ./match_check
// Exit status 0 and "ok" when every case holds.
#include "../arbitrary-hands-3d-reconstruction_amd/csrc/match_plan.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

using namespace acrmi;

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);           \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

// The objective by exhaustive enumeration: prediction i takes any free allowed truth or none.
static void enumerate(const double* cost, const unsigned char* allow, int K, int G, int i, unsigned used, int cnt, double sum, int* best_cnt,
                      double* best_sum) {
  if (i == K) {
    if (cnt > *best_cnt || (cnt == *best_cnt && sum < *best_sum)) {
      *best_cnt = cnt;
      *best_sum = sum;
    }
    return;
  }
  enumerate(cost, allow, K, G, i + 1, used, cnt, sum, best_cnt, best_sum);
  for (int g = 0; g < G; ++g)
    if (!(used & (1u << g)) && allow[i * MATCH_MAX + g])
      enumerate(cost, allow, K, G, i + 1, used | (1u << g), cnt + 1, sum + cost[i * MATCH_MAX + g], best_cnt, best_sum);
}

static void check_problem(const double* cost, const unsigned char* allow, int K, int G) {
  int match[MATCH_MAX];
  for (int i = 0; i < MATCH_MAX; ++i) match[i] = 99;
  const int pairs = match_solve(cost, allow, K, G, match);
  int want_cnt = -1;
  double want_sum = 0.0;
  enumerate(cost, allow, K, G, 0, 0u, 0, 0.0, &want_cnt, &want_sum);
  unsigned used = 0;
  int cnt = 0;
  double sum = 0.0;
  bool valid = true;
  for (int i = 0; i < K; ++i) {
    const int g = match[i];
    if (g == -1) continue;
    if (g < 0 || g >= G || (used & (1u << g)) || !allow[i * MATCH_MAX + g]) {
      valid = false;
      break;
    }
    used |= 1u << g;
    ++cnt;
    sum += cost[i * MATCH_MAX + g];
  }
  EXPECT(valid);
  EXPECT(pairs == want_cnt && cnt == want_cnt);
  EXPECT(sum == want_sum);      // integer costs: exact
}

static void check_recurrence() {
  std::mt19937 rng(24);
  double cost[MATCH_MAX * MATCH_MAX];
  unsigned char allow[MATCH_MAX * MATCH_MAX];
  long problems = 0;
  for (int K = 1; K <= 4; ++K)
    for (int G = 1; G <= 4; ++G) {
      const int pairs = K * G;
      for (int density = 0; density <= pairs; ++density) {
        // every mask of this density when there are few, else 200 random ones
        std::vector<int> pick(pairs, 0);
        std::fill(pick.begin(), pick.begin() + density, 1);
        std::sort(pick.begin(), pick.end());
        int trial = 0;
        const bool all = pairs <= 9;
        do {
          if (!all) std::shuffle(pick.begin(), pick.end(), rng);
          for (int rep = 0; rep < (all ? 2 : 1); ++rep) {
            std::memset(allow, 0, sizeof allow);
            for (int k = 0; k < MATCH_MAX * MATCH_MAX; ++k) cost[k] = -1e300;      // never read where it is not a pair
            for (int i = 0; i < K; ++i)
              for (int g = 0; g < G; ++g) {
                allow[i * MATCH_MAX + g] = (unsigned char)pick[i * G + g];
                cost[i * MATCH_MAX + g] = (double)(rng() % (rep ? 3 : 10));      // few values: many ties
              }
            check_problem(cost, allow, K, G);
            ++problems;
          }
          ++trial;
        } while (all ? std::next_permutation(pick.begin(), pick.end()) : trial < 200);
      }
    }
  std::printf("recurrence = enumeration on %ld problems\n", problems);
  // larger problems, every pair allowed and half of them
  for (int trial = 0; trial < 60; ++trial) {
    const int K = 5 + (int)(rng() % 4), G = 5 + (int)(rng() % 4);
    for (int i = 0; i < K; ++i)
      for (int g = 0; g < G; ++g) {
        cost[i * MATCH_MAX + g] = (double)(rng() % 7);
        allow[i * MATCH_MAX + g] = (unsigned char)(trial % 2 ? rng() % 2 : 1);
      }
    check_problem(cost, allow, K, G);
  }
}

static void check_tie_order() {
  double cost[MATCH_MAX * MATCH_MAX];
  unsigned char allow[MATCH_MAX * MATCH_MAX];
  int match[MATCH_MAX];
  for (int k = 0; k < MATCH_MAX * MATCH_MAX; ++k) {
    cost[k] = 2.0;
    allow[k] = 1;
  }
  // one prediction, identical truths: the lowest truth (the final state is the first best over m ascending)
  EXPECT(match_solve(cost, allow, 1, 3, match) == 1 && match[0] == 0);
  // identical predictions, one truth: the first prediction keeps it (a later equal candidate is no strict improvement)
  EXPECT(match_solve(cost, allow, 3, 1, match) == 1 && match[0] == 0 && match[1] == -1 && match[2] == -1);
  // 2 x 2, all equal: in the full state the candidate g = 0 comes first and the equal g = 1 does not replace it
  EXPECT(match_solve(cost, allow, 2, 2, match) == 2 && match[0] == 1 && match[1] == 0);
  // 3 x 3, all equal
  EXPECT(match_solve(cost, allow, 3, 3, match) == 3 && match[0] == 2 && match[1] == 1 && match[2] == 0);
  // more pairs beat a smaller sum: (0,0) alone costs 0, but (0,1) + (1,0) are two pairs
  cost[0 * MATCH_MAX + 0] = 0.0; cost[0 * MATCH_MAX + 1] = 5.0; cost[1 * MATCH_MAX + 0] = 5.0;
  allow[1 * MATCH_MAX + 1] = 0;
  EXPECT(match_solve(cost, allow, 2, 2, match) == 2 && match[0] == 1 && match[1] == 0);
  // nothing allowed
  std::memset(allow, 0, sizeof allow);
  EXPECT(match_solve(cost, allow, 8, 8, match) == 0);
  for (int i = 0; i < 8; ++i) EXPECT(match[i] == -1);
  // an unmatched first prediction: only (1, 0) is allowed
  allow[1 * MATCH_MAX + 0] = 1;
  EXPECT(match_solve(cost, allow, 2, 1, match) == 1 && match[0] == -1 && match[1] == 0);
  EXPECT(match_better(1, 9.0, 0, 0.0) && match_better(1, 1.0, 1, 2.0) && !match_better(1, 2.0, 1, 2.0) && !match_better(0, 0.0, 1, 9.0));
}

static void check_cost_and_allowed() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float p[6] = {0.f, 0.f, 3.f, 4.f, 1.f, 1.f}, g[6] = {3.f, 4.f, 3.f, 4.f, 1.f, 2.f};      // distances 5, 0, 1
  unsigned char v[3] = {1, 1, 1};
  double c = -1.0;
  EXPECT(match_pair_cost(p, g, v, nullptr, 3, 2, &c) == 3 && c == (5.0 + 0.0 + 1.0) / 3.0);
  v[1] = 0;
  EXPECT(match_pair_cost(p, g, v, nullptr, 3, 2, &c) == 2 && c == 3.0);
  v[0] = v[2] = 0;
  c = -7.0;
  EXPECT(match_pair_cost(p, g, v, nullptr, 3, 2, &c) == 0 && c == -7.0);      // not written without a counted point
  v[0] = v[1] = v[2] = 255;
  float q[6];
  std::memcpy(q, p, sizeof q);
  q[2] = nan;
  EXPECT(match_pair_cost(q, g, v, nullptr, 3, 2, &c) == 2 && c == 3.0);
  q[2] = -inf;
  EXPECT(match_pair_cost(p, q, v, nullptr, 3, 2, &c) == 2);
  const float t2[2] = {3.f, 4.f};
  EXPECT(match_pair_cost(p, g, v, t2, 3, 2, &c) == 3 && c == (0.0 + 5.0 + std::sqrt(9.0 + 9.0)) / 3.0);
  const float tn[2] = {nan, 0.f};      // a trans that is not finite: the points count, the cost is not finite
  EXPECT(match_pair_cost(p, g, v, tn, 3, 2, &c) == 3 && !(std::fabs(c) <= 1.7976931348623157e308));
  EXPECT(!match_allowed(true, true, 3, 1, c, inf));
  const float big[3] = {3e19f, -3e19f, 3e19f}, zero[3] = {0.f, 0.f, 0.f};      // finite: counted, nothing overflows in fp64
  const unsigned char one[1] = {1};
  EXPECT(match_pair_cost(big, zero, one, nullptr, 1, 3, &c) == 1 && std::isfinite(c) && c > 5e19);
  EXPECT(match_allowed(true, true, 1, 1, c, inf) && !match_allowed(true, true, 1, 1, c, 1e19f));
  const float p3[3] = {1.f, 2.f, 2.f};
  EXPECT(match_pair_cost(p3, zero, one, nullptr, 1, 3, &c) == 1 && c == 3.0);
  const float z3[3] = {1.f, 2.f, nan};      // the third coordinate decides as well
  EXPECT(match_pair_cost(z3, zero, one, nullptr, 1, 3, &c) == 0);
  // allowed: flag, truth, count, gate
  EXPECT(match_allowed(true, true, 1, 1, 0.0, 0.f) && !match_allowed(true, true, 1, 1, 1e-300, 0.f));
  EXPECT(!match_allowed(false, true, 5, 1, 0.0, inf) && !match_allowed(true, false, 5, 1, 0.0, inf));
  EXPECT(!match_allowed(true, true, 4, 5, 0.0, inf) && match_allowed(true, true, 5, 5, 0.0, inf) && !match_allowed(true, true, 0, 1, 0.0, inf));
  EXPECT(match_allowed(true, true, 1, 1, 2.5, 2.5f) && !match_allowed(true, true, 1, 1, (double)inf, inf));
  EXPECT(match_flagged(0.6f) && !match_flagged(0.5f) && !match_flagged(nan) && match_flagged(inf) && !match_flagged(-inf));
  EXPECT(match_gate_ok(0.f) && match_gate_ok(inf) && match_gate_ok(1e30f) && !match_gate_ok(nan) && !match_gate_ok(-1e-30f) && !match_gate_ok(-inf));
}

static void check_lds_and_sizes() {
  size_t largest = 0;
  for (int K = 1; K <= MATCH_MAX; ++K)
    for (int G = 1; G <= MATCH_MAX; ++G)
      for (int n : {1, 21, 64, 65, 255, 256})
        for (int D : {2, 3}) {
          const MatchLds L = match_lds(K, G, n, D);
          const size_t at[] = {L.cost, L.sum0, L.sum1, L.pred, L.truth, L.valid, L.cnt0, L.cnt1, L.choice, L.allow, L.flagged, L.total};
          const size_t size[] = {(size_t)MATCH_MAX * MATCH_MAX * 8, (size_t)MATCH_STATES * 8, (size_t)MATCH_STATES * 8, (size_t)K * n * D * 4,
                                 (size_t)G * n * D * 4, (size_t)G * n, (size_t)MATCH_STATES, (size_t)MATCH_STATES, (size_t)K * MATCH_STATES,
                                 (size_t)MATCH_MAX * MATCH_MAX, (size_t)MATCH_MAX};
          EXPECT(at[0] == 0);
          for (int k = 0; k < 11; ++k) EXPECT(at[k] + size[k] <= at[k + 1]);      // in order, no overlap
          EXPECT(L.cost % 8 == 0 && L.sum0 % 8 == 0 && L.sum1 % 8 == 0 && L.pred % 4 == 0 && L.truth % 4 == 0 && L.total % 8 == 0);
          EXPECT(L.total <= 64 * 1024);      // below the limit of a launch without an attribute
          largest = std::max(largest, L.total);
        }
  EXPECT((size_t)(2 * MATCH_MAX) * MATCH_MAX_POINTS * 3 * 4 < 50 * 1024);      // the staged rows alone
  std::printf("largest LDS of a problem: %zu bytes\n", largest);
  EXPECT(MATCH_MAX * MATCH_MAX <= MATCH_WAVE && (1 << MATCH_MAX) <= 4 * MATCH_WAVE);      // a lane per pair, four states per lane
  EXPECT(match_sizes_ok(0, 1, 1, 1, 2) && match_sizes_ok(67, 8, 8, 256, 3) && match_sizes_ok(174762, 8, 8, 256, 3));
  EXPECT(!match_sizes_ok(174763, 8, 8, 256, 3) && !match_sizes_ok(174763, 8, 1, 256, 3) && !match_sizes_ok(174763, 1, 8, 256, 3));
  EXPECT(!match_sizes_ok(-1, 1, 1, 1, 2) && !match_sizes_ok(1, 0, 1, 1, 2) && !match_sizes_ok(1, 9, 1, 1, 2) && !match_sizes_ok(1, 1, 0, 1, 2));
  EXPECT(!match_sizes_ok(1, 1, 9, 1, 2) && !match_sizes_ok(1, 1, 1, 0, 2) && !match_sizes_ok(1, 1, 1, 257, 2) && !match_sizes_ok(1, 1, 1, 1, 1));
  EXPECT(!match_sizes_ok(1, 1, 1, 1, 4) && match_sizes_ok(0x7fffffffll / 4, 1, 1, 1, 2) && !match_sizes_ok(0x7fffffffll / 4 + 1, 1, 1, 1, 2));
}

static void check_board_and_gather() {
  // one owner per board element: the eight threads name eight different (side, kind) and every one of them
  bool seen[2][4] = {};
  for (int e = 0; e < MATCH_BOARD_WORDS; ++e) {
    const int s = match_board_side(e), k = match_board_kind(e);
    EXPECT(s >= 0 && s < 2 && k >= 0 && k < 4 && !seen[s][k] && e == s * 4 + k);
    seen[s][k] = true;
  }
  EXPECT(match_board_bytes() == 64 && MATCH_BOARD_WORDS <= MATCH_WAVE);
  // the index check
  for (int Ks = 1; Ks <= MATCH_MAX; ++Ks) {
    EXPECT(match_index_ok(0, Ks) && match_index_ok(Ks - 1, Ks));
    EXPECT(!match_index_ok(-1, Ks) && !match_index_ok(Ks, Ks) && !match_index_ok(INT_MIN, Ks) && !match_index_ok(INT_MAX, Ks));
  }
  alignas(16) static float buf[16];
  EXPECT(match_gather_vec4(buf, buf + 4, 176) && match_gather_vec4(buf, buf, 4));
  EXPECT(!match_gather_vec4(buf + 1, buf, 176) && !match_gather_vec4(buf, buf + 2, 176) && !match_gather_vec4(buf, buf, 63) &&
         !match_gather_vec4(buf, buf, 2334) && !match_gather_vec4(buf, buf, 3));
  EXPECT(match_gather_grid(1, 1) == 1 && match_gather_grid(2, 128) == 1 && match_gather_grid(2, 129) == 2);
  EXPECT(match_gather_grid(0x7fffffffll, 1) == (0x7fffffffll + 255) / 256);
  EXPECT(match_gather_sizes_ok(0, 1, 1, 1) && match_gather_sizes_ok(67, 8, 8, 2334) && !match_gather_sizes_ok(1, 0, 1, 1));
  EXPECT(!match_gather_sizes_ok(1, 9, 1, 1) && !match_gather_sizes_ok(1, 1, 0, 1) && !match_gather_sizes_ok(1, 1, 9, 1) && !match_gather_sizes_ok(1, 1, 1, 0));
  EXPECT(!match_gather_sizes_ok(-1, 1, 1, 1) && match_gather_sizes_ok(1, 1, 1, 0x7fffffffll / 2) && !match_gather_sizes_ok(1, 1, 1, 0x7fffffffll / 2 + 1));
  EXPECT(!match_gather_sizes_ok(0x7fffffffll, 8, 8, 2334));
}

int main() {
  check_recurrence();
  check_tie_order();
  check_cost_and_allowed();
  check_lds_and_sizes();
  check_board_and_gather();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
