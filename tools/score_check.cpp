// Stand-alone check of csrc/score_plan.h against a plain restatement: Horn's matrix and the six-sweep
// cyclic Jacobi with loop indices instead of compile-time ones (equal bit for bit), the eigen-pair and the rotation it gives
// (proper, also for mirrored and planar point sets), the launch geometry (threads, LDS carve-up, one owner per board element),
// the board sizes, the row states (INT_MIN included), the bins (infinite and huge errors included) and what is refused.  No
// GPU, no HIP:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/score_check.cpp -o score_check
//   (or: hipcc -x c++ -Xarch_host -fsanitize=address,undefined ...)  &&  ./score_check
// Exit status 0 and "ok" when every case holds.
#include "../arbitrary-hands-3d-reconstruction_amd/csrc/score_plan.h"

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

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// The rule with run-time indices.
static double plain_horn(const double* S, double* q) {
  const double xx = S[0], xy = S[1], xz = S[2], yx = S[3], yy = S[4], yz = S[5], zx = S[6], zy = S[7], zz = S[8];
  std::vector<std::vector<double>> a(4, std::vector<double>(4, 0.0)), v(4, std::vector<double>(4, 0.0));
  a[0][0] = (xx + yy) + zz; a[1][1] = (xx - yy) - zz; a[2][2] = (yy - xx) - zz; a[3][3] = (zz - xx) - yy;
  a[0][1] = a[1][0] = yz - zy; a[0][2] = a[2][0] = zx - xz; a[0][3] = a[3][0] = xy - yx;
  a[1][2] = a[2][1] = xy + yx; a[1][3] = a[3][1] = zx + xz; a[2][3] = a[3][2] = yz + zy;
  for (int r = 0; r < 4; ++r) v[r][r] = 1.0;
  for (int sweep = 0; sweep < 6; ++sweep)
    for (int p = 0; p < 3; ++p)
      for (int k = p + 1; k < 4; ++k) {
        const double apq = a[p][k];
        if (apq == 0.0) continue;
        const double theta = (a[k][k] - a[p][p]) / (2.0 * apq);
        const double t = (theta < 0.0 ? -1.0 : 1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        a[p][p] = a[p][p] - t * apq;
        a[k][k] = a[k][k] + t * apq;
        a[p][k] = a[k][p] = 0.0;
        for (int r = 0; r < 4; ++r) {
          if (r != p && r != k) {
            const double arp = a[r][p], arq = a[r][k];
            a[r][p] = a[p][r] = c * arp - s * arq;
            a[r][k] = a[k][r] = s * arp + c * arq;
          }
          const double vrp = v[r][p], vrq = v[r][k];
          v[r][p] = c * vrp - s * vrq;
          v[r][k] = s * vrp + c * vrq;
        }
      }
  int best = 0;
  for (int k = 1; k < 4; ++k)
    if (a[k][k] > a[best][best]) best = k;
  for (int r = 0; r < 4; ++r) q[r] = v[r][best];
  return a[best][best];
}

static void products(const std::vector<double>& P, const std::vector<double>& G, double* S) {
  const size_t n = P.size() / 3;
  double mp[3] = {0, 0, 0}, mg[3] = {0, 0, 0};
  for (size_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) { mp[a] += P[3 * i + a]; mg[a] += G[3 * i + a]; }
  for (int a = 0; a < 3; ++a) { mp[a] /= (double)n; mg[a] /= (double)n; }
  for (int k = 0; k < 9; ++k) S[k] = 0.0;
  for (size_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) S[3 * a + b] += (P[3 * i + a] - mp[a]) * (G[3 * i + b] - mg[b]);
}

static void check_one(const double* S, double tol_scale) {
  double q[4], q2[4];
  const double lam = score_horn(S, q), lam2 = plain_horn(S, q2);
  EXPECT(same_bits(lam, lam2));
  for (int k = 0; k < 4; ++k) EXPECT(same_bits(q[k], q2[k]));
  // an eigen-pair of N, the largest; a unit quaternion; a proper rotation
  double a[4][4], big = 0.0;
  score_horn_matrix(S, a);
  for (int r = 0; r < 4; ++r)
    for (int k = 0; k < 4; ++k) big = std::fmax(big, std::fabs(a[r][k]));
  const double tol = 1e-13 * (big > 0 ? big : 1.0) * tol_scale;
  for (int r = 0; r < 4; ++r) {
    double nq = 0.0;
    for (int k = 0; k < 4; ++k) nq += a[r][k] * q[k];
    EXPECT(std::fabs(nq - lam * q[r]) <= tol);
  }
  EXPECT(lam >= -tol);      // the trace of N is 0: its largest eigenvalue is not negative
  EXPECT(std::fabs(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3] - 1.0) <= 1e-14);
  double R[9];
  score_quat_matrix(q, R);
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  EXPECT(std::fabs(det - 1.0) <= 1e-13);
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) {
      double d = 0.0;
      for (int m = 0; m < 3; ++m) d += R[3 * r + m] * R[3 * k + m];
      EXPECT(std::fabs(d - (r == k ? 1.0 : 0.0)) <= 1e-13);
    }
}

static void check_horn() {
  std::mt19937 rng(7);
  std::normal_distribution<double> nd(0.0, 1.0);
  for (int trial = 0; trial < 400; ++trial) {
    const int n = trial % 4 == 0 ? 3 : (trial % 4 == 1 ? 4 : (trial % 4 == 2 ? 21 : 200));
    std::vector<double> P(3 * (size_t)n), G(3 * (size_t)n);
    for (auto& x : P) x = 0.1 * nd(rng);
    // G = a rotation of P about a random axis (+ noise), mirrored every fifth trial, planar every seventh
    double ax[3] = {nd(rng), nd(rng), nd(rng)};
    const double an = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]) + 1e-300, ang = 3.0 * nd(rng);
    double q[4] = {std::cos(ang / 2), std::sin(ang / 2) * ax[0] / an, std::sin(ang / 2) * ax[1] / an, std::sin(ang / 2) * ax[2] / an};
    double R[9];
    score_quat_matrix(q, R);
    if (trial % 7 == 0)
      for (int i = 0; i < n; ++i) P[3 * (size_t)i + 2] = 0.0;
    const double noise = trial % 3 == 0 ? 0.0 : 0.01;
    for (int i = 0; i < n; ++i)
      for (int a = 0; a < 3; ++a)
        G[3 * (size_t)i + a] = 1.3 * score_rot_row(R, a, P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2]) + noise * nd(rng) + 0.5;
    if (trial % 5 == 0)
      for (int i = 0; i < n; ++i) G[3 * (size_t)i] = -G[3 * (size_t)i];
    double S[9];
    products(P, G, S);
    check_one(S, 1.0);
  }
  // hand-made matrices: zero, diagonal, equal diagonal elements (theta = 0), huge and tiny entries (theta^2 overflows: t = 0)
  const double cases[][9] = {{0, 0, 0, 0, 0, 0, 0, 0, 0},
                             {1, 0, 0, 0, 1, 0, 0, 0, 1},
                             {1, 0, 0, 0, 2, 0, 0, 0, 3},
                             {0, 1, 0, 1, 0, 0, 0, 0, 0},
                             {1e77, 3e76, -2e77, 5e76, -1e77, 2e76, 7e76, 1e76, 4e77},
                             {1e-300, 2e-300, 0, 0, 1e-300, 0, 0, 0, 1e-300},
                             {1, 1e-170, 0, -1e-170, 1e200, 0, 0, 0, 1},
                             {-1, 0, 0, 0, -1, 0, 0, 0, -1}};
  for (const auto& S : cases) check_one(S, 1e3);
  // the identity of the point sets: the quaternion is (1, 0, 0, 0) up to sign and lambda = the trace
  const double I[9] = {2, 0, 0, 0, 3, 0, 0, 0, 4};
  double q[4];
  EXPECT(score_horn(I, q) == 9.0 && std::fabs(q[0]) == 1.0 && q[1] == 0.0 && q[2] == 0.0 && q[3] == 0.0);
}

static void check_geometry() {
  const int ns[] = {1, 2, 3, 21, 63, 64, 65, 255, 256, 257, 778, 3999, 4000};
  for (int n : ns) {
    const int T = score_threads(n);
    EXPECT(T == (n <= 64 ? 64 : 256) && (T & (T - 1)) == 0 && T <= SCORE_BLOCK);
    // the carve-up of the block's LDS: the reduction area, six float arrays, the counted bytes; inside the size, inside 160 KB
    const size_t red = (size_t)SCORE_RED * SCORE_BLOCK * sizeof(double), pts = red + 6 * (size_t)n * sizeof(float);
    EXPECT(pts + (size_t)n <= score_lds_bytes(n) && score_lds_bytes(n) <= 160 * 1024 && score_lds_bytes(n) % 8 == 0);
    // every point is summed by exactly one thread, in ascending order
    std::vector<int> seen((size_t)n, 0);
    for (int t = 0; t < T; ++t) {
      int last = -1;
      for (int i = t; i < n; i += T) { ++seen[(size_t)i]; EXPECT(i > last); last = i; }
    }
    for (int i = 0; i < n; ++i) EXPECT(seen[(size_t)i] == 1);
    for (int G : {1, 2, 16}) {
      const ScoreAccPlan p = score_acc_plan(n, G);
      EXPECT(p.chunks == (n + 255) / 256 && p.point_blocks == (unsigned)(p.chunks * G) && p.grid == p.point_blocks + (unsigned)G + 1);
      // one owner per (group, point) element
      std::vector<int> own((size_t)G * n, 0);
      for (unsigned b = 0; b < p.point_blocks; ++b)
        for (int t = 0; t < SCORE_BLOCK; ++t) {
          const int g = (int)(b / p.chunks), i = (int)(b % p.chunks) * SCORE_BLOCK + t;
          if (i < n) { EXPECT(g < G); ++own[(size_t)g * n + i]; }
        }
      for (int v : own) EXPECT(v == 1);
      for (int bins : {1, 100, SCORE_MAX_BINS}) {
        EXPECT(score_group_words(n, bins) == 4 * (size_t)n + bins + 3);
        EXPECT(score_board_bytes(n, G, bins) == score_group_words(n, bins) * G * 8);
      }
    }
  }
  EXPECT(score_board_bytes(0, 2, 100) == 0 && score_board_bytes(4001, 2, 100) == 0 && score_board_bytes(21, 0, 100) == 0 &&
         score_board_bytes(21, 17, 100) == 0 && score_board_bytes(21, 2, 0) == 0 && score_board_bytes(21, 2, SCORE_MAX_BINS + 1) == 0);
  EXPECT(score_pair_bytes(2) == 64 && score_pair_bytes(16) == 4096 && score_pair_bytes(0) == 0 && score_pair_bytes(17) == 0);
  EXPECT(score_sizes_ok(0, 21) && score_sizes_ok(130, 778) && !score_sizes_ok(-1, 21) && !score_sizes_ok(1, 0) && !score_sizes_ok(1, 4001));
  EXPECT(score_sizes_ok(178956, 4000) && !score_sizes_ok(178957, 4000));      // N * n * 3 <= 2^31 - 1
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  EXPECT(score_bins_ok(1, 0.0005) && score_bins_ok(SCORE_MAX_BINS, 1e-300) && !score_bins_ok(0, 1.0) && !score_bins_ok(SCORE_MAX_BINS + 1, 1.0));
  EXPECT(!score_bins_ok(100, 0.0) && !score_bins_ok(100, -1.0) && !score_bins_ok(100, inf) && !score_bins_ok(100, nan));
}

static void check_rows_and_bins() {
  const float finf = std::numeric_limits<float>::infinity(), fnan = std::numeric_limits<float>::quiet_NaN();
  EXPECT(score_finite(0.f) && score_finite(-3e19f) && score_finite(3.4028234e38f) && !score_finite(finf) && !score_finite(-finf) && !score_finite(fnan));
  for (int G : {1, 2, 16}) {
    for (int32_t g : {INT_MIN, -1, G, G + 1, INT_MAX}) {
      EXPECT(score_row_state(g, G, true, 1.f) == 0 && score_row_state(g, G, false, 0.f) == 0);
    }
    for (int32_t g = 0; g < G; ++g) {
      EXPECT(score_row_state(g, G, false, 0.f) == 2 && score_row_state(g, G, true, 1.f) == 2 && score_row_state(g, G, true, 0.51f) == 2);
      EXPECT(score_row_state(g, G, true, 0.5f) == 1 && score_row_state(g, G, true, -3.f) == 1 && score_row_state(g, G, true, fnan) == 1);
      EXPECT(score_row_state(g, G, true, finf) == 2 && score_row_state(g, G, true, -finf) == 1);
    }
  }
  for (int bins : {1, 100, SCORE_MAX_BINS}) {
    const double w = 0.0005;
    EXPECT(score_bin(0.f, w, bins) == 0 && score_bin(finf, w, bins) == bins && score_bin(3.4e38f, w, bins) == bins);
    EXPECT(score_bin(3.4e38f, 1e-300, bins) == bins);      // the quotient itself overflows
    for (int k = 0; k <= bins + 2; k += (bins > 200 ? 97 : 1)) {
      const float e = (float)((k + 0.5) * w);
      const int b = score_bin(e, w, bins);
      EXPECT(b == (k < bins ? k : bins) && b >= 0 && b <= bins);
      const long long plain = (long long)((double)e / w);
      EXPECT(b == (plain < bins ? (int)plain : bins));
    }
  }
  EXPECT(score_norm(3.0, 4.0, 12.0) == 13.0 && score_norm(0.0, 0.0, 0.0) == 0.0);
}

int main() {
  check_horn();
  check_geometry();
  check_rows_and_bins();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
