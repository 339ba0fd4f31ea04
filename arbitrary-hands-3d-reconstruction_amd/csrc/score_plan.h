// The rule and the host side of scoring hands against ground truth (acrmi_pose_errors, acrmi_score_accumulate,
// acrmi_score_hands; the kernels are in csrc/score.hip): MPJPE / MPVPE root-aligned and
// Procrustes-aligned, the board that keeps running sums on the device, launch geometry and sizes.  Plain C++, no HIP:
// tools/score_check.cpp compiles it alone; ACRMI_HD (csrc/roi_plan.h) is `__host__ __device__` when the translation unit is HIP.
//
// THE RULE.  Inputs fp32, arithmetic fp64, every operation rounded on its own (no contraction); per-point and per-row outputs
// are the fp64 value rounded to fp32.  A ROW is one hand, a POINT SET n <= 4000 points (21 joints, 778 vertices).
//   counted point  valid[i] != 0 (or no valid array) and all six coordinates of P[i] (prediction) and G[i] (truth) finite.
//   counted row    group[row] in [0, n_groups) and flag > 0.5: SCORED; group in range, flag not set (NaN included): a MISS,
//                  counted per group, enters no error; group out of range (negative, >= n_groups, INT_MIN): not looked at.
//                  Without flags every row is flagged; without groups every row is of group 0.  A row that is not scored has
//                  -1 in every per-point output, -1 in row_f, zero counts.
//   origins        oP, oG = P[root], G[root] when root >= 0; else row `row` of two origin arrays; with neither, zero.  The
//                  origins are GOOD when the root point is counted / the six origin values are finite.
//   e_ra[i]        = |(P[i] - oP) - (G[i] - oG)| for a counted point of a row with good origins; |d| = sqrt((dx*dx + dy*dy) + dz*dz).
//   sums           a reduction over the points is: thread t of T = score_threads(n) adds its points i = t, t + T, ... in
//                  ascending i (a point that is not counted adds +0), then the T partial sums are folded by the fixed tree
//                  for (s = T / 2; s >= 1; s /= 2) v[t] = v[t] + v[t + s] for t < s; the sum is v[0].
//   Procrustes     over the c counted points: muP, muG = sum / c; Pc = P - muP, Gc = G - muG; S[a][b] = sum Pc_a * Gc_b;
//                  vP = sum (Pcx*Pcx + Pcy*Pcy) + Pcz*Pcz; Horn's symmetric 4 x 4 matrix (score_horn_matrix); cyclic Jacobi,
//                  pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), exactly 6 sweeps, no convergence test (score_jacobi_rotate); the
//                  quaternion is the eigenvector of the largest diagonal element, the lowest index on a tie; R from it
//                  (score_quat_matrix, not normalised again); scale = lambda / vP;
//                  e_pa[i] = |(scale * (R Pc[i]) + muG) - G[i]|, (R Pc)_a = (R[a][0]*Pcx + R[a][1]*Pcy) + R[a][2]*Pcz.
//                  A row has e_pa only with c >= 3 and vP > 0.
//   row_f          mean e_ra, mean e_pa (the reduction of the fp64 errors / their count; -1 without one), scale (-1 without
//                  e_pa), |(oP + trans) - oG| (-1 without trans, without good origins or with a trans that is not finite).
//   row_i          the number of points with an e_ra, with an e_pa.
//   xform          quaternion (w, x, y, z), scale, translation muG - scale * (R muP); zeros with scale -1 without e_pa.
//   pair_err       rows 2p and 2p + 1 are the (left, right) hands of pair p: |((oP_R + t_R) - (oP_L + t_L)) - (oG_R - oG_L)|
//                  when both rows are scored, have good origins and a finite trans, else -1 (the MRRPE term).
//   not counted    is -1.0f in every per-point output.
//   the board      per point set and group: sum_ra[n], sum_pa[n] fp64, cnt_ra[n], cnt_pa[n] int64, hist[n_bins + 1] int64 of the
//                  set's e_ra (score_bin: the last bin collects everything beyond the range; -1 and NaN are never binned),
//                  rows scored, rows missed; per (left group, right group): the pair_err sum fp64 and count.  Every element
//                  continues from the board's value and adds the fp32 outputs >= 0, converted to double, in ascending row order:
//                  one call of 2B rows equals two calls of B rows bit for bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "roi_plan.h"      // ACRMI_HD

namespace acrmi {

constexpr int SCORE_MAX_POINTS = 4000;      // points of a set: 25 bytes of LDS each
constexpr int SCORE_MAX_GROUPS = 16;
constexpr int SCORE_MAX_BINS = 4096;        // the histogram of a group is built in LDS
constexpr int SCORE_WAVE = 64;              // threads that work on a set of n <= 64 points
constexpr int SCORE_BLOCK = 256;            // and on a larger one; also the accumulate kernel's block
constexpr int SCORE_RED = 11;               // fp64 values reduced at once: the nine products, vP and the e_ra sum
constexpr int SCORE_ROW_F = 4, SCORE_ROW_I = 2, SCORE_XFORM = 8;
constexpr int SCORE_SWEEPS = 6;

ACRMI_HD inline int score_threads(int n) { return n <= SCORE_WAVE ? SCORE_WAVE : SCORE_BLOCK; }

// Dynamic LDS of a pose-errors block over sets of at most n points: the reduction area, x y z of P and of G, the counted bytes.
inline size_t score_lds_bytes(int n) {
  return (size_t)SCORE_RED * SCORE_BLOCK * sizeof(double) + (size_t)n * 24 + (((size_t)n + 7) & ~(size_t)7);
}

inline bool score_sizes_ok(long long N, int n) {
  return N >= 0 && n >= 1 && n <= SCORE_MAX_POINTS && N * n * 3 <= 0x7fffffffll;
}
inline bool score_groups_ok(int n_groups) { return n_groups >= 1 && n_groups <= SCORE_MAX_GROUPS; }
// n_bins in 1..SCORE_MAX_BINS, bin_width finite and > 0 (NaN fails)
inline bool score_bins_ok(int n_bins, double bin_width) {
  return n_bins >= 1 && n_bins <= SCORE_MAX_BINS && bin_width > 0.0 && bin_width <= 1.7976931348623157e308;
}

// The board of one point set, in 8-byte words: per group [sum_ra n | sum_pa n | cnt_ra n | cnt_pa n | hist n_bins + 1 | scored |
// missed]; the pair board: per (left group, right group) [sum | count].
ACRMI_HD inline size_t score_group_words(int n, int n_bins) { return 4 * (size_t)n + (size_t)n_bins + 3; }
inline size_t score_board_bytes(int n, int n_groups, int n_bins) {
  if (n < 1 || n > SCORE_MAX_POINTS || !score_groups_ok(n_groups) || n_bins < 1 || n_bins > SCORE_MAX_BINS) return 0;
  return score_group_words(n, n_bins) * (size_t)n_groups * 8;
}
inline size_t score_pair_bytes(int n_groups) { return score_groups_ok(n_groups) ? (size_t)n_groups * n_groups * 16 : 0; }

// The accumulate kernel's grid: per group ceil(n / SCORE_BLOCK) blocks own the point sums (one thread per element), then one
// block per group builds its histogram and row counts, then one block owns the pair board.
struct ScoreAccPlan {
  int chunks;
  unsigned point_blocks, grid;
};
ACRMI_HD inline ScoreAccPlan score_acc_plan(int n, int n_groups) {
  ScoreAccPlan p;
  p.chunks = (n + SCORE_BLOCK - 1) / SCORE_BLOCK;
  p.point_blocks = (unsigned)(p.chunks * n_groups);
  p.grid = p.point_blocks + (unsigned)n_groups + 1;
  return p;
}

ACRMI_HD inline bool score_finite(float x) { return fabsf(x) <= 3.4028234e38f; }

// 0: the row is not looked at; 1: a miss; 2: scored.
ACRMI_HD inline int score_row_state(int32_t group, int n_groups, bool has_flag, float flag) {
  if (group < 0 || group >= n_groups) return 0;
  return !has_flag || flag > 0.5f ? 2 : 1;
}

// The bin of an error e >= 0: min(n_bins, (int64)((double)e / bin_width)), written so that an infinite quotient is never converted.
ACRMI_HD inline int score_bin(float e, double bin_width, int n_bins) {
  const double q = (double)e / bin_width;
  return q >= (double)n_bins ? n_bins : (int)q;
}

ACRMI_HD inline double score_norm(double dx, double dy, double dz) { return sqrt((dx * dx + dy * dy) + dz * dz); }

// Horn (1987): the symmetric matrix whose largest eigenvector is the unit quaternion of the rotation that takes P onto G;
// S row-major, S[3 * a + b] = sum Pc_a * Gc_b.
ACRMI_HD inline void score_horn_matrix(const double* S, double (&a)[4][4]) {
  const double xx = S[0], xy = S[1], xz = S[2], yx = S[3], yy = S[4], yz = S[5], zx = S[6], zy = S[7], zz = S[8];
  a[0][0] = (xx + yy) + zz;
  a[1][1] = (xx - yy) - zz;
  a[2][2] = (yy - xx) - zz;
  a[3][3] = (zz - xx) - yy;
  a[0][1] = a[1][0] = yz - zy;
  a[0][2] = a[2][0] = zx - xz;
  a[0][3] = a[3][0] = xy - yx;
  a[1][2] = a[2][1] = xy + yx;
  a[1][3] = a[3][1] = zx + xz;
  a[2][3] = a[3][2] = yz + zy;
}

// One Jacobi rotation of the pair (P, Q), P < Q, on the symmetric a, accumulated into the columns of v.  A zero a[P][Q] is skipped;
// sign(0) = +1; an overflowing theta * theta gives t = 0.  Indices are compile-time constants: the matrices stay in registers.
template <int P, int Q>
ACRMI_HD inline void score_jacobi_rotate(double (&a)[4][4], double (&v)[4][4]) {
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  a[P][P] = a[P][P] - t * apq;
  a[Q][Q] = a[Q][Q] + t * apq;
  a[P][Q] = a[Q][P] = 0.0;
#if defined(__clang__)
#pragma unroll
#endif
  for (int r = 0; r < 4; ++r) {
    if (r != P && r != Q) {
      const double arp = a[r][P], arq = a[r][Q];
      a[r][P] = a[P][r] = c * arp - s * arq;
      a[r][Q] = a[Q][r] = s * arp + c * arq;
    }
    const double vrp = v[r][P], vrq = v[r][Q];
    v[r][P] = c * vrp - s * vrq;
    v[r][Q] = s * vrp + c * vrq;
  }
}

// S -> the quaternion q = (w, x, y, z); returns its eigenvalue lambda = sum Gc . (R Pc).
ACRMI_HD inline double score_horn(const double* S, double* q) {
  double a[4][4], v[4][4];
  score_horn_matrix(S, a);
#if defined(__clang__)
#pragma unroll
#endif
  for (int r = 0; r < 4; ++r) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) v[r][k] = r == k ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < SCORE_SWEEPS; ++sweep) {
    score_jacobi_rotate<0, 1>(a, v);
    score_jacobi_rotate<0, 2>(a, v);
    score_jacobi_rotate<0, 3>(a, v);
    score_jacobi_rotate<1, 2>(a, v);
    score_jacobi_rotate<1, 3>(a, v);
    score_jacobi_rotate<2, 3>(a, v);
  }
  double lam = a[0][0];
  q[0] = v[0][0]; q[1] = v[1][0]; q[2] = v[2][0]; q[3] = v[3][0];
#if defined(__clang__)
#pragma unroll
#endif
  for (int k = 1; k < 4; ++k) {
    if (a[k][k] > lam) {
      lam = a[k][k];
      q[0] = v[0][k]; q[1] = v[1][k]; q[2] = v[2][k]; q[3] = v[3][k];
    }
  }
  return lam;
}

// The rotation of the quaternion (w, x, y, z), row-major.
ACRMI_HD inline void score_quat_matrix(const double* q, double* R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
  const double xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  R[0] = ((ww + xx) - yy) - zz; R[1] = 2.0 * (xy - wz);       R[2] = 2.0 * (xz + wy);
  R[3] = 2.0 * (xy + wz);       R[4] = ((ww - xx) + yy) - zz; R[5] = 2.0 * (yz - wx);
  R[6] = 2.0 * (xz - wy);       R[7] = 2.0 * (yz + wx);       R[8] = ((ww - xx) - yy) + zz;
}

ACRMI_HD inline double score_rot_row(const double* R, int a, double x, double y, double z) {
  return (R[3 * a] * x + R[3 * a + 1] * y) + R[3 * a + 2] * z;
}

}  // namespace acrmi
