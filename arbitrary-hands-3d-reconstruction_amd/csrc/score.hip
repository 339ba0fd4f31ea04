// Scoring hands against ground truth (acrmi_pose_errors, acrmi_score_accumulate, acrmi_score_hands).
// The rule, the reduction tree and the board's layout: csrc/score_plan.h; tests/score_ref.py restates them in numpy float64.
// fp64 arithmetic, every operation rounded on its own (-ffp-contract=off).
//
//   pose_errors_kernel       one block per (row, point set).  A set of n <= 64 points is worked on by one wave, a larger one by
//                            256 threads; a launch over two sets of different classes has 256-thread blocks whose waves 1..3 only
//                            keep the barriers company in the small set.  The points are read once from global memory and staged
//                            in LDS (x, y, z of P and of G as six arrays, and the counted bytes); three passes over LDS: the
//                            means; e_ra with the nine products and vP; e_pa.  Every reduction is the plan's lane-strided sum
//                            followed by its fixed tree, in LDS.  Horn's 4 x 4 Jacobi runs in every lane on the same values
//                            (score_horn, indices compile-time constants: no scratch).
//   score_accumulate_kernel  the board.  One thread per (group, point) element loops over the rows in ascending order; one
//                            block per group builds the histogram in LDS with integer atomics and adds it to the board with
//                            one writer per bin; one block owns the pair sums, one thread per (left group, right group).
// No floating-point atomics, no atomics on global memory, one writer per element.  Data-derived indices: `group`, compared
// with the block's own group or range-checked (score_row_state), and the bin, clamped (score_bin) and only taken of e >= 0.
#include "kernels.h"
#include "score_plan.h"

#include <cmath>
#include <mutex>

namespace acrmi {

// v[k] of the T working threads -> the tree's sums, in every thread.  red: SCORE_RED * SCORE_BLOCK doubles.
template <int K>
__device__ __forceinline__ void score_tree(double* red, double (&v)[K], int tid, int T) {
  if (tid < T) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[k * SCORE_BLOCK + tid] = v[k];
  }
  __syncthreads();
  for (int s = T >> 1; s >= 1; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < K; ++k) red[k * SCORE_BLOCK + tid] = red[k * SCORE_BLOCK + tid] + red[k * SCORE_BLOCK + tid + s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = red[k * SCORE_BLOCK];
  __syncthreads();
}

__device__ __forceinline__ int32_t score_group_of(const int32_t* group, int group_side, int row) {
  return group ? group[row] : (group_side ? (row & 1) : 0);
}

__device__ __forceinline__ int score_state_of(const ScoreArgs& a, int row) {
  return score_row_state(score_group_of(a.group, a.group_side, row), a.n_groups, a.flags != nullptr,
                         a.flags ? a.flags[(size_t)row * a.flag_stride] : 1.f);
}

// The origins of a row, from global memory; false: they are not good.
__device__ __forceinline__ bool score_origins(const ScoreSet& st, int row, double* oP, double* oG) {
  const float *p, *g;
  if (st.root >= 0) {
    const size_t at = (size_t)row * st.n + st.root;
    if (st.valid && st.valid[at] == 0) return false;
    p = st.P + 3 * at;
    g = st.G + 3 * at;
  } else if (st.oP) {
    if (st.o_valid && st.o_valid[(size_t)row * st.o_valid_stride] == 0) return false;
    p = st.oP + (size_t)row * st.o_stride;
    g = st.oG + (size_t)row * st.o_stride;
  } else {
    oP[0] = oP[1] = oP[2] = oG[0] = oG[1] = oG[2] = 0.0;
    return true;
  }
  const float p0 = p[0], p1 = p[1], p2 = p[2], g0 = g[0], g1 = g[1], g2 = g[2];
  oP[0] = p0; oP[1] = p1; oP[2] = p2; oG[0] = g0; oG[1] = g1; oG[2] = g2;
  return score_finite(p0) && score_finite(p1) && score_finite(p2) && score_finite(g0) && score_finite(g1) && score_finite(g2);
}

// oP + trans of a row; false: no finite trans.
__device__ __forceinline__ bool score_placed(const ScoreSet& st, int row, const double* oP, double* placed) {
  if (!st.trans) return false;
  const float t0 = st.trans[3 * (size_t)row], t1 = st.trans[3 * (size_t)row + 1], t2 = st.trans[3 * (size_t)row + 2];
  placed[0] = oP[0] + (double)t0; placed[1] = oP[1] + (double)t1; placed[2] = oP[2] + (double)t2;
  return score_finite(t0) && score_finite(t1) && score_finite(t2);
}

__global__ void __launch_bounds__(SCORE_BLOCK) pose_errors_kernel(ScoreArgs a) {
  extern __shared__ double s_red[];
  const ScoreSet& st = a.set[blockIdx.y];
  const int row = blockIdx.x, tid = threadIdx.x, n = st.n, T = score_threads(n);
  float* s_px = (float*)(s_red + SCORE_RED * SCORE_BLOCK);
  float *s_py = s_px + n, *s_pz = s_py + n, *s_gx = s_pz + n, *s_gy = s_gx + n, *s_gz = s_gy + n;
  uint8_t* s_c = (uint8_t*)(s_gz + n);
  const size_t base = (size_t)row * n;
  const int state = score_state_of(a, row);
  double oP[3], oG[3];
  const bool origins = score_origins(st, row, oP, oG);

  // the MRRPE term of pair row / 2, by the left row's block
  if (st.pair_err && tid == 0 && (row & 1) == 0 && row + 1 < a.N) {
    float err = -1.f;
    double qP[3], qG[3], pl[3], pr[3];
    if (state == 2 && score_state_of(a, row + 1) == 2 && origins && score_origins(st, row + 1, qP, qG) &&
        score_placed(st, row, oP, pl) && score_placed(st, row + 1, qP, pr))
      err = (float)score_norm((pr[0] - pl[0]) - (qG[0] - oG[0]), (pr[1] - pl[1]) - (qG[1] - oG[1]), (pr[2] - pl[2]) - (qG[2] - oG[2]));
    st.pair_err[row >> 1] = err;
  }

  if (state != 2) {      // a miss, or not looked at: nothing of the row is read
    for (int i = tid; i < n; i += blockDim.x) {
      st.e_ra[base + i] = -1.f;
      st.e_pa[base + i] = -1.f;
    }
    if (tid == 0) {
#pragma unroll
      for (int k = 0; k < SCORE_ROW_F; ++k) st.row_f[(size_t)row * SCORE_ROW_F + k] = -1.f;
      st.row_i[(size_t)row * SCORE_ROW_I] = st.row_i[(size_t)row * SCORE_ROW_I + 1] = 0;
      if (st.xform) {
#pragma unroll
        for (int k = 0; k < SCORE_XFORM; ++k) st.xform[(size_t)row * SCORE_XFORM + k] = k == 4 ? -1.f : 0.f;
      }
    }
    return;
  }

  // pass 1: stage the points, count them, sum them
  double m[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (tid < T) {
    for (int i = tid; i < n; i += T) {
      const float* p = st.P + 3 * (base + i);
      const float* g = st.G + 3 * (base + i);
      const float px = p[0], py = p[1], pz = p[2], gx = g[0], gy = g[1], gz = g[2];
      const bool on = (!st.valid || st.valid[base + i] != 0) && score_finite(px) && score_finite(py) && score_finite(pz) &&
                      score_finite(gx) && score_finite(gy) && score_finite(gz);
      s_px[i] = px; s_py[i] = py; s_pz[i] = pz; s_gx[i] = gx; s_gy[i] = gy; s_gz[i] = gz;
      s_c[i] = on ? 1 : 0;
      if (on) {
        m[0] = m[0] + (double)px; m[1] = m[1] + (double)py; m[2] = m[2] + (double)pz;
        m[3] = m[3] + (double)gx; m[4] = m[4] + (double)gy; m[5] = m[5] + (double)gz;
        m[6] = m[6] + 1.0;
      }
    }
  }
  score_tree(s_red, m, tid, T);
  const int c = (int)m[6];
  double muP[3] = {0.0, 0.0, 0.0}, muG[3] = {0.0, 0.0, 0.0};
  if (c > 0) {
    const double cd = (double)c;
    muP[0] = m[0] / cd; muP[1] = m[1] / cd; muP[2] = m[2] / cd;
    muG[0] = m[3] / cd; muG[1] = m[4] / cd; muG[2] = m[5] / cd;
  }

  // pass 2: e_ra, the nine products, vP
  double r[SCORE_RED];
#pragma unroll
  for (int k = 0; k < SCORE_RED; ++k) r[k] = 0.0;
  if (tid < T) {
    for (int i = tid; i < n; i += T) {
      float era = -1.f;
      if (s_c[i]) {
        const double px = s_px[i], py = s_py[i], pz = s_pz[i], gx = s_gx[i], gy = s_gy[i], gz = s_gz[i];
        const double ax = px - muP[0], ay = py - muP[1], az = pz - muP[2];
        const double bx = gx - muG[0], by = gy - muG[1], bz = gz - muG[2];
        r[0] = r[0] + ax * bx; r[1] = r[1] + ax * by; r[2] = r[2] + ax * bz;
        r[3] = r[3] + ay * bx; r[4] = r[4] + ay * by; r[5] = r[5] + ay * bz;
        r[6] = r[6] + az * bx; r[7] = r[7] + az * by; r[8] = r[8] + az * bz;
        r[9] = r[9] + ((ax * ax + ay * ay) + az * az);
        if (origins) {
          const double e = score_norm((px - oP[0]) - (gx - oG[0]), (py - oP[1]) - (gy - oG[1]), (pz - oP[2]) - (gz - oG[2]));
          r[10] = r[10] + e;
          era = (float)e;
        }
      }
      st.e_ra[base + i] = era;
    }
  }
  score_tree(s_red, r, tid, T);
  const double vP = r[9];
  const bool pa = c >= 3 && vP > 0.0;
  double q[4] = {0.0, 0.0, 0.0, 0.0}, R[9], scale = -1.0;
  if (pa) {
    const double lam = score_horn(r, q);
    score_quat_matrix(q, R);
    scale = lam / vP;
  }

  // pass 3: e_pa
  double w[1] = {0.0};
  if (tid < T) {
    for (int i = tid; i < n; i += T) {
      float epa = -1.f;
      if (pa && s_c[i]) {
        const double ax = (double)s_px[i] - muP[0], ay = (double)s_py[i] - muP[1], az = (double)s_pz[i] - muP[2];
        const double e = score_norm((scale * score_rot_row(R, 0, ax, ay, az) + muG[0]) - (double)s_gx[i],
                                    (scale * score_rot_row(R, 1, ax, ay, az) + muG[1]) - (double)s_gy[i],
                                    (scale * score_rot_row(R, 2, ax, ay, az) + muG[2]) - (double)s_gz[i]);
        w[0] = w[0] + e;
        epa = (float)e;
      }
      st.e_pa[base + i] = epa;
    }
  }
  score_tree(s_red, w, tid, T);

  if (tid == 0) {
    const int c_ra = origins ? c : 0, c_pa = pa ? c : 0;
    float* rf = st.row_f + (size_t)row * SCORE_ROW_F;
    rf[0] = c_ra > 0 ? (float)(r[10] / (double)c_ra) : -1.f;
    rf[1] = c_pa > 0 ? (float)(w[0] / (double)c_pa) : -1.f;
    rf[2] = (float)scale;
    double pl[3];
    rf[3] = origins && score_placed(st, row, oP, pl) ? (float)score_norm(pl[0] - oG[0], pl[1] - oG[1], pl[2] - oG[2]) : -1.f;
    st.row_i[(size_t)row * SCORE_ROW_I] = c_ra;
    st.row_i[(size_t)row * SCORE_ROW_I + 1] = c_pa;
    if (st.xform) {
      float* xf = st.xform + (size_t)row * SCORE_XFORM;
      xf[0] = (float)q[0]; xf[1] = (float)q[1]; xf[2] = (float)q[2]; xf[3] = (float)q[3];
      xf[4] = (float)scale;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        xf[5 + k] = pa ? (float)(muG[k] - scale * score_rot_row(R, k, muP[0], muP[1], muP[2])) : 0.f;
    }
  }
}

hipError_t launch_pose_errors(const ScoreArgs& a, hipStream_t s) {
  if (a.N <= 0 || a.n_sets < 1 || a.n_sets > 2) return hipErrorInvalidValue;
  int n_max = 0;
  for (int k = 0; k < a.n_sets; ++k) {
    if (!score_sizes_ok(a.N, a.set[k].n) || a.set[k].root >= a.set[k].n) return hipErrorInvalidValue;
    n_max = a.set[k].n > n_max ? a.set[k].n : n_max;
  }
  {
    std::lock_guard<std::recursive_mutex> lock(launch_mutex());
    static unsigned char init[MAX_DEVICES] = {};
    if (first_use_on_device(init)) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pose_errors_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)score_lds_bytes(SCORE_MAX_POINTS));
      if (e != hipSuccess) return e;
    }
  }
  hipLaunchKernelGGL(pose_errors_kernel, dim3((unsigned)a.N, (unsigned)a.n_sets), dim3(score_threads(n_max)), score_lds_bytes(n_max), s, a);
  return hipGetLastError();
}

__global__ void __launch_bounds__(SCORE_BLOCK) score_accumulate_kernel(ScoreAccArgs a) {
  __shared__ unsigned s_hist[SCORE_MAX_BINS + 3];      // bins 0..n_bins, then scored, missed
  const ScoreAccPlan plan = score_acc_plan(a.n, a.n_groups);
  const unsigned blk = blockIdx.x;
  const int tid = threadIdx.x;
  const size_t gw = score_group_words(a.n, a.n_bins);
  if (blk < plan.point_blocks) {
    const int g = (int)(blk / plan.chunks), i = (int)(blk % plan.chunks) * SCORE_BLOCK + tid;
    if (i >= a.n) return;
    int64_t* b = a.board + gw * g;
    double sra = __longlong_as_double(b[i]), spa = __longlong_as_double(b[a.n + i]);
    int64_t cra = b[2 * (size_t)a.n + i], cpa = b[3 * (size_t)a.n + i];
    for (int row = 0; row < a.N; ++row) {
      if (score_group_of(a.group, a.group_side, row) != g) continue;
      const float era = a.e_ra[(size_t)row * a.n + i], epa = a.e_pa[(size_t)row * a.n + i];
      if (era >= 0.f) { sra = sra + (double)era; ++cra; }
      if (epa >= 0.f) { spa = spa + (double)epa; ++cpa; }
    }
    b[i] = __double_as_longlong(sra);
    b[a.n + i] = __double_as_longlong(spa);
    b[2 * (size_t)a.n + i] = cra;
    b[3 * (size_t)a.n + i] = cpa;
  } else if (blk < plan.point_blocks + (unsigned)a.n_groups) {
    const int g = (int)(blk - plan.point_blocks);
    for (int k = tid; k < a.n_bins + 3; k += SCORE_BLOCK) s_hist[k] = 0;
    __syncthreads();
    for (int row = 0; row < a.N; ++row) {
      if (score_group_of(a.group, a.group_side, row) != g) continue;      // (uniform: the whole block skips the row)
      for (int i = tid; i < a.n; i += SCORE_BLOCK) {
        const float era = a.e_ra[(size_t)row * a.n + i];
        if (era >= 0.f) atomicAdd(&s_hist[score_bin(era, a.bin_width, a.n_bins)], 1u);
      }
    }
    for (int row = tid; row < a.N; row += SCORE_BLOCK) {
      if (score_group_of(a.group, a.group_side, row) != g) continue;
      const int state = score_row_state(g, a.n_groups, a.flags != nullptr, a.flags ? a.flags[(size_t)row * a.flag_stride] : 1.f);
      atomicAdd(&s_hist[a.n_bins + (state == 2 ? 1 : 2)], 1u);
    }
    __syncthreads();
    int64_t* h = a.board + gw * g + 4 * (size_t)a.n;
    for (int k = tid; k < a.n_bins + 3; k += SCORE_BLOCK) h[k] += (int64_t)s_hist[k];
  } else if (a.pair_err && a.pair_board) {
    const int G = a.n_groups;
    for (int slot = tid; slot < G * G; slot += SCORE_BLOCK) {
      const int gl = slot / G, gr = slot % G;
      double sum = __longlong_as_double(a.pair_board[2 * slot]);
      int64_t cnt = a.pair_board[2 * slot + 1];
      for (int p = 0; 2 * p + 1 < a.N; ++p) {
        if (score_group_of(a.group, a.group_side, 2 * p) != gl || score_group_of(a.group, a.group_side, 2 * p + 1) != gr) continue;
        const float e = a.pair_err[p];
        if (e >= 0.f) { sum = sum + (double)e; ++cnt; }
      }
      a.pair_board[2 * slot] = __double_as_longlong(sum);
      a.pair_board[2 * slot + 1] = cnt;
    }
  }
}

hipError_t launch_score_accumulate(const ScoreAccArgs& a, hipStream_t s) {
  if (a.N <= 0 || !score_sizes_ok(a.N, a.n) || !score_groups_ok(a.n_groups) || !score_bins_ok(a.n_bins, a.bin_width))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(score_accumulate_kernel, dim3(score_acc_plan(a.n, a.n_groups).grid), dim3(SCORE_BLOCK), 0, s, a);
  return hipGetLastError();
}

}  // namespace acrmi
