// The rule of the fused MANO fitter (csrc/mano_fit.hip, acrmi_mano_fit), stated once for the kernel, the
// C entry and tools/mano_fit_check.cpp: the parameters of a hand, the loss with its cotangents, the Adam step and the state
// row.  Plain C++, no HIP, like mano_grad_plan.h; templates over the scalar type (the kernel runs all of it in double on
// float storage, the check program in double throughout).
//
// PARAMETERS.  64 floats per hand: pose[0:48] (root rotation 0..2, articulation 3..47), betas 48..57, trans 58..60,
// cam (s, tx, ty) 61..63 - five groups, each with a learning rate of its own; the five groups fill the 64 floats.
//
// FUNCTION.  (verts, joints, center) = mano_kernel<false>(pose, betas, side, center_idx) in its axis-angle mode;
// J3 = joints + trans, V3 = verts + trans, P2 = joints[:, :2] * s + (tx, ty) (csrc/mano.hip's pj2d: root-aligned joints, trans
// plays no part).
//
// LOSS per hand:  sum_j w3[j] |J3_j - Y3_j|^2 + sum_j w2[j] |P2_j - Y2_j|^2 + wv sum_v |V3_v - YV_v|^2
//                 + lam_pose |pose[3:48] - prior[3:48]|^2 + lam_beta |betas - prior[48:58]|^2.
// A missing target removes its term; a weight that is exactly 0 removes its point and its target is not read into the
// arithmetic.  center itself is not in the loss: its cotangent is zero.
//
// SUMMATION ORDER.  Joint terms: fit_joint writes the 7 terms of joint j (loss, g_trans[3], g_cam[3]); fit_fold adds the
// 21 joints in ascending order.  Vertex terms: thread t of 256 adds its vertices t, t + 256, ... in ascending order, a wave
// folds its 64 lanes by the shuffle tree (offsets 32, 16, ..., 1), the 4 waves are added as (0 + 1) + (2 + 3).  Regulariser:
// slot i is lane i of one wave, folded by the same tree.  loss = joints + vertices + regulariser, in this order.
//
// UPDATE.  torch.optim.Adam, operation by operation (no weight decay, no amsgrad); t counts from 1 and is carried in the state;
// lr == 0 freezes a group: its parameters, m and v keep their bytes.
#pragma once
#include <math.h>

#include "roi_plan.h"      // ACRMI_HD

namespace acrmi {

constexpr int FIT_THREADS = 256;            // one workgroup per hand
constexpr int FIT_PARAMS = 64;
constexpr int FIT_POSE = 0, FIT_BETAS = 48, FIT_TRANS = 58, FIT_CAM = 61;
constexpr int FIT_PRIOR = 58;               // a prior row: pose[48] | betas[10]
constexpr int FIT_GROUPS = 5;               // root, pose, betas, trans, cam
constexpr int FIT_MAX_STEPS = 1024;         // per launch; longer fits chain calls through the state
// the state row of a hand: parameters | m | v | t | loss of the last evaluated step | loss of the first | 0
constexpr int FIT_STATE_M = 64, FIT_STATE_V = 128, FIT_STATE_T = 192, FIT_STATE_LOSS = 193, FIT_STATE_LOSS0 = 194;
constexpr int FIT_STATE = 196;

constexpr int fit_group(int slot) { return slot < 3 ? 0 : (slot < FIT_BETAS ? 1 : (slot < FIT_TRANS ? 2 : (slot < FIT_CAM ? 3 : 4))); }
constexpr bool fit_steps_ok(int steps) { return steps >= 0 && steps <= FIT_MAX_STEPS; }
constexpr bool fit_center_ok(int center_idx) { return center_idx >= -1 && center_idx <= 20; }

ACRMI_HD inline float fit_sqrt(float x) { return sqrtf(x); }
ACRMI_HD inline double fit_sqrt(double x) { return sqrt(x); }

// One joint.  x [3]: the root-aligned joint (before trans); y3 [3] / y2 [2]: its targets, NULL = no such term.  Writes g [3],
// the cotangent of x, and term [7] = {loss, g_trans[3], g_cam[3]} of this joint.
template <typename T>
ACRMI_HD inline void fit_joint(const T x[3], const T trans[3], const T cam[3], const float* y3, float w3, const float* y2,
                               float w2, T g[3], T term[7]) {
  g[0] = g[1] = g[2] = (T)0;
  for (int i = 0; i < 7; ++i) term[i] = (T)0;
  if (y3 && w3 != 0.f) {
    T e = (T)0;
    for (int d = 0; d < 3; ++d) {
      const T r = (x[d] + trans[d]) - (T)y3[d];
      const T gd = (T)2 * (T)w3 * r;
      e += r * r;
      g[d] += gd;
      term[1 + d] = gd;
    }
    term[0] += (T)w3 * e;
  }
  if (y2 && w2 != 0.f) {
    T e = (T)0;
    for (int d = 0; d < 2; ++d) {
      const T r = (x[d] * cam[0] + cam[1 + d]) - (T)y2[d];
      const T gp = (T)2 * (T)w2 * r;
      e += r * r;
      g[d] += gp * cam[0];
      term[4] += gp * x[d];
      term[5 + d] = gp;
    }
    term[0] += (T)w2 * e;
  }
}

// term i of the 21 joints, ascending
template <typename T>
ACRMI_HD inline T fit_fold(const T (*terms)[7], int i) {
  T s = (T)0;
  for (int j = 0; j < 21; ++j) s += terms[j][i];
  return s;
}

// One vertex coordinate: v the root-aligned value, y its target -> the residual r; its cotangent is 2 wv r (also g_trans's
// share), its loss wv r^2.
template <typename T>
ACRMI_HD inline T fit_vertex_residual(T v, T trans, float y) { return (v + trans) - (T)y; }

// The regulariser of slot `slot` holding p: adds its cotangent to *g, returns its loss term (0 for trans and cam).
template <typename T>
ACRMI_HD inline T fit_prior(int slot, T p, float prior, T lam_pose, T lam_beta, T* g) {
  const T lam = (slot >= 3 && slot < FIT_BETAS) ? lam_pose : ((slot >= FIT_BETAS && slot < FIT_TRANS) ? lam_beta : (T)0);
  if (lam == (T)0) return (T)0;
  const T d = p - (T)prior;
  *g += (T)2 * lam * d;
  return lam * d * d;
}

// Adam's bias corrections of step t (>= 1): 1 - b1^t and sqrt(1 - b2^t), in double as torch computes them.
ACRMI_HD inline void fit_adam_bias(double b1, double b2, double t, double* bc1, double* bc2_sqrt) {
  *bc1 = 1.0 - pow(b1, t);
  *bc2_sqrt = sqrt(1.0 - pow(b2, t));
}

// One parameter: arithmetic in T, storage in S.  lr == 0: nothing is written.
template <typename S, typename T>
ACRMI_HD inline void fit_adam(S* p, S* m, S* v, T g, T lr, T b1, T b2, T eps, T bc1, T bc2_sqrt) {
  if (lr == (T)0) return;
  const S m1 = (S)(b1 * (T)*m + ((T)1 - b1) * g);
  const S v1 = (S)(b2 * (T)*v + ((T)1 - b2) * g * g);
  *m = m1;
  *v = v1;
  const T denom = fit_sqrt((T)v1) / bc2_sqrt + eps;
  *p = (S)((T)*p - lr / bc1 * ((T)m1 / denom));
}

}  // namespace acrmi
