// The small pieces of the MANO backward (csrc/mano_grad.hip, acrmi_mano_backward), each next to the
// forward piece it differentiates: the axis-angle -> rotation map, one link of the kinematic chain, the rest-pose removal.
// Plain C++, no HIP: tools/mano_grad_check.cpp compiles it alone and holds every backward to central differences of its
// forward in double; ACRMI_HD (csrc/roi_plan.h) is `__host__ __device__` when the translation unit is HIP.
//
// The forward pieces are csrc/mano.hip's statements: mano_kernel calls their float instantiation, the backward and the
// fitter run this joint level in double (csrc/mano_grad.hip says why) through csrc/mano_stages.h.  The backward pieces are the chain rule through exactly those operations, the 1e-8 inside the norm included:
// it makes the map smooth at a zero axis-angle, and its derivative is taken as it stands.  Matrices are row major; a rigid
// transform is its upper 3 x 4 block [R | t], 12 values.
//
// The backward always works from the fp32 tables, also when ACRMI_OPT_MANO_FP16 makes the forward read f16 copies: the
// gradient is that of mano_kernel<false>.
#pragma once
#include <math.h>

#include "roi_plan.h"      // ACRMI_HD

namespace acrmi {

constexpr int MANO_GRAD_THREADS = 256;      // one workgroup per hand
constexpr int MANO_GRAD_GROUPS = 16;        // vertex groups of the skinning backward: thread = (group, joint)

ACRMI_HD inline float mg_sqrt(float x) { return sqrtf(x); }
ACRMI_HD inline double mg_sqrt(double x) { return sqrt(x); }
ACRMI_HD inline float mg_sin(float x) { return sinf(x); }
ACRMI_HD inline double mg_sin(double x) { return sin(x); }
ACRMI_HD inline float mg_cos(float x) { return cosf(x); }
ACRMI_HD inline double mg_cos(double x) { return cos(x); }

// What both directions of the axis-angle map need: batch_rodrigues + quat2mat (mano/manolayer.py:396-434).
template <typename T>
struct ManoRodrigues {
  T angle, n[3], sn, cs, qn, q[4];      // q = (w, x, y, z), normalised
};

template <typename T>
ACRMI_HD inline void mano_rodrigues_state(const T a[3], ManoRodrigues<T>* s) {
  const T ex = a[0] + (T)1e-8f, ey = a[1] + (T)1e-8f, ez = a[2] + (T)1e-8f;
  s->angle = mg_sqrt(ex * ex + ey * ey + ez * ez);
  s->n[0] = a[0] / s->angle; s->n[1] = a[1] / s->angle; s->n[2] = a[2] / s->angle;
  const T half = s->angle * (T)0.5f;
  s->sn = mg_sin(half);
  s->cs = mg_cos(half);
  T w = s->cs, x = s->sn * s->n[0], y = s->sn * s->n[1], z = s->sn * s->n[2];
  s->qn = mg_sqrt(w * w + x * x + y * y + z * z);
  w /= s->qn; x /= s->qn; y /= s->qn; z /= s->qn;
  s->q[0] = w; s->q[1] = x; s->q[2] = y; s->q[3] = z;
}

// axis-angle a -> R [9]
template <typename T>
ACRMI_HD inline void mano_rodrigues(const T a[3], T R[9]) {
  ManoRodrigues<T> s;
  mano_rodrigues_state(a, &s);
  const T w = s.q[0], x = s.q[1], y = s.q[2], z = s.q[3];
  const T w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
  const T wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
  R[0] = w2 + x2 - y2 - z2; R[1] = 2 * xy - 2 * wz;    R[2] = 2 * wy + 2 * xz;
  R[3] = 2 * wz + 2 * xy;   R[4] = w2 - x2 + y2 - z2;  R[5] = 2 * yz - 2 * wx;
  R[6] = 2 * xz - 2 * wy;   R[7] = 2 * wx + 2 * yz;    R[8] = w2 - x2 - y2 + z2;
}

// The cotangent gR [9] of R -> the cotangent ga [3] of the axis-angle a: back through quat2mat, the normalisation of the
// quaternion, (cos, sin * axis) of the half angle, axis = a / angle and angle = |a + 1e-8|.
template <typename T>
ACRMI_HD inline void mano_rodrigues_backward(const T a[3], const T gR[9], T ga[3]) {
  ManoRodrigues<T> s;
  mano_rodrigues_state(a, &s);
  const T w = s.q[0], x = s.q[1], y = s.q[2], z = s.q[3];
  const T* g = gR;
  T gq[4];
  gq[0] = 2 * (w * (g[0] + g[4] + g[8]) + (z * (g[3] - g[1]) + y * (g[2] - g[6]) + x * (g[7] - g[5])));
  gq[1] = 2 * (x * (g[0] - g[4] - g[8]) + (y * (g[1] + g[3]) + z * (g[2] + g[6]) + w * (g[7] - g[5])));
  gq[2] = 2 * (y * (g[4] - g[0] - g[8]) + (x * (g[1] + g[3]) + w * (g[2] - g[6]) + z * (g[5] + g[7])));
  gq[3] = 2 * (z * (g[8] - g[0] - g[4]) + (w * (g[3] - g[1]) + x * (g[2] + g[6]) + y * (g[5] + g[7])));
  // q = q0 / |q0|
  const T dot = gq[0] * w + gq[1] * x + gq[2] * y + gq[3] * z;
  T g0[4];
  for (int i = 0; i < 4; ++i) g0[i] = (gq[i] - s.q[i] * dot) / s.qn;
  // q0 = (cos(half), sin(half) * n)
  const T g_cs = g0[0];
  const T g_sn = g0[1] * s.n[0] + g0[2] * s.n[1] + g0[3] * s.n[2];
  const T gn[3] = {g0[1] * s.sn, g0[2] * s.sn, g0[3] * s.sn};
  const T g_half = g_sn * s.cs - g_cs * s.sn;
  // n = a / angle, half = angle / 2
  const T g_angle = g_half * (T)0.5f - (gn[0] * a[0] + gn[1] * a[1] + gn[2] * a[2]) / (s.angle * s.angle);
  // angle = sqrt(sum (a + 1e-8)^2)
  for (int i = 0; i < 3; ++i) ga[i] = gn[i] / s.angle + g_angle * ((a[i] + (T)1e-8f) / s.angle);
}

// One link of the chain, G = P . [R | t ; 0 1] (mano/manolayer.py:187-223): P the parent's transform, t = J_j - J_parent.
template <typename T>
ACRMI_HD inline void mano_link(const T P[12], const T R[9], const T t[3], T G[12]) {
  for (int r = 0; r < 3; ++r) {
    const T p0 = P[r * 4], p1 = P[r * 4 + 1], p2 = P[r * 4 + 2], p3 = P[r * 4 + 3];
    G[r * 4 + 0] = p0 * R[0] + p1 * R[3] + p2 * R[6];
    G[r * 4 + 1] = p0 * R[1] + p1 * R[4] + p2 * R[7];
    G[r * 4 + 2] = p0 * R[2] + p1 * R[5] + p2 * R[8];
    G[r * 4 + 3] = p0 * t[0] + p1 * t[1] + p2 * t[2] + p3;
  }
}

// gG [12], the cotangent of the link's G: gP += gG . M^T; gR [9] and gt [3] are the rows of P^T . gG (written, not added).
template <typename T>
ACRMI_HD inline void mano_link_backward(const T P[12], const T R[9], const T t[3], const T gG[12], T gP[12], T gR[9], T gt[3]) {
  for (int r = 0; r < 3; ++r) {
    const T g0 = gG[r * 4], g1 = gG[r * 4 + 1], g2 = gG[r * 4 + 2], g3 = gG[r * 4 + 3];
    for (int c = 0; c < 3; ++c) gP[r * 4 + c] += (g0 * R[c * 3] + g1 * R[c * 3 + 1] + g2 * R[c * 3 + 2]) + g3 * t[c];
    gP[r * 4 + 3] += g3;
  }
  for (int c = 0; c < 3; ++c) {
    const T p0 = P[c], p1 = P[4 + c], p2 = P[8 + c];
    for (int k = 0; k < 3; ++k) gR[c * 3 + k] = p0 * gG[k] + p1 * gG[4 + k] + p2 * gG[8 + k];
    gt[c] = p0 * gG[3] + p1 * gG[7] + p2 * gG[11];
  }
}

// Rest-pose removal, A = G - [0 | G . [J; 0]] (mano/manolayer.py:226-228).
template <typename T>
ACRMI_HD inline void mano_rest(const T G[12], const T J[3], T A[12]) {
  for (int r = 0; r < 3; ++r) {
    A[r * 4] = G[r * 4]; A[r * 4 + 1] = G[r * 4 + 1]; A[r * 4 + 2] = G[r * 4 + 2];
    A[r * 4 + 3] = G[r * 4 + 3] - (G[r * 4] * J[0] + G[r * 4 + 1] * J[1] + G[r * 4 + 2] * J[2]);
  }
}

// gA [12] -> gG += ..., gJ += ...
template <typename T>
ACRMI_HD inline void mano_rest_backward(const T G[12], const T J[3], const T gA[12], T gG[12], T gJ[3]) {
  for (int r = 0; r < 3; ++r) {
    const T g3 = gA[r * 4 + 3];
    for (int c = 0; c < 3; ++c) gG[r * 4 + c] += gA[r * 4 + c] - g3 * J[c];
    gG[r * 4 + 3] += g3;
  }
  for (int c = 0; c < 3; ++c) gJ[c] -= gA[3] * G[c] + gA[7] * G[4 + c] + gA[11] * G[8 + c];
}

}  // namespace acrmi
