// The statements the three MANO kernels share - the forward (csrc/mano.hip), the backward (csrc/mano_grad.hip) and the fused
// fitter (csrc/mano_fit.hip) - each stated once, as `__device__ inline` functions over the callers' own __shared__ arrays:
// the kinematic tree, the 64-lane sum, the per-vertex blend of the joint transforms, and the stages of the fp64 joint level
// and the dense fp32 vertex level that the backward and the fitter run on the way forward and on the way back.  The
// per-joint arithmetic (Rodrigues, one chain link, rest-pose removal and their backwards) is csrc/mano_grad_plan.h's.
//
// A stage is called by all MANO_GRAD_THREADS threads of the workgroup, in uniform control flow; its comment names what
// must be complete (written and behind a barrier) on entry and which barriers it contains.  A stage ends WITHOUT a barrier
// unless it says otherwise: what it wrote is the caller's to fence.  Every sum has one fixed order, which is part of the
// stage: the gradient of a hand is the same bytes from the backward and from the dense fitter.
#pragma once
#include "kernels.h"
#include "mano_grad_plan.h"
#include "mano_plan.h"

namespace acrmi {

namespace {

// ---- the kinematic tree: joint 0 is the wrist, five fingers of three joints each (mano/manolayer.py:187-223) ----
__constant__ int mano_parent[16] = {-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14};
__constant__ int mano_depth[16] = {0, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3};
// output joint q is chain joint mano_reorder[q] (< 16) or fingertip mano_reorder[q] - 16 (mano/manolayer.py:241-254)
__constant__ int mano_reorder[21] = {0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20};
__constant__ int mano_tips[2][5] = ACRMI_MANO_TIPS;  // [left, right]

// the output joint that `src` (mano_reorder's value) is written to
__device__ inline int mano_output_of(int src) {
  int at = 0;
  for (int q = 0; q < 21; ++q)
    if (mano_reorder[q] == src) at = q;
  return at;
}

// The sum of a wave's 64 lanes by the shuffle tree (offsets 32, 16, ..., 1); lane 0 holds it.
template <typename T>
__device__ inline T wave_sum(T s) {
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  return s;
}

// ---- the per-vertex blend (linear blend skinning, mano/manolayer.py:230-240): Tm = sum_j w[j] A[j], joints ascending,
// from a vertex's 16 weights ----
__device__ inline void mano_blend(const float (*A)[12], const float* w, float Tm[12]) {
#pragma unroll
  for (int e = 0; e < 12; ++e) Tm[e] = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float wj = w[j];
#pragma unroll
    for (int e = 0; e < 12; ++e) Tm[e] += A[j][e] * wj;
  }
}

// o = Tm . [x; y; z; 1]; o may be where x, y, z came from
__device__ inline void mano_blend_apply(const float Tm[12], float x, float y, float z, float o[3]) {
  const float ox = Tm[0] * x + Tm[1] * y + Tm[2] * z + Tm[3];
  const float oy = Tm[4] * x + Tm[5] * y + Tm[6] * z + Tm[7];
  const float oz = Tm[8] * x + Tm[9] * y + Tm[10] * z + Tm[11];
  o[0] = ox; o[1] = oy; o[2] = oz;
}

// o = Tm[:3,:3]^T . g: the cotangent of the blended point from that of the skinned one; o may be where g came from
__device__ inline void mano_blend_apply_t(const float Tm[12], float g0, float g1, float g2, float o[3]) {
  const float o0 = Tm[0] * g0 + Tm[4] * g1 + Tm[8] * g2;
  const float o1 = Tm[1] * g0 + Tm[5] * g1 + Tm[9] * g2;
  const float o2 = Tm[2] * g0 + Tm[6] * g1 + Tm[10] * g2;
  o[0] = o0; o[1] = o1; o[2] = o2;
}

// ---- the stages of the backward and the fitter: the joint level (16 joints) in fp64, the vertex level in fp32
// (csrc/mano_grad.hip says why), always the fp32 tables.  The caller declares the arrays; this names them. ----
struct ManoJointLevel {
  double (*AA)[3];      // axis-angle, hands_mean added
  double (*R)[9];
  double (*J)[3];
  double (*G)[12];
  double (*GA)[12], (*GG)[12], (*GJ)[3], (*GR)[9];      // the cotangents of A, G, J, R
  float (*A)[12];
};

// The 16 rotations from the 48 pose values at `pose` (global memory or LDS).  No barrier.
__device__ inline void mano_rotations(const ManoJointLevel& L, const float* pose, const float* hands_mean, int tid) {
  if (tid < 16) {
    double aa[3] = {pose[3 * tid], pose[3 * tid + 1], pose[3 * tid + 2]};
    if (tid > 0) {
      aa[0] += hands_mean[3 * (tid - 1)];
      aa[1] += hands_mean[3 * (tid - 1) + 1];
      aa[2] += hands_mean[3 * (tid - 1) + 2];
    }
    L.AA[tid][0] = aa[0]; L.AA[tid][1] = aa[1]; L.AA[tid][2] = aa[2];
    mano_rodrigues(aa, L.R[tid]);
  }
}

// The pose blend's 135 coefficients, R[1..15] - I.  On entry: R.  No barrier.
__device__ inline void mano_pose_map(const ManoJointLevel& L, float* sPoseMap, int tid) {
  if (tid < 135) {
    const int k9 = tid % 9;
    sPoseMap[tid] = (float)(L.R[1 + tid / 9][k9] - ((k9 == 0 || k9 == 4 || k9 == 8) ? 1.0 : 0.0));
  }
}

// The dense vertex level on the way forward, csrc/mano.hip's on one slice that owns every vertex: pose map, shape blend
// (in fp64: sVd, and its rounding sV), joint regression from sVd into J, pose blend onto sV (v_posed).  On entry: R and
// sBeta written, not yet fenced.  Three barriers: the first statement, after the shape blend, after the regression.
__device__ inline void mano_dense_forward(const ManoTables& T, const ManoJointLevel& L, const float* sBeta, float* sPoseMap,
                                          double* sVd, float* sV, int tid, int lane, int wave) {
  __syncthreads();
  mano_pose_map(L, sPoseMap, tid);
  for (int i = tid; i < NV3; i += MANO_GRAD_THREADS) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 10; ++k) s += (double)T.shapedirs_t[k * NV3 + i] * (double)sBeta[k];
    s += (double)T.v_template[i];
    sVd[i] = s;
    sV[i] = (float)s;
  }
  __syncthreads();
  for (int o = wave * 12; o < wave * 12 + 12; ++o) {
    const int j = o / 3, d = o % 3;
    double s = 0.0;
    for (int v = lane; v < NV; v += 64) s += (double)T.jreg[j * NV + v] * sVd[v * 3 + d];
    s = wave_sum(s);
    if (lane == 0) L.J[j][d] = s;
  }
  __syncthreads();
  for (int i = tid; i < NV3; i += MANO_GRAD_THREADS) {
    float s = 0.f;
    for (int k = 0; k < 135; ++k) s += T.posedirs_t[k * NV3 + i] * sPoseMap[k];
    sV[i] += s;
  }
}

// The kinematic chain, level by level below the root, then the rest-pose removal into A (rounded to float).  On entry: J
// complete; R complete or written by this thread (mano_rotations).  Four barriers, one after each level; none after A.
__device__ inline void mano_chain(const ManoJointLevel& L, int tid) {
  for (int level = 0; level < 4; ++level) {
    if (tid < 16 && mano_depth[tid] == level) {
      const int j = tid, p = mano_parent[j];
      if (p < 0) {
        for (int r = 0; r < 3; ++r) {
          L.G[j][r * 4 + 0] = L.R[j][r * 3]; L.G[j][r * 4 + 1] = L.R[j][r * 3 + 1]; L.G[j][r * 4 + 2] = L.R[j][r * 3 + 2];
          L.G[j][r * 4 + 3] = L.J[0][r];
        }
      } else {
        const double t[3] = {L.J[j][0] - L.J[p][0], L.J[j][1] - L.J[p][1], L.J[j][2] - L.J[p][2]};
        mano_link(L.G[p], L.R[j], t, L.G[j]);
      }
    }
    __syncthreads();
  }
  if (tid < 16) {
    double A[12];
    mano_rest(L.G[tid], L.J[tid], A);
#pragma unroll
    for (int e = 0; e < 12; ++e) L.A[tid][e] = (float)A[e];
  }
}

// The walk back starts: gG from the cotangents sGJtr of the 21 unaligned joints - a chain joint feeds gG[:, :3, 3] -
// and a fingertip's cotangent lands on its skinned vertex: added to sGV[tip] when sGV holds all vertices (DENSE), written to
// sGV[q] when it holds the five tips.  On entry: sGJtr complete, with DENSE sGV too.  No barrier.
template <bool DENSE>
__device__ inline void mano_seed(const ManoJointLevel& L, const float (*sGJtr)[3], float* sGV, int side, int tid) {
  if (tid < 16) {
    const int at = mano_output_of(tid);
    for (int e = 0; e < 12; ++e) L.GG[tid][e] = (e & 3) == 3 ? (double)sGJtr[at][e >> 2] : 0.0;
  } else if (tid >= 64 && tid < 64 + 15) {
    const int q = (tid - 64) / 3, d = (tid - 64) % 3;
    const int at = mano_output_of(16 + q);
    if constexpr (DENSE) sGV[mano_tips[side][q] * 3 + d] += sGJtr[at][d];
    else sGV[q * 3 + d] = sGJtr[at][d];
  }
}

// Skinning backward over all vertices: gA[j] = sum_v w[v,j] * g_out[v] (x) [v_posed[v]; 1].  Thread (group, j) adds the
// vertices group, group + 16, ... in ascending order; the 16 partial sums of an element are then added in group order, in
// fp64.  Then g_vposed[v] = Tm[:3,:3]^T g_out[v] in place (a vertex is one thread's).  On entry: sV (v_posed), sGV
// (g_out), A complete.  One barrier, between the partial sums and their fold.
__device__ inline void mano_skin_backward(const ManoTables& T, const ManoJointLevel& L, const float* sV, float* sGV,
                                          float (*sPart)[16][12], int tid) {
  {
    const int j = tid & 15, grp = tid >> 4;
    float acc[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) acc[e] = 0.f;
    for (int v = grp; v < NV; v += MANO_GRAD_GROUPS) {
      const float w = T.weights[v * 16 + j];
      const float x[4] = {sV[v * 3], sV[v * 3 + 1], sV[v * 3 + 2], 1.f};
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float wg = w * sGV[v * 3 + r];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r * 4 + c] += wg * x[c];
      }
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) sPart[grp][j][e] = acc[e];
  }
  __syncthreads();
  if (tid < 192) {
    double s = 0.0;
    for (int g = 0; g < MANO_GRAD_GROUPS; ++g) s += (double)sPart[g][tid / 12][tid % 12];
    L.GA[tid / 12][tid % 12] = s;
  }
  for (int v = tid; v < NV; v += MANO_GRAD_THREADS) {
    float Tm[12];
    mano_blend(L.A, T.weights + v * 16, Tm);
    mano_blend_apply_t(Tm, sGV[v * 3], sGV[v * 3 + 1], sGV[v * 3 + 2], sGV + v * 3);
  }
}

// Rest-pose removal backward, then the chain from the leaves to the root - a parent gathers its children in ascending
// order - then the root, G_0 = [R_0 | J_0]: gR and gJ of all 16 joints.  On entry: GA, GG, and GJ (zeros) complete.  Five
// barriers: after the rest pose, after each of the three levels, and a last one after the root.
__device__ inline void mano_chain_backward(const ManoJointLevel& L, int tid) {
  if (tid < 16) mano_rest_backward(L.G[tid], L.J[tid], L.GA[tid], L.GG[tid], L.GJ[tid]);
  __syncthreads();
  for (int level = 2; level >= 0; --level) {
    if (tid < 16 && mano_depth[tid] == level) {
      const int p = tid;
      for (int j = p + 1; j < 16; ++j) {
        if (mano_parent[j] != p) continue;
        const double t[3] = {L.J[j][0] - L.J[p][0], L.J[j][1] - L.J[p][1], L.J[j][2] - L.J[p][2]};
        double gt[3];
        mano_link_backward(L.G[p], L.R[j], t, L.GG[j], L.GG[p], L.GR[j], gt);
        for (int d = 0; d < 3; ++d) {
          L.GJ[j][d] += gt[d];
          L.GJ[p][d] -= gt[d];
        }
      }
    }
    __syncthreads();
  }
  if (tid < 12) {
    const int r = tid >> 2, c = tid & 3;
    if (c < 3) L.GR[0][r * 3 + c] = L.GG[0][tid];
    else L.GJ[0][r] += L.GG[0][tid];
  }
  __syncthreads();
}

// Pose blend backward over all vertices: g_posemap[k] = posedirs[k,:] . g_vposed along the rows of the transposed table,
// a wave per row; gR[1 + k / 9] += g_posemap.  On entry: sGV (g_vposed) and GR complete.  No barrier.
__device__ inline void mano_pose_blend_backward(const ManoTables& T, const ManoJointLevel& L, const float* sGV, int lane, int wave) {
  for (int k = wave; k < 135; k += 4) {
    const float* prow = T.posedirs_t + (size_t)k * NV3;
    float s = 0.f;
#pragma unroll 4
    for (int i = lane; i < NV3; i += 64) s += prow[i] * sGV[i];
    s = wave_sum(s);
    if (lane == 0) L.GR[1 + k / 9][k % 9] += (double)s;
  }
}

// Rodrigues backward: gR -> the 48 pose gradients at `g_poses` (global memory or LDS); hands_mean is an additive constant.
// On entry: GR complete.  No barrier.
__device__ inline void mano_rotations_backward(const ManoJointLevel& L, float* g_poses, int tid) {
  if (tid < 16) {
    double ga[3];
    mano_rodrigues_backward(L.AA[tid], L.GR[tid], ga);
    g_poses[3 * tid] = (float)ga[0]; g_poses[3 * tid + 1] = (float)ga[1]; g_poses[3 * tid + 2] = (float)ga[2];
  }
}

// Shape backward over all vertices: g_vshaped = g_vposed + J_regressor^T gJ in sGV, then g_betas[k] = shapedirs[k,:] .
// g_vshaped, a wave per row, to `g_betas` (global memory or LDS).  On entry: sGV (g_vposed) and GJ complete.  One barrier,
// between the two.
__device__ inline void mano_shape_backward(const ManoTables& T, const ManoJointLevel& L, float* sGV, float* g_betas, int tid,
                                           int lane, int wave) {
  for (int i = tid; i < NV3; i += MANO_GRAD_THREADS) {
    const int v = i / 3, d = i - 3 * v;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) s += T.jreg[j * NV + v] * (float)L.GJ[j][d];
    sGV[i] += s;
  }
  __syncthreads();
  for (int k = wave; k < 10; k += 4) {
    const float* srow = T.shapedirs_t + (size_t)k * NV3;
    float s = 0.f;
#pragma unroll 4
    for (int i = lane; i < NV3; i += 64) s += srow[i] * sGV[i];
    s = wave_sum(s);
    if (lane == 0) g_betas[k] = s;
  }
}

}  // namespace

}  // namespace acrmi
