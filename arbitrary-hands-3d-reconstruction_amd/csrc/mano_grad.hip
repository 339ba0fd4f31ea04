// MANO backward (acrmi_mano_backward): the gradient of what mano_kernel<false> (csrc/mano.hip) computes
// in its axis-angle mode, with respect to the 48 pose values and the 10 betas of every hand, from the cotangents of verts,
// joints and center.  One workgroup of 256 threads per hand, like the forward: recompute the forward's intermediates in LDS
// with the forward's own statements (R, pose map, v_shaped, J, v_posed, G, A), then walk back - root alignment, joints,
// skinning, rest-pose removal, kinematic chain, pose blend, shape blend, Rodrigues.  The recompute and the walk back from
// the joints on are the stages of csrc/mano_stages.h, which the fused fitter (csrc/mano_fit.hip) calls too; the per-joint
// arithmetic is csrc/mano_grad_plan.h's.  This file keeps what is the backward's alone: loading the cotangents and the root
// alignment.
//
// TWO PRECISIONS.  The vertex level - blend shapes, skinning, their 778- and 2334-term sums - is the forward's fp32.  The
// joint level - the 16 rotations, the regressed joints J (with the v_shaped they are regressed from), G, A and everything
// the walk back does per joint - is fp64: it is a few thousand operations per hand, and it is where fp32 loses the
// gradient.  A cotangent on `center` alone makes the root's gradient c . dR/da (J_j - J_0), which can cancel 100-fold; fp32
// joints alone then put the row 4.6e-6 off its float64 value, three quarters of the bar.
//
// Every sum has one fixed order (lane-strided partial sums folded by a shuffle tree, or a serial loop): no atomics, and the
// result of a row does not depend on the batch it is in.  The one large table read, the 1.26 MB pose blend table, runs
// along the rows of the transposed table exactly as in the forward.  The backward ALWAYS reads the fp32 tables, also when
// ACRMI_OPT_MANO_FP16 is set: gradients through the f16 copies are not built.
#include "mano_stages.h"

namespace acrmi {

__global__ __launch_bounds__(MANO_GRAD_THREADS) void mano_backward_kernel(const ManoGradArgs a) {
  const int row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int side = a.side ? (a.side[row] != 0) : (row & 1);
  const ManoTables& T = a.t[side];
  // the joint level (16 joints) in fp64, the vertex level (778 vertices) in fp32 - see the header comment
  __shared__ double sAA[16][3];      // axis-angle, hands_mean added
  __shared__ double sR[16][9];
  __shared__ double sJ[16][3];
  __shared__ double sG[16][12];
  __shared__ double sGA[16][12];
  __shared__ double sGG[16][12];
  __shared__ double sGJ[16][3];
  __shared__ double sGR[16][9];
  __shared__ double sVd[NV3];        // v_shaped for the joint regression; afterwards its storage holds sPart
  __shared__ float sPoseMap[136];
  __shared__ float sBeta[10];
  __shared__ float sV[NV3];          // v_shaped, then v_posed
  __shared__ float sGV[NV3];         // cotangent of the skinned vertices, then of v_posed, then of v_shaped
  __shared__ float sA[16][12];
  __shared__ float sGJtr[21][3];     // cotangent of the 21 unaligned joints
  __shared__ float sRed[4][3];
  float (*sPart)[16][12] = reinterpret_cast<float (*)[16][12]>(sVd);      // [MANO_GRAD_GROUPS][16][12]
  static_assert(sizeof(float) * MANO_GRAD_GROUPS * 16 * 12 <= sizeof(double) * NV3, "sPart lives in sVd");
  const ManoJointLevel L = {sAA, sR, sJ, sG, sGA, sGG, sGJ, sGR, sA};

  // ---- recompute (csrc/mano_stages.h): the forward's statements on one slice that owns every vertex ----
  const float* pose = a.poses + (size_t)row * a.pose_stride;
  if (tid < 10) sBeta[tid] = a.betas[(size_t)row * a.beta_stride + tid];
  mano_rotations(L, pose, T.hands_mean, tid);
  mano_dense_forward(T, L, sBeta, sPoseMap, sVd, sV, tid, lane, wave);
  mano_chain(L, tid);

  // ---- root alignment and joints: the cotangents of the unaligned vertices (sGV) and of the 21 unaligned joints ----
  const float* gv = a.g_verts ? a.g_verts + (size_t)row * NV3 : nullptr;
  const float* gj = a.g_joints ? a.g_joints + (size_t)row * 63 : nullptr;
  const float* gc = a.g_center ? a.g_center + (size_t)row * 3 : nullptr;
  {
    // thread t adds the values i = t, t + 256, ... : 256 = 1 mod 3, so the coordinate of its m-th value is (t + m) % 3
    float s3[3] = {0.f, 0.f, 0.f};
    for (int i = tid, d = tid % 3; i < NV3; i += MANO_GRAD_THREADS, d = d == 2 ? 0 : d + 1) {
      const float g = gv ? gv[i] : 0.f;
      sGV[i] = g;
      s3[0] += d == 0 ? g : 0.f;
      s3[1] += d == 1 ? g : 0.f;
      s3[2] += d == 2 ? g : 0.f;
    }
    for (int d = 0; d < 3; ++d) {
      const float s = wave_sum(s3[d]);
      if (lane == 0) sRed[wave][d] = s;
    }
  }
  if (tid < 63) sGJtr[tid / 3][tid % 3] = gj ? gj[tid] : 0.f;
  __syncthreads();
  if (tid < 3 && a.center_idx >= 0) {
    // every output is x - jtr[center_idx], and center is jtr[center_idx] itself
    float s = ((sRed[0][tid] + sRed[1][tid]) + (sRed[2][tid] + sRed[3][tid]));
    for (int j = 0; j < 21; ++j) s += sGJtr[j][tid];
    sGJtr[a.center_idx][tid] += (gc ? gc[tid] : 0.f) - s;
  }
  if (tid >= 64 && tid < 64 + 48) {      // the chain joints feed gG[:, :3, 3]; gG, gJ start here
    const int j = (tid - 64) / 3;
    sGJ[j][(tid - 64) % 3] = 0.0;
  }
  __syncthreads();
  // ---- the walk back (csrc/mano_stages.h): skinning, rest-pose removal and chain, pose blend, Rodrigues, shape ----
  mano_seed<true>(L, sGJtr, sGV, side, tid);
  __syncthreads();
  mano_skin_backward(T, L, sV, sGV, sPart, tid);
  __syncthreads();
  mano_chain_backward(L, tid);
  mano_pose_blend_backward(T, L, sGV, lane, wave);
  __syncthreads();
  mano_rotations_backward(L, a.g_poses + (size_t)row * 48, tid);
  mano_shape_backward(T, L, sGV, a.g_betas + (size_t)row * 10, tid, lane, wave);
}

hipError_t launch_mano_backward(const ManoGradArgs& a, hipStream_t s) {
  if (a.H <= 0) return hipSuccess;
  hipLaunchKernelGGL(mano_backward_kernel, dim3(a.H), dim3(MANO_GRAD_THREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace acrmi
