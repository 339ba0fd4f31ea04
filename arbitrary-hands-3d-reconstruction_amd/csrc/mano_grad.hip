// MANO backward (acrmi_mano_backward): the gradient of what mano_kernel<false> (csrc/mano.hip) computes
// in its axis-angle mode, with respect to the 48 pose values and the 10 betas of every hand, from the cotangents of verts,
// joints and center.  One workgroup of 256 threads per hand, like the forward: recompute the forward's intermediates in LDS
// with the forward's own statements (R, pose map, v_shaped, J, v_posed, G, A), then walk back - root alignment, joints,
// skinning, rest-pose removal, kinematic chain, pose blend, shape blend, Rodrigues (csrc/mano_grad_plan.h).
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
#include "kernels.h"
#include "mano_grad_plan.h"
#include "mano_plan.h"

namespace acrmi {

namespace {

__constant__ int g_parent[16] = {-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14};
__constant__ int g_depth[16] = {0, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3};
__constant__ int g_reorder[21] = {0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20};
__constant__ int g_tips[2][5] = ACRMI_MANO_TIPS;  // [left, right]

template <typename T>
__device__ inline T wave_sum(T s) {
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  return s;      // lane 0 holds the sum
}

}  // namespace

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

  // ---- recompute: the forward's statements (csrc/mano.hip) on one slice that owns every vertex ----
  const float* pose = a.poses + (size_t)row * a.pose_stride;
  if (tid < 10) sBeta[tid] = a.betas[(size_t)row * a.beta_stride + tid];
  if (tid < 16) {
    double aa[3] = {pose[3 * tid], pose[3 * tid + 1], pose[3 * tid + 2]};
    if (tid > 0) {
      aa[0] += T.hands_mean[3 * (tid - 1)];
      aa[1] += T.hands_mean[3 * (tid - 1) + 1];
      aa[2] += T.hands_mean[3 * (tid - 1) + 2];
    }
    sAA[tid][0] = aa[0]; sAA[tid][1] = aa[1]; sAA[tid][2] = aa[2];
    mano_rodrigues(aa, sR[tid]);
  }
  __syncthreads();
  if (tid < 135) {
    const int k9 = tid % 9;
    sPoseMap[tid] = (float)(sR[1 + tid / 9][k9] - ((k9 == 0 || k9 == 4 || k9 == 8) ? 1.0 : 0.0));
  }
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
    if (lane == 0) sJ[j][d] = s;
  }
  __syncthreads();
  for (int i = tid; i < NV3; i += MANO_GRAD_THREADS) {
    float s = 0.f;
    for (int k = 0; k < 135; ++k) s += T.posedirs_t[k * NV3 + i] * sPoseMap[k];
    sV[i] += s;
  }
  for (int level = 0; level < 4; ++level) {
    if (tid < 16 && g_depth[tid] == level) {
      const int j = tid, p = g_parent[j];
      if (p < 0) {
        for (int r = 0; r < 3; ++r) {
          sG[j][r * 4 + 0] = sR[j][r * 3]; sG[j][r * 4 + 1] = sR[j][r * 3 + 1]; sG[j][r * 4 + 2] = sR[j][r * 3 + 2];
          sG[j][r * 4 + 3] = sJ[0][r];
        }
      } else {
        const double t[3] = {sJ[j][0] - sJ[p][0], sJ[j][1] - sJ[p][1], sJ[j][2] - sJ[p][2]};
        mano_link(sG[p], sR[j], t, sG[j]);
      }
    }
    __syncthreads();
  }
  if (tid < 16) {
    double A[12];
    mano_rest(sG[tid], sJ[tid], A);
#pragma unroll
    for (int e = 0; e < 12; ++e) sA[tid][e] = (float)A[e];
  }

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
  if (tid < 16) {
    int at = 0;
    for (int q = 0; q < 21; ++q)
      if (g_reorder[q] == tid) at = q;
    for (int e = 0; e < 12; ++e) sGG[tid][e] = (e & 3) == 3 ? (double)sGJtr[at][e >> 2] : 0.0;
  } else if (tid >= 64 && tid < 64 + 15) {      // a fingertip is a skinned vertex: its cotangent lands there
    const int q = (tid - 64) / 3, d = (tid - 64) % 3;
    int at = 0;
    for (int k = 0; k < 21; ++k)
      if (g_reorder[k] == 16 + q) at = k;
    sGV[g_tips[side][q] * 3 + d] += sGJtr[at][d];
  }
  __syncthreads();

  // ---- skinning: gA[j] = sum_v w[v,j] * g_out[v] (x) [v_posed[v]; 1].  Thread (group, j) adds the vertices group,
  // group + 16, ... in ascending order; the 16 partial sums of an element are then added in group order ----
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
    sGA[tid / 12][tid % 12] = s;
  }
  // g_vposed[v] = Tm[:3,:3]^T g_out[v], Tm = sum_j w[v,j] A[j] as the forward builds it (in place: a vertex is one thread's)
  for (int v = tid; v < NV; v += MANO_GRAD_THREADS) {
    float Tm[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) Tm[e] = 0.f;
    const float* wv = T.weights + v * 16;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float w = wv[j];
#pragma unroll
      for (int e = 0; e < 12; ++e) Tm[e] += sA[j][e] * w;
    }
    const float g0 = sGV[v * 3], g1 = sGV[v * 3 + 1], g2 = sGV[v * 3 + 2];
    sGV[v * 3] = Tm[0] * g0 + Tm[4] * g1 + Tm[8] * g2;
    sGV[v * 3 + 1] = Tm[1] * g0 + Tm[5] * g1 + Tm[9] * g2;
    sGV[v * 3 + 2] = Tm[2] * g0 + Tm[6] * g1 + Tm[10] * g2;
  }
  __syncthreads();

  // ---- rest-pose removal, then the chain from the leaves to the root: a parent gathers its children in ascending order ----
  if (tid < 16) mano_rest_backward(sG[tid], sJ[tid], sGA[tid], sGG[tid], sGJ[tid]);
  __syncthreads();
  for (int level = 2; level >= 0; --level) {
    if (tid < 16 && g_depth[tid] == level) {
      const int p = tid;
      for (int j = p + 1; j < 16; ++j) {
        if (g_parent[j] != p) continue;
        const double t[3] = {sJ[j][0] - sJ[p][0], sJ[j][1] - sJ[p][1], sJ[j][2] - sJ[p][2]};
        double gt[3];
        mano_link_backward(sG[p], sR[j], t, sGG[j], sGG[p], sGR[j], gt);
        for (int d = 0; d < 3; ++d) {
          sGJ[j][d] += gt[d];
          sGJ[p][d] -= gt[d];
        }
      }
    }
    __syncthreads();
  }
  if (tid < 12) {      // the root: G_0 = [R_0 | J_0]
    const int r = tid >> 2, c = tid & 3;
    if (c < 3) sGR[0][r * 3 + c] = sGG[0][tid];
    else sGJ[0][r] += sGG[0][tid];
  }
  __syncthreads();

  // ---- pose blend: g_posemap[k] = posedirs[k,:] . g_vposed, rows of the transposed table; gR[1 + k / 9] += g_posemap ----
  for (int k = wave; k < 135; k += 4) {
    const float* prow = T.posedirs_t + (size_t)k * NV3;
    float s = 0.f;
#pragma unroll 4
    for (int i = lane; i < NV3; i += 64) s += prow[i] * sGV[i];
    s = wave_sum(s);
    if (lane == 0) sGR[1 + k / 9][k % 9] += (double)s;
  }
  __syncthreads();
  // ---- Rodrigues: gR -> the cotangent of the axis-angle; hands_mean is an additive constant ----
  if (tid < 16) {
    double ga[3];
    mano_rodrigues_backward(sAA[tid], sGR[tid], ga);
    float* out = a.g_poses + (size_t)row * 48 + 3 * tid;
    out[0] = (float)ga[0]; out[1] = (float)ga[1]; out[2] = (float)ga[2];
  }
  // ---- shape: g_vshaped = g_vposed + J_regressor^T gJ; g_betas[k] = shapedirs[k,:] . g_vshaped ----
  for (int i = tid; i < NV3; i += MANO_GRAD_THREADS) {
    const int v = i / 3, d = i - 3 * v;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) s += T.jreg[j * NV + v] * (float)sGJ[j][d];
    sGV[i] += s;
  }
  __syncthreads();
  for (int k = wave; k < 10; k += 4) {
    const float* srow = T.shapedirs_t + (size_t)k * NV3;
    float s = 0.f;
#pragma unroll 4
    for (int i = lane; i < NV3; i += 64) s += srow[i] * sGV[i];
    s = wave_sum(s);
    if (lane == 0) a.g_betas[(size_t)row * 10 + k] = s;
  }
}

hipError_t launch_mano_backward(const ManoGradArgs& a, hipStream_t s) {
  if (a.H <= 0) return hipSuccess;
  hipLaunchKernelGGL(mano_backward_kernel, dim3(a.H), dim3(MANO_GRAD_THREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace acrmi
