// Fused MANO fitter (acrmi_mano_fit): `steps` Adam iterations per hand in ONE launch, against 3-D joints,
// 2-D key points through the weak-perspective camera, vertices, or any mix (csrc/mano_fit_plan.h states the parameters, the loss,
// its cotangents, the update and the state row).  One workgroup of 256 threads per hand, like the backward; the 64 parameters,
// Adam's m and v and the targets of the hand live in LDS for the whole launch; every step runs forward, loss and cotangents,
// backward and the update without leaving the workgroup.
//
// The forward recompute and the walk back are the backward's (csrc/mano_grad.hip): both kernels call the stages of
// csrc/mano_stages.h - the joint level in fp64, the vertex level in fp32, always the fp32 tables.  What the fit needs beyond the
// backward's recompute - the root-aligned joints, the fingertips and, with a vertex target, the skinned vertices - is the blend of
// csrc/mano_stages.h applied to the fp64 chain's transforms.  This file keeps what is the fitter's alone: the prologue, the
// sparse level's 15 coordinates, the loss with its cotangents and the Adam step.
//
// TWO VERTEX LEVELS (the template argument).  DENSE, with a vertex target (or dense=1): all 778 vertices as in the backward, the
// 1.26 MB pose blend table is streamed twice per step.  SPARSE, without one: the only vertices that matter are the five
// fingertips.  A prologue computes J_template = Jreg . v_template and J_dirs[k] = Jreg . shapedirs[k] in fp64 into LDS once
// per launch and copies the 15 tip columns of the blend tables (135 x 15 + 10 x 15 values) and the tips' skinning weights; a
// step then touches no global memory at all.
//
// Every sum has one fixed order (mano_fit_plan.h); no atomics; a hand's result does not depend on the batch it is in.
#include "mano_fit_plan.h"
#include "mano_stages.h"

namespace acrmi {

static_assert(FIT_THREADS == MANO_GRAD_THREADS, "the walk back is the backward's, thread for thread");

// The sparse level fits two workgroups per CU into the register file without scratch; the dense level, which keeps the 16 joint
// transforms in registers across its vertex loops, does not (864 bytes of scratch per lane when capped): one per CU.
template <bool DENSE>
__global__ __launch_bounds__(FIT_THREADS, DENSE ? 1 : 2) void mano_fit_kernel(const ManoFitArgs a) {
  const int row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int side = a.side ? (a.side[row] != 0) : (row & 1);
  const ManoTables& T = a.t[side];
  constexpr int NVL = DENSE ? NV3 : 15;      // the vertex coordinates this instantiation holds: all, or the five tips'
  // the optimiser's state and the targets
  __shared__ float sP[FIT_PARAMS], sM[FIT_PARAMS], sVar[FIT_PARAMS], sGrad[FIT_PARAMS];
  __shared__ float sY3[63], sW3[21], sY2[42], sW2[21], sPrior[FIT_PARAMS];
  __shared__ float sYV[DENSE ? NV3 : 1];
  __shared__ double sLoss[2];      // first, last evaluated step
  // the joint level in fp64, the vertex level in fp32 (csrc/mano_grad.hip says why)
  __shared__ double sAA[16][3];
  __shared__ double sR[16][9];
  __shared__ double sJ[16][3];
  __shared__ double sG[16][12];
  __shared__ double sGA[16][12];
  __shared__ double sGG[16][12];
  __shared__ double sGJ[16][3];
  __shared__ double sGR[16][9];
  __shared__ double sJtr[21][3];     // the 21 unaligned joints
  __shared__ double sTerm[21][7];    // fit_joint's terms
  __shared__ double sSum[8];         // their sums over the joints
  __shared__ double sVd[DENSE ? NV3 : 1];      // v_shaped for the joint regression; afterwards its storage holds sPart
  __shared__ double sJT[DENSE ? 1 : 48];       // sparse: Jreg . v_template
  __shared__ double sJD[DENSE ? 1 : 480];      // sparse: Jreg . shapedirs[k], [10][48]
  __shared__ float sPD[DENSE ? 1 : 135 * 15];  // sparse: the tip columns of the pose blend table
  __shared__ float sSD[DENSE ? 1 : 10 * 15];   //         of the shape blend table
  __shared__ float sVT[DENSE ? 1 : 15];        //         of v_template
  __shared__ float sW[5][16];        // the tips' skinning weights
  __shared__ float sPoseMap[136];
  __shared__ float sV[NVL];          // v_shaped, then v_posed
  __shared__ float sGV[NVL];         // cotangent of the skinned vertices, then of v_posed, then of v_shaped
  __shared__ float sA[16][12];
  __shared__ float sTip[5][3];       // the skinned fingertips
  __shared__ float sGJtr[21][3];     // cotangent of the 21 unaligned joints
  __shared__ float sRed[4][4];       // per wave: the sums of the vertex cotangents [3] and of the squared residuals
  float (*sPart)[16][12] = reinterpret_cast<float (*)[16][12]>(sVd);      // dense: [MANO_GRAD_GROUPS][16][12]
  static_assert(!DENSE || sizeof(float) * MANO_GRAD_GROUPS * 16 * 12 <= sizeof(double) * NV3, "sPart lives in sVd");
  const ManoJointLevel L = {sAA, sR, sJ, sG, sGA, sGG, sGJ, sGR, sA};

  float* st = a.state + (size_t)row * FIT_STATE;
  if (tid < FIT_PARAMS) {
    sP[tid] = st[tid];
    sM[tid] = st[FIT_STATE_M + tid];
    sVar[tid] = st[FIT_STATE_V + tid];
    sGrad[tid] = 0.f;
  }
  const float t0 = st[FIT_STATE_T];
  if (tid == 0) { sLoss[0] = (double)st[FIT_STATE_LOSS0]; sLoss[1] = (double)st[FIT_STATE_LOSS]; }
  const bool has3 = a.y3 != nullptr, has2 = a.y2 != nullptr;
  const float wv = (DENSE && a.yv) ? (a.wv ? a.wv[row] : 1.f) : 0.f;
  const bool hasV = DENSE && a.yv != nullptr && wv != 0.f;
  const int steps = a.steps;
  if (steps > 0) {
    if (tid < 63) sY3[tid] = has3 ? a.y3[(size_t)row * 63 + tid] : 0.f;
    if (tid < 42) sY2[tid] = has2 ? a.y2[(size_t)row * 42 + tid] : 0.f;
    if (tid >= 64 && tid < 85) sW3[tid - 64] = has3 ? (a.w3 ? a.w3[(size_t)row * 21 + tid - 64] : 1.f) : 0.f;
    if (tid >= 96 && tid < 117) sW2[tid - 96] = has2 ? (a.w2 ? a.w2[(size_t)row * 21 + tid - 96] : 1.f) : 0.f;
    if (tid >= 128 && tid < 128 + FIT_PARAMS)
      sPrior[tid - 128] = (a.prior && tid - 128 < FIT_PRIOR) ? a.prior[(size_t)row * FIT_PRIOR + tid - 128] : 0.f;
    if (tid < 80) sW[tid / 16][tid % 16] = T.weights[mano_tips[side][tid / 16] * 16 + tid % 16];
    if constexpr (DENSE) {
      if (hasV)
        for (int i = tid; i < NV3; i += FIT_THREADS) sYV[i] = a.yv[(size_t)row * NV3 + i];
    } else {
      // the prologue of the sparse level: 11 x 48 dot products of length 778 in fp64, 132 per wave, and the tip columns
      for (int o = wave; o < 11 * 48; o += 4) {
        const int k = o / 48, jd = o % 48, j = jd / 3, d = jd % 3;
        const float* col = k == 0 ? T.v_template : T.shapedirs_t + (size_t)(k - 1) * NV3;
        double s = 0.0;
        for (int v = lane; v < NV; v += 64) s += (double)T.jreg[j * NV + v] * (double)col[v * 3 + d];
        s = wave_sum(s);
        if (lane == 0) {
          if (k == 0) sJT[jd] = s;
          else sJD[(k - 1) * 48 + jd] = s;
        }
      }
      for (int i = tid; i < 135 * 15; i += FIT_THREADS) {
        const int k = i / 15, c = i % 15;
        sPD[i] = T.posedirs_t[(size_t)k * NV3 + mano_tips[side][c / 3] * 3 + c % 3];
      }
      if (tid < 150) {
        const int k = tid / 15, c = tid % 15;
        sSD[tid] = T.shapedirs_t[(size_t)k * NV3 + mano_tips[side][c / 3] * 3 + c % 3];
      }
      if (tid < 15) sVT[tid] = T.v_template[mano_tips[side][tid / 3] * 3 + tid % 3];
    }
  }
  __syncthreads();

  for (int step = 1; step <= steps; ++step) {
    // ---- forward: the recompute both levels share with the backward (csrc/mano_stages.h), then csrc/mano.hip's tips, joints
    // and root alignment ----
    mano_rotations(L, sP, T.hands_mean, tid);
    const float* sBeta = sP + FIT_BETAS;
    if constexpr (DENSE) {
      mano_dense_forward(T, L, sBeta, sPoseMap, sVd, sV, tid, lane, wave);
    } else {
      if (tid >= 192 && tid < 192 + 48) {      // J = J_template + J_dirs . betas
        const int jd = tid - 192;
        double s = sJT[jd];
#pragma unroll
        for (int k = 0; k < 10; ++k) s += sJD[k * 48 + jd] * (double)sBeta[k];
        sJ[jd / 3][jd % 3] = s;
      }
      if (tid >= 64 && tid < 64 + 15) {
        const int i = tid - 64;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 10; ++k) s += (double)sSD[k * 15 + i] * (double)sBeta[k];
        s += (double)sVT[i];
        sV[i] = (float)s;
      }
      __syncthreads();
      mano_pose_map(L, sPoseMap, tid);
      __syncthreads();
      if (tid < 15) {
        float s = 0.f;
        for (int k = 0; k < 135; ++k) s += sPD[k * 15 + tid] * sPoseMap[k];
        sV[tid] += s;
      }
    }
    mano_chain(L, tid);
    __syncthreads();
    if (tid < 5) {      // the fingertips: the forward's skinning of one vertex
      const int at = DENSE ? mano_tips[side][tid] * 3 : tid * 3;
      float Tm[12];
      mano_blend(sA, sW[tid], Tm);
      mano_blend_apply(Tm, sV[at], sV[at + 1], sV[at + 2], sTip[tid]);
    }
    __syncthreads();
    if (tid < 63) {
      const int j = tid / 3, d = tid % 3, src = mano_reorder[j];
      sJtr[j][d] = src < 16 ? sG[src][d * 4 + 3] : (double)sTip[src - 16][d];
    }
    __syncthreads();

    // ---- loss and cotangents (mano_fit_plan.h) ----
    double cen[3] = {0.0, 0.0, 0.0};
    if (a.center_idx >= 0) { cen[0] = sJtr[a.center_idx][0]; cen[1] = sJtr[a.center_idx][1]; cen[2] = sJtr[a.center_idx][2]; }
    if (tid < 21) {
      const double x[3] = {sJtr[tid][0] - cen[0], sJtr[tid][1] - cen[1], sJtr[tid][2] - cen[2]};
      const double tr[3] = {sP[FIT_TRANS], sP[FIT_TRANS + 1], sP[FIT_TRANS + 2]};
      const double cam[3] = {sP[FIT_CAM], sP[FIT_CAM + 1], sP[FIT_CAM + 2]};
      double g[3], term[7];
      fit_joint(x, tr, cam, has3 ? sY3 + 3 * tid : nullptr, sW3[tid], has2 ? sY2 + 2 * tid : nullptr, sW2[tid], g, term);
      sGJtr[tid][0] = (float)g[0]; sGJtr[tid][1] = (float)g[1]; sGJtr[tid][2] = (float)g[2];
#pragma unroll
      for (int i = 0; i < 7; ++i) sTerm[tid][i] = term[i];
    }
    if constexpr (DENSE) {
      // the skinned vertices (csrc/mano.hip), their residuals and cotangents; sV keeps v_posed for the walk back
      float s4[4] = {0.f, 0.f, 0.f, 0.f};
      if (hasV) {
        const float c0 = (float)cen[0], c1 = (float)cen[1], c2 = (float)cen[2];
        const float t0f = sP[FIT_TRANS], t1f = sP[FIT_TRANS + 1], t2f = sP[FIT_TRANS + 2];
        for (int v = tid; v < NV; v += FIT_THREADS) {
          float Tm[12], o[3];
          mano_blend(sA, T.weights + v * 16, Tm);
          mano_blend_apply(Tm, sV[v * 3], sV[v * 3 + 1], sV[v * 3 + 2], o);
          const float r0 = fit_vertex_residual(o[0] - c0, t0f, sYV[v * 3]);
          const float r1 = fit_vertex_residual(o[1] - c1, t1f, sYV[v * 3 + 1]);
          const float r2 = fit_vertex_residual(o[2] - c2, t2f, sYV[v * 3 + 2]);
          const float g0 = 2.f * wv * r0, g1 = 2.f * wv * r1, g2 = 2.f * wv * r2;
          sGV[v * 3] = g0; sGV[v * 3 + 1] = g1; sGV[v * 3 + 2] = g2;
          s4[0] += g0; s4[1] += g1; s4[2] += g2;
          s4[3] += (r0 * r0 + r1 * r1) + r2 * r2;
        }
      } else {
        for (int i = tid; i < NV3; i += FIT_THREADS) sGV[i] = 0.f;
      }
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const float s = wave_sum(s4[d]);
        if (lane == 0) sRed[wave][d] = s;
      }
    } else {
      if (tid >= 64 && tid < 80) sRed[(tid - 64) >> 2][tid & 3] = 0.f;
    }
    __syncthreads();
    if (tid >= 32 && tid < 39) sSum[tid - 32] = fit_fold(sTerm, tid - 32);
    if (tid < 3 && a.center_idx >= 0) {
      // every output is x - jtr[center_idx]; center itself carries no cotangent
      float s = ((sRed[0][tid] + sRed[1][tid]) + (sRed[2][tid] + sRed[3][tid]));
      for (int j = 0; j < 21; ++j) s += sGJtr[j][tid];
      sGJtr[a.center_idx][tid] += 0.f - s;
    }
    if (tid >= 64 && tid < 64 + 48) {
      const int j = (tid - 64) / 3;
      sGJ[j][(tid - 64) % 3] = 0.0;
    }
    __syncthreads();

    // ---- the walk back (csrc/mano_stages.h): the backward's, from the joints on; the sparse level restricts the vertex sums
    // to the five tips ----
    mano_seed<DENSE>(L, sGJtr, sGV, side, tid);
    __syncthreads();
    if constexpr (DENSE) {
      mano_skin_backward(T, L, sV, sGV, sPart, tid);
    } else {
      if (tid < 192) {      // gA[j] over the five tips, ascending
        const int j = tid / 12, e = tid % 12, r = e >> 2, c = e & 3;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 5; ++q) s += (double)(sW[q][j] * sGV[q * 3 + r]) * (c < 3 ? (double)sV[q * 3 + c] : 1.0);
        sGA[j][e] = s;
      }
      __syncthreads();
      if (tid < 5) {
        float Tm[12];
        mano_blend(sA, sW[tid], Tm);
        mano_blend_apply_t(Tm, sGV[tid * 3], sGV[tid * 3 + 1], sGV[tid * 3 + 2], sGV + tid * 3);
      }
    }
    __syncthreads();
    mano_chain_backward(L, tid);
    if constexpr (DENSE) {
      mano_pose_blend_backward(T, L, sGV, lane, wave);
    } else {
      if (tid < 135) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 15; ++i) s += sPD[tid * 15 + i] * sGV[i];
        sGR[1 + tid / 9][tid % 9] += (double)s;
      }
    }
    __syncthreads();
    mano_rotations_backward(L, sGrad, tid);
    if (tid >= 128 && tid < 131) {      // trans: the joints' share, then the vertices'
      const int d = tid - 128;
      sGrad[FIT_TRANS + d] = (float)(sSum[1 + d] + (double)((sRed[0][d] + sRed[1][d]) + (sRed[2][d] + sRed[3][d])));
    } else if (tid >= 131 && tid < 134) {
      sGrad[FIT_CAM + tid - 131] = (float)sSum[4 + tid - 131];
    }
    if constexpr (DENSE) {
      mano_shape_backward(T, L, sGV, sGrad + FIT_BETAS, tid, lane, wave);
    } else {
      if (tid >= 64 && tid < 74) {      // g_betas[k] = shapedirs[k, tips] . g_vposed + J_dirs[k] . gJ
        const int k = tid - 64;
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 15; ++i) s += (double)sSD[k * 15 + i] * (double)sGV[i];
        for (int jd = 0; jd < 48; ++jd) s += sJD[k * 48 + jd] * sGJ[jd / 3][jd % 3];
        sGrad[FIT_BETAS + k] = (float)s;
      }
    }
    __syncthreads();

    // ---- regulariser, loss value and the Adam step: wave 0, slot = lane ----
    if (tid < FIT_PARAMS) {
      double g = (double)sGrad[tid];
      double reg = fit_prior(tid, (double)sP[tid], sPrior[tid], a.lam_pose, a.lam_beta, &g);
      reg = wave_sum(reg);
      const float gf = (float)g;
      sGrad[tid] = gf;
      const double t = (double)t0 + (double)step;
      if (tid == 0) {
        const double lv = (double)wv * (double)((sRed[0][3] + sRed[1][3]) + (sRed[2][3] + sRed[3][3]));
        const double loss = (sSum[0] + lv) + reg;
        if (t == 1.0) sLoss[0] = loss;
        sLoss[1] = loss;
      }
      double bc1, bc2s;
      fit_adam_bias(a.b1, a.b2, t, &bc1, &bc2s);
      fit_adam(&sP[tid], &sM[tid], &sVar[tid], (double)gf, a.lr[fit_group(tid)], a.b1, a.b2, a.eps, bc1, bc2s);
    }
    __syncthreads();
  }

  // ---- the state row and the outputs ----
  if (tid < FIT_PARAMS) {
    if (steps > 0) {
      st[tid] = sP[tid];
      st[FIT_STATE_M + tid] = sM[tid];
      st[FIT_STATE_V + tid] = sVar[tid];
      if (a.grad) a.grad[(size_t)row * FIT_PARAMS + tid] = sGrad[tid];
    }
    const float p = sP[tid];
    if (tid < FIT_BETAS) a.poses[(size_t)row * 48 + tid] = p;
    else if (tid < FIT_TRANS) a.betas[(size_t)row * 10 + tid - FIT_BETAS] = p;
    else if (tid < FIT_CAM) a.trans[(size_t)row * 3 + tid - FIT_TRANS] = p;
    else a.cam[(size_t)row * 3 + tid - FIT_CAM] = p;
  }
  if (tid == 0) {
    if (steps > 0) {
      st[FIT_STATE_T] = t0 + (float)steps;
      st[FIT_STATE_LOSS] = (float)sLoss[1];
      st[FIT_STATE_LOSS0] = (float)sLoss[0];
    }
    a.loss[(size_t)row * 2] = (float)sLoss[0];
    a.loss[(size_t)row * 2 + 1] = (float)sLoss[1];
  }
}

hipError_t launch_mano_fit(const ManoFitArgs& a, hipStream_t s) {
  if (a.H <= 0) return hipSuccess;
  if (a.yv || a.dense) hipLaunchKernelGGL(mano_fit_kernel<true>, dim3(a.H), dim3(FIT_THREADS), 0, s, a);
  else hipLaunchKernelGGL(mano_fit_kernel<false>, dim3(a.H), dim3(FIT_THREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace acrmi
