// The boxes of the next frame from the key points of this one, on the device (acrmi_track_boxes; DESIGN.md "Tracking on the
// device"): pj2d_org [n,2,21,2] in the pixels of the original frames and the detection flags of slots [n,2,ACRMI_SLOT] ->
// int32 boxes [n,4] = (l, t, r, b), by the rule of csrc/track_plan.h.
// One wave per region: the 42 points of a region's two hands on lanes 0..41 (hand = lane / 21).  A hand takes part only when
// its flag is > 0.5 (a NaN flag is not), and the coordinates of a hand that does not are never loaded.  A lane without a
// point - lanes 42..63, an unflagged hand, a point with a coordinate that is not finite - holds (+inf, -inf), the identity of
// min / max, so after the butterfly every lane holds the extent of the points that took part, and "no point" is lo > hi.
// fminf / fmaxf of fp32 values are exact; everything behind them is track_plan.h in double, on lane 0, which writes the
// four integers.  Four regions per block of 256, one launch for any n.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "track_plan.h"

namespace acrmi {

constexpr int TRACK_POINTS = 42;      // 2 hands x 21 key points

__global__ __launch_bounds__(256) void track_boxes_kernel(const float* __restrict__ pj2d_org, const float* __restrict__ slots,
                                                          const int32_t* __restrict__ frame_hw, int n, int slot_floats,
                                                          int flag_at, double scale, int min_size, int32_t* __restrict__ boxes) {
  const int lane = threadIdx.x & 63;
  const long region = (long)blockIdx.x * 4 + (threadIdx.x >> 6);      // uniform over the wave
  if (region >= n) return;
  float lo_x = INFINITY, lo_y = INFINITY, hi_x = -INFINITY, hi_y = -INFINITY;
  if (lane < TRACK_POINTS) {
    const long hand = region * 2 + lane / 21;
    if (slots[hand * slot_floats + flag_at] > 0.5f) {
      const float* p = pj2d_org + (hand * 21 + lane % 21) * 2;
      const float x = p[0], y = p[1];
      if (track_finite(x) && track_finite(y)) { lo_x = hi_x = x; lo_y = hi_y = y; }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    lo_x = fminf(lo_x, __shfl_xor(lo_x, m, 64)); lo_y = fminf(lo_y, __shfl_xor(lo_y, m, 64));
    hi_x = fmaxf(hi_x, __shfl_xor(hi_x, m, 64)); hi_y = fmaxf(hi_y, __shfl_xor(hi_y, m, 64));
  }
  if (lane == 0) {
    int32_t box[4];
    track_box(lo_x <= hi_x, lo_x, lo_y, hi_x, hi_y, frame_hw[region * 2], frame_hw[region * 2 + 1], scale, min_size, box);
    int32_t* o = boxes + region * 4;
    o[0] = box[0]; o[1] = box[1]; o[2] = box[2]; o[3] = box[3];
  }
}

hipError_t launch_track_boxes(const float* pj2d_org, const float* slots, const int32_t* frame_hw, int n, int slot_floats,
                              int flag_at, double scale, int min_size, int32_t* boxes, hipStream_t s) {
  hipLaunchKernelGGL(track_boxes_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, pj2d_org, slots, frame_hw, n, slot_floats,
                     flag_at, scale, min_size, boxes);
  return hipGetLastError();
}

}  // namespace acrmi
