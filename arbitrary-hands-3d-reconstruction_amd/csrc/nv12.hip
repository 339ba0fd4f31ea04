// NV12 video surfaces (a Y plane [H, y_pitch] and a half-height plane of interleaved U, V bytes [H/2, uv_pitch], the layout
// hardware and software decoders hand out) as the input of pre-processing: DESIGN.md "NV12 input".
//
// The colour rule is integer and restated from OpenCV's published cvtColor(COLOR_YUV2BGR_NV12) source
// (modules/imgproc/src/color_yuv.simd.hpp, YUV420sp2RGB8Invoker / cvtYuv42xxp2RGB8, ITUR_BT_601_SHIFT = 20): chroma is
// nearest - the four luma samples of a 2x2 block share one U, V pair - and for a coefficient row (cy, cub, cug, cvg, cvr, y_off)
//   y = max(0, Y - y_off) * cy;  u = U - 128;  v = V - 128;  r = 1 << 19
//   R = clamp((y + cvr v + r) >> 20);  G = clamp((y + cug u + cvg v + r) >> 20);  B = clamp((y + cub u + r) >> 20)
// with an arithmetic shift and a clamp to 0..255.  The host refuses rows whose int32 sums could overflow
// (nv12_coef in csrc/acrmi_ops.hip).  tests/nv12_ref.py is the numpy statement of the same rule; tests require equality.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace acrmi {

// (nv12_pixel, the rule for one pixel: csrc/kernels.h, shared with preprocess_rois_nv12_kernel of csrc/preprocess.hip, the
// kernel of acrmi_preprocess_nv12 and acrmi_preprocess_rois_nv12: NV12 -> RGB -> white square pad -> cubic resize)

// ------------------------------------------------------------------------------------------------
// Plain conversion at full resolution: the frames the overlays are drawn over, and what a caller looks at to see what the
// network was fed.  One thread per 2x2 luma block, so each U, V pair is loaded once; blockIdx.y = the frame, the blocks of a
// frame in a grid-stride loop (frames of one launch may differ in size).  dst is a tight [H, W, 3] image, RGB or BGR.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nv12_to_rgb_kernel(const Nv12DstBatch pb, const Nv12Coef k, int bgr) {
  const int f = blockIdx.y;
  const int H = pb.f[f].H, W = pb.f[f].W;
  const size_t y_pitch = (size_t)pb.f[f].y_pitch, uv_pitch = (size_t)pb.f[f].uv_pitch;
  const uint8_t* __restrict__ yp = pb.f[f].y;
  const uint8_t* __restrict__ uvp = pb.f[f].uv;
  uint8_t* __restrict__ dst = pb.f[f].dst;
  const int bw = W >> 1;
  const long blocks = (long)(H >> 1) * bw;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < blocks; i += (long)gridDim.x * 256) {
    const int bx = (int)(i % bw), by = (int)(i / bw);
    const uint8_t* c = uvp + (size_t)by * uv_pitch + 2 * bx;
    const int U = c[0], V = c[1];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const uint8_t* yr = yp + (size_t)(2 * by + dy) * y_pitch + 2 * bx;
      uint8_t* o = dst + ((size_t)(2 * by + dy) * W + 2 * bx) * 3;
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        int R, G, B;
        nv12_pixel(k, yr[dx], U, V, R, G, B);
        o[3 * dx] = (uint8_t)(bgr ? B : R);
        o[3 * dx + 1] = (uint8_t)G;
        o[3 * dx + 2] = (uint8_t)(bgr ? R : B);
      }
    }
  }
}

hipError_t launch_nv12_to_rgb(const Nv12DstBatch& pb, const Nv12Coef& k, int n, int bgr, hipStream_t s) {
  long most = 1;
  for (int i = 0; i < n; ++i) {
    const long b = (long)(pb.f[i].H >> 1) * (pb.f[i].W >> 1);
    if (b > most) most = b;
  }
  long g = (most + 255) / 256;
  if (g > 1024) g = 1024;
  hipLaunchKernelGGL(nv12_to_rgb_kernel, dim3((unsigned)g, (unsigned)n), dim3(256), 0, s, pb, k, bgr);
  return hipGetLastError();
}

}  // namespace acrmi
