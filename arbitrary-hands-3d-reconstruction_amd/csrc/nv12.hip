// NV12 video surfaces (a Y plane [H, y_pitch] and a half-height plane of interleaved U, V bytes [H/2, uv_pitch], the layout
// hardware and software decoders hand out) as the input of pre-processing: DESIGN.md "NV12 input".
//
// The colour rule is integer and restated from OpenCV's published cvtColor(COLOR_YUV2BGR_NV12) source
// (modules/imgproc/src/color_yuv.simd.hpp, YUV420sp2RGB8Invoker / cvtYuv42xxp2RGB8, ITUR_BT_601_SHIFT = 20): chroma is
// nearest - the four luma samples of a 2x2 block share one U, V pair - and for a coefficient row (cy, cub, cug, cvg, cvr, y_off)
//   y = max(0, Y - y_off) * cy;  u = U - 128;  v = V - 128;  r = 1 << 19
//   R = clamp((y + cvr v + r) >> 20);  G = clamp((y + cug u + cvg v + r) >> 20);  B = clamp((y + cub u + r) >> 20)
// with an arithmetic shift and a clamp to 0..255.  The host refuses rows whose int32 sums could overflow
// (acrmi_preprocess_nv12).  tests/nv12_ref.py is the numpy statement of the same rule; tests require equality.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace acrmi {

// (nv12_pixel, the rule for one pixel: csrc/kernels.h, shared with csrc/roi.hip)

// ------------------------------------------------------------------------------------------------
// Fused path: NV12 -> RGB -> white square pad -> OpenCV's fixed-point cubic resize to out_size^2.  This is
// preprocess_frames_kernel (csrc/elementwise.hip) with the tap load replaced: each of the 16 taps is converted to 8-bit
// R, G, B by the rule above BEFORE it enters the int32 cubic sums, so the result is byte for byte what "convert the whole
// frame, then preprocess_frames_kernel" gives, and no full-resolution RGB frame ever exists.  Taps outside the frame are the
// white pad (255, 255, 255), not a converted value.  A tap inside reads y[iy * y_pitch + ix] and the two bytes at
// uv[(iy >> 1) * uv_pitch + (ix & ~1)]: with H and W even, never beyond byte W - 1 of a row, whatever the pitch.
// Up to NV12_FRAMES_PER_LAUNCH frames per launch, their geometry by value in the kernel arguments (64 x 32 bytes + the
// coefficient row: 2.1 KB of the 4 KB argument block).  256 consecutive output pixels never straddle a frame.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void preprocess_nv12_kernel(const Nv12Batch pb, const Nv12Coef k, int n, int out_size,
                                                              uint8_t* __restrict__ out) {
  const long total = (long)n * out_size * out_size;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ox = i % out_size;
    const int oy = (i / out_size) % out_size;
    const int f = i / ((long)out_size * out_size);
    const int H = pb.f[f].H, W = pb.f[f].W;
    const size_t y_pitch = (size_t)pb.f[f].y_pitch, uv_pitch = (size_t)pb.f[f].uv_pitch;
    // imgaug compute_paddings_to_reach_aspect_ratio(shape, 1.0): pad the shorter side, the extra pixel bottom / right
    const int S = H > W ? H : W;
    const int pad_top = H < W ? (W - H) / 2 : 0, pad_left = W < H ? (H - W) / 2 : 0;
    const double scale = (double)S / (double)out_size;
    int sy, sx, cy[4], cx[4];
    cv_cubic_taps(oy, scale, sy, cy);
    cv_cubic_taps(ox, scale, sx, cx);
    int acc[3] = {0, 0, 0};
    const uint8_t* __restrict__ yp = pb.f[f].y;
    const uint8_t* __restrict__ uvp = pb.f[f].uv;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      int yy = sy - 1 + a;
      yy = yy < 0 ? 0 : (yy >= S ? S - 1 : yy);
      const int iy = yy - pad_top;
      int row[3] = {0, 0, 0};
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        int xx = sx - 1 + b;
        xx = xx < 0 ? 0 : (xx >= S ? S - 1 : xx);
        const int ix = xx - pad_left;
        int v0 = 255, v1 = 255, v2 = 255;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
          const uint8_t* c = uvp + (size_t)(iy >> 1) * uv_pitch + (ix & ~1);
          nv12_pixel(k, yp[(size_t)iy * y_pitch + ix], c[0], c[1], v0, v1, v2);
        }
        row[0] += cx[b] * v0; row[1] += cx[b] * v1; row[2] += cx[b] * v2;
      }
      acc[0] += cy[a] * row[0]; acc[1] += cy[a] * row[1]; acc[2] += cy[a] * row[2];
    }
    uint8_t* o = out + (size_t)i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int r = (acc[c] + (1 << 21)) >> 22;
      o[c] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
    }
  }
}

hipError_t launch_preprocess_nv12(const Nv12Batch& pb, const Nv12Coef& k, int n, int out_size, uint8_t* out, hipStream_t s) {
  const long total = (long)n * out_size * out_size;
  long g = (total + 255) / 256;
  if (g > 256L * 32) g = 256L * 32;
  hipLaunchKernelGGL(preprocess_nv12_kernel, dim3((unsigned)g), dim3(256), 0, s, pb, k, n, out_size, out);
  return hipGetLastError();
}

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
