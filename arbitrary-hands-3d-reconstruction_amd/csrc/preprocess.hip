// Input pre-processing (acr/utils.py:1315-1337; DESIGN.md "NV12 input", "Regions of interest"): a BGR frame,
// an NV12 surface or a window of either -> white-padded square (imgaug 0.4.0 Pad: the extra pixel goes to bottom / right) ->
// cv2.resize(..., (512, 512), INTER_CUBIC) -> RGB uint8.
// The resize is OpenCV's uint8 path restated from its published source (modules/imgproc/src/resize.cpp), bit for bit:
//   fx = (float)((dx + 0.5) * scale - 0.5) with scale in double, sx = floor(fx), fx -= sx;
//   coefficients interpolateCubic(fx) with A = -0.75 in float, stored as short = round-half-even(c * 2048)
//   (INTER_RESIZE_COEF_BITS = 11); horizontal pass in int32 over 4 border-clamped columns; vertical pass in int32
//   over 4 border-clamped rows; dst = saturate((v + 2^21) >> 22)   (FixedPtCast<int, uchar, 22>).
// oracle/preprocess.py is the CPU statement of the same algorithm; tests require equality.
//
// One thread per output pixel, and ONE body for it, cubic_pixel: the kernels differ only in where a record's geometry comes
// from and in how a tap is loaded (a lambda that holds its pointers and pitches by value).  A frame is the window
// (0, 0, W, H) of itself, so frames of different sizes (acrmi_preprocess_frames, acrmi_preprocess_nv12) run the window
// kernels with the plan of the full frame.  The cubic footprint is clamped to the window's padded square, so a tap is a
// pixel of the window or the white pad - on the unpadded axis the clamped border of the WINDOW, on the padded axis white -
// and never a neighbouring pixel of the frame: the bytes are those of cropping first.  The kernels trust the window
// (0 <= t, t + h <= H, 0 <= l, l + w <= W of its frame: csrc/roi_plan.h) and read nothing outside it; source offsets are
// computed in size_t.
// Up to ROIS_PER_LAUNCH windows per launch, their geometry by value in the kernel arguments (64 x 24 bytes, NV12: 64 x 40
// bytes + the coefficient row, of the 4 KB argument block; no device table to allocate or upload).  256 consecutive output
// pixels never straddle a window (512 * 512 % 256 == 0).
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace acrmi {

// One output pixel of an h x w image: tap(iy, ix, v0, v1, v2) loads the R, G, B of the image's pixel (iy, ix), which is
// inside the image.
template <class Tap>
__device__ inline void cubic_pixel(int h, int w, int out_size, int oy, int ox, const Tap& tap, uint8_t* __restrict__ o) {
  // imgaug compute_paddings_to_reach_aspect_ratio(shape, 1.0): pad the shorter side, the extra pixel bottom / right
  const int S = h > w ? h : w;
  const int pad_top = h < w ? (w - h) / 2 : 0, pad_left = w < h ? (h - w) / 2 : 0;
  const double scale = (double)S / (double)out_size;
  int sy, sx, cy[4], cx[4];
  cv_cubic_taps(oy, scale, sy, cy);
  cv_cubic_taps(ox, scale, sx, cx);
  int acc[3] = {0, 0, 0};
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    int yy = sy - 1 + a;
    yy = yy < 0 ? 0 : (yy >= S ? S - 1 : yy);      // border rows / columns of the padded square are clamped
    const int iy = yy - pad_top;
    int row[3] = {0, 0, 0};
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      int xx = sx - 1 + b;
      xx = xx < 0 ? 0 : (xx >= S ? S - 1 : xx);
      const int ix = xx - pad_left;
      int v0 = 255, v1 = 255, v2 = 255;           // white padding (acr/utils.py:1303-1308)
      if (iy >= 0 && iy < h && ix >= 0 && ix < w) tap(iy, ix, v0, v1, v2);
      row[0] += cx[b] * v0; row[1] += cx[b] * v1; row[2] += cx[b] * v2;
    }
    acc[0] += cy[a] * row[0]; acc[1] += cy[a] * row[1]; acc[2] += cy[a] * row[2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int r = (acc[c] + (1 << 21)) >> 22;
    o[c] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
  }
}

// Frames of ONE size in one allocation (acrmi_preprocess; bench.py times it): scalar geometry, one launch for any n.  The
// 1080p source (6.2 MB/frame) is read once through L2.
__global__ __launch_bounds__(256) void preprocess_kernel(const uint8_t* __restrict__ bgr, int n, int H, int W, int out_size,
                                                         uint8_t* __restrict__ out) {
  const long total = (long)n * out_size * out_size;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ox = i % out_size;
    const int oy = (i / out_size) % out_size;
    const int f = i / ((long)out_size * out_size);
    const uint8_t* src = bgr + (size_t)f * H * W * 3;
    cubic_pixel(H, W, out_size, oy, ox,
                [=](int iy, int ix, int& v0, int& v1, int& v2) {
                  const uint8_t* p = src + ((size_t)iy * W + ix) * 3;
                  v0 = p[2]; v1 = p[1]; v2 = p[0];          // BGR -> RGB (acr/utils.py:1318)
                },
                out + (size_t)i * 3);
  }
}

// Windows of BGR frames.  The host has moved the pointer to the window's first pixel; the pitch is the frame's.
__global__ __launch_bounds__(256) void preprocess_rois_kernel(const RoiBgrBatch rb, int n, int out_size, uint8_t* __restrict__ out) {
  const long total = (long)n * out_size * out_size;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ox = i % out_size;
    const int oy = (i / out_size) % out_size;
    const int f = i / ((long)out_size * out_size);
    const uint8_t* __restrict__ src = rb.r[f].src;
    const size_t pitch = rb.r[f].pitch;
    cubic_pixel(rb.r[f].h, rb.r[f].w, out_size, oy, ox,
                [=](int iy, int ix, int& v0, int& v1, int& v2) {
                  const uint8_t* p = src + (size_t)iy * pitch + (size_t)ix * 3;
                  v0 = p[2]; v1 = p[1]; v2 = p[0];          // BGR -> RGB
                },
                out + (size_t)i * 3);
  }
}

// Windows of NV12 surfaces.  A tap at window position (iy, ix) is the frame's pixel (t + iy, l + ix): luma there, chroma at
// uv[((t + iy) >> 1) * uv_pitch + ((l + ix) & ~1)] - in FRAME coordinates, so odd l and t are legal - converted to 8-bit
// R, G, B by nv12_pixel (csrc/nv12.hip states the rule) BEFORE it enters the int32 cubic sums, so the result is byte for
// byte what "convert the whole frame, then the BGR kernel" gives, and no full-resolution RGB frame ever exists.  Taps outside
// the window are the white pad (255, 255, 255), not a converted value.  With H and W even, never beyond byte W - 1 of a row,
// whatever the pitch.
__global__ __launch_bounds__(256) void preprocess_rois_nv12_kernel(const RoiNv12Batch rb, const Nv12Coef k, int n, int out_size,
                                                                   uint8_t* __restrict__ out) {
  const long total = (long)n * out_size * out_size;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ox = i % out_size;
    const int oy = (i / out_size) % out_size;
    const int f = i / ((long)out_size * out_size);
    const uint8_t* __restrict__ yp = rb.r[f].y;
    const uint8_t* __restrict__ uvp = rb.r[f].uv;
    const size_t y_pitch = (size_t)rb.r[f].y_pitch, uv_pitch = (size_t)rb.r[f].uv_pitch;
    const int l = rb.r[f].l, t = rb.r[f].t;
    cubic_pixel(rb.r[f].h, rb.r[f].w, out_size, oy, ox,
                [=](int iy, int ix, int& v0, int& v1, int& v2) {
                  const int fy = t + iy, fx = l + ix;
                  const uint8_t* c = uvp + (size_t)(fy >> 1) * uv_pitch + (size_t)(fx & ~1);
                  nv12_pixel(k, yp[(size_t)fy * y_pitch + (size_t)fx], c[0], c[1], v0, v1, v2);
                },
                out + (size_t)i * 3);
  }
}

// one thread per output pixel in blocks of 256, at most 256 * 32 blocks: the kernels loop over the rest
static unsigned pixel_grid(int n, int out_size) {
  const long total = (long)n * out_size * out_size;
  long g = (total + 255) / 256;
  if (g > 256L * 32) g = 256L * 32;
  return (unsigned)g;
}

hipError_t launch_preprocess(const uint8_t* bgr, int n, int H, int W, int out_size, uint8_t* out, hipStream_t s) {
  hipLaunchKernelGGL(preprocess_kernel, dim3(pixel_grid(n, out_size)), dim3(256), 0, s, bgr, n, H, W, out_size, out);
  return hipGetLastError();
}

hipError_t launch_preprocess_rois(const RoiBgrBatch& rb, int n, int out_size, uint8_t* out, hipStream_t s) {
  hipLaunchKernelGGL(preprocess_rois_kernel, dim3(pixel_grid(n, out_size)), dim3(256), 0, s, rb, n, out_size, out);
  return hipGetLastError();
}

hipError_t launch_preprocess_rois_nv12(const RoiNv12Batch& rb, const Nv12Coef& k, int n, int out_size, uint8_t* out,
                                       hipStream_t s) {
  hipLaunchKernelGGL(preprocess_rois_nv12_kernel, dim3(pixel_grid(n, out_size)), dim3(256), 0, s, rb, k, n, out_size, out);
  return hipGetLastError();
}

}  // namespace acrmi
