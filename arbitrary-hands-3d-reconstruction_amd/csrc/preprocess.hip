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
#include "roi_plan.h"

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

// The two window kernels again, with the boxes in device memory (DESIGN.md "Tracking on the device").  The record holds the
// FRAME; the kernel reads boxes[box] and makes the plan itself with the host's own functions (csrc/roi_plan.h), so whatever
// the box holds - garbage, an inverted box, the int32 extremes - the window lies inside the frame, and one without pixels
// is the whole frame with status 1.  The plan is a dozen integer operations against 16 taps x 3 channels, and uniform over a
// block: the record index is made scalar (256 consecutive output pixels never straddle a window, and every trip of the
// loop moves a block by a multiple of 256), so the box arrives through the scalar cache and the plan runs on the scalar unit.
// The body and the tap lambdas are those of the kernels above: the same bytes.  The thread of output pixel (0, 0) of a
// region writes that region's `offsets` row and status word.
__device__ inline void write_roi_row(const RoiPlan& p, int st, int box, float* __restrict__ offsets, int32_t* __restrict__ status) {
  if (offsets) {
    float row[10];
    roi_offsets_row(p, row);
    float* o = offsets + (size_t)box * 10;
#pragma unroll
    for (int i = 0; i < 10; ++i) o[i] = row[i];
  }
  if (status) status[box] = st;
}

__global__ __launch_bounds__(256) void preprocess_rois_dev_kernel(const RoiBgrDevBatch rb, const int32_t* __restrict__ boxes, int n,
                                                                  int out_size, uint8_t* __restrict__ out,
                                                                  float* __restrict__ offsets, int32_t* __restrict__ status) {
  const long total = (long)n * out_size * out_size;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ox = i % out_size;
    const int oy = (i / out_size) % out_size;
    const int f = __builtin_amdgcn_readfirstlane((int)(i / ((long)out_size * out_size)));
    const int box = rb.r[f].box;
    const int32_t* __restrict__ q = boxes + (size_t)box * 4;
    RoiPlan p{};
    const int st = roi_plan_or_frame(rb.r[f].H, rb.r[f].W, q[0], q[1], q[2], q[3], &p);
    const size_t pitch = (size_t)rb.r[f].W * 3;
    const uint8_t* __restrict__ src = rb.r[f].frame + (size_t)p.t * pitch + (size_t)p.l * 3;
    cubic_pixel(p.b - p.t, p.r - p.l, out_size, oy, ox,
                [=](int iy, int ix, int& v0, int& v1, int& v2) {
                  const uint8_t* c = src + (size_t)iy * pitch + (size_t)ix * 3;
                  v0 = c[2]; v1 = c[1]; v2 = c[0];          // BGR -> RGB
                },
                out + (size_t)i * 3);
    if (ox == 0 && oy == 0) write_roi_row(p, st, box, offsets, status);
  }
}

__global__ __launch_bounds__(256) void preprocess_rois_nv12_dev_kernel(const RoiNv12DevBatch rb, const Nv12Coef k,
                                                                       const int32_t* __restrict__ boxes, int n, int out_size,
                                                                       uint8_t* __restrict__ out, float* __restrict__ offsets,
                                                                       int32_t* __restrict__ status) {
  const long total = (long)n * out_size * out_size;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ox = i % out_size;
    const int oy = (i / out_size) % out_size;
    const int f = __builtin_amdgcn_readfirstlane((int)(i / ((long)out_size * out_size)));
    const int box = rb.r[f].box;
    const int32_t* __restrict__ q = boxes + (size_t)box * 4;
    RoiPlan p{};
    const int st = roi_plan_or_frame(rb.r[f].H, rb.r[f].W, q[0], q[1], q[2], q[3], &p);
    const uint8_t* __restrict__ yp = rb.r[f].y;
    const uint8_t* __restrict__ uvp = rb.r[f].uv;
    const size_t y_pitch = (size_t)rb.r[f].y_pitch, uv_pitch = (size_t)rb.r[f].uv_pitch;
    const int l = p.l, t = p.t;
    cubic_pixel(p.b - p.t, p.r - p.l, out_size, oy, ox,
                [=](int iy, int ix, int& v0, int& v1, int& v2) {
                  const int fy = t + iy, fx = l + ix;
                  const uint8_t* c = uvp + (size_t)(fy >> 1) * uv_pitch + (size_t)(fx & ~1);
                  nv12_pixel(k, yp[(size_t)fy * y_pitch + (size_t)fx], c[0], c[1], v0, v1, v2);
                },
                out + (size_t)i * 3);
    if (ox == 0 && oy == 0) write_roi_row(p, st, box, offsets, status);
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

hipError_t launch_preprocess_rois_dev(const RoiBgrDevBatch& rb, const int32_t* boxes, int n, int out_size, uint8_t* out,
                                      float* offsets, int32_t* status, hipStream_t s) {
  hipLaunchKernelGGL(preprocess_rois_dev_kernel, dim3(pixel_grid(n, out_size)), dim3(256), 0, s, rb, boxes, n, out_size, out, offsets,
                     status);
  return hipGetLastError();
}

hipError_t launch_preprocess_rois_nv12_dev(const RoiNv12DevBatch& rb, const Nv12Coef& k, const int32_t* boxes, int n, int out_size,
                                           uint8_t* out, float* offsets, int32_t* status, hipStream_t s) {
  hipLaunchKernelGGL(preprocess_rois_nv12_dev_kernel, dim3(pixel_grid(n, out_size)), dim3(256), 0, s, rb, k, boxes, n, out_size, out,
                     offsets, status);
  return hipGetLastError();
}

}  // namespace acrmi
