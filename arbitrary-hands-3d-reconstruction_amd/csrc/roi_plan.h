// Host side of region-of-interest pre-processing (acrmi_roi_offsets, acrmi_preprocess_rois, acrmi_preprocess_rois_nv12;
// DESIGN.md "Regions of interest"): the clamp of a box to its frame, the emptiness check, the square pad of the window and
// the `offsets` row.  Plain C++, no HIP: tools/roi_plan_check.cpp compiles it alone.
//
// The rule is the reference's image_crop_pad with a bbox (acr/utils.py:1287-1301).  A box (l, t, r, b), r and b exclusive,
// becomes four crop amounts
//   crop_trbl = (max(0, t), max(0, W - r), max(0, H - b), max(0, l))
// the window is frame[ct : H - cb, cl : W - cr], and the window is then a frame of its own size: padded to a square (imgaug
// 0.4.0 compute_paddings_to_reach_aspect_ratio(shape, 1.0): the shorter side, the extra pixel bottom / right) and resized.
// The row is [padded h, padded w, ct, cr, cb, cl, pt, pr, pb, pl], as image_crop_pad returns it.  A window without pixels is
// refused (imgaug's Crop would keep one pixel).
// The window kernels that take their boxes from device memory (csrc/preprocess.hip, DESIGN.md "Tracking on the device") run the
// same functions on the GPU: ACRMI_HD is `__host__ __device__` when the translation unit is HIP and nothing in plain C++.
#pragma once
#include <stdint.h>

#ifndef ACRMI_HD
#ifdef __HIP__
#define ACRMI_HD __host__ __device__
#else
#define ACRMI_HD
#endif
#endif

namespace acrmi {

struct RoiPlan {
  int32_t l, t, r, b;      // the clamped window in frame pixels: rows [t, b), columns [l, r), inside the frame
  int32_t crop[4];         // top, right, bottom, left
  int32_t pad[4];          // top, right, bottom, left of the window's square
  int32_t S;               // the side of the padded square = max(window h, window w)
};

// The pad of an h x w image to a square: the arithmetic acrmi_preprocess_frames uses for a frame of this size.
ACRMI_HD inline void roi_square_pad(int h, int w, int32_t pad_trbl[4]) {
  pad_trbl[0] = pad_trbl[1] = pad_trbl[2] = pad_trbl[3] = 0;
  if (w < h) { const int d = h - w; pad_trbl[1] = (d + 1) / 2; pad_trbl[3] = d / 2; }
  else if (h < w) { const int d = w - h; pad_trbl[0] = d / 2; pad_trbl[2] = (d + 1) / 2; }
}

// Clamps the box to the H x W frame and fills *p.  False - *p untouched - when H or W is not positive or the window has no
// pixels (an inverted box, or one that lies outside the frame).  The differences are taken in 64 bits: any int32 box is fine.
ACRMI_HD inline bool roi_plan(int H, int W, int32_t l, int32_t t, int32_t r, int32_t b, RoiPlan* p) {
  if (H <= 0 || W <= 0) return false;
  const int64_t ct = t > 0 ? (int64_t)t : 0, cl = l > 0 ? (int64_t)l : 0;
  const int64_t cr = (int64_t)W - r > 0 ? (int64_t)W - r : 0, cb = (int64_t)H - b > 0 ? (int64_t)H - b : 0;
  const int64_t h = (int64_t)H - ct - cb, w = (int64_t)W - cl - cr;
  if (h <= 0 || w <= 0) return false;
  // h, w > 0 bound every crop amount by the frame's size
  p->l = (int32_t)cl; p->t = (int32_t)ct; p->r = (int32_t)(W - cr); p->b = (int32_t)(H - cb);
  p->crop[0] = (int32_t)ct; p->crop[1] = (int32_t)cr; p->crop[2] = (int32_t)cb; p->crop[3] = (int32_t)cl;
  roi_square_pad((int)h, (int)w, p->pad);
  p->S = (int32_t)(h > w ? h : w);
  return true;
}

ACRMI_HD inline void roi_offsets_row(const RoiPlan& p, float o[10]) {
  o[0] = o[1] = (float)p.S;
  for (int i = 0; i < 4; ++i) {
    o[2 + i] = (float)p.crop[i];
    o[6 + i] = (float)p.pad[i];
  }
}

// What the device does with a box, where nothing can be refused: the plan of the box and 0, or - the box leaves no pixel of the
// frame - the plan of the whole frame (0, 0, W, H) and 1.  H and W must be positive (with either <= 0, *p is left untouched).
ACRMI_HD inline int roi_plan_or_frame(int H, int W, int32_t l, int32_t t, int32_t r, int32_t b, RoiPlan* p) {
  if (roi_plan(H, W, l, t, r, b, p)) return 0;
  (void)roi_plan(H, W, 0, 0, W, H, p);
  return 1;
}

}  // namespace acrmi
