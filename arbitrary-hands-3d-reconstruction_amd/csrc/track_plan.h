// The box of the NEXT frame of a video loop from the key points of this one (acrmi_track_box, acrmi_track_boxes; DESIGN.md
// "Tracking on the device"): acr.utils.boxes_from_keypoints restated for fp32 points, once for the host and for the device.
// Plain C++, no HIP: tools/track_plan_check.cpp compiles it alone; ACRMI_HD (csrc/roi_plan.h) is `__host__ __device__` when
// the translation unit is HIP.
//
// The rule, per item:
//   the points whose two coordinates are both finite take part; lo, hi = their per-axis min and max
//   centre = (lo + hi) / 2;  side = max(max(hi - lo) * scale, min_size)
//   l, t = floor(centre - side / 2);  r, b = ceil(centre + side / 2)
//   dx = -l if l < 0 else (W - r if r > W else 0), dy alike: the box is moved back inside the frame ...
//   box = (max(0, l + dx), max(0, t + dy), min(W, r + dx), min(H, b + dy))      ... and cut where it is larger than the frame
//   no finite point: the whole frame (0, 0, W, H)
// and one clause the numpy function does not have, because the device cannot raise: a result without pixels (r <= l or
// b <= t) is the whole frame too.  That happens when the side is lost against the centre in the 53 bits of a double: the point
// (3e38, 40) in a 96 x 160 frame gives (0, 8, 0, 72).
// Everything behind the min / max runs in DOUBLE, operation for operation in numpy's order, and max() / min() are Python's
// (the first argument unless the second is strictly larger / smaller - which is what decides a NaN), so the integers are equal
// to numpy's, not close.  The min and max of fp32 values are exact, so the caller may reduce in fp32.  The library is built with
// -ffp-contract=off: no operation here may be fused.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "roi_plan.h"      // ACRMI_HD

namespace acrmi {

ACRMI_HD inline bool track_finite(float v) { return v >= -FLT_MAX && v <= FLT_MAX; }      // false for NaN and +-inf

ACRMI_HD inline double track_pymax(double a, double b) { return b > a ? b : a; }
ACRMI_HD inline double track_pymin(double a, double b) { return b < a ? b : a; }
// (the values that reach this are 0 .. about the frame's size; the guard keeps the conversion defined for any double)
ACRMI_HD inline int32_t track_to_i32(double v) {
  return v >= 2147483647.0 ? INT32_MAX : (v <= -2147483648.0 ? INT32_MIN : (v == v ? (int32_t)v : 0));
}

// any: at least one point took part, and then (lo_x, lo_y) / (hi_x, hi_y) are the min / max of those points.  scale finite
// and > 0, min_size >= 1.  A frame whose H or W is not positive has no box: (0, 0, 0, 0).
ACRMI_HD inline void track_box(bool any, float lo_x, float lo_y, float hi_x, float hi_y, int H, int W, double scale, int min_size,
                               int32_t box[4]) {
  if (H <= 0 || W <= 0) { box[0] = box[1] = box[2] = box[3] = 0; return; }
  box[0] = 0; box[1] = 0; box[2] = W; box[3] = H;
  if (!any) return;
  const double lx = (double)lo_x, ly = (double)lo_y, hx = (double)hi_x, hy = (double)hi_y;
  const double cx = (lx + hx) / 2, cy = (ly + hy) / 2;
  const double ex = hx - lx, ey = hy - ly;
  const double side = track_pymax((ey > ex ? ey : ex) * scale, (double)min_size);
  const double half = side / 2;
  const double l = floor(cx - half), t = floor(cy - half), r = ceil(cx + half), b = ceil(cy + half);
  const double dx = l < 0 ? -l : (r > W ? (double)W - r : 0.0);
  const double dy = t < 0 ? -t : (b > H ? (double)H - b : 0.0);
  const int32_t bl = track_to_i32(track_pymax(0.0, l + dx)), bt = track_to_i32(track_pymax(0.0, t + dy));
  const int32_t br = track_to_i32(track_pymin((double)W, r + dx)), bb = track_to_i32(track_pymin((double)H, b + dy));
  if (br <= bl || bb <= bt) return;      // no pixels: the whole frame
  box[0] = bl; box[1] = bt; box[2] = br; box[3] = bb;
}

// The rule on n_pts points [n_pts][2] in host memory (n_pts may be 0).
inline void track_box_of_points(const float* pts, int n_pts, int H, int W, double scale, int min_size, int32_t box[4]) {
  bool any = false;
  float lo[2] = {0.f, 0.f}, hi[2] = {0.f, 0.f};
  for (int i = 0; i < n_pts; ++i) {
    const float x = pts[2 * i], y = pts[2 * i + 1];
    if (!track_finite(x) || !track_finite(y)) continue;
    if (!any) { lo[0] = hi[0] = x; lo[1] = hi[1] = y; any = true; continue; }
    lo[0] = x < lo[0] ? x : lo[0]; hi[0] = x > hi[0] ? x : hi[0];
    lo[1] = y < lo[1] ? y : lo[1]; hi[1] = y > hi[1] ? y : hi[1];
  }
  track_box(any, lo[0], lo[1], hi[0], hi[1], H, W, scale, min_size, box);
}

}  // namespace acrmi
