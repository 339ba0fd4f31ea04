// How a network map is drawn over frames at their own resolution (heatmap_kernel and region_heatmap_kernel of csrc/overlay.hip,
// segm_kernel of csrc/segm.hip; DESIGN.md "Key-point and heat-map views" and section 23): the rule stated once, for the host and
// for the device.  Plain C++, no HIP: tools/segm_check.cpp compiles it alone; ACRMI_HD (csrc/roi_plan.h) is
// `__host__ __device__` when the translation unit is HIP.  tests/map_view_ref.py restates it in numpy.
//
// The map is h x w cells and covers the 512 x 512 canvas; the frames are H x W.  Everything is fp32, every operation rounded on
// its own (the library is built with -ffp-contract=off).
//   view       of frame f: row f of `view` (sx, sy, ox, oy), else region_view_row of row f of `offsets`, else none
//   canvas     of pixel x: (x + 0.5 - ox) / sx under a view and (x + 0.5) * (512 / W) without one: steps 1-2 of DESIGN.md
//              section 10.  A pixel is COVERED when sx > 0 and sy > 0 (false for NaN) and 0 <= cx < 512 and 0 <= cy < 512.
//   taps       map_tap(cx, w / 512, w), map_tap(cy, h / 512, h): the half-pixel-centre bilinear rule
//   value      ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d) of the four cells; a non-finite cell propagates as the
//              formula says
//   footprint  the cells a tile of pixels samples, so that a kernel can stage them in LDS when they fit its capacity and read
//              every tap from memory when they do not
//   jet        byte = clamp(383 - |4 i - 255 k|, 0, 255) for entry i, k = 3, 2, 1 for red, green, blue: the piece-wise linear
//              "jet" floor(255 clamp(1.5 - |4 t - k|, 0, 1) + 0.5), t = i / 255, in exact integers
//   blend      byte = floor(weight * colour + (1 - weight) * img)
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "region_view_plan.h"      // region_view_row; ACRMI_HD

namespace acrmi {

struct Tap { int i0, i1; float l0, l1; };

// source position of canvas coordinate c on a map of n cells (scale m = n / 512): the half-pixel-centre bilinear rule
ACRMI_HD inline Tap map_tap(float c, float m, int n) {
  const float s = fmaxf(c * m - 0.5f, 0.f);
  Tap t;
  t.i0 = (int)s < n - 1 ? (int)s : n - 1;
  t.i1 = t.i0 + 1 < n - 1 ? t.i0 + 1 : n - 1;
  t.l1 = s - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}

struct MapView { bool has; float sx, sy, ox, oy; };

// the view of frame f: `view` [n, 4], else `offsets` [n, 10], else none (both null)
ACRMI_HD inline MapView map_frame_view(const float* view, const float* offsets, int f) {
  float row[4];
  if (view) {
    for (int k = 0; k < 4; ++k) row[k] = view[f * 4 + k];
  } else if (offsets) {      // as ops.view_from_offsets / render_prep_kernel
    region_view_row(offsets + (size_t)f * 10, row);
  } else {
    return MapView{false, 1.f, 1.f, 0.f, 0.f};
  }
  return MapView{true, row[0], row[1], row[2], row[3]};
}

// canvas coordinate of pixel x: s, o = the view's scale and shift along this axis, k = 512 / (the frame's size along it)
ACRMI_HD inline float map_canvas(int x, bool has_view, float s, float o, float k) {
  return has_view ? ((float)x + 0.5f - o) / s : ((float)x + 0.5f) * k;
}

ACRMI_HD inline bool map_covered(float cx, float cy, float sx, float sy) {
  return sx > 0.f && sy > 0.f && cx >= 0.f && cx < 512.f && cy >= 0.f && cy < 512.f;
}

ACRMI_HD inline float map_value(const Tap& ty, const Tap& tx, float a, float b, float c, float d) {
  return ty.l0 * (tx.l0 * a + tx.l1 * b) + ty.l1 * (tx.l0 * c + tx.l1 * d);
}

// channel c (0 = red) of entry i of the jet
ACRMI_HD inline int map_jet(int i, int c) {
  const int d = 4 * i - 255 * (3 - c), v = 383 - (d < 0 ? -d : d);
  return v < 0 ? 0 : v > 255 ? 255 : v;
}

ACRMI_HD inline uint8_t map_blend(float weight, int colour, int img) {
  return (uint8_t)floorf(weight * (float)colour + (1.f - weight) * (float)img);
}

// What a tile of pixels [X0, X1) x [Y0, Y1) (not empty, inside the frame) samples.  The canvas coordinate is monotone in the
// pixel coordinate and the taps are monotone in the canvas coordinate, so the taps of the first and of the last pixel (clamped
// into the canvas) bound those of every covered pixel between them.  any = 0: no pixel of the tile is covered.
struct MapFootprint { int any, ix, iy, fw, fh; };

ACRMI_HD inline MapFootprint map_footprint(int X0, int X1, int Y0, int Y1, const MapView& v, int H, int W, int h, int w) {
  MapFootprint f = {0, 0, 0, 0, 0};
  const float kx = 512.f / (float)W, ky = 512.f / (float)H;
  const float cx_a = map_canvas(X0, v.has, v.sx, v.ox, kx), cx_b = map_canvas(X1 - 1, v.has, v.sx, v.ox, kx);
  const float cy_a = map_canvas(Y0, v.has, v.sy, v.oy, ky), cy_b = map_canvas(Y1 - 1, v.has, v.sy, v.oy, ky);
  if (!(v.sx > 0.f && v.sy > 0.f && cx_b >= 0.f && cx_a < 512.f && cy_b >= 0.f && cy_a < 512.f)) return f;      // (false for NaN)
  const float mx = (float)w / 512.f, my = (float)h / 512.f;
  f.any = 1;
  f.ix = map_tap(fminf(fmaxf(cx_a, 0.f), 512.f), mx, w).i0;
  f.iy = map_tap(fminf(fmaxf(cy_a, 0.f), 512.f), my, h).i0;
  f.fw = map_tap(fminf(fmaxf(cx_b, 0.f), 512.f), mx, w).i1 - f.ix + 1;
  f.fh = map_tap(fminf(fmaxf(cy_b, 0.f), 512.f), my, h).i1 - f.iy + 1;
  return f;
}

// the footprint's cells of cell_floats floats each fit a staging area of `capacity` floats
ACRMI_HD inline bool map_staged(const MapFootprint& f, int cell_floats, int capacity) {
  return f.any && (long long)f.fw * f.fh * cell_floats <= capacity;
}

}  // namespace acrmi
