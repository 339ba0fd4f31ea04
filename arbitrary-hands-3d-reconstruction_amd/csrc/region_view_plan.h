// Where a region of interest sits in its frame, for the views drawn over regions (acrmi_render_regions,
// acrmi_overlay_regions, acrmi_draw_region_heatmaps; DESIGN.md "Views over regions"): the rule stated once, for the host and
// for the device.  Plain C++, no HIP: tools/region_view_check.cpp compiles it alone; ACRMI_HD (csrc/roi_plan.h) is
// `__host__ __device__` when the translation unit is HIP.
//
// A region has an `offsets` row o = [padded h, padded w, ct, cr, cb, cl, pt, pr, pb, pl] (csrc/roi_plan.h) and a frame index;
// the frames are H x W.  Everything is fp32, every operation rounded on its own (the library is built with -ffp-contract=off).
//   view     (sx, sy, ox, oy) = (o[0] / 512, o[1] / 512, o[5] - o[9], o[2] - o[6]): frame x = canvas x * sx + ox, the map of
//            pj2d -> pj2d_org (csrc/mano.hip), of render_prep_kernel, map_frame_view (csrc/map_view_plan.h) and ops.view_from_offsets
//   window   l = o[5], t = o[2], r = W - o[3], b = H - o[4], each clamped into [0, W] / [0, H] with a clamp that sends NaN to 0;
//            pixel x belongs to the window when its centre does: l <= x + 0.5 < r, that is x0 <= x < x1 with
//            x0 = ceil(l - 0.5), x1 = ceil(r - 0.5) - for the whole numbers the pre-processing writes, x0 = l and x1 = r
//   draws    the frame index is inside [0, n_frames), sx > 0 and sy > 0 (false for NaN), and the window has a pixel
//            (x0 < x1 and y0 < y1).  A region that does not draw contributes nothing: no mesh, no tint.
// 0 <= x0 <= x1 <= W and 0 <= y0 <= y1 <= H hold for every row, whatever it holds, so a kernel that stays inside the window
// stays inside the frame.
#pragma once
#include <math.h>
#include <stdint.h>

#include "roi_plan.h"      // ACRMI_HD

namespace acrmi {

struct RegionView {
  float sx, sy, ox, oy;      // the view
  int x0, x1, y0, y1;        // the window in whole pixels, x1 / y1 exclusive
  int draws;                 // 0 / 1
};

// v into [0, hi]; NaN -> 0
ACRMI_HD inline float region_clamp(float v, float hi) { return v > 0.f ? (v < hi ? v : hi) : 0.f; }

ACRMI_HD inline void region_view_row(const float* o, float view[4]) {
  view[0] = o[0] / 512.f;
  view[1] = o[1] / 512.f;
  view[2] = o[5] - o[9];
  view[3] = o[2] - o[6];
}

ACRMI_HD inline RegionView region_view(const float* o, int frame, int n_frames, int H, int W) {
  RegionView v;
  float row[4];
  region_view_row(o, row);
  v.sx = row[0]; v.sy = row[1]; v.ox = row[2]; v.oy = row[3];
  const float fw = (float)W, fh = (float)H;
  const float l = region_clamp(o[5], fw), t = region_clamp(o[2], fh);
  const float r = region_clamp(fw - o[3], fw), b = region_clamp(fh - o[4], fh);
  v.x0 = (int)ceilf(l - 0.5f); v.x1 = (int)ceilf(r - 0.5f);
  v.y0 = (int)ceilf(t - 0.5f); v.y1 = (int)ceilf(b - 0.5f);
  if (v.x1 < v.x0) v.x1 = v.x0;
  if (v.y1 < v.y0) v.y1 = v.y0;
  v.draws = frame >= 0 && frame < n_frames && v.sx > 0.f && v.sy > 0.f && v.x0 < v.x1 && v.y0 < v.y1;
  return v;
}

}  // namespace acrmi
