// Stand-alone check of the part-segmentation rules (csrc/segm_plan.h) and of the map sampling they share
// with the heat-map views (csrc/map_view_plan.h): the taps on recorded values, the strict arg-max with ties, NaN and infinities,
// the colour table against its stated formula, the footprint of a tile - the segmentation's and the heat maps', whole or clipped
// by a region's window - against the taps of every one of its pixels (views that scale, shift, face away or hold NaN and
// infinities included), and the
// statistics records - a frame's pixels pushed through chunks and folded - against a plain restatement written in this file.
// No GPU, no HIP:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/segm_check.cpp -o segm_check  &&  ./segm_check
//   (or: hipcc -x c++ -Xarch_host -fsanitize=address,undefined ...)
// Exit status 0 and "ok" when every case holds.
#include "../arbitrary-hands-3d-reconstruction_amd/csrc/segm_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

using namespace acrmi;

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);           \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  std::mt19937 rng(23);

  // ---- taps: recorded values ----
  {
    // a 512-pixel row over a 256-cell map without a view: pixel x sits at canvas x + 0.5, source (x + 0.5) / 2 - 0.5
    const float m = 256.f / 512.f;
    Tap t = map_tap(map_canvas(0, false, 1.f, 0.f, 1.f), m, 256);
    EXPECT(t.i0 == 0 && t.i1 == 1 && t.l1 == 0.f && t.l0 == 1.f);      // clamped at the edge
    t = map_tap(map_canvas(1, false, 1.f, 0.f, 1.f), m, 256);
    EXPECT(t.i0 == 0 && t.i1 == 1 && t.l1 == 0.25f && t.l0 == 0.75f);
    t = map_tap(map_canvas(2, false, 1.f, 0.f, 1.f), m, 256);
    EXPECT(t.i0 == 0 && t.i1 == 1 && t.l1 == 0.75f && t.l0 == 0.25f);
    t = map_tap(map_canvas(511, false, 1.f, 0.f, 1.f), m, 256);
    EXPECT(t.i0 == 255 && t.i1 == 255 && t.l1 == 0.25f);      // both taps the last cell
    // a 256-pixel row over a 256-cell map: the pixel is the cell, l1 = 0
    for (int x = 0; x < 256; ++x) {
      t = map_tap(map_canvas(x, false, 1.f, 0.f, 2.f), m, 256);
      EXPECT(t.i0 == x && t.l1 == 0.f && t.l0 == 1.f);
    }
    // a view: scale 3.75, shift -420 (a 1920-wide frame padded to a square)
    t = map_tap(map_canvas(960, true, 3.75f, 0.f, 0.f), m, 256);
    EXPECT(t.i0 == 127 && t.i1 == 128);
    t = map_tap(512.f, m, 256);      // the clamp of the footprint's far end
    EXPECT(t.i0 == 255 && t.i1 == 255);
    t = map_tap(0.f, m, 1);          // a map of one cell
    EXPECT(t.i0 == 0 && t.i1 == 0);
    EXPECT(map_covered(0.f, 511.9f, 1.f, 1.f) && !map_covered(512.f, 0.f, 1.f, 1.f) && !map_covered(-0.001f, 0.f, 1.f, 1.f));
    EXPECT(!map_covered(nan, 0.f, 1.f, 1.f) && !map_covered(0.f, 0.f, 0.f, 1.f) && !map_covered(0.f, 0.f, 1.f, -1.f) &&
           !map_covered(0.f, 0.f, nan, 1.f) && !map_covered(inf, 0.f, 1.f, 1.f));
  }

  // ---- arg-max: strict, the lowest class wins a tie, a NaN never wins ----
  {
    const Tap u = {0, 0, 1.f, 0.f};      // the value is cell a's
    auto label = [&](std::vector<float> v) { return segm_label(v.data(), v.data(), v.data(), v.data(), u, u, (int)v.size()); };
    EXPECT(label({1.f, 2.f, 3.f}) == 2 && label({3.f, 2.f, 1.f}) == 0 && label({1.f, 3.f, 3.f}) == 1 && label({2.f, 2.f, 2.f}) == 0);
    EXPECT(label({nan, 5.f, 6.f}) == 0 && label({1.f, nan, 0.5f}) == 0 && label({1.f, nan, 2.f}) == 2 && label({-inf, -inf, -inf}) == 0);
    EXPECT(label({0.f, 3e38f, 3e38f}) == 1 && label({-3e38f, -1e38f, 3e38f}) == 2 && label({0.f, -0.f, 0.f}) == 0);
    // under a zero weight an infinite cell is 0 * inf = NaN, as the formula says: it never wins, and in class 0 it keeps label 0
    EXPECT(label({0.f, inf, -1.f}) == 0 && label({-inf, 1.f, 2.f}) == 0);
    {
      const Tap h2 = {0, 1, 0.5f, 0.5f};
      const float p[3] = {0.f, inf, inf}, q[3] = {-inf, 1.f, 0.f};
      EXPECT(segm_label(p, p, p, p, h2, h2, 3) == 1 && segm_label(q, q, q, q, h2, h2, 3) == 1);
    }
    // 0 * inf is NaN: an infinite cell under a zero weight poisons the value, as the formula says
    const Tap half = {0, 1, 0.5f, 0.5f};
    const float a[3] = {0.f, inf, 1.f}, b[3] = {0.f, -inf, 2.f};
    EXPECT(segm_label(a, b, a, b, half, half, 3) == 2);      // class 1 = inf - inf = NaN
    // random cells against a restatement that collects the values first
    std::uniform_real_distribution<float> uni(-4.f, 4.f);
    for (int n = 0; n < 4000; ++n) {
      const int C = 3 + 2 * (int)(rng() % 31);
      std::vector<float> cell[4];
      for (auto& c : cell) {
        c.resize(C);
        for (float& v : c) v = (rng() % 9 == 0) ? 1.f : uni(rng);      // (1.0: ties)
      }
      if (n % 5 == 0) cell[rng() % 4][rng() % C] = (n % 10 == 0) ? nan : inf;
      Tap ty, tx;
      ty.l1 = (float)(rng() % 5) / 4.f; ty.l0 = 1.f - ty.l1; tx.l1 = (float)(rng() % 9) / 8.f; tx.l0 = 1.f - tx.l1;
      std::vector<float> v(C);
      for (int c = 0; c < C; ++c) {
        const float top = tx.l0 * cell[0][c] + tx.l1 * cell[1][c], bot = tx.l0 * cell[2][c] + tx.l1 * cell[3][c];
        v[c] = ty.l0 * top + ty.l1 * bot;
      }
      int want = 0;
      for (int c = 1; c < C; ++c)
        if (v[c] > v[want]) want = c;      // (v[want] NaN only for want = 0: nothing beats it)
      EXPECT(segm_label(cell[0].data(), cell[1].data(), cell[2].data(), cell[3].data(), ty, tx, C) == want);
    }
  }

  // ---- classes, sides, colours ----
  {
    EXPECT(segm_classes_ok(3) && segm_classes_ok(33) && segm_classes_ok(63) && !segm_classes_ok(1) && !segm_classes_ok(4) &&
           !segm_classes_ok(32) && !segm_classes_ok(65) && !segm_classes_ok(-3) && !segm_classes_ok(0));
    EXPECT(segm_dim_ok(1) && segm_dim_ok(16384) && !segm_dim_ok(0) && !segm_dim_ok(16385) && !segm_dim_ok(-1));
    EXPECT(segm_side(0, 33) == -1 && segm_side(1, 33) == 1 && segm_side(16, 33) == 1 && segm_side(17, 33) == 0 && segm_side(32, 33) == 0 &&
           segm_side(33, 33) == -1 && segm_side(255, 33) == -1 && segm_side(1, 3) == 1 && segm_side(2, 3) == 0);
    // the jet: byte = floor(255 clamp(1.5 - |4 t - k|, 0, 1) + 0.5), t = i / 255, k = 3, 2, 1
    for (int i = 0; i < 256; ++i)
      for (int c = 0; c < 3; ++c) {
        double v255 = 382.5 - std::abs(4 * i - 255 * (3 - c));      // 255 (1.5 - |4 t - k|), exact in binary
        v255 = v255 < 0 ? 0 : v255 > 255 ? 255 : v255;
        EXPECT(map_jet(i, c) == (int)std::floor(v255 + 0.5));
      }
    uint8_t rgb[63 * 3], bgr[63 * 3];
    segm_default_colors(false, 33, rgb);
    segm_default_colors(true, 33, bgr);
    EXPECT(rgb[0] == 0 && rgb[1] == 0 && rgb[2] == 0);
    for (int l = 1; l < 33; ++l) {
      const int i = l <= 16 ? 128 + 8 * (l - 1) : 127 - 8 * (l - 17);
      EXPECT(i >= 0 && i <= 255 && segm_color_index(l, 33) == i);
      for (int c = 0; c < 3; ++c) EXPECT(rgb[3 * l + c] == map_jet(i, c) && bgr[3 * l + 2 - c] == rgb[3 * l + c]);
      for (int k = 1; k < l; ++k)      // no two parts share a colour
        EXPECT(rgb[3 * l] != rgb[3 * k] || rgb[3 * l + 1] != rgb[3 * k + 1] || rgb[3 * l + 2] != rgb[3 * k + 2]);
    }
    segm_default_colors(false, 63, rgb);      // the largest C: the index is clamped into the table, nothing is written beyond 63 rows
    EXPECT(segm_color_index(31, 63) == 255 && segm_color_index(62, 63) == 0 && segm_color_index(1, 3) == 128 && segm_color_index(2, 3) == 127);
    EXPECT(map_blend(0.7f, 255, 0) == 178 && map_blend(0.7f, 0, 255) == 76 && map_blend(1.f, 200, 13) == 200 && map_blend(0.f, 200, 13) == 13);
  }

  // ---- footprint: it holds the taps of every covered pixel of the tile ----
  {
    struct View { bool has; float sx, sy, ox, oy; };
    const View views[] = {{false, 1, 1, 0, 0},        {true, 1.f, 1.f, 0.f, 0.f},     {true, 3.75f, 3.75f, 0.f, -420.f},
                          {true, 0.25f, 0.5f, 3.f, 7.f}, {true, 1.f, 1.f, 300.f, -300.f}, {true, 1.f, 1.f, 1e9f, 0.f},
                          {true, -1.f, 1.f, 0.f, 0.f},  {true, nan, 1.f, 0.f, 0.f},     {true, 1.f, 1.f, nan, 0.f},
                          {true, 1.f, 1.f, inf, -inf},  {true, 0.f, 0.f, 0.f, 0.f},     {true, 1e-30f, 1e30f, 0.f, 0.f}};
    const int sizes[][4] = {{512, 512, 256, 256}, {97, 203, 256, 256}, {16, 16, 256, 256}, {333, 517, 40, 56}, {1080, 1920, 256, 256}, {64, 128, 8, 8}};
    // the segmentation's tile, and the heat maps' - whole, and its share of a region's window, which ends between tile boundaries
    const int tiles[][2] = {{SEGM_TW, SEGM_TH}, {128, 32}};
    for (const View& v : views)
      for (const auto& sz : sizes)
        for (const auto& tile : tiles)
          for (int windowed = 0; windowed <= (tile[0] == 128); ++windowed) {
            const int H = sz[0], W = sz[1], h = sz[2], w = sz[3], TW = tile[0], TH = tile[1];
            const int wx0 = windowed ? W / 7 + 1 : 0, wx1 = windowed ? W - W / 5 - 1 : W;
            const int wy0 = windowed ? H / 9 + 1 : 0, wy1 = windowed ? H - H / 3 - 1 : H;
            const float kx = 512.f / (float)W, ky = 512.f / (float)H, mx = (float)w / 512.f, my = (float)h / 512.f;
            const MapView mv = {v.has, v.sx, v.sy, v.ox, v.oy};
            for (int T0 = 0; T0 < H; T0 += TH * 5)
              for (int L0 = 0; L0 < W; L0 += TW * 3) {
                const int X0 = std::max(L0, wx0), X1 = std::min({L0 + TW, W, wx1}), Y0 = std::max(T0, wy0), Y1 = std::min({T0 + TH, H, wy1});
                if (X0 >= X1 || Y0 >= Y1) continue;
                const MapFootprint f = map_footprint(X0, X1, Y0, Y1, mv, H, W, h, w);
                if (f.any) EXPECT(f.ix >= 0 && f.iy >= 0 && f.fw >= 1 && f.fh >= 1 && f.ix + f.fw <= w && f.iy + f.fh <= h);
                for (int y = Y0; y < Y1; ++y)
                  for (int x = X0; x < X1; ++x) {
                    const float cx = map_canvas(x, v.has, v.sx, v.ox, kx), cy = map_canvas(y, v.has, v.sy, v.oy, ky);
                    if (!map_covered(cx, cy, v.sx, v.sy)) continue;
                    EXPECT(f.any);
                    const Tap tx = map_tap(cx, mx, w), ty = map_tap(cy, my, h);
                    EXPECT(tx.i0 >= f.ix && tx.i1 < f.ix + f.fw && ty.i0 >= f.iy && ty.i1 < f.iy + f.fh);
                  }
              }
          }
    // the frame's view: the `view` row, else the row of `offsets`, else none
    {
      const float rows[8] = {9, 9, 9, 9, 2.f, 0.5f, 100.f, -7.f}, o[20] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1024, 256, 30, 0, 0, 100, 10, 0, 0, 40};
      MapView m = map_frame_view(rows, o, 1);
      EXPECT(m.has && m.sx == 2.f && m.sy == 0.5f && m.ox == 100.f && m.oy == -7.f);
      m = map_frame_view(nullptr, o, 1);
      EXPECT(m.has && m.sx == 2.f && m.sy == 0.5f && m.ox == 60.f && m.oy == 20.f);
      m = map_frame_view(nullptr, nullptr, 1);
      EXPECT(!m.has && m.sx == 1.f && m.sy == 1.f && m.ox == 0.f && m.oy == 0.f);
    }
    // the network's own case fits the staged capacity, whole cells of 36 floats; a small image over the whole map does not
    const MapView whole = {false, 1.f, 1.f, 0.f, 0.f}, away = {true, 1.f, 1.f, 600.f, 0.f};
    const MapFootprint net = map_footprint(64, 128, 16, 32, whole, 512, 512, 256, 256);
    EXPECT(net.ix == 31 && net.iy == 7 && net.fw == 34 && net.fh == 10 && map_staged(net, 36, SEGM_LDS_FLOATS));
    EXPECT(segm_cell_floats(33, true) == 36 && segm_cell_floats(33, false) == 33 && segm_cell_floats(3, true) == 4 && segm_cell_floats(63, true) == 64);
    const MapFootprint edge = map_footprint(0, 64, 0, 16, whole, 512, 512, 256, 256);
    EXPECT(edge.ix == 0 && edge.fw == 33 && edge.fh == 9);
    const MapFootprint small = map_footprint(0, 16, 0, 16, whole, 16, 16, 256, 256);
    EXPECT(small.any && small.ix == 7 && small.fw == 242 && small.fh == 242 && !map_staged(small, 36, SEGM_LDS_FLOATS) &&
           !map_staged(small, 33, SEGM_LDS_FLOATS));
    const MapFootprint none = map_footprint(0, 64, 0, 16, away, 512, 512, 256, 256);
    EXPECT(!none.any && !map_staged(none, 36, SEGM_LDS_FLOATS));
    // the heat maps' capacity of 48 * 48 cells: a 64 x 64 map over a 16 x 16 image is beyond it, over the first tile of a 158 x 96 image within
    const MapFootprint all = map_footprint(0, 16, 0, 16, whole, 16, 16, 64, 64), part = map_footprint(0, 128, 0, 32, whole, 96, 158, 64, 64);
    EXPECT(all.ix == 1 && all.fw == 62 && all.fh == 62 && !map_staged(all, 1, 48 * 48));
    EXPECT(part.ix == 0 && part.iy == 0 && part.fw == 53 && part.fh == 22 && map_staged(part, 1, 48 * 48));
  }

  // ---- statistics: pixels -> chunk records -> folded record -> outputs, against a plain count ----
  for (int rep = 0; rep < 12; ++rep) {
    const int C = rep % 3 == 0 ? 3 : rep % 3 == 1 ? 5 : 33, H = 1 + (int)(rng() % 70), W = 1 + (int)(rng() % 90), F = 7;
    const bool with_ids = rep % 2 == 0;
    std::vector<uint8_t> lab((size_t)H * W);
    std::vector<int32_t> ids((size_t)H * W);
    for (size_t i = 0; i < lab.size(); ++i) {
      const unsigned r = rng() % 16;
      lab[i] = r < 8 ? 0 : r == 8 ? 255 : r == 9 ? (uint8_t)C : (uint8_t)(rng() % C);      // (C itself: no label, not counted)
      ids[i] = (rng() % 3 == 0) ? -1 : (int32_t)(rng() % (6 * F));
    }
    if (rep == 3) std::fill(lab.begin(), lab.end(), (uint8_t)0);      // no hand at all
    if (rep == 4)
      for (auto& l : lab) l = l >= 1 && l <= (C - 1) / 2 ? 0 : l;      // the right side is empty
    const int chunks = segm_stats_chunks(H);
    EXPECT(segm_stats_ws_ints(2, H, W) == (size_t)2 * chunks * SEGM_STATS_REC);
    std::vector<int32_t> ws((size_t)chunks * SEGM_STATS_REC, 0x5a5a5a5a);      // the caller zeroes nothing
    for (int k = 0; k < chunks; ++k) {
      int32_t* rec = ws.data() + (size_t)k * SEGM_STATS_REC;
      segm_rec_clear(rec);
      for (int y = k * SEGM_STATS_ROWS; y < std::min(H, (k + 1) * SEGM_STATS_ROWS); ++y)
        for (int x = 0; x < W; ++x) segm_rec_pixel(rec, x, y, lab[(size_t)y * W + x], with_ids ? ids[(size_t)y * W + x] : -1, with_ids ? F : 0, C);
    }
    int32_t rec[SEGM_STATS_REC];
    for (int i = 0; i < SEGM_STATS_REC; ++i) {
      rec[i] = ws[i];
      for (int k = 1; k < chunks; ++k) rec[i] = segm_rec_fold(i, rec[i], ws[(size_t)k * SEGM_STATS_REC + i]);
    }
    std::vector<int32_t> counts(C), want_counts(C, 0);
    int32_t boxes[8], agree[6], want_boxes[8] = {0, 0, 0, 0, 0, 0, 0, 0}, want_agree[6] = {0, 0, 0, 0, 0, 0};
    segm_rec_outputs(rec, C, counts.data(), boxes, with_ids ? agree : nullptr);
    for (int s = 0; s < 2; ++s) {
      int l = W, t = H, r = 0, b = 0;
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          const int v = lab[(size_t)y * W + x];
          const bool mine = v >= 1 && v < C && (s == 1) == (v <= (C - 1) / 2);
          if (s == 0 && v < C) ++want_counts[v];
          const int32_t id = ids[(size_t)y * W + x];
          const bool sil = with_ids && id >= 0 && ((id / F) % 2) == s;
          want_agree[3 * s] += mine && sil;
          want_agree[3 * s + 1] += mine;
          want_agree[3 * s + 2] += sil;
          if (mine) { l = std::min(l, x); t = std::min(t, y); r = std::max(r, x + 1); b = std::max(b, y + 1); }
        }
      if (r > 0) { want_boxes[4 * s] = l; want_boxes[4 * s + 1] = t; want_boxes[4 * s + 2] = r; want_boxes[4 * s + 3] = b; }
    }
    EXPECT(counts == want_counts);
    for (int i = 0; i < 8; ++i) EXPECT(boxes[i] == want_boxes[i]);
    if (with_ids)
      for (int i = 0; i < 6; ++i) EXPECT(agree[i] == want_agree[i]);
  }
  EXPECT(segm_stats_ws_ints(0, 16, 16) == 0 && segm_stats_ws_ints(-1, 16, 16) == 0 && segm_stats_ws_ints(1, 0, 16) == 0 &&
         segm_stats_ws_ints(1, 16, 16385) == 0 && segm_stats_ws_ints(65536, 16, 16) == 0 &&
         segm_stats_ws_ints(65535, 16384, 16384) == (size_t)65535 * 1024 * SEGM_STATS_REC);

  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
