// Key-point skeleton and centre heat-map views over the frames (DESIGN.md "Key-point and heat-map views").  The reference
// draws them on the host with PIL and cv2 (acr/visualization.py:228-300); nothing of those is used here, only the
// conventions: the joint order and tree, the colours, the painter's order, bilinear maps in false colour at weight 0.7.
//
//   skeleton_kernel   one 256-thread block per (128 x 32 pixel tile, frame).  The hands of the frame are found in hand
//                     order (ballot + mbcnt compaction of the hand -> frame index), two at a time their 21 key points are
//                     snapped and turned into 61 primitive records each in LDS (bone / disc, clipped pixel box, the int64
//                     constants of the bone test), and every thread walks the records that meet the tile for its 4 x 4
//                     pixels.  The rule is integer throughout; the last primitive that covers a pixel wins.
//   heatmap_kernel    the same tiling; the part of the left and right maps a tile samples (and the 256 x 3 colour table)
//                     is staged in LDS - 16-bit maps of a 16-bit storage program are converted to fp32 there - and every
//                     thread samples, colours and blends its pixels in fp32, each operation rounded on its own.  One read
//                     of the image, two writes.
//   region_heatmap_kernel  the same tiling, for regions of interest (DESIGN.md "Views over regions"): the regions of the
//                     frame whose window meets the tile are found in region order (the skeleton's compaction), one after the
//                     other the part of their two maps the tile's share of the window samples is staged, and every thread
//                     keeps the LARGEST colour index of each of its pixels per side in registers; after the last region
//                     the image is read once, blended once and written to both outputs.
// The two heat-map kernels take the frame's view, coverage, taps, value, the footprint of a tile and the blend from
// csrc/map_view_plan.h, where the rule is stated once (csrc/segm.hip draws by it too).
// Pixels move as 4 pixels = 3 dwords per thread and row when the row length is a multiple of 4 and the buffers are dword
// aligned, byte by byte otherwise.  A thread reads and writes only its own pixels, so drawing in place is safe; there are
// no atomics on global memory, so the result is deterministic.
#include "kernels.h"
#include "px_rows.h"          // load_px, store_px, get_byte, set_byte, dword_rows
#include "map_view_plan.h"    // the map-sampling rule of the heat maps
#include "region_view_plan.h"

#include <hip/hip_fp16.h>

#include <climits>
#include <cstring>

namespace acrmi {

namespace {

constexpr int TW = 128, TH = 32;      // block tile: 32 threads x 4 pixels wide, 8 threads x 4 rows high
constexpr int PX = 4, ROWS = 4, ROW_STEP = 8;
constexpr int HAND_PRIMS = 61;        // 20 x (bone, disc, parent's disc) + the wrist's disc
constexpr int PAIR = 2;               // hands whose records are resident in LDS at a time
constexpr float COORD_LIMIT = 16384.f;
constexpr long long CROSS_LIMIT = 1ll << 18;
constexpr int MAP_CAP = 48 * 48;      // map cells per side staged in LDS; a larger footprint is read from memory

struct Prim {
  int x0, x1, y0, y1;      // inclusive pixel box, clipped to the image; empty (x0 > x1) when the primitive is dropped
  int ax, ay, dx, dy;      // bone: start and direction; disc: the centre in (ax, ay)
  long long L2, lim;       // bone: |d|^2 and w^2 |d|^2; disc: L2 = -1 and lim = r^2 + r
  int color, pad;
};

__device__ inline int lane_rank(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
}

// the skeleton of mano/skeleton.txt (first 21 rows): five fingers of four joints, tip to base, then the wrist
__device__ inline int skeleton_parent(int i) { return i == 20 ? -1 : ((i & 3) == 3 ? 20 : i + 1); }
// mano2interhand_mapper (acr/visualization.py:25): skeleton joint i is MANO joint ...
__device__ inline int skeleton_mano_joint(int i) { return i == 20 ? 0 : (i & ~3) + 4 - (i & 3); }

__device__ inline bool prim_covers(const Prim& r, int x, int y) {
  const int ux = x - r.ax, uy = y - r.ay;
  if (r.L2 < 0) return (long long)(ux * ux + uy * uy) <= r.lim;      // (|u| <= r inside the box)
  const long long dot = (long long)ux * r.dx + (long long)uy * r.dy;
  if (dot < 0 || dot > r.L2) return false;
  long long cr = (long long)ux * r.dy - (long long)uy * r.dx;
  cr = cr < 0 ? -cr : cr;
  if (cr >= CROSS_LIMIT) return false;
  return 4 * cr * cr <= r.lim;
}

}  // namespace

// ---- skeleton ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void skeleton_kernel(SkeletonArgs a) {
  __shared__ Prim s_prim[PAIR * HAND_PRIMS];
  __shared__ int s_k[PAIR][21][2];
  __shared__ int s_far[PAIR][21];
  __shared__ int s_bad[PAIR];
  __shared__ int s_box[4];
  __shared__ int s_list[256];
  __shared__ int s_cnt[4];
  __shared__ uint32_t s_col[64];
  const int tid = threadIdx.x, f = blockIdx.z;
  const int X0 = blockIdx.x * TW, Y0 = blockIdx.y * TH;
  const int xt = X0 + PX * (tid & 31), yt = Y0 + (tid >> 5);
  if (tid < 63) s_col[tid] = a.colors[tid];
  int cid[ROWS][PX];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int j = 0; j < PX; ++j) cid[r][j] = -1;

  // the hands of this frame, in hand order: with `slots` they are 2 f and 2 f + 1, else the index is searched
  const int hb = a.slots ? 2 * f : 0, he = a.slots ? min(2 * f + 2, a.n_hands) : a.n_hands;
  for (int base = hb; base < he; base += 256) {
    const int h = base + tid;
    bool mine = false;
    if (h < he) mine = a.slots ? a.slots[(size_t)h * a.slot_stride + a.flag_at] > 0.5f : a.hand_frame[h] == f;
    const unsigned long long mask = __ballot(mine);
    const int wave = tid >> 6;
    if ((tid & 63) == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = s_cnt[w];
      off += w < wave ? c : 0;
      total += c;
    }
    if (mine) s_list[off + lane_rank(mask)] = h;
    __syncthreads();
    for (int j0 = 0; j0 < total; j0 += PAIR) {
      const int nh = min(PAIR, total - j0);
      if (tid < 4) s_box[tid] = (tid & 1) ? INT_MIN : INT_MAX;      // x0, x1, y0, y1 of everything these hands draw
      if (tid < PAIR) s_bad[tid] = 0;
      __syncthreads();
      if (tid < nh * 21) {      // snap: truncation toward zero
        const int q = tid / 21, i = tid - q * 21;
        const float* kp = a.kps + ((size_t)s_list[j0 + q] * 21 + skeleton_mano_joint(i)) * 2;
        float fx = kp[0], fy = kp[1];
        if (a.normalized) {      // (pj2d + 1) / 2 * 512, acr/visualization.py:241
          fx = ((fx + 1.f) / 2.f) * 512.f;
          fy = ((fy + 1.f) / 2.f) * 512.f;
        }
        if (!(fabsf(fx) < INFINITY && fabsf(fy) < INFINITY)) atomicOr(&s_bad[q], 1);      // NaN / inf: the hand is not drawn
        const bool far = !(fabsf(fx) < COORD_LIMIT && fabsf(fy) < COORD_LIMIT);
        s_k[q][i][0] = far ? 0 : (int)fx;
        s_k[q][i][1] = far ? 0 : (int)fy;
        s_far[q][i] = far;
      }
      __syncthreads();
      if (tid < nh * HAND_PRIMS) {      // records in painter's order: per joint bone(i, p), disc(i), disc(p)
        const int q = tid / HAND_PRIMS, p = tid - q * HAND_PRIMS;
        const int i = p == 60 ? 20 : p / 3, kind = p == 60 ? 1 : p - 3 * (p / 3);
        const int par = skeleton_parent(i);
        Prim r{};
        bool ok = !s_bad[q];
        int m = 0;
        if (kind == 0) {
          ok = ok && !s_far[q][i] && !s_far[q][par];
          const int bx = s_k[q][par][0], by = s_k[q][par][1];
          r.ax = s_k[q][i][0]; r.ay = s_k[q][i][1];
          r.dx = bx - r.ax; r.dy = by - r.ay;
          r.L2 = (long long)r.dx * r.dx + (long long)r.dy * r.dy;
          r.lim = (long long)(a.line_width * a.line_width) * r.L2;
          ok = ok && r.L2 > 0;
          r.color = par;
          m = a.line_width;      // a covered pixel is within w / 2 of the segment
          r.x0 = min(r.ax, bx) - m; r.x1 = max(r.ax, bx) + m;
          r.y0 = min(r.ay, by) - m; r.y1 = max(r.ay, by) + m;
        } else {
          const int j = kind == 1 ? i : par;
          ok = ok && !s_far[q][j];
          r.ax = s_k[q][j][0]; r.ay = s_k[q][j][1];
          r.L2 = -1;
          r.lim = (long long)a.circle_rad * a.circle_rad + a.circle_rad;
          r.color = j;
          m = a.circle_rad;      // r^2 + r < (r + 1)^2
          r.x0 = r.ax - m; r.x1 = r.ax + m; r.y0 = r.ay - m; r.y1 = r.ay + m;
        }
        r.x0 = max(r.x0, 0); r.x1 = min(r.x1, a.W - 1);
        r.y0 = max(r.y0, 0); r.y1 = min(r.y1, a.H - 1);
        ok = ok && r.x0 <= r.x1 && r.y0 <= r.y1;
        if (!ok) { r.x0 = 1; r.x1 = 0; r.y0 = 1; r.y1 = 0; }
        s_prim[tid] = r;
        if (ok) {
          atomicMin(&s_box[0], r.x0); atomicMax(&s_box[1], r.x1);
          atomicMin(&s_box[2], r.y0); atomicMax(&s_box[3], r.y1);
        }
      }
      __syncthreads();
      if (s_box[0] < X0 + TW && s_box[1] >= X0 && s_box[2] < Y0 + TH && s_box[3] >= Y0) {      // (the same for every thread)
        for (int p = 0; p < nh * HAND_PRIMS; ++p) {
          const Prim& r = s_prim[p];
          if (r.x1 < X0 || r.x0 >= X0 + TW || r.y1 < Y0 || r.y0 >= Y0 + TH) continue;
          if (r.x1 < xt || r.x0 > xt + PX - 1) continue;
#pragma unroll
          for (int rr = 0; rr < ROWS; ++rr) {
            const int y = yt + ROW_STEP * rr;
            if (y < r.y0 || y > r.y1) continue;
#pragma unroll
            for (int j = 0; j < PX; ++j) {
              const int x = xt + j;
              if (x >= r.x0 && x <= r.x1 && prim_covers(r, x, y)) cid[rr][j] = r.color;
            }
          }
        }
      }
      __syncthreads();      // the records are rewritten by the next pair
    }
  }

  if (xt >= a.W) return;
  const bool in_place = a.img_in == a.img_out;
  const int n = min(PX, a.W - xt);
#pragma unroll
  for (int rr = 0; rr < ROWS; ++rr) {
    const int y = yt + ROW_STEP * rr;
    if (y >= a.H) continue;
    const bool any = cid[rr][0] >= 0 || cid[rr][1] >= 0 || cid[rr][2] >= 0 || cid[rr][3] >= 0;
    if (in_place && !any) continue;      // nothing to move
    const size_t at = (((size_t)f * a.H + y) * a.W + xt) * 3;
    uint32_t d[3];
    load_px(a.img_in + at, a.wide, n, d);
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      if (cid[rr][j] < 0) continue;
#pragma unroll
      for (int c = 0; c < 3; ++c) set_byte(d, 3 * j + c, s_col[cid[rr][j] * 3 + c]);
    }
    store_px(a.img_out + at, a.wide, n, d);
  }
}

// ---- heat maps --------------------------------------------------------------------------------------------------------
namespace {

__device__ inline float map_load(const void* p, int dtype, size_t at) {
  if (dtype == 0) return static_cast<const float*>(p)[at];
  const uint16_t bits = static_cast<const uint16_t*>(p)[at];
  if (dtype == 1) return __half2float(__ushort_as_half(bits));
  return __uint_as_float((uint32_t)bits << 16);      // bf16
}

// the cells of footprint fp (which fits MAP_CAP) of the `views` maps that start at element fb -> s_map, as fp32
__device__ inline void stage_maps(float (*s_map)[MAP_CAP], const HeatmapBase& a, int views, size_t fb, const MapFootprint& fp, int tid) {
  for (int v = 0; v < views; ++v)
    for (int t = tid; t < fp.fw * fp.fh; t += 256) {
      const int r = t / fp.fw, c = t - r * fp.fw;
      s_map[v][t] = map_load(a.maps[v], a.dtype, fb + ((size_t)(fp.iy + r) * a.w + fp.ix + c) * a.pix_stride);
    }
}

// the colour index of a covered pixel from its taps: the four cells from s_map (one map's staged footprint) or, not staged,
// from `map` at element fb; bilinear value * 255 truncated, as .byte() does; NaN -> 0
__device__ inline int color_index(const float* s_map, bool staged, const MapFootprint& fp, const void* map, const HeatmapBase& a,
                                  size_t fb, const Tap& ty, const Tap& tx) {
  float p00, p01, p10, p11;
  if (staged) {
    const int r0 = (ty.i0 - fp.iy) * fp.fw - fp.ix, r1 = (ty.i1 - fp.iy) * fp.fw - fp.ix;
    p00 = s_map[r0 + tx.i0]; p01 = s_map[r0 + tx.i1]; p10 = s_map[r1 + tx.i0]; p11 = s_map[r1 + tx.i1];
  } else {
    const size_t r0 = (size_t)ty.i0 * a.w, r1 = (size_t)ty.i1 * a.w;
    p00 = map_load(map, a.dtype, fb + (r0 + tx.i0) * a.pix_stride);
    p01 = map_load(map, a.dtype, fb + (r0 + tx.i1) * a.pix_stride);
    p10 = map_load(map, a.dtype, fb + (r1 + tx.i0) * a.pix_stride);
    p11 = map_load(map, a.dtype, fb + (r1 + tx.i1) * a.pix_stride);
  }
  return (int)fminf(fmaxf(map_value(ty, tx, p00, p01, p10, p11) * 255.f, 0.f), 255.f);
}

}  // namespace

__global__ __launch_bounds__(256) void heatmap_kernel(HeatmapArgs a) {
  __shared__ float s_map[2][MAP_CAP];
  __shared__ uint32_t s_lut[768];
  const int tid = threadIdx.x, f = blockIdx.z;
  const int X0 = blockIdx.x * TW, Y0 = blockIdx.y * TH;
  const int xt = X0 + PX * (tid & 31), yt = Y0 + (tid >> 5);
  const int views = a.maps[1] ? 2 : 1;
  for (int t = tid; t < 768; t += 256) s_lut[t] = a.lut[t];

  const MapView vw = map_frame_view(a.view, a.offsets, f);      // the `view` row, else region_view_row(the `offsets` row), else none
  const float kx = 512.f / (float)a.W, ky = 512.f / (float)a.H;
  const float mx = (float)a.w / 512.f, my = (float)a.h / 512.f;
  // what this tile samples (the same for every thread), staged when it fits
  const MapFootprint fp = map_footprint(X0, min(X0 + TW, a.W), Y0, min(Y0 + TH, a.H), vw, a.H, a.W, a.h, a.w);
  const bool staged = map_staged(fp, 1, MAP_CAP);
  const size_t fb = (size_t)f * a.frame_stride;
  if (staged) stage_maps(s_map, a, views, fb, fp, tid);
  __syncthreads();
  if (xt >= a.W) return;
  const int n = min(PX, a.W - xt);
#pragma unroll
  for (int rr = 0; rr < ROWS; ++rr) {
    const int y = yt + ROW_STEP * rr;
    if (y >= a.H) continue;
    const size_t at = (((size_t)f * a.H + y) * a.W + xt) * 3;
    uint32_t d[3], o[2][3];
    load_px(a.img_in + at, a.wide, n, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[0][k] = o[1][k] = d[k];
    const float cy = map_canvas(y, vw.has, vw.sy, vw.oy, ky);
    if (fp.any && cy >= 0.f && cy < 512.f) {
      const Tap ty = map_tap(cy, my, a.h);
#pragma unroll
      for (int j = 0; j < PX; ++j) {
        const float cx = map_canvas(xt + j, vw.has, vw.sx, vw.ox, kx);
        if (!map_covered(cx, cy, vw.sx, vw.sy)) continue;
        const Tap tx = map_tap(cx, mx, a.w);
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          if (v >= views) continue;
          const int idx = color_index(s_map[v], staged, fp, a.maps[v], a, fb, ty, tx);
#pragma unroll
          for (int c = 0; c < 3; ++c)
            set_byte(o[v], 3 * j + c, map_blend(a.weight, (int)s_lut[idx * 3 + c], (int)get_byte(d, 3 * j + c)));
        }
      }
    }
    store_px(a.out[0] + at, a.wide, n, o[0]);
    if (views == 2) store_px(a.out[1] + at, a.wide, n, o[1]);
  }
}

// ---- heat maps of regions -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void region_heatmap_kernel(RegionHeatmapArgs a) {
  __shared__ float s_map[2][MAP_CAP];
  __shared__ uint32_t s_lut[768];
  __shared__ int s_list[256];
  __shared__ int s_cnt[4];
  const int tid = threadIdx.x, f = blockIdx.z;
  const int X0 = blockIdx.x * TW, Y0 = blockIdx.y * TH;
  const int X1 = min(X0 + TW, a.W), Y1 = min(Y0 + TH, a.H);      // exclusive
  const int xt = X0 + PX * (tid & 31), yt = Y0 + (tid >> 5);
  const int views = a.maps[1] ? 2 : 1;
  for (int t = tid; t < 768; t += 256) s_lut[t] = a.lut[t];
  const float mx = (float)a.w / 512.f, my = (float)a.h / 512.f;
  int best[2][ROWS][PX];      // the largest colour index of a covering region, -1: no region covers the pixel
#pragma unroll
  for (int v = 0; v < 2; ++v)
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
      for (int j = 0; j < PX; ++j) best[v][r][j] = -1;

  for (int base = 0; base < a.n; base += 256) {
    // the regions of this frame that draw and whose window meets the tile, in region order
    const int reg = base + tid;
    bool mine = false;
    if (reg < a.n && a.region_frame[reg] == f) {
      const RegionView rv = region_view(a.offsets + (size_t)reg * 10, f, a.n_frames, a.H, a.W);
      mine = rv.draws && rv.x0 < X1 && rv.x1 > X0 && rv.y0 < Y1 && rv.y1 > Y0;
    }
    const unsigned long long mask = __ballot(mine);
    const int wave = tid >> 6;
    if ((tid & 63) == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    int off = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = s_cnt[w];
      off += w < wave ? c : 0;
      total += c;
    }
    if (mine) s_list[off + lane_rank(mask)] = reg;
    __syncthreads();
    for (int k = 0; k < total; ++k) {      // (everything up to the per-pixel part is the same for every thread)
      const int i = __builtin_amdgcn_readfirstlane(s_list[k]);
      const RegionView rv = region_view(a.offsets + (size_t)i * 10, f, a.n_frames, a.H, a.W);
      const MapView vw = {true, rv.sx, rv.sy, rv.ox, rv.oy};
      // the tile's share of the window: not empty, and inside the frame (region_view_plan.h); what it samples, staged when it fits
      const int wx0 = max(X0, rv.x0), wx1 = min(X1, rv.x1), wy0 = max(Y0, rv.y0), wy1 = min(Y1, rv.y1);
      const MapFootprint fp = map_footprint(wx0, wx1, wy0, wy1, vw, a.H, a.W, a.h, a.w);
      const bool staged = map_staged(fp, 1, MAP_CAP);
      const size_t fb = (size_t)i * a.frame_stride;
      if (staged) stage_maps(s_map, a, views, fb, fp, tid);
      __syncthreads();
      if (fp.any) {
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) {
          const int y = yt + ROW_STEP * rr;
          if (y < wy0 || y >= wy1) continue;
          const float cy = map_canvas(y, true, vw.sy, vw.oy, 0.f);
          if (!(cy >= 0.f && cy < 512.f)) continue;
          const Tap ty = map_tap(cy, my, a.h);
#pragma unroll
          for (int j = 0; j < PX; ++j) {
            const int x = xt + j;
            if (x < wx0 || x >= wx1) continue;
            const float cx = map_canvas(x, true, vw.sx, vw.ox, 0.f);
            if (!map_covered(cx, cy, vw.sx, vw.sy)) continue;
            const Tap tx = map_tap(cx, mx, a.w);
#pragma unroll
            for (int v = 0; v < 2; ++v) {
              if (v >= views) continue;
              best[v][rr][j] = max(best[v][rr][j], color_index(s_map[v], staged, fp, a.maps[v], a, fb, ty, tx));
            }
          }
        }
      }
      __syncthreads();      // s_map (and, after the last region, s_list) is rewritten
    }
  }

  if (xt >= a.W) return;
  const int n = min(PX, a.W - xt);
#pragma unroll
  for (int rr = 0; rr < ROWS; ++rr) {
    const int y = yt + ROW_STEP * rr;
    if (y >= a.H) continue;
    const size_t at = (((size_t)f * a.H + y) * a.W + xt) * 3;
    uint32_t d[3], o[2][3];
    load_px(a.img_in + at, a.wide, n, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[0][k] = o[1][k] = d[k];
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int j = 0; j < PX; ++j) {
        const int idx = best[v][rr][j];
        if (idx < 0) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c)
          set_byte(o[v], 3 * j + c, map_blend(a.weight, (int)s_lut[idx * 3 + c], (int)get_byte(d, 3 * j + c)));
      }
    store_px(a.out[0] + at, a.wide, n, o[0]);
    if (views == 2) store_px(a.out[1] + at, a.wide, n, o[1]);
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------
// get_keypoint_rgb (acr/visualization.py:331-381) over mano/skeleton.txt, in skeleton order, RGB: finger tips and the wrist
// fall through to the last branch
const uint8_t kSkeletonRGB[21][3] = {
    {230, 230, 0}, {255, 51, 51},  {255, 102, 102}, {255, 153, 153}, {230, 230, 0}, {51, 255, 51},   {102, 255, 102},
    {153, 255, 153}, {230, 230, 0}, {255, 153, 51}, {255, 178, 102}, {255, 204, 153}, {230, 230, 0}, {51, 153, 255},
    {102, 178, 255}, {153, 204, 255}, {230, 230, 0}, {255, 51, 255}, {255, 102, 255}, {255, 153, 255}, {230, 230, 0}};

void skeleton_default_colors(bool bgr, uint8_t* out63) {
  for (int i = 0; i < 21; ++i)
    for (int c = 0; c < 3; ++c) out63[i * 3 + c] = kSkeletonRGB[i][bgr ? 2 - c : c];
}

// the piece-wise linear "jet" of csrc/map_view_plan.h
void heatmap_default_lut(bool bgr, uint8_t* out768) {
  for (int i = 0; i < 256; ++i)
    for (int c = 0; c < 3; ++c) out768[i * 3 + (bgr ? 2 - c : c)] = (uint8_t)map_jet(i, c);
}

hipError_t launch_skeleton(const SkeletonArgs& a0, hipStream_t s) {
  SkeletonArgs a = a0;
  a.wide = dword_rows(a.img_in, a.W) && dword_rows(a.img_out, a.W);
  hipLaunchKernelGGL(skeleton_kernel, dim3((a.W + TW - 1) / TW, (a.H + TH - 1) / TH, a.n_frames), dim3(256), 0, s, a);
  return hipGetLastError();
}

static int heatmap_wide(const HeatmapBase& a) {
  return dword_rows(a.img_in, a.W) && dword_rows(a.out[0], a.W) && (!a.maps[1] || dword_rows(a.out[1], a.W));
}

hipError_t launch_heatmap(const HeatmapArgs& a0, hipStream_t s) {
  HeatmapArgs a = a0;
  a.wide = heatmap_wide(a);
  hipLaunchKernelGGL(heatmap_kernel, dim3((a.W + TW - 1) / TW, (a.H + TH - 1) / TH, a.n), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_region_heatmap(const RegionHeatmapArgs& a0, hipStream_t s) {
  RegionHeatmapArgs a = a0;
  a.wide = heatmap_wide(a);
  hipLaunchKernelGGL(region_heatmap_kernel, dim3((a.W + TW - 1) / TW, (a.H + TH - 1) / TH, a.n_frames), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace acrmi
