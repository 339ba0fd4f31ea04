// The hand-part segmentation as an output: label maps at the frames' resolution, the 'segm' view, and
// the statistics of the masks.  The rule is csrc/segm_plan.h, on the map sampling of csrc/map_view_plan.h that the heat-map
// views share, each stated once for the host and the device.
//
//   segm_kernel        one 256-thread block per (SEGM_TW x SEGM_TH pixel tile, frame), every thread 4 pixels of one row.  The
//                      cells of the logits the tile samples are staged in LDS - whole cells in 16-byte pieces when the
//                      buffer allows it (a cell of the network's buffer is 36 floats = 144 bytes) - and every thread
//                      interpolates the C classes of its pixels from four cells, keeps the strict arg-max, and writes the
//                      label, the drawn view, or both.  A footprint beyond the staged capacity (an image much smaller than
//                      the map) is read from memory tap by tap.  One read of the logits, one of the image.
//   segm_stats_kernel  one block per (SEGM_STATS_ROWS rows, frame): histogram of the labels, box of each side's pixels,
//                      agreement with the rasteriser's ids, in LDS; one record per block in the workspace.
//   segm_reduce_kernel one block per frame: a thread per record word folds the frame's chunks in order and is the only
//                      writer of its outputs.
// Pixels move as in csrc/overlay.hip (csrc/px_rows.h); a thread reads and writes only its own pixels, so drawing in place is
// safe.  No atomics on global memory: the results are the same words on every run, and a frame's do not depend on its batch.
#include "kernels.h"
#include "px_rows.h"
#include "segm_plan.h"

#include <climits>

namespace acrmi {

namespace {

constexpr int PX = 4;
constexpr int TXN = SEGM_TW / PX;      // threads along a row of the tile
static_assert(TXN * SEGM_TH == 256, "one thread per 4 pixels of the tile");

// the strict arg-max over the classes of one pixel from its four cells; VEC: the cells are cell_floats = round-up-4(C) floats
// apart and 16-byte aligned, and the last piece's lanes beyond C are not looked at
template <bool VEC>
__device__ inline int label_of(const float* pa, const float* pb, const float* pc, const float* pd, const Tap& ty, const Tap& tx, int C) {
  if (!VEC) return segm_label(pa, pb, pc, pd, ty, tx, C);
  float best = 0.f;
  int label = 0;
  for (int k = 0; k < C; k += 4) {
    const float4 a = *reinterpret_cast<const float4*>(pa + k), b = *reinterpret_cast<const float4*>(pb + k);
    const float4 c = *reinterpret_cast<const float4*>(pc + k), d = *reinterpret_cast<const float4*>(pd + k);
    const float v0 = map_value(ty, tx, a.x, b.x, c.x, d.x);
    if (k == 0) best = v0;
    else segm_take(v0, k, best, label);
    if (k + 1 < C) segm_take(map_value(ty, tx, a.y, b.y, c.y, d.y), k + 1, best, label);
    if (k + 2 < C) segm_take(map_value(ty, tx, a.z, b.z, c.z, d.z), k + 2, best, label);
    if (k + 3 < C) segm_take(map_value(ty, tx, a.w, b.w, c.w, d.w), k + 3, best, label);
  }
  return label;
}

}  // namespace

__global__ __launch_bounds__(256) void segm_kernel(SegmArgs a) {
  __shared__ float4 s_cells4[SEGM_LDS_FLOATS / 4];
  __shared__ uint32_t s_col[192];
  float* s_cells = reinterpret_cast<float*>(s_cells4);
  const int tid = threadIdx.x, f = blockIdx.z;
  const int X0 = blockIdx.x * SEGM_TW, Y0 = blockIdx.y * SEGM_TH;
  const int xt = X0 + PX * (tid % TXN), y = Y0 + tid / TXN;
  if (tid < 3 * a.C) s_col[tid] = a.colors[tid];

  const MapView v = map_frame_view(a.view, a.offsets, f);
  const float kx = 512.f / (float)a.W, ky = 512.f / (float)a.H;
  const float mx = (float)a.w / 512.f, my = (float)a.h / 512.f;

  // what this tile samples (the same for every thread), staged when it fits
  const MapFootprint fp = map_footprint(X0, min(X0 + SEGM_TW, a.W), Y0, min(Y0 + SEGM_TH, a.H), v, a.H, a.W, a.h, a.w);
  const bool vec = a.vec != 0;
  const int cell = segm_cell_floats(a.C, vec);
  const bool staged = map_staged(fp, cell, SEGM_LDS_FLOATS);
  const float* frame = a.logits + (size_t)f * a.frame_stride;
  if (staged) {
    if (vec) {
      const int q = cell / 4, total = fp.fw * fp.fh * q;
      for (int t = tid; t < total; t += 256) {
        const int at = t / q, k = t - at * q, r = at / fp.fw, c = at - r * fp.fw;
        s_cells4[t] = *reinterpret_cast<const float4*>(frame + ((size_t)(fp.iy + r) * a.w + fp.ix + c) * a.pix_stride + 4 * k);
      }
    } else {
      const int total = fp.fw * fp.fh * cell;
      for (int t = tid; t < total; t += 256) {
        const int at = t / cell, k = t - at * cell, r = at / fp.fw, c = at - r * fp.fw;
        s_cells[t] = frame[((size_t)(fp.iy + r) * a.w + fp.ix + c) * a.pix_stride + k];
      }
    }
  }
  __syncthreads();
  if (xt >= a.W || y >= a.H) return;
  const int n = min(PX, a.W - xt);

  int lab[PX];
#pragma unroll
  for (int j = 0; j < PX; ++j) lab[j] = SEGM_NONE;
  const float cy = map_canvas(y, v.has, v.sy, v.oy, ky);
  if (fp.any && cy >= 0.f && cy < 512.f) {
    const Tap ty = map_tap(cy, my, a.h);
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      if (j >= n) continue;
      const float cx = map_canvas(xt + j, v.has, v.sx, v.ox, kx);
      if (!map_covered(cx, cy, v.sx, v.sy)) continue;
      const Tap tx = map_tap(cx, mx, a.w);
      if (staged) {
        const int r0 = (ty.i0 - fp.iy) * fp.fw - fp.ix, r1 = (ty.i1 - fp.iy) * fp.fw - fp.ix;
        const float *pa = s_cells + (r0 + tx.i0) * cell, *pb = s_cells + (r0 + tx.i1) * cell;
        const float *pc = s_cells + (r1 + tx.i0) * cell, *pd = s_cells + (r1 + tx.i1) * cell;
        lab[j] = vec ? label_of<true>(pa, pb, pc, pd, ty, tx, a.C) : label_of<false>(pa, pb, pc, pd, ty, tx, a.C);
      } else {
        const float* r0 = frame + (size_t)ty.i0 * a.w * a.pix_stride;
        const float* r1 = frame + (size_t)ty.i1 * a.w * a.pix_stride;
        lab[j] = label_of<false>(r0 + (size_t)tx.i0 * a.pix_stride, r0 + (size_t)tx.i1 * a.pix_stride,
                                 r1 + (size_t)tx.i0 * a.pix_stride, r1 + (size_t)tx.i1 * a.pix_stride, ty, tx, a.C);
      }
    }
  }

  const size_t px = ((size_t)f * a.H + y) * a.W + xt;
  if (a.labels) {
    if (a.wide_labels) {
      *reinterpret_cast<uint32_t*>(a.labels + px) = (uint32_t)lab[0] | (uint32_t)lab[1] << 8 | (uint32_t)lab[2] << 16 | (uint32_t)lab[3] << 24;
    } else {
#pragma unroll
      for (int j = 0; j < PX; ++j)
        if (j < n) a.labels[px + j] = (uint8_t)lab[j];
    }
  }
  if (a.out) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < PX; ++j) any = any || (lab[j] >= 1 && lab[j] < a.C);
    if (a.out == a.img_in && !any) return;      // nothing to move
    uint32_t d[3];
    load_px(a.img_in + 3 * px, a.wide, n, d);
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      if (!(lab[j] >= 1 && lab[j] < a.C)) continue;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        set_byte(d, 3 * j + c, map_blend(a.weight, (int)s_col[3 * lab[j] + c], (int)get_byte(d, 3 * j + c)));
    }
    store_px(a.out + 3 * px, a.wide, n, d);
  }
}

// ---- statistics ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void segm_stats_kernel(SegmStatsArgs a, int wide) {
  __shared__ int s_rec[SEGM_STATS_REC];
  const int tid = threadIdx.x, chunk = blockIdx.x, f = blockIdx.y;
  if (tid < SEGM_STATS_REC) s_rec[tid] = (tid >= SEGM_REC_BOX && tid < SEGM_REC_AGREE) ? (((tid - SEGM_REC_BOX) & 2) ? -1 : INT_MAX) : 0;
  __syncthreads();
  const int y0 = chunk * SEGM_STATS_ROWS, rows = min(SEGM_STATS_ROWS, a.H - y0);
  const size_t base = ((size_t)f * a.H + y0) * a.W;
  const int total = rows * a.W;      // (at most 16 x 16384)
  const int half = (a.C - 1) / 2;
  // what the thread keeps in registers: background pixels, the box of each side, the agreement counts
  int zeros = 0, bx0[2] = {INT_MAX, INT_MAX}, by0[2] = {INT_MAX, INT_MAX}, bx1[2] = {-1, -1}, by1[2] = {-1, -1};
  int inter[2] = {0, 0}, sil[2] = {0, 0};
  auto pixel = [&](int i, int label, int id) {
    int s = -1;
    if (label == 0) {
      ++zeros;
    } else if (label < a.C) {
      atomicAdd(&s_rec[label], 1);      // (LDS)
      s = label <= half ? 1 : 0;
      const int yy = i / a.W, xx = i - yy * a.W;
#pragma unroll
      for (int k = 0; k < 2; ++k)
        if (s == k) {
          bx0[k] = min(bx0[k], xx); bx1[k] = max(bx1[k], xx);
          by0[k] = min(by0[k], y0 + yy); by1[k] = max(by1[k], y0 + yy);
        }
    }
    if (id >= 0) {
      const int q = (id / a.n_faces) & 1;
#pragma unroll
      for (int k = 0; k < 2; ++k)
        if (q == k) { ++sil[k]; inter[k] += s == k; }
    }
  };
  if (wide) {      // 4 labels = one dword; W % 4 == 0, so the four are of one row
    for (int i = 4 * tid; i < total; i += 4 * 256) {
      const uint32_t l4 = *reinterpret_cast<const uint32_t*>(a.labels + base + i);
      int4 id4 = make_int4(-1, -1, -1, -1);
      if (a.ids) id4 = *reinterpret_cast<const int4*>(a.ids + base + i);
      pixel(i, l4 & 255, id4.x); pixel(i + 1, (l4 >> 8) & 255, id4.y);
      pixel(i + 2, (l4 >> 16) & 255, id4.z); pixel(i + 3, l4 >> 24, id4.w);
    }
  } else {
    for (int i = tid; i < total; i += 256) pixel(i, a.labels[base + i], a.ids ? a.ids[base + i] : -1);
  }
  if (zeros) atomicAdd(&s_rec[0], zeros);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (bx1[k] >= 0) {
      atomicMin(&s_rec[SEGM_REC_BOX + 4 * k], bx0[k]); atomicMin(&s_rec[SEGM_REC_BOX + 4 * k + 1], by0[k]);
      atomicMax(&s_rec[SEGM_REC_BOX + 4 * k + 2], bx1[k]); atomicMax(&s_rec[SEGM_REC_BOX + 4 * k + 3], by1[k]);
    }
    if (sil[k]) { atomicAdd(&s_rec[SEGM_REC_AGREE + 2 * k], inter[k]); atomicAdd(&s_rec[SEGM_REC_AGREE + 2 * k + 1], sil[k]); }
  }
  __syncthreads();
  if (tid < SEGM_STATS_REC) a.ws[((size_t)f * gridDim.x + chunk) * SEGM_STATS_REC + tid] = s_rec[tid];
}

__global__ __launch_bounds__(128) void segm_reduce_kernel(SegmStatsArgs a, int chunks) {
  __shared__ int32_t s_rec[SEGM_STATS_REC];
  const int tid = threadIdx.x, f = blockIdx.x;
  if (tid < SEGM_STATS_REC) {
    const int32_t* rec = a.ws + (size_t)f * chunks * SEGM_STATS_REC + tid;
    int32_t acc = rec[0];
    for (int k = 1; k < chunks; ++k) acc = segm_rec_fold(tid, acc, rec[(size_t)k * SEGM_STATS_REC]);
    s_rec[tid] = acc;
  }
  __syncthreads();
  // one writer per output word: counts by class, then the eight box words, then the six agree words
  if (tid < a.C) a.counts[(size_t)f * a.C + tid] = s_rec[tid];
  if (tid >= 64 && tid < 72) {
    const int k = tid - 64, s = k >> 2;
    const bool any = s_rec[SEGM_REC_BOX + 4 * s + 2] >= 0;
    a.boxes[(size_t)f * 8 + k] = any ? s_rec[SEGM_REC_BOX + k] + ((k & 2) ? 1 : 0) : 0;
  }
  if (a.agree && tid >= 72 && tid < 78) {
    const int k = tid - 72, s = k / 3, what = k - 3 * s, half = (a.C - 1) / 2;
    int32_t v;
    if (what == 1) {
      v = 0;
      for (int c = s ? 1 : half + 1; c <= (s ? half : a.C - 1); ++c) v += s_rec[c];
    } else {
      v = s_rec[SEGM_REC_AGREE + 2 * s + (what ? 1 : 0)];
    }
    a.agree[(size_t)f * 6 + k] = v;
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
hipError_t launch_segm(const SegmArgs& a0, hipStream_t s) {
  SegmArgs a = a0;
  a.wide = a.out && dword_rows(a.img_in, a.W) && dword_rows(a.out, a.W);
  a.wide_labels = a.labels && dword_rows(a.labels, a.W);
  // whole cells in 16-byte pieces: every cell starts 16-byte aligned and holds round-up-4(C) <= pix_stride readable floats
  a.vec = a.pix_stride % 4 == 0 && a.frame_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(a.logits) & 15) == 0;
  hipLaunchKernelGGL(segm_kernel, dim3((a.W + SEGM_TW - 1) / SEGM_TW, (a.H + SEGM_TH - 1) / SEGM_TH, a.n), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_segm_stats(const SegmStatsArgs& a, hipStream_t s) {
  const int chunks = segm_stats_chunks(a.H);
  const int wide = dword_rows(a.labels, a.W) && (!a.ids || (reinterpret_cast<uintptr_t>(a.ids) & 15) == 0);
  hipLaunchKernelGGL(segm_stats_kernel, dim3(chunks, a.n), dim3(256), 0, s, a, wide);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(segm_reduce_kernel, dim3(a.n), dim3(128), 0, s, a, chunks);
  return hipGetLastError();
}

}  // namespace acrmi
