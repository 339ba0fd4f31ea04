// The hand-part segmentation as an output (acrmi_segm_labels, acrmi_segm_stats, acrmi_segment): the
// rule stated once, for the host and for the device.  Plain C++, no HIP: tools/segm_check.cpp compiles it alone; ACRMI_HD
// (csrc/roi_plan.h) is `__host__ __device__` when the translation unit is HIP.  tests/segm_ref.py restates it in numpy.
//
// The logits are a map of h x w cells of C classes (NHWC; a cell is pix_stride floats, a frame frame_stride floats); the
// frames are H x W.  Everything is fp32, every operation rounded on its own (the library is built with -ffp-contract=off).
// The frame's view, the canvas coordinate, COVERED, the taps, the footprint of a tile, the jet and the blend are the heat-map
// views' own: csrc/map_view_plan.h.  What is segmentation's:
//   value    map_value of every class c, v_c: bilinear LOGITS, not nearest labels
//   label    best = v_0, label = 0; for c = 1 .. C-1 in order, c is taken when v_c > best - strict: the lowest class wins a
//            tie and a NaN never wins (a NaN in class 0 keeps label 0).  A pixel that is not covered: SEGM_NONE = 255.
//   sides    C is odd, 3 <= C <= 63.  Class 0 is background, classes 1 .. (C-1)/2 are the RIGHT hand's parts and the rest the
//            LEFT hand's (acr/model.py:141-144 drops channel 0 and takes the first half as the right hand's); side index 0 =
//            left, 1 = right, as everywhere in the project.  Which part index is which bone is not known: the reference
//            ships no list.
//   view     for 1 <= label < C: byte = floor(weight * colour[label] + (1 - weight) * img); background and uncovered pixels
//            keep the input byte for byte
//   colours  right part p = label - 1 takes the jet LUT[128 + 8 p], left part p = label - 1 - (C-1)/2 takes LUT[127 - 8 p]
//            (the index clamped into the table: C = 33 never leaves it); exact integers, flipped for BGR
//   stats    counts[c] = pixels of label c (255 is not counted); box of a side = the smallest (l, t, r, b) around its pixels,
//            r and b EXCLUSIVE as roi_plan.h's boxes, all zeros when the side has no pixel; agree of a side = (pixels in
//            mask and silhouette, mask pixels, silhouette pixels), a pixel being in side s's silhouette when its rasteriser
//            id is >= 0 and ((id / n_faces) & 1) == s (the left mesh of a pair is the even one in every order
//            Engine.render and render_regions produce: id = (2 * row + hand) * F + face).
//   tree     segm_stats_kernel: block (chunk, frame) takes SEGM_STATS_ROWS rows of its frame and leaves one record of
//            SEGM_STATS_REC int32 (sums, minima, maxima) at ws[(frame * chunks + chunk) * SEGM_STATS_REC]; segm_reduce_kernel:
//            one thread per record word folds the chunks of its frame in chunk order and is the only writer of its output
//            words.  Integers: any order gives the same words.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "map_view_plan.h"      // Tap, map_value, map_jet, ...; ACRMI_HD

namespace acrmi {

constexpr int SEGM_NONE = 255;                    // ACRMI_SEGM_NONE
constexpr int SEGM_MIN_C = 3, SEGM_MAX_C = 63;
constexpr int SEGM_MAX_DIM = 16384;               // h, w, H, W
constexpr int SEGM_MAX_FRAMES = 65535;            // one grid layer per frame
// segm_kernel: a block of 256 threads draws SEGM_TW x SEGM_TH pixels, every thread 4 pixels of one row; the cells the tile
// samples are staged in LDS when they fit SEGM_LDS_FLOATS (on the 512 x 512 network input an inner tile samples 34 x 10 cells
// of the 256 x 256 map - pixel 64 reads cell 31, pixel 127 cell 64 - 340 cells of 36 floats = 48960 bytes; three blocks share
// the 160 KiB of a CU), else every tap is read from memory
constexpr int SEGM_TW = 64, SEGM_TH = 16;
constexpr int SEGM_LDS_FLOATS = 344 * 36;         // 49536 bytes
constexpr int SEGM_STATS_ROWS = 16;
constexpr int SEGM_STATS_REC = 80;                // 64 counts, 2 x (min x, min y, max x, max y), 2 x (intersection, silhouette), 4 unused
constexpr int SEGM_REC_BOX = 64, SEGM_REC_AGREE = 72;

// one step of the arg-max: class c with value v against the best so far
ACRMI_HD inline void segm_take(float v, int c, float& best, int& label) {
  if (v > best) { best = v; label = c; }
}

// the label of one covered pixel from its four cells (C floats each)
ACRMI_HD inline int segm_label(const float* a, const float* b, const float* c, const float* d, const Tap& ty, const Tap& tx, int C) {
  float best = map_value(ty, tx, a[0], b[0], c[0], d[0]);
  int label = 0;
  for (int k = 1; k < C; ++k) segm_take(map_value(ty, tx, a[k], b[k], c[k], d[k]), k, best, label);
  return label;
}

ACRMI_HD inline bool segm_classes_ok(int C) { return C >= SEGM_MIN_C && C <= SEGM_MAX_C && (C & 1) == 1; }
ACRMI_HD inline bool segm_dim_ok(int v) { return v > 0 && v <= SEGM_MAX_DIM; }

// 1 = right, 0 = left, -1 = background, SEGM_NONE or no label at all
ACRMI_HD inline int segm_side(int label, int C) { return label < 1 || label >= C ? -1 : (label <= (C - 1) / 2 ? 1 : 0); }

// jet entry of a label (1 <= label < C)
ACRMI_HD inline int segm_color_index(int label, int C) {
  const int half = (C - 1) / 2;
  const int i = label <= half ? 128 + 8 * (label - 1) : 127 - 8 * (label - 1 - half);
  return i < 0 ? 0 : i > 255 ? 255 : i;
}

// colors [C][3] in the image's channel order; row 0 (background, never drawn) is zero
ACRMI_HD inline void segm_default_colors(bool bgr, int C, uint8_t* colors) {
  for (int c = 0; c < 3; ++c) colors[c] = 0;
  for (int l = 1; l < C; ++l)
    for (int c = 0; c < 3; ++c) colors[3 * l + (bgr ? 2 - c : c)] = (uint8_t)map_jet(segm_color_index(l, C), c);
}

// floats of a staged cell: whole 16-byte pieces when the cells can be read so (vec), else the C classes
ACRMI_HD inline int segm_cell_floats(int C, bool vec) { return vec ? (C + 3) & ~3 : C; }

// ---- statistics ----
ACRMI_HD inline int segm_stats_chunks(int H) { return (H + SEGM_STATS_ROWS - 1) / SEGM_STATS_ROWS; }
// int32 words of acrmi_segm_stats' workspace; 0 when the sizes are not valid
ACRMI_HD inline size_t segm_stats_ws_ints(int n, int H, int W) {
  if (n < 0 || n > SEGM_MAX_FRAMES || !segm_dim_ok(H) || !segm_dim_ok(W)) return 0;
  return (size_t)n * segm_stats_chunks(H) * SEGM_STATS_REC;
}

// an empty record: sums 0, minima INT32_MAX, maxima -1
ACRMI_HD inline void segm_rec_clear(int32_t* rec) {
  for (int i = 0; i < SEGM_STATS_REC; ++i) rec[i] = 0;
  for (int s = 0; s < 2; ++s) {
    rec[SEGM_REC_BOX + 4 * s] = rec[SEGM_REC_BOX + 4 * s + 1] = INT32_MAX;
    rec[SEGM_REC_BOX + 4 * s + 2] = rec[SEGM_REC_BOX + 4 * s + 3] = -1;
  }
}

// one pixel into a record; id < 0 or n_faces <= 0: no silhouette
ACRMI_HD inline void segm_rec_pixel(int32_t* rec, int x, int y, int label, int32_t id, int n_faces, int C) {
  if (label < C) ++rec[label];
  const int s = segm_side(label, C);
  if (s >= 0) {
    int32_t* b = rec + SEGM_REC_BOX + 4 * s;
    if (x < b[0]) b[0] = x;
    if (y < b[1]) b[1] = y;
    if (x > b[2]) b[2] = x;
    if (y > b[3]) b[3] = y;
  }
  if (n_faces > 0 && id >= 0) {
    const int q = (id / n_faces) & 1;
    ++rec[SEGM_REC_AGREE + 2 * q + 1];
    if (q == s) ++rec[SEGM_REC_AGREE + 2 * q];
  }
}

// word i of a record folded over the chunks: sums are added, minima and maxima taken
ACRMI_HD inline int32_t segm_rec_fold(int i, int32_t acc, int32_t v) {
  if (i >= SEGM_REC_BOX && i < SEGM_REC_AGREE) return ((i - SEGM_REC_BOX) & 2) ? (v > acc ? v : acc) : (v < acc ? v : acc);
  return acc + v;
}

// a frame's folded record -> its output rows: counts [C], boxes [2][4], agree [2][3] (agree may be null)
ACRMI_HD inline void segm_rec_outputs(const int32_t* rec, int C, int32_t* counts, int32_t* boxes, int32_t* agree) {
  for (int c = 0; c < C; ++c) counts[c] = rec[c];
  const int half = (C - 1) / 2;
  for (int s = 0; s < 2; ++s) {
    const int32_t* b = rec + SEGM_REC_BOX + 4 * s;
    const bool any = b[2] >= 0;
    boxes[4 * s] = any ? b[0] : 0;
    boxes[4 * s + 1] = any ? b[1] : 0;
    boxes[4 * s + 2] = any ? b[2] + 1 : 0;
    boxes[4 * s + 3] = any ? b[3] + 1 : 0;
    if (agree) {
      int32_t mask = 0;
      for (int c = s ? 1 : half + 1; c <= (s ? half : C - 1); ++c) mask += rec[c];
      agree[3 * s] = rec[SEGM_REC_AGREE + 2 * s];
      agree[3 * s + 1] = mask;
      agree[3 * s + 2] = rec[SEGM_REC_AGREE + 2 * s + 1];
    }
  }
}

}  // namespace acrmi
