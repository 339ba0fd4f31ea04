// The rule of NV12 output (acrmi_nv12_out_matrix, acrmi_rgb_to_nv12, acrmi_nv12_compose; DESIGN.md "NV12 output"): the
// ten-integer coefficient row, the five named rows, the overflow check and the rule for one 2x2 block.  Plain C++, no HIP:
// tools/nv12_out_check.cpp compiles it alone.  The kernels of csrc/nv12_out.hip run the same block functions on the GPU:
// ACRMI_HD is `__host__ __device__` when the translation unit is HIP and nothing in plain C++.
//
// All arithmetic is int32, the shift is arithmetic, results clamp to 0..255.  For a row
// (cry, cgy, cby, cru, cgu, cbu, crv, cgv, cbv, y_off):
//   per pixel:      Y = clamp((cry R + cgy G + cby B + (y_off << 20) + (1 << 19)) >> 20)
//   per 2x2 block:  R4, G4, B4 = the sums of the four pixels' R, G, B   (0..1020)
//                   U = clamp((cru R4 + cgu G4 + cbu B4 + (128 << 22) + (1 << 21)) >> 22)
//                   V = clamp((crv R4 + cgv G4 + cbv B4 + (128 << 22) + (1 << 21)) >> 22)
// Chroma is the mean of the block, the division by four folded into the shift: for four equal pixels it is the per-pixel
// value, the counterpart of the input rule's nearest chroma (csrc/nv12.hip).
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

struct Nv12OutCoef {
  int32_t cry, cgy, cby, cru, cgu, cbu, crv, cgv, cbv, y_off;
};

// By ACRMI_NV12_* (the names of the input side; a name selects both rows).  The four bt* rows: round(x * 2^20) of the textbook
// forms - luma Kr, Kg, Kb (times 219/255 in limited range), chroma -0.5 Kr/(1-Kb), -0.5 Kg/(1-Kb), 0.5 for U and 0.5,
// -0.5 Kg/(1-Kr), -0.5 Kb/(1-Kr) for V (times 224/255 in limited range).  cv601: the constants of OpenCV's RGB -> YUV 4:2:0
// code as remembered, NOT verified against its source; no equality with cv2 is claimed for any row (cv2 writes no NV12, and
// its I420 path takes chroma from one pixel of the block, not the mean).
static const int32_t kNv12OutMatrix[5][10] = {
    {269484, 528482, 102760, -155188, -305135, 460324, 460324, -385875, -74448, 16},      // cv601
    {269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897, 16},      // bt601
    {313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262, 0},       // bt601-full
    {191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230, 16},       // bt709
    {222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074, 0},        // bt709-full
};

// Ten integers -> *k.  False - *k untouched - for a row the rule is not defined for: y_off outside 0..255, or sums that could
// leave int32:
//   255 (|cry| + |cgy| + |cby|) + (y_off << 20) + 2^19 >= 2^31
//   1020 max(|cru| + |cgu| + |cbu|, |crv| + |cgv| + |cbv|) + (128 << 22) + 2^21 >= 2^31
// (the full-range rows reach 0.75 of the range in chroma).  *why, when given, says which.
inline bool nv12_out_row(const int32_t* c, Nv12OutCoef* k, const char** why = nullptr) {
  auto mag = [](int32_t v) { return v < 0 ? -(int64_t)v : (int64_t)v; };
  const char* w = nullptr;
  if (c[9] < 0 || c[9] > 255) {
    w = "y_off outside 0..255";
  } else {
    const int64_t luma = mag(c[0]) + mag(c[1]) + mag(c[2]);
    const int64_t cu = mag(c[3]) + mag(c[4]) + mag(c[5]), cv = mag(c[6]) + mag(c[7]) + mag(c[8]);
    if (255 * luma + ((int64_t)c[9] << 20) + (1LL << 19) >= (1LL << 31)) w = "the luma sum could overflow int32";
    else if (1020 * (cu > cv ? cu : cv) + (128LL << 22) + (1LL << 21) >= (1LL << 31)) w = "a chroma sum could overflow int32";
  }
  if (why) *why = w;
  if (w) return false;
  k->cry = c[0]; k->cgy = c[1]; k->cby = c[2];
  k->cru = c[3]; k->cgu = c[4]; k->cbu = c[5];
  k->crv = c[6]; k->cgv = c[7]; k->cbv = c[8];
  k->y_off = c[9];
  return true;
}

ACRMI_HD inline int nv12_out_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

ACRMI_HD inline int nv12_out_luma(const Nv12OutCoef& k, int R, int G, int B) {
  return nv12_out_clamp8((k.cry * R + k.cgy * G + k.cby * B + (k.y_off << 20) + (1 << 19)) >> 20);
}

// R4, G4, B4: the sums over the block
ACRMI_HD inline void nv12_out_chroma(const Nv12OutCoef& k, int R4, int G4, int B4, int* U, int* V) {
  *U = nv12_out_clamp8((k.cru * R4 + k.cgu * G4 + k.cbu * B4 + (128 << 22) + (1 << 21)) >> 22);
  *V = nv12_out_clamp8((k.crv * R4 + k.cgv * G4 + k.cbv * B4 + (128 << 22) + (1 << 21)) >> 22);
}

// One 2x2 block of the plain conversion.  rgb[p] = (R, G, B) of pixel p in the order (0,0), (0,1), (1,0), (1,1).
ACRMI_HD inline void nv12_out_block(const Nv12OutCoef& k, const int rgb[4][3], int y[4], int* U, int* V) {
  int s[3] = {0, 0, 0};
  for (int p = 0; p < 4; ++p) {
    y[p] = nv12_out_luma(k, rgb[p][0], rgb[p][1], rgb[p][2]);
    s[0] += rgb[p][0]; s[1] += rgb[p][1]; s[2] += rgb[p][2];
  }
  nv12_out_chroma(k, s[0], s[1], s[2], U, V);
}

// One 2x2 block of compose.  drawn[p]: the drawn frame's (R, G, B); shown[p]: what the input rule makes of the source's
// (Y[p], U, V) - the picture the drawing started from; src_y, src_u, src_v: the source bytes.  A pixel is changed when its
// drawn triple differs from its shown one: a changed pixel gets Y(drawn), any changed pixel gives the block U, V of the four
// drawn triples, everything else keeps the source bytes.
ACRMI_HD inline void nv12_out_compose_block(const Nv12OutCoef& k, const int drawn[4][3], const int shown[4][3], const int src_y[4],
                                            int src_u, int src_v, int y[4], int* U, int* V) {
  bool any = false;
  int s[3] = {0, 0, 0};
  for (int p = 0; p < 4; ++p) {
    const bool changed = drawn[p][0] != shown[p][0] || drawn[p][1] != shown[p][1] || drawn[p][2] != shown[p][2];
    y[p] = changed ? nv12_out_luma(k, drawn[p][0], drawn[p][1], drawn[p][2]) : src_y[p];
    any = any || changed;
    s[0] += drawn[p][0]; s[1] += drawn[p][1]; s[2] += drawn[p][2];
  }
  *U = src_u;
  *V = src_v;
  if (any) nv12_out_chroma(k, s[0], s[1], s[2], U, V);
}

}  // namespace acrmi
