// Which hand of frame t is which hand of frame t-1 when several hands of a side are decoded per frame (acrmi_associate,
// acrmi_forward_tracks, acrmi_assoc_step): the rule, once for the host and for the device.  Plain C++,
// no HIP: tools/assoc_check.cpp compiles it alone; ACRMI_HD (csrc/roi_plan.h) is `__host__ __device__` when the translation
// unit is HIP.  Integers throughout, so host, device and the numpy restatement (tests/assoc_ref.py) agree exactly.
//
// State, per (stream, side): next_id (starts at 0) and K = max_hand track slots of (live, miss, id, cy, cx); a slot that is
// not live is free.  One frame of one (stream, side), K rows in rank order:
//   1 detections   rank j is a detection iff flag > 0.5 and the flat index, read as a float v, has 0 <= v < 4096 (NaN fails
//                  both; a float that fails is never converted); centre (cy, cx) = ((int)v >> 6, (int)v & 63)
//   2 matching     c(t, j) = dy * dy + dx * dx between live track t and detection j; a candidate iff c <= gate * gate; take the
//                  candidate with the smallest (c, t, j) among tracks and detections not yet taken until none is left - greedy,
//                  not an optimal assignment
//   3 matched      miss = 0, the centre becomes the detection's; id and filter state stay
//   4 unmatched    miss += 1; with max_miss >= 0 and miss > max_miss the slot becomes free
//   5 births       unmatched detections in rank order take the lowest free slot, else evict the unmatched live track with
//                  the largest miss (lower slot on a tie): live = 1, miss = 0, id = next_id++, the detection's centre, `born`
//                  (the caller clears the slot's filter init flag)
//   6 order        perm[k] = the rank whose row becomes row k: the detection of slot k, and the remaining ranks in ascending
//                  order into the slots without a detection in ascending order; track_id[k] = the slot's id, or -1 where the
//                  slot has no detection in this frame
// gate: 0..ASSOC_GATE_ANY map pixels, ASSOC_GATE_ANY = any distance (two centres of a 64 x 64 map are < 90 apart); max_miss:
// -1 = a track never expires, else >= 0.  The package's defaults (engine.TrackTable: gate 8, max_miss 5) are defaults of
// parameters, NOT measurements: nobody here has video from a trained checkpoint ("What is not known").
// capacity * max_hand <= ASSOC_MAX_TRACKS: a hand's state is 3 * 64 floats + an init flag + its share of the two AssocSide,
// about 0.8 KB, so the largest table is about 52 MB - the bound keeps a mistyped capacity from taking gigabytes.
#pragma once
#include <stdint.h>

#include "roi_plan.h"      // ACRMI_HD

namespace acrmi {

constexpr int ASSOC_MAX_HAND = 8;            // = ACRMI_MAX_HAND
constexpr int ASSOC_GATE_ANY = 128;
constexpr int ASSOC_MAX_TRACKS = 65536;
constexpr int ASSOC_SLOT_FLOATS = 176;       // = ACRMI_SLOT
constexpr int ASSOC_FLAG = 0, ASSOC_FLATIND = 1;      // = ACRMI_SLOT_FLAG, ACRMI_SLOT_FLATIND

struct AssocSide {      // the tracks of one (stream, side): ASSOC_STATE_INTS int32, all zero = every slot free
  int32_t next_id;
  int32_t live[ASSOC_MAX_HAND], miss[ASSOC_MAX_HAND], id[ASSOC_MAX_HAND], cy[ASSOC_MAX_HAND], cx[ASSOC_MAX_HAND];
};
constexpr int ASSOC_STATE_INTS = 1 + 5 * ASSOC_MAX_HAND;
static_assert(sizeof(AssocSide) == ASSOC_STATE_INTS * sizeof(int32_t), "AssocSide is plain int32");

struct AssocStep {      // one frame's result per slot, and the step's scratch (the device keeps it in LDS: no private arrays)
  int32_t perm[ASSOC_MAX_HAND];       // the rank whose row becomes row k
  int32_t track_id[ASSOC_MAX_HAND];   // the slot's id, -1 without a detection in this frame
  int32_t det[ASSOC_MAX_HAND];        // the detection (rank) of slot k in this frame, -1 = none
  int32_t born[ASSOC_MAX_HAND];       // 1: the slot's track starts in this frame
  int32_t dcy[ASSOC_MAX_HAND], dcx[ASSOC_MAX_HAND], dstate[ASSOC_MAX_HAND];   // per rank: centre; 0 no detection, 1 open, 2 taken
};

inline bool assoc_params_ok(int max_hand, int gate, int max_miss) {
  return max_hand >= 1 && max_hand <= ASSOC_MAX_HAND && gate >= 0 && gate <= ASSOC_GATE_ANY && max_miss >= -1;
}

ACRMI_HD inline bool assoc_detection(float flag, float v, int32_t* cy, int32_t* cx) {
  if (!(flag > 0.5f)) return false;               // NaN: no
  if (!(v >= 0.f && v < 4096.f)) return false;    // NaN, negative, huge: no, and not converted
  const int32_t i = (int32_t)v;
  *cy = i >> 6;
  *cx = i & 63;
  return true;
}

// rows: row j (rank j of this side) starts at rows + j * stride floats.  K in 1..ASSOC_MAX_HAND, gate and max_miss valid.
ACRMI_HD inline void assoc_step(AssocSide& s, int K, int gate, int max_miss, const float* rows, int stride, AssocStep& o) {
  for (int j = 0; j < K; ++j) {
    int32_t cy = 0, cx = 0;
    o.dstate[j] = assoc_detection(rows[j * stride + ASSOC_FLAG], rows[j * stride + ASSOC_FLATIND], &cy, &cx) ? 1 : 0;
    o.dcy[j] = cy;
    o.dcx[j] = cx;
    o.det[j] = -1;
    o.born[j] = 0;
  }
  const int32_t g2 = gate * gate;
  for (int round = 0; round < K; ++round) {
    int32_t bc = 0x7fffffff;
    int bt = -1, bj = -1;
    for (int t = 0; t < K; ++t) {
      if (!s.live[t] || o.det[t] >= 0) continue;
      for (int j = 0; j < K; ++j) {
        if (o.dstate[j] != 1) continue;
        const int32_t dy = o.dcy[j] - s.cy[t], dx = o.dcx[j] - s.cx[t];
        const int32_t c = dy * dy + dx * dx;
        if (c <= g2 && c < bc) { bc = c; bt = t; bj = j; }      // strict: the lowest (t, j) keeps a tie
      }
    }
    if (bt < 0) break;
    o.det[bt] = bj;
    o.dstate[bj] = 2;
    s.miss[bt] = 0;
    s.cy[bt] = o.dcy[bj];
    s.cx[bt] = o.dcx[bj];
  }
  for (int t = 0; t < K; ++t) {
    if (!s.live[t] || o.det[t] >= 0) continue;
    if (s.miss[t] < 0x7fffffff) ++s.miss[t];
    if (max_miss >= 0 && s.miss[t] > max_miss) s.live[t] = 0;
  }
  for (int j = 0; j < K; ++j) {
    if (o.dstate[j] != 1) continue;
    int t = -1;
    for (int k = K - 1; k >= 0; --k)
      if (!s.live[k]) t = k;
    if (t < 0) {
      int32_t bm = -1;
      for (int k = 0; k < K; ++k)
        if (o.det[k] < 0 && s.miss[k] > bm) { bm = s.miss[k]; t = k; }
    }
    if (t < 0) continue;      // (cannot happen: at most K detections for K slots)
    s.live[t] = 1;
    s.miss[t] = 0;
    s.id[t] = s.next_id;
    s.next_id = s.next_id == 0x7fffffff ? 0 : s.next_id + 1;
    s.cy[t] = o.dcy[j];
    s.cx[t] = o.dcx[j];
    o.det[t] = j;
    o.born[t] = 1;
    o.dstate[j] = 2;
  }
  int rest = 0;      // the next rank that no slot has taken
  for (int k = 0; k < K; ++k) {
    if (o.det[k] >= 0) {
      o.perm[k] = o.det[k];
      o.track_id[k] = s.id[k];
      continue;
    }
    while (rest < K && o.dstate[rest] == 2) ++rest;
    o.perm[k] = rest < K ? rest : k;
    o.track_id[k] = -1;
    ++rest;
  }
}

}  // namespace acrmi
