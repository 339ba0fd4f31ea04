// Host side of the per-stream smoothing launches (acrmi_smooth_streams): validation of the caller's stream ids and the
// grouping of one launch's frames by stream.  Plain C++, no HIP: tools/smooth_plan_check.cpp compiles it alone.
//
// A launch carries up to SMOOTH_FRAMES_PER_LAUNCH frames.  Its SmoothBatch travels BY VALUE in the kernel arguments (like
// RoiBgrBatch): per stream present in the launch - in the order of first appearance - the stream's row of the table and
// its first frame, and per frame the next frame of the same stream.  One workgroup walks one stream's chain, so frames
// that share an id are filtered in batch order and streams never meet.
#pragma once
#include <stdint.h>

namespace acrmi {

constexpr int SMOOTH_FRAMES_PER_LAUNCH = 256;
constexpr int SMOOTH_MAX_STREAMS = 65536;
constexpr uint16_t SMOOTH_END = 0xffff;

struct SmoothBatch {
  int32_t row[SMOOTH_FRAMES_PER_LAUNCH];      // [stream of the launch]: its row of the table
  uint16_t first[SMOOTH_FRAMES_PER_LAUNCH];   // [stream of the launch]: its first frame (index within the launch)
  uint16_t next[SMOOTH_FRAMES_PER_LAUNCH];    // [frame of the launch]: the next frame of the same stream, or SMOOTH_END
};

// Index of the first id outside [lowest, capacity), or -1 when all n are fine.  lowest = -1 where "-1 = leave this frame
// alone" is allowed, 0 where every id must name a stream.
inline int smooth_bad_id(const int32_t* ids, int n, int capacity, int lowest) {
  for (int i = 0; i < n; ++i)
    if (ids[i] < lowest || ids[i] >= capacity) return i;
  return -1;
}

// Groups the m <= SMOOTH_FRAMES_PER_LAUNCH frames of one launch (ids == nullptr: all of them stream 0; ids already
// validated) and returns the number of streams present; frames with id -1 belong to none.  last: scratch of `capacity`
// ints, all -1 on entry and all -1 again on return (the last frame seen of every stream while the launch is planned).
inline int smooth_plan(const int32_t* ids, int m, SmoothBatch* b, int32_t* last) {
  int groups = 0;
  for (int i = 0; i < m; ++i) {
    const int32_t s = ids ? ids[i] : 0;
    b->next[i] = SMOOTH_END;
    if (s < 0) continue;
    if (last[s] < 0) {
      b->row[groups] = s;
      b->first[groups] = (uint16_t)i;
      ++groups;
    } else {
      b->next[last[s]] = (uint16_t)i;
    }
    last[s] = i;
  }
  for (int k = 0; k < groups; ++k) last[b->row[k]] = -1;
  return groups;
}

}  // namespace acrmi
