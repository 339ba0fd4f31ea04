// How the view kernels (csrc/overlay.hip, csrc/segm.hip) move pixels: 4 pixels of one row = 3 dwords per thread when the row
// length is a multiple of 4 and the buffers are dword aligned (`wide`), byte by byte otherwise.  Channel c of pixel j is byte
// 3 j + c.  A thread reads and writes only its own pixels, so drawing in place is safe.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace acrmi {

__device__ inline void load_px(const uint8_t* p, bool wide, int n, uint32_t d[3]) {
  if (wide) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    d[0] = q[0]; d[1] = q[1]; d[2] = q[2];
    return;
  }
  d[0] = d[1] = d[2] = 0;
#pragma unroll
  for (int k = 0; k < 12; ++k)
    if (k < 3 * n) d[k >> 2] |= (uint32_t)p[k] << ((k & 3) * 8);
}

__device__ inline void store_px(uint8_t* p, bool wide, int n, const uint32_t d[3]) {
  if (wide) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    q[0] = d[0]; q[1] = d[1]; q[2] = d[2];
    return;
  }
#pragma unroll
  for (int k = 0; k < 12; ++k)
    if (k < 3 * n) p[k] = (uint8_t)(d[k >> 2] >> ((k & 3) * 8));
}

__device__ inline uint32_t get_byte(const uint32_t d[3], int k) { return (d[k >> 2] >> ((k & 3) * 8)) & 0xffu; }
__device__ inline void set_byte(uint32_t d[3], int k, uint32_t v) {
  d[k >> 2] = (d[k >> 2] & ~(0xffu << ((k & 3) * 8))) | (v << ((k & 3) * 8));
}

inline bool dword_rows(const void* p, int W) { return W % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace acrmi
