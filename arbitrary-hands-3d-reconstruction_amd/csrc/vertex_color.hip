// Per-vertex colours for the mesh overlay (the rules once, in csrc/vertex_color_plan.h):
//   vertex_colors_kernel   one thread per (mesh, vertex): value + flag -> colour through a 256-entry table held in the kernel
//                          arguments (as the heat-map kernels hold theirs).
//   contact_values_kernel  one thread per (hand, vertex): the K partner pairs of the hand read in ascending rank -> the distance
//                          to the nearest partner and the inside flag.
// One writer per element, no atomics, no host visit; a row alone equals the row in a batch because a thread reads its own
// row's pairs only.
#include "kernels.h"
#include "vertex_color_plan.h"

namespace acrmi {

__global__ __launch_bounds__(VCOL_BLOCK) void vertex_colors_kernel(VertexColorArgs a) {
  const int v = blockIdx.x * VCOL_BLOCK + threadIdx.x, m = blockIdx.y;
  if (v >= a.V) return;
  const size_t at = (size_t)m * a.V + v;      // < M * V <= (2^31 - 1) / 3
  float c[3];
  vertex_color(a.values[at], a.flags ? a.flags[at] : 0, a.base_rgb + 3 * m, a.lut, a.flag_rgb, a.lo, a.hi, a.reverse, c);
  a.vcol[at * 3] = c[0]; a.vcol[at * 3 + 1] = c[1]; a.vcol[at * 3 + 2] = c[2];
}

__global__ __launch_bounds__(VCOL_BLOCK) void contact_values_kernel(ContactValuesArgs a) {
  const int v = blockIdx.x * VCOL_BLOCK + threadIdx.x, hand = blockIdx.y;      // hand = (b*K + k)*2 + side
  if (v >= a.V) return;
  const int side = hand & 1, bk = hand >> 1, b = bk / a.K, k = bk - b * a.K;
  float value;
  int32_t flag;
  contact_value(a.d2, a.s, a.cross, b, a.K, k, side, a.V, v, a.max_depth, &value, &flag);
  const size_t at = (size_t)hand * a.V + v;
  a.value[at] = value;
  a.flag[at] = flag;
}

// grid.y carries the mesh / hand: at most 65535 per launch, more as successive launches over shifted pointers
hipError_t launch_vertex_colors(const VertexColorArgs& a0, hipStream_t s) {
  for (int m0 = 0; m0 < a0.M; m0 += 65535) {
    VertexColorArgs a = a0;
    const int n = a0.M - m0 < 65535 ? a0.M - m0 : 65535;
    a.values += (size_t)m0 * a.V;
    if (a.flags) a.flags += (size_t)m0 * a.V;
    a.base_rgb += (size_t)m0 * 3;
    a.vcol += (size_t)m0 * a.V * 3;
    a.M = n;
    hipLaunchKernelGGL(vertex_colors_kernel, dim3((a.V + VCOL_BLOCK - 1) / VCOL_BLOCK, n), dim3(VCOL_BLOCK), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_contact_values(const ContactValuesArgs& a0, hipStream_t s) {
  // whole rows per launch: a row's pairs and hands move together
  const int rows_per = 65535 / (2 * a0.K) > 0 ? 65535 / (2 * a0.K) : 1;
  for (int b0 = 0; b0 < a0.B; b0 += rows_per) {
    ContactValuesArgs a = a0;
    const int n = a0.B - b0 < rows_per ? a0.B - b0 : rows_per;
    const size_t pair_off = (size_t)b0 * a.K * a.K * 2 * a.V, hand_off = (size_t)b0 * a.K * 2 * a.V;
    a.d2 += pair_off;
    if (a.s) a.s += pair_off;
    if (a.cross) a.cross += pair_off;
    a.value += hand_off;
    a.flag += hand_off;
    a.B = n;
    hipLaunchKernelGGL(contact_values_kernel, dim3((a.V + VCOL_BLOCK - 1) / VCOL_BLOCK, n * a.K * 2), dim3(VCOL_BLOCK), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace acrmi
