// Rules of the per-vertex colour views (acrmi_vertex_colors, acrmi_contact_values; the kernels are in
// csrc/vertex_color.hip): a scalar per vertex -> a colour per vertex, and the results of a contact measure -> a scalar and a
// flag per vertex of every hand.  Plain C++, no HIP: tools/vertex_color_check.cpp compiles it alone; ACRMI_HD (csrc/roi_plan.h)
// is `__host__ __device__` when the translation unit is HIP.
//
// All fp32, every operation rounded on its own (-ffp-contract=off), `/` and sqrt correctly rounded.
//  colour   flag != 0: the flag colour.  Else a NaN value: the mesh's base colour.  Else t = (v - lo) / (hi - lo) clamped to
//           [0, 1] (infinities clamp; a NaN quotient, which only hi - lo = +inf can give, is 0), i = (int)(t * 255), with
//           `reverse` 255 - i, colour_c = (float)lut[i][c] / 255.
//  values   hand (b, k, side) of B rows at K hands per side; its partners in ascending rank: left rank k -> pairs
//           (b*K + k)*K + j, direction 0; right rank k -> pairs (b*K + i)*K + k, direction 1.  Per vertex m2 = the smallest d2
//           over the partners (strict < from +inf: NaN and +inf never win), value = sqrt(m2), NaN when m2 stayed +inf; flag = 1
//           when in any partner pair d2 <= m*m (m = max_depth, the product in fp32) and the vertex is inside by the measure's
//           rule: s < 0 (nearest vertex), cross odd (surface).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "roi_plan.h"      // ACRMI_HD

namespace acrmi {

constexpr int VCOL_BLOCK = 256;      // threads per block of both kernels, one vertex (of one mesh / hand) each

// hi > lo, both finite (false for NaN)
inline bool vertex_color_range_ok(float lo, float hi) {
  return lo >= -3.4028234e38f && hi <= 3.4028234e38f && hi > lo;
}
// M * V * 3 elements of the output within 2^31 - 1
inline bool vertex_color_sizes_ok(long long M, long long V) {
  return M >= 0 && V >= 1 && (M == 0 || V <= 0x7fffffffll / 3 / M);
}
// B * K * K pairs of 2 * V values in, B * K * 2 * V out, all within 2^31 - 1
inline bool contact_values_sizes_ok(long long B, long long K, long long V) {
  return B >= 0 && K >= 1 && V >= 1 && (B == 0 || B * K * K <= 0x7fffffffll / 2 / V);
}

// index into the 256-entry table of a value that is not NaN
ACRMI_HD inline int vertex_color_index(float v, float lo, float hi, int reverse) {
  float t = (v - lo) / (hi - lo);
  t = t > 0.f ? (t < 1.f ? t : 1.f) : 0.f;      // (a NaN quotient - inf / inf of a range that overflows - is 0: the index stays in the table)
  const int i = (int)(t * 255.f);
  return reverse ? 255 - i : i;
}

// the colour of one vertex -> out[3]
ACRMI_HD inline void vertex_color(float v, int32_t flag, const float* base, const uint8_t* lut, const float* flag_rgb, float lo,
                                  float hi, int reverse, float* out) {
  if (flag != 0) {
    out[0] = flag_rgb[0]; out[1] = flag_rgb[1]; out[2] = flag_rgb[2];
  } else if (v != v) {
    out[0] = base[0]; out[1] = base[1]; out[2] = base[2];
  } else {
    const uint8_t* e = lut + 3 * vertex_color_index(v, lo, hi, reverse);
    out[0] = (float)e[0] / 255.f; out[1] = (float)e[1] / 255.f; out[2] = (float)e[2] / 255.f;
  }
}

// partner q (0..K-1) of hand (b, k, side): its pair
ACRMI_HD inline long long contact_values_pair(int b, int K, int k, int side, int q) {
  return side == 0 ? ((long long)b * K + k) * K + q : ((long long)b * K + q) * K + k;
}

// vertex v of hand (b, k, side): d2 [B*K*K, 2, V]; exactly one of s (fp32) and cross (int32), shaped alike
ACRMI_HD inline void contact_value(const float* d2, const float* s, const int32_t* cross, int b, int K, int k, int side, int V, int v,
                                   float max_depth, float* value, int32_t* flag) {
  const float m2lim = max_depth * max_depth;
  float m2 = INFINITY;
  int32_t fl = 0;
  for (int q = 0; q < K; ++q) {
    const size_t at = ((size_t)contact_values_pair(b, K, k, side, q) * 2 + side) * V + v;
    const float d = d2[at];
    if (d < m2) m2 = d;
    const bool inside = s ? s[at] < 0.f : (cross[at] & 1) != 0;
    if (d <= m2lim && inside) fl = 1;
  }
  *value = m2 < INFINITY ? sqrtf(m2) : NAN;
  *flag = fl;
}

}  // namespace acrmi
