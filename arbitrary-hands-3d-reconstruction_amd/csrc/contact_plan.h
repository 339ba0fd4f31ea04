// Host rules of the contact / interpenetration measure between two meshes (acrmi_mesh_contact, acrmi_contact; DESIGN.md
// section 19; the kernels are in csrc/contact.hip): launch geometry and chunking, workspace size, the enumeration of a
// frame's pairs from the slot flags, and the orientation sign of a topology.  Plain C++, no HIP: tools/contact_check.cpp
// compiles it alone; ACRMI_HD (csrc/roi_plan.h) is `__host__ __device__` when the translation unit is HIP.
//
// The measure (fp32, every operation rounded on its own):
//   P_m[i] = verts[m,i] + trans[m];  N_m[i] = sign[m] * sum over the incident faces, in the order of the vertex -> faces table,
//   of (v1 - v0) x (v2 - v0) taken on verts as given, NOT normalised.  For the ordered pair (a, b) and vertex i of a:
//   d2(i,j) = (dx*dx + dy*dy) + dz*dz, d = P_a[i] - P_b[j];  nn[i] = the j of the smallest d2 below +inf, the lowest j on a tie
//   (a NaN or +inf d2 never wins; none: nn = -1, d2 = +inf, s = 0);  s[i] = (dx*Nx + dy*Ny) + dz*Nz with N_b[nn[i]].
//   contact: d2 <= r*r;  inside: s < 0 and d2 <= m*m.  Both directions of a pair, and the pair's summary.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "roi_plan.h"      // ACRMI_HD

namespace acrmi {

constexpr int CONTACT_MAX_VERTS = 4000;      // = RENDER_MAX_VERTS: 12 bytes of LDS per vertex of the other mesh, 48000 bytes
constexpr int CONTACT_CHUNK = 128;           // vertices i of one pair-kernel block, one per thread (two waves)
constexpr int CONTACT_REDUCE_THREADS = 256;  // the reduce kernel's block
constexpr int CONTACT_MAX_HAND = 8;          // = ACRMI_MAX_HAND
constexpr int CONTACT_SLOT_FLOATS = 176;     // = ACRMI_SLOT
constexpr int CONTACT_FLAG = 0;              // = ACRMI_SLOT_FLAG
constexpr int CONTACT_SUM_F = 4;             // floats of a pair's summary: min d2, depth2 of side 0, of side 1, 0
constexpr int CONTACT_SUM_I = 6;             // ints: closest i, closest j, contact count side 0, 1, inside count side 0, 1

struct ContactPlan {
  bool ok;              // false: the sizes are refused (ACRMI_EINVAL)
  int chunks;           // blocks along i: ceil(n_verts / CONTACT_CHUNK)
  unsigned grid[3];     // the pair kernel's grid: (pair, chunk of i, direction)
  size_t lds_bytes;     // its dynamic LDS: the other mesh's positions, x[4] y[4] z[4] per four vertices
  size_t ws_bytes;      // the workspace: P and N records of every mesh
};

// Bytes of workspace for n_meshes meshes of n_verts vertices: float4 P[n_meshes][n_verts], then float4 N[n_meshes][n_verts].
inline size_t contact_workspace_bytes(int n_meshes, int n_verts) {
  if (n_meshes <= 0 || n_verts <= 0) return 0;
  return (size_t)n_meshes * (size_t)n_verts * 32;
}

// n_pairs >= 1.  Refused: n_verts outside 1..CONTACT_MAX_VERTS, n_meshes < 1, more than 2^31 - 1 output elements
// (n_pairs * 2 * n_verts) or records (n_meshes * n_verts).  The pairs run along the grid's x extent (up to 2^31 - 1); the
// chunks - at most 32 - along y.
inline ContactPlan contact_plan(int n_meshes, int n_verts, int n_pairs) {
  ContactPlan p{};
  if (n_meshes < 1 || n_pairs < 1 || n_verts < 1 || n_verts > CONTACT_MAX_VERTS) return p;
  if ((long long)n_pairs * 2 * n_verts > 0x7fffffffll || (long long)n_meshes * n_verts > 0x7fffffffll) return p;
  p.chunks = (n_verts + CONTACT_CHUNK - 1) / CONTACT_CHUNK;
  p.grid[0] = (unsigned)n_pairs;
  p.grid[1] = (unsigned)p.chunks;
  p.grid[2] = 2;
  p.lds_bytes = (size_t)((n_verts + 3) / 4) * 48;
  p.ws_bytes = contact_workspace_bytes(n_meshes, n_verts);
  p.ok = true;
  return p;
}

// A pair is computed when both indices name a mesh; everything else (negative: skipped on purpose; >= n_meshes: garbage) is the
// skipped pair: nn = -1, d2 = +inf, s = 0, zero counts, (i, j) = (-1, -1).
ACRMI_HD inline bool contact_pair_valid(int32_t a, int32_t b, int n_meshes) {
  return a >= 0 && b >= 0 && a < n_meshes && b < n_meshes;
}

// contact_dist: finite and >= 0; max_depth: >= 0, +inf allowed (NaN fails both).
inline bool contact_params_ok(float contact_dist, float max_depth) {
  return contact_dist >= 0.f && contact_dist <= 3.4028234e38f && max_depth >= 0.f;
}

// The pairs of a frame (acrmi_contact): rows of K (left, right) slot pairs, mesh (b*K + k)*2 + h.  Pair (b*K + i)*K + j is
// (left rank i, right rank j); a pair with either flag not > 0.5 (NaN included) is skipped: (-1, -1).
ACRMI_HD inline long long contact_pair_index(int b, int K, int i, int j) { return ((long long)b * K + i) * K + j; }
ACRMI_HD inline void contact_frame_pair(int b, int K, int i, int j, float flag_left, float flag_right, int32_t pair[2]) {
  const bool on = flag_left > 0.5f && flag_right > 0.5f;
  pair[0] = on ? (b * K + i) * 2 : -1;
  pair[1] = on ? (b * K + j) * 2 + 1 : -1;
}

// Orientation of a closed mesh: the sign of six times its signed volume, sum over the faces of v0 . (v1 x v2), in double, by
// face; +1 when it is exactly 0 (or NaN).  +1: the face normals (v1 - v0) x (v2 - v0) point outwards.
inline int contact_orientation_sign(const float* verts, const int32_t* faces, int n_faces) {
  double vol = 0.0;
  for (int f = 0; f < n_faces; ++f) {
    const float* p0 = verts + 3 * (size_t)faces[3 * f];
    const float* p1 = verts + 3 * (size_t)faces[3 * f + 1];
    const float* p2 = verts + 3 * (size_t)faces[3 * f + 2];
    const double ax = p0[0], ay = p0[1], az = p0[2], bx = p1[0], by = p1[1], bz = p1[2], cx = p2[0], cy = p2[1], cz = p2[2];
    vol += ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
  }
  return vol < 0.0 ? -1 : 1;
}

}  // namespace acrmi
