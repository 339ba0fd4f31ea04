// The surface contact measure between two meshes (acrmi_mesh_surface_contact, acrmi_surface_contact; DESIGN.md section 20;
// the kernels are in csrc/contact.hip): the distance from every vertex to the other mesh's SURFACE with the point on
// it, and containment by counting the crossings of a ray.  Here: the rule as functions shared by host and device, the launch
// geometry, the limits and the workspace size.  Plain C++, no HIP: tools/surface_contact_check.cpp compiles it alone; ACRMI_HD
// (csrc/roi_plan.h) is `__host__ __device__` when the translation unit is HIP.
//
// The rule (fp32, every operation rounded on its own; the library is built with -ffp-contract=off and `/` is correctly rounded):
//   dot(a,b) = (ax*bx + ay*by) + az*bz;  a cross component is (a*b) - (c*d);  P_m[i] = verts[m,i] + trans[m].
//   For the ordered pair (a, b), vertex p = P_a[i] and face f of b with corners A, B, C = P_b[f0], P_b[f1], P_b[f2]:
//   closest point (Ericson, Real-Time Collision Detection 5.1.5; every comparison is false on NaN, the first true branch wins)
//     ab = B-A, ac = C-A, ap = p-A, d1 = dot(ab,ap), d2 = dot(ac,ap);  bp = p-B, d3 = dot(ab,bp), d4 = dot(ac,bp);
//     cp = p-C, d5 = dot(ab,cp), d6 = dot(ac,cp);  vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4;
//     e43 = d4-d3, e56 = d5-d6
//     1. d1<=0 && d2<=0: q = A                       2. d3>=0 && d4<=d3: q = B
//     3. vc<=0 && d1>=0 && d3<=0: q = A + (d1/(d1-d3))*ab
//     4. d6>=0 && d5<=d6: q = C                      5. vb<=0 && d2>=0 && d6<=0: q = A + (d2/(d2-d6))*ac
//     6. va<=0 && e43>=0 && e56>=0: q = B + (e43/(e43+e56))*(C-B)
//     7. otherwise: den = 1/((va+vb)+vc), q = (A + ab*(vb*den)) + ac*(vc*den)
//     e = p-q, D2(i,f) = dot(e,e).  face[i] = the f with the smallest D2 below +inf, the lowest f on a tie (NaN and +inf never
//     win; degenerate faces need no special case); d2[i] that value, point[i] that face's q; none: face -1, d2 +inf, point 0.
//   containment by the crossings of the ray from p towards +Z.  For each face edge u -> v (mesh vertex indices; the edges
//     f0->f1, f1->f2, f2->f0): lo, hi = the positions of min(u,v), max(u,v); E = (hi.x-lo.x)*(p.y-lo.y) - (hi.y-lo.y)*(p.x-lo.x);
//     sc = (E >= 0) ? +1 : -1; the edge's sign is sc when u < v, -sc when u > v, 0 when u == v.  The face COVERS p when its three
//     signs are equal and not zero.  The ray meets the face's plane IN FRONT of p when o = dot(ap, n), n = ab x ac, and n.z have
//     strictly opposite signs (neither zero; NaN fails).  cross[i] = the number of faces that do both; inside: cross[i] odd.
//     The edge value is computed identically by the two faces that share an edge, so the count is exact on a closed mesh.
//   flags and summary, per direction (surface distance is not symmetric): in contact: face >= 0 and d2 <= r*r; inside: face >= 0,
//     cross odd and d2 <= m*m; min_d2[dir] with closest[dir] = (i, face), the lowest i on a tie, (-1, -1) without one;
//     n_contact[dir], n_inside[dir]; depth2[dir] = the largest d2 among the inside vertices, 0 without one.
//   a skipped pair (an index outside [0, n_meshes)): face -1, d2 +inf, point 0, cross 0, zero counts.
// There is no cull, here or in the kernel: every face is tested against every vertex.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "contact_plan.h"      // CONTACT_MAX_VERTS, CONTACT_CHUNK, contact_pair_valid, contact_params_ok, ACRMI_HD

namespace acrmi {

constexpr int SURFACE_FACE_TILE = 256;        // faces of the other mesh staged in LDS at a time
constexpr int SURFACE_FACE_BYTES = 48;        // a face record: three 16-byte rows (corner x, y, z, the sign of the edge leaving it)
constexpr int SURFACE_MAX_FACES = 8000;       // = 2 * CONTACT_MAX_VERTS: a closed mesh has 2 V - 4 faces
constexpr int SURFACE_SUM_F = 4;              // floats of a pair's summary: min d2 of direction 0, 1, depth2 of direction 0, 1
constexpr int SURFACE_SUM_I = 8;              // ints: closest (i, face) of direction 0, of 1, contact count 0, 1, inside count 0, 1

struct SurfaceVec { float x, y, z; };

ACRMI_HD inline float surface_dot(SurfaceVec a, SurfaceVec b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
ACRMI_HD inline SurfaceVec surface_sub(SurfaceVec a, SurfaceVec b) { return SurfaceVec{a.x - b.x, a.y - b.y, a.z - b.z}; }
ACRMI_HD inline SurfaceVec surface_cross(SurfaceVec a, SurfaceVec b) {
  return SurfaceVec{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// a + s * u per component (the product rounded, then the sum)
ACRMI_HD inline SurfaceVec surface_along(SurfaceVec a, float s, SurfaceVec u) {
  return SurfaceVec{a.x + s * u.x, a.y + s * u.y, a.z + s * u.z};
}

// The closest point of triangle (A, B, C) to p -> the branch taken (1..7), q and D2 = |p - q|^2.  The three quotients and the
// reciprocal of the rule are ONE division here, numerator and denominator chosen by the branch: the quotient's bits are those
// of the rule's, and a vertex branch does not use it.
ACRMI_HD inline int surface_closest(SurfaceVec p, SurfaceVec A, SurfaceVec B, SurfaceVec C, SurfaceVec* q_out, float* d2_out) {
  const SurfaceVec ab = surface_sub(B, A), ac = surface_sub(C, A), ap = surface_sub(p, A);
  const float d1 = surface_dot(ab, ap), d2 = surface_dot(ac, ap);
  const SurfaceVec bp = surface_sub(p, B);
  const float d3 = surface_dot(ab, bp), d4 = surface_dot(ac, bp);
  const SurfaceVec cp = surface_sub(p, C);
  const float d5 = surface_dot(ab, cp), d6 = surface_dot(ac, cp);
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float e43 = d4 - d3, e56 = d5 - d6;
  int br = 7;
  float num = 1.f, den = (va + vb) + vc;
  if (d1 <= 0.f && d2 <= 0.f) br = 1;
  else if (d3 >= 0.f && d4 <= d3) br = 2;
  else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { br = 3; num = d1; den = d1 - d3; }
  else if (d6 >= 0.f && d5 <= d6) br = 4;
  else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { br = 5; num = d2; den = d2 - d6; }
  else if (va <= 0.f && e43 >= 0.f && e56 >= 0.f) { br = 6; num = e43; den = e43 + e56; }
  const float t = num / den;
  SurfaceVec q;
  if (br == 1) q = A;
  else if (br == 2) q = B;
  else if (br == 4) q = C;
  else if (br == 3) q = surface_along(A, t, ab);
  else if (br == 5) q = surface_along(A, t, ac);
  else if (br == 6) q = surface_along(B, t, surface_sub(C, B));
  else q = surface_along(surface_along(A, vb * t, ab), vc * t, ac);
  const SurfaceVec e = surface_sub(p, q);
  *q_out = q;
  *d2_out = surface_dot(e, e);
  return br;
}

// The order of an edge u -> v of a face: +1 when u < v, -1 when u > v, 0 when u == v.
ACRMI_HD inline int surface_edge_order(int32_t u, int32_t v) { return u < v ? 1 : (u > v ? -1 : 0); }

// The sign of edge U -> V (positions of u and v; order = surface_edge_order(u, v)) at p: the edge value is taken from the
// position of the lower index to that of the higher, whichever way the face runs along it.
ACRMI_HD inline int surface_edge_sign(SurfaceVec p, SurfaceVec U, SurfaceVec V, int order) {
  const SurfaceVec lo = order > 0 ? U : V, hi = order > 0 ? V : U;
  const float E = (hi.x - lo.x) * (p.y - lo.y) - (hi.y - lo.y) * (p.x - lo.x);
  const int sc = E >= 0.f ? 1 : -1;
  return order > 0 ? sc : (order < 0 ? -sc : 0);
}

// Does the ray from p towards +Z cross the face (A, B, C)?  o0, o1, o2: the orders of the edges A -> B, B -> C, C -> A.
ACRMI_HD inline bool surface_crosses(SurfaceVec p, SurfaceVec A, SurfaceVec B, SurfaceVec C, int o0, int o1, int o2) {
  const int s0 = surface_edge_sign(p, A, B, o0), s1 = surface_edge_sign(p, B, C, o1), s2 = surface_edge_sign(p, C, A, o2);
  const bool covers = s0 == s1 && s1 == s2 && s0 != 0;
  const SurfaceVec ab = surface_sub(B, A), ac = surface_sub(C, A), ap = surface_sub(p, A);
  const SurfaceVec n = surface_cross(ab, ac);
  const float o = surface_dot(ap, n);
  const bool front = (o > 0.f && n.z < 0.f) || (o < 0.f && n.z > 0.f);
  return covers && front;
}

// contact_plan's fields with the chunking and the (pair, chunk, direction) grid as it states them; here lds_bytes is the pair
// kernel's one tile of face records and ws_bytes the P records of every mesh, then the face records of every mesh.
struct SurfacePlan : ContactPlan {
  int tiles;            // LDS tiles of the other mesh's faces: ceil(n_faces / SURFACE_FACE_TILE)
};

// Bytes of workspace: float4 P[n_meshes][n_verts], then three float4 per face [n_meshes][n_faces].
inline size_t surface_workspace_bytes(int n_meshes, int n_verts, int n_faces) {
  if (n_meshes <= 0 || n_verts <= 0 || n_faces <= 0) return 0;
  return (size_t)n_meshes * ((size_t)n_verts * 16 + (size_t)n_faces * SURFACE_FACE_BYTES);
}

// n_pairs >= 1.  Refused: what contact_plan refuses (n_verts outside 1..CONTACT_MAX_VERTS, n_meshes < 1, n_meshes * n_verts
// records beyond 2^31 - 1), n_faces outside 1..SURFACE_MAX_FACES, more than 2^31 - 1 output elements (n_pairs * 2 * n_verts * 3:
// the points) or face records (n_meshes * n_faces * 3).
inline SurfacePlan surface_plan(int n_meshes, int n_verts, int n_faces, int n_pairs) {
  SurfacePlan p{};
  if (n_faces < 1 || n_faces > SURFACE_MAX_FACES || (long long)n_pairs * 6 * n_verts > 0x7fffffffll ||
      (long long)n_meshes * n_faces * 3 > 0x7fffffffll)
    return p;
  static_cast<ContactPlan&>(p) = contact_plan(n_meshes, n_verts, n_pairs);
  if (!p.ok) return p;
  p.tiles = (n_faces + SURFACE_FACE_TILE - 1) / SURFACE_FACE_TILE;
  p.lds_bytes = (size_t)SURFACE_FACE_TILE * SURFACE_FACE_BYTES;
  p.ws_bytes = surface_workspace_bytes(n_meshes, n_verts, n_faces);
  return p;
}

}  // namespace acrmi
