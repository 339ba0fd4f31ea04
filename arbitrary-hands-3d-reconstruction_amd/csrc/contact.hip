// The two contact measures between meshes, on one frame (setup - pair - reduce over the grid (pair, chunk of 128 vertices i,
// direction) of csrc/contact_plan.h).  All fp32, every operation rounded on its own (-ffp-contract=off), so that the numpy
// restatements under tests/ restate them bit for bit.
//   vertex   acrmi_mesh_contact / acrmi_contact; the rule: csrc/contact_plan.h.  The nearest-vertex
//            half-space heuristic (tests/contact_ref.py).
//   surface  acrmi_mesh_surface_contact / acrmi_surface_contact; the rule and the limits:
//            csrc/surface_contact_plan.h.  Every vertex against every face of the other mesh: the closest point of the triangle
//            (Ericson 5.1.5) and the crossing of the +Z ray (tests/surface_contact_ref.py).
//
//   contact_setup_kernel   one block per mesh: P = v + trans (place_mesh) and the signed, un-normalised vertex normal N (the
//                          vertex -> faces table's order, as render_setup_kernel sums it) as two 16-byte records per vertex in
//                          the workspace.  A mesh that sits in several pairs is prepared once.
//   surface_setup_kernel   the same P, and one 48-byte record per face - three rows (corner x, y, z, the order of the edge that
//                          leaves the corner: +1 / -1 / 0).
//   contact_pair_kernel    the other mesh's positions staged in LDS, four vertices to three 16-byte records (x[4], y[4], z[4]);
//                          every lane reads the SAME records (three ds_read_b128 per four j, broadcasts: no bank conflicts) and
//                          keeps the running (d2, j) of its own vertex in registers; the side value is evaluated once, at the end.
//   surface_pair_kernel    the other mesh's face records staged in LDS in tiles of SURFACE_FACE_TILE; every lane reads the SAME
//                          three rows of a face (ds_read_b128 broadcasts) and keeps the running (d2, face, q, cross) of its own
//                          vertex in registers.
//   contact_reduce_kernel  one block per pair: the summary, from the per-vertex outputs; one body, instantiated per measure.
// No atomics on global memory; every output element has one writer and every reduction a fixed or order-free form (integer
// sums, maxima, a lexicographic minimum), so a pair computed alone equals the same pair computed in a batch.
#include "kernels.h"
#include "surface_contact_plan.h"

#include <cmath>

namespace acrmi {

namespace {

constexpr float kInf = __builtin_huge_valf();

__device__ inline SurfaceVec vec3(float4 r) { return SurfaceVec{r.x, r.y, r.z}; }

// What both setup kernels begin with: the mesh's topology blob and where its vertices are placed.
struct PlacedMesh {
  const int32_t* topo;
  const float* V;      // the mesh's vertices as given
  float4* P;           // its position records in the workspace
  float tx, ty, tz;
  bool tr;             // trans is there: a position is v + t (without: v itself, not v + 0)
  __device__ float4 at(int v, float w) const {      // the placed vertex v, w beside it
    const float x = V[v * 3], y = V[v * 3 + 1], z = V[v * 3 + 2];
    return tr ? make_float4(x + tx, y + ty, z + tz, w) : make_float4(x, y, z, w);
  }
};
__device__ inline PlacedMesh place_mesh(const ContactFrame& a, int m) {
  PlacedMesh p{(a.mesh_topo && a.mesh_topo[m] == 1 && a.topo[1]) ? a.topo[1] : a.topo[0], a.verts + (size_t)m * a.n_verts * 3,
               a.ws + (size_t)m * a.n_verts, 0.f, 0.f, 0.f, a.trans != nullptr};
  if (p.tr) { p.tx = a.trans[(size_t)m * 3]; p.ty = a.trans[(size_t)m * 3 + 1]; p.tz = a.trans[(size_t)m * 3 + 2]; }
  return p;
}

}  // namespace

__global__ __launch_bounds__(256) void contact_setup_kernel(ContactArgs a) {
  const int m = blockIdx.x, tid = threadIdx.x;
  const PlacedMesh p = place_mesh(a, m);
  const float* V = p.V;
  const int32_t* faces = p.topo + 2;
  const int32_t* row = faces + 3 * a.n_faces;
  const int32_t* col = row + a.n_verts + 1;
  const float sg = (a.sign && a.sign[m] < 0) ? -1.f : 1.f;
  float4* N = a.ws + ((size_t)a.n_meshes + m) * a.n_verts;
  for (int v = tid; v < a.n_verts; v += 256) {
    p.P[v] = p.at(v, 0.f);
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int e = row[v]; e < row[v + 1]; ++e) {
      const int f = col[e];
      const float* p0 = V + 3 * faces[3 * f];
      const float* p1 = V + 3 * faces[3 * f + 1];
      const float* p2 = V + 3 * faces[3 * f + 2];
      const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
      const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
      nx += ay * bz - az * by;
      ny += az * bx - ax * bz;
      nz += ax * by - ay * bx;
    }
    N[v] = make_float4(nx * sg, ny * sg, nz * sg, 0.f);
  }
}

__global__ __launch_bounds__(256) void surface_setup_kernel(SurfaceContactArgs a) {
  const int m = blockIdx.x, tid = threadIdx.x;
  const PlacedMesh p = place_mesh(a, m);
  const int32_t* faces = p.topo + 2;
  float4* F = a.ws + (size_t)a.n_meshes * a.n_verts + (size_t)m * a.n_faces * 3;
  for (int v = tid; v < a.n_verts; v += 256) p.P[v] = p.at(v, 0.f);
  for (int f = tid; f < a.n_faces; f += 256) {      // (the corners from verts again, not from P: no barrier, the same bits)
    const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    const int32_t idx[3] = {i0, i1, i2};
    const float ord[3] = {(float)surface_edge_order(i0, i1), (float)surface_edge_order(i1, i2), (float)surface_edge_order(i2, i0)};
#pragma unroll
    for (int c = 0; c < 3; ++c) F[3 * f + c] = p.at(idx[c], ord[c]);
  }
}

__global__ __launch_bounds__(CONTACT_CHUNK) void contact_pair_kernel(ContactArgs a) {
  extern __shared__ float4 s_p[];      // P of the other mesh in groups of four: x[4], y[4], z[4] of vertices 4g .. 4g + 3
  const int pair = blockIdx.x, dir = blockIdx.z, tid = threadIdx.x;
  const int i = blockIdx.y * CONTACT_CHUNK + tid;
  int32_t ma = a.pairs[2 * (size_t)pair], mb = a.pairs[2 * (size_t)pair + 1];
  const size_t o = ((size_t)pair * 2 + dir) * a.n_verts + i;
  if (!contact_pair_valid(ma, mb, a.n_meshes)) {      // (uniform over the block)
    if (i < a.n_verts) { a.nn[o] = -1; a.d2[o] = kInf; a.side[o] = 0.f; }
    return;
  }
  if (dir) { const int32_t t = ma; ma = mb; mb = t; }
  const float4* Pb = a.ws + (size_t)mb * a.n_verts;
  const int groups = (a.n_verts + 3) >> 2;
  float* s_f = (float*)s_p;
  for (int j = tid; j < 4 * groups; j += CONTACT_CHUNK) {      // the pad of the last group is NaN: it never wins
    const float4 q = j < a.n_verts ? Pb[j] : make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), 0.f);
    float* g = s_f + (j >> 2) * 12 + (j & 3);
    g[0] = q.x; g[4] = q.y; g[8] = q.z;
  }
  __syncthreads();
  if (i >= a.n_verts) return;
  const float4 p = a.ws[(size_t)ma * a.n_verts + i];
  float best = kInf;
  int bj = -1;
#pragma unroll 2
  for (int g = 0; g < groups; ++g) {      // every lane reads the same three records: broadcasts
    const float4 X = s_p[3 * g], Y = s_p[3 * g + 1], Z = s_p[3 * g + 2];
    const float qx[4] = {X.x, X.y, X.z, X.w}, qy[4] = {Y.x, Y.y, Y.z, Y.w}, qz[4] = {Z.x, Z.y, Z.z, Z.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float dx = p.x - qx[u], dy = p.y - qy[u], dz = p.z - qz[u];
      const float d = (dx * dx + dy * dy) + dz * dz;
      const bool lt = d < best;      // strict: the lowest j keeps a tie; false for NaN and for +inf
      best = lt ? d : best;
      bj = lt ? 4 * g + u : bj;
    }
  }
  float sv = 0.f;
  if (bj >= 0) {
    const float* g = s_f + (bj >> 2) * 12 + (bj & 3);
    const float4 n = a.ws[((size_t)a.n_meshes + mb) * a.n_verts + bj];
    const float dx = p.x - g[0], dy = p.y - g[4], dz = p.z - g[8];
    sv = (dx * n.x + dy * n.y) + dz * n.z;
  }
  a.nn[o] = bj;
  a.d2[o] = best;
  a.side[o] = sv;
}

__global__ __launch_bounds__(CONTACT_CHUNK) void surface_pair_kernel(SurfaceContactArgs a) {
  __shared__ float4 s_face[SURFACE_FACE_TILE * 3];
  static_assert(sizeof(s_face) == (size_t)SURFACE_FACE_TILE * SURFACE_FACE_BYTES, "the tile the plan states");
  const int pair = blockIdx.x, dir = blockIdx.z, tid = threadIdx.x;
  const int i = blockIdx.y * CONTACT_CHUNK + tid;
  int32_t ma = a.pairs[2 * (size_t)pair], mb = a.pairs[2 * (size_t)pair + 1];
  const size_t o = ((size_t)pair * 2 + dir) * a.n_verts + i;
  const bool mine = i < a.n_verts;
  if (!contact_pair_valid(ma, mb, a.n_meshes)) {      // (uniform over the block)
    if (mine) {
      a.face[o] = -1; a.d2[o] = kInf; a.cross[o] = 0;
      a.point[3 * o] = 0.f; a.point[3 * o + 1] = 0.f; a.point[3 * o + 2] = 0.f;
    }
    return;
  }
  if (dir) { const int32_t t = ma; ma = mb; mb = t; }
  const float4* Fb = a.ws + (size_t)a.n_meshes * a.n_verts + (size_t)mb * a.n_faces * 3;
  // (a lane beyond the mesh keeps the barriers company on vertex 0 and writes nothing)
  const SurfaceVec p = vec3(a.ws[(size_t)ma * a.n_verts + (mine ? i : 0)]);
  float best = kInf;
  int bf = -1, cross = 0;
  SurfaceVec bq{0.f, 0.f, 0.f};
  for (int base = 0; base < a.n_faces; base += SURFACE_FACE_TILE) {
    const int nf = min(SURFACE_FACE_TILE, a.n_faces - base);
    __syncthreads();      // the tile before has been read by every lane
    for (int r = tid; r < 3 * nf; r += CONTACT_CHUNK) s_face[r] = Fb[(size_t)3 * base + r];
    __syncthreads();
    for (int f = 0; f < nf; ++f) {      // every lane reads the same three rows: broadcasts
      const float4 ra = s_face[3 * f], rb = s_face[3 * f + 1], rc = s_face[3 * f + 2];
      const SurfaceVec A = vec3(ra), B = vec3(rb), C = vec3(rc);
      SurfaceVec q;
      float d;
      surface_closest(p, A, B, C, &q, &d);
      const bool lt = d < best;      // strict: the lowest face keeps a tie; false for NaN and for +inf
      best = lt ? d : best;
      bf = lt ? base + f : bf;
      bq.x = lt ? q.x : bq.x; bq.y = lt ? q.y : bq.y; bq.z = lt ? q.z : bq.z;
      cross += surface_crosses(p, A, B, C, (int)ra.w, (int)rb.w, (int)rc.w) ? 1 : 0;
    }
  }
  if (!mine) return;
  a.face[o] = bf;
  a.d2[o] = best;
  a.cross[o] = cross;
  a.point[3 * o] = bq.x; a.point[3 * o + 1] = bq.y; a.point[3 * o + 2] = bq.z;
}

namespace {

struct MinKey { float d2; int i; };
__device__ inline MinKey min_key(MinKey x, MinKey y) {      // the smaller d2, the lower i on a tie (i = -1 only beside +inf)
  return (y.d2 < x.d2 || (y.d2 == x.d2 && y.i < x.i)) ? y : x;
}

// What the reduce needs to know of a measure: its arguments; the per-vertex index that is >= 0 where the vertex has a
// neighbour (and is the summary's partner of the closest i); what "inside" tests beside d2 <= m*m, given `has`; and DIRS, the directions
// whose minimum the summary keeps - 1: that of direction 0 alone (the vertex distance is symmetric), 2: both.
struct VertexMeasure {
  using Args = ContactArgs;
  static constexpr int DIRS = 1, SUM_F = CONTACT_SUM_F, SUM_I = CONTACT_SUM_I;
  static __device__ const int32_t* index(const Args& a) { return a.nn; }
  static __device__ bool inside(const Args& a, size_t o, bool has) {      // (the side value is loaded beside d2, has or not)
    const float s = a.side[o];
    return has && s < 0.f;
  }
};
struct SurfaceMeasure {
  using Args = SurfaceContactArgs;
  static constexpr int DIRS = 2, SUM_F = SURFACE_SUM_F, SUM_I = SURFACE_SUM_I;
  static __device__ const int32_t* index(const Args& a) { return a.face; }
  static __device__ bool inside(const Args& a, size_t o, bool has) { return has && (a.cross[o] & 1); }
};

}  // namespace

// The summary of a pair: floats [min d2 of the DIRS directions | depth2 of direction 0, 1 | 0 ...], ints [(closest i, its
// partner) of the DIRS directions | contact count of direction 0, 1 | inside count of direction 0, 1] - the layouts the two
// plan headers state.
template <class M>
__global__ __launch_bounds__(CONTACT_REDUCE_THREADS) void contact_reduce_kernel(typename M::Args a) {
  constexpr int T = CONTACT_REDUCE_THREADS, DIRS = M::DIRS;
  static_assert(DIRS + 2 <= M::SUM_F && 2 * DIRS + 4 == M::SUM_I, "the summary the plan states");
  __shared__ float s_d2[DIRS][T];
  __shared__ int s_i[DIRS][T];
  __shared__ int s_cnt[4][T];
  __shared__ float s_dep[2][T];
  const int pair = blockIdx.x, tid = threadIdx.x;
  const float r2 = a.contact_dist * a.contact_dist, m2 = a.max_depth * a.max_depth;
  const int32_t* index = M::index(a);
  MinKey k[DIRS];
#pragma unroll
  for (int dir = 0; dir < DIRS; ++dir) k[dir] = MinKey{kInf, -1};
  int cnt[4] = {0, 0, 0, 0};      // contact direction 0, 1, inside direction 0, 1
  float dep[2] = {0.f, 0.f};
#pragma unroll
  for (int dir = 0; dir < 2; ++dir) {
    const size_t base = ((size_t)pair * 2 + dir) * a.n_verts;
    for (int i = tid; i < a.n_verts; i += T) {
      const float d = a.d2[base + i];
      const bool has = index[base + i] >= 0;
      if constexpr (DIRS == 2) {
        if (has && d < k[dir].d2) { k[dir].d2 = d; k[dir].i = i; }      // ascending i per thread: strict keeps the lowest
      } else {
        if (dir == 0 && has && d < k[0].d2) { k[0].d2 = d; k[0].i = i; }
      }
      const bool contact = has && d <= r2, inside = M::inside(a, base + i, has) && d <= m2;
      cnt[dir] += contact ? 1 : 0;
      cnt[2 + dir] += inside ? 1 : 0;
      dep[dir] = inside ? fmaxf(dep[dir], d) : dep[dir];
    }
  }
#pragma unroll
  for (int dir = 0; dir < DIRS; ++dir) { s_d2[dir][tid] = k[dir].d2; s_i[dir][tid] = k[dir].i; }
#pragma unroll
  for (int q = 0; q < 4; ++q) s_cnt[q][tid] = cnt[q];
  s_dep[0][tid] = dep[0]; s_dep[1][tid] = dep[1];
  __syncthreads();
  for (int w = T / 2; w > 0; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int dir = 0; dir < DIRS; ++dir) {
        const MinKey r = min_key(MinKey{s_d2[dir][tid], s_i[dir][tid]}, MinKey{s_d2[dir][tid + w], s_i[dir][tid + w]});
        s_d2[dir][tid] = r.d2; s_i[dir][tid] = r.i;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) s_cnt[q][tid] += s_cnt[q][tid + w];
      s_dep[0][tid] = fmaxf(s_dep[0][tid], s_dep[0][tid + w]);
      s_dep[1][tid] = fmaxf(s_dep[1][tid], s_dep[1][tid + w]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    float* sf = a.sum_f + (size_t)pair * M::SUM_F;
    int32_t* si = a.sum_i + (size_t)pair * M::SUM_I;
#pragma unroll
    for (int dir = 0; dir < DIRS; ++dir) {
      const int bi = s_i[dir][0];
      sf[dir] = s_d2[dir][0];
      si[2 * dir] = bi;
      si[2 * dir + 1] = bi >= 0 ? index[((size_t)pair * 2 + dir) * a.n_verts + bi] : -1;
    }
    sf[DIRS] = s_dep[0][0]; sf[DIRS + 1] = s_dep[1][0];
#pragma unroll
    for (int q = DIRS + 2; q < M::SUM_F; ++q) sf[q] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) si[2 * DIRS + q] = s_cnt[q][0];
  }
}

// setup, pair and reduce of a measure on stream s; lds: the pair kernel's dynamic LDS.
template <class M>
static hipError_t launch_measure(void (*setup)(typename M::Args), void (*pair)(typename M::Args), const ContactPlan& p, size_t lds,
                                 const typename M::Args& a, hipStream_t s) {
  if (!p.ok) return hipErrorInvalidValue;
  hipLaunchKernelGGL(setup, dim3(a.n_meshes), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pair, dim3(p.grid[0], p.grid[1], p.grid[2]), dim3(CONTACT_CHUNK), lds, s, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(contact_reduce_kernel<M>, dim3(a.n_pairs), dim3(CONTACT_REDUCE_THREADS), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_contact(const ContactArgs& a, hipStream_t s) {
  const ContactPlan p = contact_plan(a.n_meshes, a.n_verts, a.n_pairs);
  return launch_measure<VertexMeasure>(contact_setup_kernel, contact_pair_kernel, p, p.lds_bytes, a, s);
}

hipError_t launch_surface_contact(const SurfaceContactArgs& a, hipStream_t s) {      // (its tile of faces is static LDS)
  return launch_measure<SurfaceMeasure>(surface_setup_kernel, surface_pair_kernel, surface_plan(a.n_meshes, a.n_verts, a.n_faces, a.n_pairs),
                                        0, a, s);
}

// acrmi_contact / acrmi_surface_contact: the pairs of every row from the slot flags (contact_frame_pair), each mesh's topology
// (hand type = slot index) and sign; thread t < n_pairs writes pair t, thread t < n_meshes describes mesh t.
__global__ void contact_prep_kernel(const float* __restrict__ slots, int B, int K, int sign_left, int sign_right,
                                    int32_t* __restrict__ pairs, int32_t* __restrict__ mesh_topo, int32_t* __restrict__ sign) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n_pairs = (long long)B * K * K, n_meshes = 2ll * B * K;
  if (t < n_pairs) {
    const int j = (int)(t % K), i = (int)((t / K) % K), b = (int)(t / ((long long)K * K));
    const float fl = slots[((size_t)(b * K + i) * 2) * CONTACT_SLOT_FLOATS + CONTACT_FLAG];
    const float fr = slots[((size_t)(b * K + j) * 2 + 1) * CONTACT_SLOT_FLOATS + CONTACT_FLAG];
    contact_frame_pair(b, K, i, j, fl, fr, pairs + 2 * t);
  }
  if (t < n_meshes) {
    mesh_topo[t] = (int32_t)(t & 1);
    sign[t] = (t & 1) ? sign_right : sign_left;
  }
}

hipError_t launch_contact_prep(const float* slots, int B, int K, int sign_left, int sign_right, int32_t* pairs, int32_t* mesh_topo,
                               int32_t* sign, hipStream_t s) {
  const long long n = (long long)B * K * (K > 2 ? K : 2);
  hipLaunchKernelGGL(contact_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, slots, B, K, sign_left, sign_right,
                     pairs, mesh_topo, sign);
  return hipGetLastError();
}

}  // namespace acrmi
