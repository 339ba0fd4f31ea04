// The surface contact measure between two meshes (acrmi_mesh_surface_contact / acrmi_surface_contact; DESIGN.md section 20;
// the rule, the launch geometry and the limits: csrc/surface_contact_plan.h).  Every vertex against every face of the other
// mesh: the closest point of the triangle (Ericson 5.1.5) and the crossing of the +Z ray, all fp32, every operation rounded
// on its own (-ffp-contract=off), so that tests/surface_contact_ref.py restates it bit for bit.
//
//   surface_setup_kernel   one block per mesh: P = v + trans as one 16-byte record per vertex, and one 48-byte record per
//                          face - three rows (corner x, y, z, the order of the edge that leaves the corner: +1 / -1 / 0).
//                          A mesh that sits in several pairs is prepared once.
//   surface_pair_kernel    grid (pair, chunk of 128 vertices i, direction), the grid of contact_pair_kernel: the other
//                          mesh's face records staged in LDS in tiles of SURFACE_FACE_TILE; every lane reads the SAME three
//                          rows of a face (ds_read_b128 broadcasts: no bank conflicts) and keeps the running (d2, face, q,
//                          cross) of its own vertex in registers.
//   surface_reduce_kernel  one block per pair: the summary of both directions, from the per-vertex outputs.
// No atomics on global memory; every output element has one writer and every reduction an order-free form (integer sums,
// maxima, a lexicographic minimum), so a pair computed alone equals the same pair computed in a batch.
#include "kernels.h"
#include "surface_contact_plan.h"

namespace acrmi {

namespace {

constexpr float kInf = __builtin_huge_valf();

__device__ inline SurfaceVec vec3(float4 r) { return SurfaceVec{r.x, r.y, r.z}; }

struct SurfaceMinKey { float d2; int i; };
__device__ inline SurfaceMinKey surface_min_key(SurfaceMinKey x, SurfaceMinKey y) {      // the smaller d2, the lower i on a tie
  return (y.d2 < x.d2 || (y.d2 == x.d2 && y.i < x.i)) ? y : x;
}

}  // namespace

__global__ __launch_bounds__(256) void surface_setup_kernel(SurfaceContactArgs a) {
  const int m = blockIdx.x, tid = threadIdx.x;
  const int32_t* topo = (a.mesh_topo && a.mesh_topo[m] == 1 && a.topo[1]) ? a.topo[1] : a.topo[0];
  const int32_t* faces = topo + 2;
  const float* V = a.verts + (size_t)m * a.n_verts * 3;
  float tx = 0.f, ty = 0.f, tz = 0.f;
  if (a.trans) { tx = a.trans[(size_t)m * 3]; ty = a.trans[(size_t)m * 3 + 1]; tz = a.trans[(size_t)m * 3 + 2]; }
  const bool tr = a.trans != nullptr;
  float4* P = a.ws + (size_t)m * a.n_verts;
  float4* F = a.ws + (size_t)a.n_meshes * a.n_verts + (size_t)m * a.n_faces * 3;
  for (int v = tid; v < a.n_verts; v += 256) {
    const float x = V[v * 3], y = V[v * 3 + 1], z = V[v * 3 + 2];
    P[v] = tr ? make_float4(x + tx, y + ty, z + tz, 0.f) : make_float4(x, y, z, 0.f);
  }
  for (int f = tid; f < a.n_faces; f += 256) {      // (the corners from verts again, not from P: no barrier, the same bits)
    const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    const int32_t idx[3] = {i0, i1, i2};
    const float ord[3] = {(float)surface_edge_order(i0, i1), (float)surface_edge_order(i1, i2), (float)surface_edge_order(i2, i0)};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float x = V[idx[c] * 3], y = V[idx[c] * 3 + 1], z = V[idx[c] * 3 + 2];
      F[3 * f + c] = tr ? make_float4(x + tx, y + ty, z + tz, ord[c]) : make_float4(x, y, z, ord[c]);
    }
  }
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

__global__ __launch_bounds__(SURFACE_REDUCE_THREADS) void surface_reduce_kernel(SurfaceContactArgs a) {
  constexpr int T = SURFACE_REDUCE_THREADS;
  __shared__ float s_d2[2][T];
  __shared__ int s_i[2][T];
  __shared__ int s_cnt[4][T];
  __shared__ float s_dep[2][T];
  const int pair = blockIdx.x, tid = threadIdx.x;
  const float r2 = a.contact_dist * a.contact_dist, m2 = a.max_depth * a.max_depth;
  SurfaceMinKey k[2] = {{kInf, -1}, {kInf, -1}};
  int cnt[4] = {0, 0, 0, 0};      // contact direction 0, 1, inside direction 0, 1
  float dep[2] = {0.f, 0.f};
#pragma unroll
  for (int dir = 0; dir < 2; ++dir) {
    const size_t base = ((size_t)pair * 2 + dir) * a.n_verts;
    for (int i = tid; i < a.n_verts; i += T) {
      const float d = a.d2[base + i];
      const bool has = a.face[base + i] >= 0;
      if (has && d < k[dir].d2) { k[dir].d2 = d; k[dir].i = i; }      // ascending i per thread: strict keeps the lowest
      const bool contact = has && d <= r2, inside = has && (a.cross[base + i] & 1) && d <= m2;
      cnt[dir] += contact ? 1 : 0;
      cnt[2 + dir] += inside ? 1 : 0;
      dep[dir] = inside ? fmaxf(dep[dir], d) : dep[dir];
    }
  }
#pragma unroll
  for (int dir = 0; dir < 2; ++dir) { s_d2[dir][tid] = k[dir].d2; s_i[dir][tid] = k[dir].i; s_dep[dir][tid] = dep[dir]; }
#pragma unroll
  for (int q = 0; q < 4; ++q) s_cnt[q][tid] = cnt[q];
  __syncthreads();
  for (int w = T / 2; w > 0; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int dir = 0; dir < 2; ++dir) {
        const SurfaceMinKey r = surface_min_key(SurfaceMinKey{s_d2[dir][tid], s_i[dir][tid]},
                                                SurfaceMinKey{s_d2[dir][tid + w], s_i[dir][tid + w]});
        s_d2[dir][tid] = r.d2; s_i[dir][tid] = r.i;
        s_dep[dir][tid] = fmaxf(s_dep[dir][tid], s_dep[dir][tid + w]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) s_cnt[q][tid] += s_cnt[q][tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    float* sf = a.sum_f + (size_t)pair * SURFACE_SUM_F;
    int32_t* si = a.sum_i + (size_t)pair * SURFACE_SUM_I;
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
      const int bi = s_i[dir][0];
      sf[dir] = s_d2[dir][0];
      sf[2 + dir] = s_dep[dir][0];
      si[2 * dir] = bi;
      si[2 * dir + 1] = bi >= 0 ? a.face[((size_t)pair * 2 + dir) * a.n_verts + bi] : -1;
    }
    si[4] = s_cnt[0][0]; si[5] = s_cnt[1][0]; si[6] = s_cnt[2][0]; si[7] = s_cnt[3][0];
  }
}

hipError_t launch_surface_contact(const SurfaceContactArgs& a, hipStream_t s) {
  const SurfacePlan p = surface_plan(a.n_meshes, a.n_verts, a.n_faces, a.n_pairs);
  if (!p.ok) return hipErrorInvalidValue;
  hipLaunchKernelGGL(surface_setup_kernel, dim3(a.n_meshes), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(surface_pair_kernel, dim3(p.grid[0], p.grid[1], p.grid[2]), dim3(CONTACT_CHUNK), 0, s, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(surface_reduce_kernel, dim3(a.n_pairs), dim3(SURFACE_REDUCE_THREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace acrmi
