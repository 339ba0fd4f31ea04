// Contact and interpenetration between two meshes (acrmi_mesh_contact / acrmi_contact; the rule and the
// launch geometry: csrc/contact_plan.h).  The nearest-vertex half-space heuristic, all fp32, every operation rounded on its
// own (-ffp-contract=off), so that tests/contact_ref.py restates it bit for bit.
//
//   contact_setup_kernel   one block per mesh: P = v + trans and the signed, un-normalised vertex normal N (the vertex -> faces
//                          table's order, as render_setup_kernel sums it) as two 16-byte records per vertex in the workspace.
//                          A mesh that sits in several pairs is prepared once.
//   contact_pair_kernel    grid (pair, chunk of 128 vertices i, direction): the other mesh's positions staged in LDS, four
//                          vertices to three 16-byte records (x[4], y[4], z[4]); every lane reads the SAME records (three
//                          ds_read_b128 per four j, broadcasts: no bank conflicts) and keeps the running (d2, j) of its own
//                          vertex in registers; the side value is evaluated once, at the end.
//   contact_reduce_kernel  one block per pair: the summary, from the per-vertex outputs.
// No atomics on global memory; every output element has one writer and every reduction a fixed or order-free form (integer
// sums, maxima, a lexicographic minimum), so a pair computed alone equals the same pair computed in a batch.
#include "kernels.h"
#include "contact_plan.h"

#include <cmath>

namespace acrmi {

namespace {
constexpr float kInf = __builtin_huge_valf();
}

__global__ __launch_bounds__(256) void contact_setup_kernel(ContactArgs a) {
  const int m = blockIdx.x, tid = threadIdx.x;
  const int32_t* topo = (a.mesh_topo && a.mesh_topo[m] == 1 && a.topo[1]) ? a.topo[1] : a.topo[0];
  const int32_t* faces = topo + 2;
  const int32_t* row = faces + 3 * a.n_faces;
  const int32_t* col = row + a.n_verts + 1;
  const float* V = a.verts + (size_t)m * a.n_verts * 3;
  float tx = 0.f, ty = 0.f, tz = 0.f;
  if (a.trans) { tx = a.trans[m * 3]; ty = a.trans[m * 3 + 1]; tz = a.trans[m * 3 + 2]; }
  const float sg = (a.sign && a.sign[m] < 0) ? -1.f : 1.f;
  float4* P = a.ws + (size_t)m * a.n_verts;
  float4* N = a.ws + ((size_t)a.n_meshes + m) * a.n_verts;
  for (int v = tid; v < a.n_verts; v += 256) {
    const float x = V[v * 3], y = V[v * 3 + 1], z = V[v * 3 + 2];
    P[v] = a.trans ? make_float4(x + tx, y + ty, z + tz, 0.f) : make_float4(x, y, z, 0.f);
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

namespace {

struct MinKey { float d2; int i; };
__device__ inline MinKey min_key(MinKey x, MinKey y) {      // the smaller d2, the lower i on a tie (i = -1 only beside +inf)
  return (y.d2 < x.d2 || (y.d2 == x.d2 && y.i < x.i)) ? y : x;
}

}  // namespace

__global__ __launch_bounds__(CONTACT_REDUCE_THREADS) void contact_reduce_kernel(ContactArgs a) {
  constexpr int T = CONTACT_REDUCE_THREADS;
  __shared__ float s_d2[T];
  __shared__ int s_i[T];
  __shared__ int s_cnt[4][T];
  __shared__ float s_dep[2][T];
  const int pair = blockIdx.x, tid = threadIdx.x;
  const float r2 = a.contact_dist * a.contact_dist, m2 = a.max_depth * a.max_depth;
  MinKey k{kInf, -1};
  int cnt[4] = {0, 0, 0, 0};      // contact side 0, 1, inside side 0, 1
  float dep[2] = {0.f, 0.f};
#pragma unroll
  for (int dir = 0; dir < 2; ++dir) {
    const size_t base = ((size_t)pair * 2 + dir) * a.n_verts;
    for (int i = tid; i < a.n_verts; i += T) {
      const float d = a.d2[base + i], s = a.side[base + i];
      const bool has = a.nn[base + i] >= 0;
      if (dir == 0 && has && d < k.d2) { k.d2 = d; k.i = i; }      // ascending i per thread: strict keeps the lowest
      const bool contact = has && d <= r2, inside = has && s < 0.f && d <= m2;
      cnt[dir] += contact ? 1 : 0;
      cnt[2 + dir] += inside ? 1 : 0;
      dep[dir] = inside ? fmaxf(dep[dir], d) : dep[dir];
    }
  }
  s_d2[tid] = k.d2; s_i[tid] = k.i;
#pragma unroll
  for (int q = 0; q < 4; ++q) s_cnt[q][tid] = cnt[q];
  s_dep[0][tid] = dep[0]; s_dep[1][tid] = dep[1];
  __syncthreads();
  for (int w = T / 2; w > 0; w >>= 1) {
    if (tid < w) {
      const MinKey r = min_key(MinKey{s_d2[tid], s_i[tid]}, MinKey{s_d2[tid + w], s_i[tid + w]});
      s_d2[tid] = r.d2; s_i[tid] = r.i;
#pragma unroll
      for (int q = 0; q < 4; ++q) s_cnt[q][tid] += s_cnt[q][tid + w];
      s_dep[0][tid] = fmaxf(s_dep[0][tid], s_dep[0][tid + w]);
      s_dep[1][tid] = fmaxf(s_dep[1][tid], s_dep[1][tid + w]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int bi = s_i[0];
    float* sf = a.sum_f + (size_t)pair * CONTACT_SUM_F;
    int32_t* si = a.sum_i + (size_t)pair * CONTACT_SUM_I;
    sf[0] = s_d2[0]; sf[1] = s_dep[0][0]; sf[2] = s_dep[1][0]; sf[3] = 0.f;
    si[0] = bi;
    si[1] = bi >= 0 ? a.nn[(size_t)pair * 2 * a.n_verts + bi] : -1;
    si[2] = s_cnt[0][0]; si[3] = s_cnt[1][0]; si[4] = s_cnt[2][0]; si[5] = s_cnt[3][0];
  }
}

hipError_t launch_contact(const ContactArgs& a, hipStream_t s) {
  const ContactPlan p = contact_plan(a.n_meshes, a.n_verts, a.n_pairs);
  if (!p.ok) return hipErrorInvalidValue;
  hipLaunchKernelGGL(contact_setup_kernel, dim3(a.n_meshes), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(contact_pair_kernel, dim3(p.grid[0], p.grid[1], p.grid[2]), dim3(CONTACT_CHUNK), p.lds_bytes, s, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(contact_reduce_kernel, dim3(a.n_pairs), dim3(CONTACT_REDUCE_THREADS), 0, s, a);
  return hipGetLastError();
}

// acrmi_contact: the pairs of every row from the slot flags (contact_frame_pair), each mesh's topology (hand type = slot
// index) and sign; thread t < n_pairs writes pair t, thread t < n_meshes describes mesh t.
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
