// Mesh overlay: a batched triangle rasteriser (DESIGN.md "Rendering").  The reference draws the two MANO meshes over the
// frame with pyrender / pytorch3d (acr/visualization.py:108-218, acr/renderer/*); nothing of those is used here, only
// their conventions: the pinhole camera at cam_trans, visible_weight, the base colours.
//
//   render_setup_kernel  one block per mesh: project + snap the vertices to 1/256 pixel (through the frame's viewport, or the
//                        mesh's own: DESIGN.md "Views over regions"), vertex normals through the
//                        vertex->faces table (fixed summation order), one record per triangle (integer edge functions with
//                        the top-left rule folded into the constant, 1/Z and shade/Z at the vertices), its pixel box, and
//                        the mesh's pixel box.
//   render_tile_kernel   one 256-thread block per (16x16 pixel tile, frame): meshes of this frame whose box meets the tile
//                        -> their triangle boxes tested 256 at a time and compacted IN ORDER (ballot + mbcnt) into a list in
//                        LDS -> every thread walks the list for its own pixel: exact coverage in int64, fp32 depth (1/Z,
//                        larger wins, strict > so the lower global face id wins a tie), shade, blend, store.
//                        With a colour per vertex (RenderArgs::vcol) its second instantiation takes the
//                        base colour of a covered pixel from the three vertices of the winning triangle instead of rgb[mesh].
// The depth buffer is a register per pixel; there are no atomics on global memory, so the result is deterministic.
#include "kernels.h"
#include "region_view_plan.h"

#include <cstring>
#include <vector>

namespace acrmi {

namespace {

constexpr int TILE = 16;              // 16 x 16 pixels = one thread per pixel
constexpr int LIST_CAP = 1024;        // compacted face ids held in LDS between two flushes
constexpr float SNAP = 256.f;         // sub-pixel units per pixel
constexpr float SNAP_MAX = 4194304.f; // 2^22: largest snapped coordinate a triangle may carry
constexpr float Z_NEAR = 0.05f;       // metres; a triangle with a vertex at or in front of it is dropped whole
constexpr uint32_t NB_SWAPPED = 8u;   // TriRecord::nb

struct TriRecord {   // 80 bytes; edge k is the one OPPOSITE vertex k (its value / area = the barycentric weight of vertex k)
  int32_t A[3], B[3];
  int32_t c_lo[3], c_hi[3];   // C of A*x + B*y + C, MINUS 1 on the edges that do not own their pixels (top-left rule)
  uint32_t nb;                // bit k (0..2): edge k carries that -1; bit 3: vertices 1 and 2 are the face's in the blob SWAPPED
                              // (re-oriented to positive area) - read by the per-vertex colour path alone
  float inv_area;             // 1 / (twice the area, sub-pixel units squared)
  float iz[3], sz[3];         // 1/Z and shade/Z at the vertices
};
static_assert(sizeof(TriRecord) == 80, "TriRecord layout");

struct Box { short x0, x1, y0, y1; };   // inclusive pixel range; empty (x0 > x1) for a dropped triangle

__device__ inline int lane_rank(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
}

// Position of this thread among the threads of the block whose `pred` is set, in thread order (-1 when not set), and how
// many there are.  cnt: 2 x 4 ints in LDS, used alternately (`phase` flips per call), so that ONE barrier per call is enough:
// the barrier of call k+1 separates the reads of call k from the writes of call k+2.
__device__ inline int block_compact(bool pred, int (*cnt)[4], int& phase, int& total) {
  const unsigned long long mask = __ballot(pred);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) cnt[phase][wave] = __popcll(mask);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int c = cnt[phase][w];
    off += w < wave ? c : 0;
    tot += c;
  }
  phase ^= 1;
  total = tot;
  return pred ? off + lane_rank(mask) : -1;
}

}  // namespace

// ---- setup ------------------------------------------------------------------------------------------------------------
// LDS per vertex: snapped x, y (int), the depth value 1/Z (sx/Z with a per-mesh view; not > 0: the vertex cannot be drawn), shade.
__global__ __launch_bounds__(256) void render_setup_kernel(RenderArgs a) {
  extern __shared__ int s_dyn[];
  int* sx = s_dyn;
  int* sy = sx + a.n_verts;
  float* siz = (float*)(sy + a.n_verts);
  float* ssh = siz + a.n_verts;
  __shared__ int s_box[4];
  const int m = blockIdx.x, tid = threadIdx.x;
  int4* mesh_box = (int4*)a.ws;
  const int frame = a.mesh_frame[m];
  if (frame < 0 || frame >= a.n_frames) {      // not drawn: the tile kernel never looks at this mesh's records
    if (tid == 0) mesh_box[m] = make_int4(1, 0, 1, 0);
    return;
  }
  const int32_t* topo = (a.mesh_topo && a.mesh_topo[m] == 1 && a.topo[1]) ? a.topo[1] : a.topo[0];
  const int32_t* faces = topo + 2;
  const int32_t* row = faces + 3 * a.n_faces;
  const int32_t* col = row + a.n_verts + 1;
  const float* V = a.verts + (size_t)m * a.n_verts * 3;
  float tx = 0.f, ty = 0.f, tz = 0.f;
  if (a.trans) { tx = a.trans[m * 3]; ty = a.trans[m * 3 + 1]; tz = a.trans[m * 3 + 2]; }
  float vsx = 1.f, vsy = 1.f, vox = 0.f, voy = 0.f;
  // the viewport of the mesh's frame, or - views over regions - the mesh's own; with its own the depths of two cameras of
  // different scale are compared, so they are put into one virtual camera of the frame: sx / Z instead of 1 / Z
  float depth_num = 1.f;
  if (a.mesh_view) {
    vsx = a.mesh_view[m * 4]; vsy = a.mesh_view[m * 4 + 1]; vox = a.mesh_view[m * 4 + 2]; voy = a.mesh_view[m * 4 + 3];
    depth_num = vsx;
  } else if (a.view) {
    vsx = a.view[frame * 4]; vsy = a.view[frame * 4 + 1]; vox = a.view[frame * 4 + 2]; voy = a.view[frame * 4 + 3];
  }
  if (tid < 4) s_box[tid] = (tid & 1) ? -32768 : 32767;      // x0, x1, y0, y1
  for (int v = tid; v < a.n_verts; v += 256) {
    const float X = V[v * 3] + tx, Y = V[v * 3 + 1] + ty, Z = V[v * 3 + 2] + tz;
    // canvas (512) position, then the frame's viewport; every operation rounded on its own (-ffp-contract=off) so that
    // the restatement in tests/render_ref.py snaps to the same integers
    const float xc = 256.f + (a.focal * X) / Z, yc = 256.f + (a.focal * Y) / Z;
    const float xs = (xc * vsx + vox) * SNAP, ys = (yc * vsy + voy) * SNAP;
    const bool ok = Z > Z_NEAR && fabsf(xs) <= SNAP_MAX && fabsf(ys) <= SNAP_MAX;      // (false for NaN)
    sx[v] = ok ? (int)rintf(xs) : 0;
    sy[v] = ok ? (int)rintf(ys) : 0;
    siz[v] = ok ? depth_num / Z : -1.f;      // (not > 0, NaN included: the vertex is not drawn)
    // vertex normal: sum of the un-normalised face normals, in the table's order
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
    const float len = sqrtf(nx * nx + ny * ny + nz * nz);
    ssh[v] = 0.3f + 0.7f * (len > 0.f ? fabsf(nz) / len : 0.f);
  }
  __syncthreads();
  TriRecord* recs = (TriRecord*)(a.ws + a.ws_rec_off) + (size_t)m * a.n_faces;
  Box* boxes = (Box*)(a.ws + a.ws_box_off) + (size_t)m * a.n_faces;
  for (int f = tid; f < a.n_faces; f += 256) {
    int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    Box bx{32767, -32768, 32767, -32768};
    TriRecord r{};
    bool ok = siz[i0] > 0.f && siz[i1] > 0.f && siz[i2] > 0.f;
    if (ok) {
      long long area = (long long)(sx[i1] - sx[i0]) * (sy[i2] - sy[i0]) - (long long)(sy[i1] - sy[i0]) * (sx[i2] - sx[i0]);
      if (area < 0) { const int t = i1; i1 = i2; i2 = t; area = -area; r.nb = NB_SWAPPED; }
      ok = area != 0;
      if (ok) {
        const int vi[3] = {i0, i1, i2};
        const int x[3] = {sx[i0], sx[i1], sx[i2]}, y[3] = {sy[i0], sy[i1], sy[i2]};
        const int xmin = min(x[0], min(x[1], x[2])), xmax = max(x[0], max(x[1], x[2]));
        const int ymin = min(y[0], min(y[1], y[2])), ymax = max(y[0], max(y[1], y[2]));
        // pixel centres (256 i + 128) inside [min, max]
        const int px0 = (xmin + 127) >> 8, px1 = (xmax - 128) >> 8, py0 = (ymin + 127) >> 8, py1 = (ymax - 128) >> 8;
        ok = px0 <= px1 && py0 <= py1;
        if (ok) {
          bx = Box{(short)px0, (short)px1, (short)py0, (short)py1};
          for (int k = 0; k < 3; ++k) {      // edge k: from vertex k+1 to vertex k+2
            const int p = (k + 1) % 3, q = (k + 2) % 3;
            const int A = y[p] - y[q], B = x[q] - x[p];
            long long C = (long long)x[p] * y[q] - (long long)x[q] * y[p];
            const bool owns = A > 0 || (A == 0 && B > 0);      // left edge, or top edge: pixels ON it are inside
            if (!owns) { C -= 1; r.nb |= 1u << k; }
            r.A[k] = A; r.B[k] = B;
            r.c_lo[k] = (int32_t)(uint32_t)(unsigned long long)C;
            r.c_hi[k] = (int32_t)(C >> 32);
            r.iz[k] = siz[vi[k]];
            r.sz[k] = ssh[vi[k]] * siz[vi[k]];
          }
          r.inv_area = 1.f / (float)area;
          atomicMin(&s_box[0], px0); atomicMax(&s_box[1], px1);
          atomicMin(&s_box[2], py0); atomicMax(&s_box[3], py1);
        }
      }
    }
    recs[f] = r;
    boxes[f] = bx;
  }
  __syncthreads();
  if (tid == 0) mesh_box[m] = make_int4(s_box[0], s_box[1], s_box[2], s_box[3]);
}

// ---- tiles ------------------------------------------------------------------------------------------------------------
struct PixelState {
  float best;      // largest 1/Z so far
  int id;          // its global face id (-1: not covered)
  float shade;
};

__device__ inline void shade_list(const TriRecord* __restrict__ recs, const int* s_list, int n, int px, int py, PixelState& st) {
  for (int i = 0; i < n; ++i) {
    const int gid = __builtin_amdgcn_readfirstlane(s_list[i]);      // the same record for every thread: scalar loads
    const TriRecord& r = recs[gid];
    long long e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const long long C = (long long)(((unsigned long long)(uint32_t)r.c_hi[k] << 32) | (uint32_t)r.c_lo[k]);
      e[k] = (long long)r.A[k] * px + ((long long)r.B[k] * py + C);
    }
    if ((e[0] | e[1] | e[2]) >= 0) {
      const float b0 = (float)(e[0] + (r.nb & 1)) * r.inv_area, b1 = (float)(e[1] + ((r.nb >> 1) & 1)) * r.inv_area,
                  b2 = (float)(e[2] + ((r.nb >> 2) & 1)) * r.inv_area;
      const float d = b0 * r.iz[0] + b1 * r.iz[1] + b2 * r.iz[2];
      if (d > st.best) {
        st.best = d;
        st.id = gid;
        st.shade = (b0 * r.sz[0] + b1 * r.sz[1] + b2 * r.sz[2]) / d;
      }
    }
  }
}

// The base colour of a covered pixel from the colours of its visible triangle's vertices: the record's
// barycentrics recomputed for this pixel - the same operations in the same order as shade_list, so d is the depth value that won -
// and the face's three indices from the topology blob, vertices 1 and 2 exchanged when the record was re-oriented.
// Bounds: gid < n_meshes * n_faces names a record the setup kernel wrote for a drawn mesh; the indices come from a blob that
// acrmi_mesh_topology validated (each in [0, n_verts)), so vcol is read inside [n_meshes, n_verts, 3] whatever the colours hold.
__device__ inline void vertex_base_color(const RenderArgs& a, const TriRecord* __restrict__ recs, int gid, int px, int py, float* base) {
  const TriRecord& r = recs[gid];
  float b[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const long long C = (long long)(((unsigned long long)(uint32_t)r.c_hi[k] << 32) | (uint32_t)r.c_lo[k]);
    const long long e = (long long)r.A[k] * px + ((long long)r.B[k] * py + C);
    b[k] = (float)(e + ((r.nb >> k) & 1)) * r.inv_area;
  }
  const float w0 = b[0] * r.iz[0], w1 = b[1] * r.iz[1], w2 = b[2] * r.iz[2];
  const float d = (w0 + w1) + w2;
  const int mesh = gid / a.n_faces, f = gid - mesh * a.n_faces;
  const int32_t* topo = (a.mesh_topo && a.mesh_topo[mesh] == 1 && a.topo[1]) ? a.topo[1] : a.topo[0];
  const int32_t* face = topo + 2 + 3 * f;
  const bool swapped = (r.nb & NB_SWAPPED) != 0;
  const int i0 = face[0], i1 = swapped ? face[2] : face[1], i2 = swapped ? face[1] : face[2];
  const float* vc = a.vcol + (size_t)mesh * a.n_verts * 3;
  const float *c0 = vc + 3 * i0, *c1 = vc + 3 * i1, *c2 = vc + 3 * i2;
#pragma unroll
  for (int c = 0; c < 3; ++c) base[c] = ((w0 * c0[c] + w1 * c1[c]) + w2 * c2[c]) / d;
}

// COLOR: the base colour of a pixel comes from a.vcol (vertex_base_color) instead of a.rgb; everything else is the same code.
template <bool COLOR>
__global__ __launch_bounds__(256) void render_tile_kernel(RenderArgs a) {
  __shared__ int s_list[LIST_CAP];
  __shared__ int s_mesh[256];
  __shared__ int s_cnt[2][4];
  const int tid = threadIdx.x;
  const int tiles_x = (a.W + TILE - 1) / TILE;
  const int tile_x = blockIdx.x % tiles_x, tile_y = blockIdx.x / tiles_x, frame = blockIdx.y;
  const int x0 = tile_x * TILE, y0 = tile_y * TILE, x1 = x0 + TILE - 1, y1 = y0 + TILE - 1;
  const int ix = x0 + (tid & 15), iy = y0 + (tid >> 4);
  const bool in_image = ix < a.W && iy < a.H;
  const int px = ix * 256 + 128, py = iy * 256 + 128;
  const int4* mesh_box = (const int4*)a.ws;
  const TriRecord* recs = (const TriRecord*)(a.ws + a.ws_rec_off);
  const Box* boxes = (const Box*)(a.ws + a.ws_box_off);
  PixelState st{-1.f, -1, 0.f};
  int phase = 0, n_list = 0;
  for (int m0 = 0; m0 < a.n_meshes; m0 += 256) {
    const int m = m0 + tid;
    bool hit = false;
    if (m < a.n_meshes && a.mesh_frame[m] == frame) {
      const int4 b = mesh_box[m];
      hit = b.x <= x1 && b.y >= x0 && b.z <= y1 && b.w >= y0;
    }
    int n_hit;
    const int pos = block_compact(hit, s_cnt, phase, n_hit);
    if (n_hit == 0) continue;
    if (pos >= 0) s_mesh[pos] = m;
    __syncthreads();
    for (int j = 0; j < n_hit; ++j) {
      const int mesh = s_mesh[j];
      const Box* mb = boxes + (size_t)mesh * a.n_faces;
      for (int f0 = 0; f0 < a.n_faces; f0 += 256) {
        if (n_list + 256 > LIST_CAP) {      // (uniform) no room for another 256 candidates: shade what is there
          __syncthreads();
          shade_list(recs, s_list, n_list, px, py, st);
          __syncthreads();
          n_list = 0;
        }
        const int f = f0 + tid;
        bool cand = false;
        if (f < a.n_faces) {
          const Box b = mb[f];
          cand = b.x0 <= x1 && b.x1 >= x0 && b.y0 <= y1 && b.y1 >= y0;
        }
        int n_new;
        const int at = block_compact(cand, s_cnt, phase, n_new);
        if (at >= 0) s_list[n_list + at] = mesh * a.n_faces + f;
        n_list += n_new;
      }
    }
    __syncthreads();      // s_mesh is rewritten by the next 256 meshes
  }
  if (n_list) {
    __syncthreads();
    shade_list(recs, s_list, n_list, px, py, st);
  }
  if (!in_image) return;
  const size_t pix = ((size_t)frame * a.H + iy) * a.W + ix;
  if (a.ids_out) a.ids_out[pix] = st.id;
  const bool in_place = a.img_in == a.img_out;
  if (st.id < 0) {
    if (!in_place) {
      a.img_out[pix * 3] = a.img_in[pix * 3];
      a.img_out[pix * 3 + 1] = a.img_in[pix * 3 + 1];
      a.img_out[pix * 3 + 2] = a.img_in[pix * 3 + 2];
    }
    return;
  }
  float vbase[3];
  const float* rgb;
  if (COLOR) {
    vertex_base_color(a, recs, st.id, px, py, vbase);
    rgb = vbase;
  } else {
    rgb = a.rgb + (size_t)(st.id / a.n_faces) * 3;
  }
  const float w = a.visible_weight, iw = 1.f - w;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = floorf(((w * 255.f) * rgb[c]) * st.shade + iw * (float)a.img_in[pix * 3 + c]);
    a.img_out[pix * 3 + c] = (uint8_t)fminf(fmaxf(v, 0.f), 255.f);
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------
long long mesh_topology_ints(int n_faces, int n_verts) { return 2ll + 3ll * n_faces + (n_verts + 1ll) + 3ll * n_faces; }

// blob = [n_faces, n_verts | faces 3F | row V+1 | col 3F]: col[row[v] .. row[v+1]) = the faces that name vertex v, one entry
// per corner, by face and then by corner.  false: an index outside [0, n_verts).
bool build_mesh_topology(const int32_t* faces, int n_faces, int n_verts, int32_t* blob) {
  for (long long i = 0; i < 3ll * n_faces; ++i)
    if (faces[i] < 0 || faces[i] >= n_verts) return false;
  blob[0] = n_faces; blob[1] = n_verts;
  int32_t* bf = blob + 2;
  int32_t* row = bf + 3ll * n_faces;
  int32_t* col = row + n_verts + 1;
  std::memcpy(bf, faces, sizeof(int32_t) * 3 * (size_t)n_faces);
  std::memset(row, 0, sizeof(int32_t) * ((size_t)n_verts + 1));
  for (long long i = 0; i < 3ll * n_faces; ++i) row[faces[i] + 1]++;
  for (int v = 0; v < n_verts; ++v) row[v + 1] += row[v];
  std::vector<int32_t> fill(row, row + n_verts);
  for (int f = 0; f < n_faces; ++f)
    for (int k = 0; k < 3; ++k) col[fill[faces[3 * f + k]]++] = f;
  return true;
}

static size_t align256(size_t n) { return (n + 255) / 256 * 256; }

size_t render_workspace_bytes(int n_meshes, int n_faces) {
  return align256((size_t)n_meshes * sizeof(int4)) + align256((size_t)n_meshes * n_faces * sizeof(Box)) +
         (size_t)n_meshes * n_faces * sizeof(TriRecord);
}

hipError_t launch_render(const RenderArgs& a0, hipStream_t s) {
  RenderArgs a = a0;
  a.ws_box_off = align256((size_t)a.n_meshes * sizeof(int4));
  a.ws_rec_off = a.ws_box_off + align256((size_t)a.n_meshes * a.n_faces * sizeof(Box));
  hipLaunchKernelGGL(render_setup_kernel, dim3(a.n_meshes), dim3(256), (size_t)a.n_verts * 16, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int tiles = ((a.W + TILE - 1) / TILE) * ((a.H + TILE - 1) / TILE);
  if (a.vcol) hipLaunchKernelGGL(render_tile_kernel<true>, dim3(tiles, a.n_frames), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(render_tile_kernel<false>, dim3(tiles, a.n_frames), dim3(256), 0, s, a);
  return hipGetLastError();
}

// acrmi_render: flags and hand types from the slots, the viewport from the `offsets` rows (csrc/mano.hip pj2d -> pj2d_org)
__global__ void render_prep_kernel(const float* __restrict__ slots, const float* __restrict__ offsets, int B, int slot_stride,
                                   int flag_at, float r0, float g0, float b0, float r1, float g1, float b1,
                                   int32_t* __restrict__ mesh_frame, int32_t* __restrict__ mesh_topo, float* __restrict__ rgb,
                                   float* __restrict__ view) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= 2 * B) return;
  const int b = m >> 1, h = m & 1;
  mesh_frame[m] = slots[(size_t)m * slot_stride + flag_at] > 0.5f ? b : -1;
  mesh_topo[m] = h;
  rgb[m * 3] = h ? r1 : r0; rgb[m * 3 + 1] = h ? g1 : g0; rgb[m * 3 + 2] = h ? b1 : b0;
  if (h == 0 && view) {
    const float* of = offsets + (size_t)b * 10;
    region_view_row(of, view + b * 4);
  }
}

// acrmi_render_regions / acrmi_overlay_regions: mesh (hand) 2 i + h belongs to region i; it goes into the region's frame
// when its flag is set and the region draws (csrc/region_view_plan.h), and is mapped by its region's view.  mesh_topo, rgb
// and mesh_view may be null (the skeleton needs the frames only).
__global__ void render_region_prep_kernel(const float* __restrict__ slots, const float* __restrict__ offsets,
                                          const int32_t* __restrict__ region_frame, int n, int n_frames, int H, int W,
                                          int slot_stride, int flag_at, float r0, float g0, float b0, float r1, float g1,
                                          float b1, int32_t* __restrict__ mesh_frame, int32_t* __restrict__ mesh_topo,
                                          float* __restrict__ rgb, float* __restrict__ mesh_view) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= 2 * n) return;
  const int i = m >> 1, h = m & 1;
  const int frame = region_frame[i];
  const RegionView rv = region_view(offsets + (size_t)i * 10, frame, n_frames, H, W);
  mesh_frame[m] = (rv.draws && slots[(size_t)m * slot_stride + flag_at] > 0.5f) ? frame : -1;
  if (mesh_topo) mesh_topo[m] = h;
  if (rgb) { rgb[m * 3] = h ? r1 : r0; rgb[m * 3 + 1] = h ? g1 : g0; rgb[m * 3 + 2] = h ? b1 : b0; }
  if (mesh_view) { mesh_view[m * 4] = rv.sx; mesh_view[m * 4 + 1] = rv.sy; mesh_view[m * 4 + 2] = rv.ox; mesh_view[m * 4 + 3] = rv.oy; }
}

hipError_t launch_render_region_prep(const float* slots, const float* offsets, const int32_t* region_frame, int n, int n_frames,
                                     int H, int W, int slot_stride, int flag_at, const float* colors, int32_t* mesh_frame,
                                     int32_t* mesh_topo, float* rgb, float* mesh_view, hipStream_t s) {
  static const float kNone[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const float* c = colors ? colors : kNone;
  hipLaunchKernelGGL(render_region_prep_kernel, dim3((2 * n + 255) / 256), dim3(256), 0, s, slots, offsets, region_frame, n,
                     n_frames, H, W, slot_stride, flag_at, c[0], c[1], c[2], c[3], c[4], c[5], mesh_frame, mesh_topo, rgb,
                     mesh_view);
  return hipGetLastError();
}

hipError_t launch_render_prep(const float* slots, const float* offsets, int B, int slot_stride, int flag_at, const float* colors,
                              int32_t* mesh_frame, int32_t* mesh_topo, float* rgb, float* view, hipStream_t s) {
  hipLaunchKernelGGL(render_prep_kernel, dim3((2 * B + 255) / 256), dim3(256), 0, s, slots, offsets, B, slot_stride, flag_at,
                     colors[0], colors[1], colors[2], colors[3], colors[4], colors[5], mesh_frame, mesh_topo, rgb,
                     offsets ? view : nullptr);
  return hipGetLastError();
}

}  // namespace acrmi
