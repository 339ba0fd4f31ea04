// NV12 video surfaces as the OUTPUT (DESIGN.md "NV12 output"): packed RGB / BGR frames -> a pitched Y plane and a pitched plane of
// interleaved U, V bytes, what a hardware encoder takes.  The rule is integer and stated once in csrc/nv12_out_plan.h (one 2x2
// block: four luma bytes from their own pixels, one U, V pair from the mean of the block); tests/nv12_out_ref.py is its numpy
// statement and the tests require equality.
//
// Two kernels, both pure streaming (3 bytes in and 1.5 out per pixel; compose 4.5 in and 1.5 out), no LDS, no atomics, nothing
// exchanged between lanes: a thread owns whole 2x2 blocks, reads what they need and writes them.
//   rgb_to_nv12_kernel   the plain conversion of a whole frame
//   nv12_compose_kernel  the drawn frame over its source surface: new bytes only where the drawn frame differs from what the
//                        input rule (nv12_pixel, csrc/kernels.h) makes of the source, the source's own bytes elsewhere
// blockIdx.y = the frame, its geometry by value in the arguments; the units of a frame in a grid-stride loop (the frames of a
// launch may differ in size).
//
// The wide path: a unit is two rows of eight pixels (four blocks) - 2 x 24 bytes in as three 8-byte words a row, two 8-byte Y
// stores and one 8-byte UV store (compose: two 8-byte Y loads and one 8-byte UV load more); adjacent lanes touch adjacent
// words.  A frame takes it when W is a multiple of 8 and every plane's base and pitch are multiples of 8, which the kernel
// works out from its arguments (uniform over the block).  Any other frame goes block by block with byte accesses: the same
// functions on the same integers, so the same bytes.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace acrmi {

namespace {

__device__ inline bool aligned8(const void* p, int pitch) { return (((uintptr_t)p | (uintptr_t)(unsigned)pitch) & 7) == 0; }

// byte j of a row of 24 held as three little-endian 8-byte words
__device__ inline int byte_of(const uint2 (&q)[3], int j) {
  const unsigned w = (j & 4) ? q[j >> 3].y : q[j >> 3].x;
  return (int)((w >> ((j & 3) * 8)) & 255u);
}

// pixel px (0..7) of such a row -> (R, G, B)
__device__ inline void triple_of(const uint2 (&q)[3], int px, int bgr, int* rgb) {
  const int c0 = byte_of(q, 3 * px), c1 = byte_of(q, 3 * px + 1), c2 = byte_of(q, 3 * px + 2);
  rgb[0] = bgr ? c2 : c0;
  rgb[1] = c1;
  rgb[2] = bgr ? c0 : c2;
}

__device__ inline void triple_at(const uint8_t* p, int bgr, int* rgb) {
  const int c0 = p[0], c1 = p[1], c2 = p[2];
  rgb[0] = bgr ? c2 : c0;
  rgb[1] = c1;
  rgb[2] = bgr ? c0 : c2;
}

// byte j (0..7) of an 8-byte word that starts as zero.  The empty asm hides where v came from.  Without it hipcc (HIP 7.2.26015,
// AMD clang 22.0.0git roc-7.2.0) fuses the shift, the clamp and the packing of two neighbouring bytes into v_ashr_pk_u8_i32 and
// ORs the other two bytes over its result (v_or3_b32) as if bits 31:16 of that result were zero; on gfx950 they are not, and
// bytes 2 and 3 of the stored word carry extra bits while bytes 0 and 1 are right.  tools/ashr_pk_u8_repro.hip reproduces it in
// one small kernel; when it prints 0 with the compiler in use, this asm may go.
__device__ inline void put_byte(uint2& w, int j, int v) {
  asm volatile("" : "+v"(v));
  if (j & 4) w.y |= (unsigned)v << ((j & 3) * 8);
  else w.x |= (unsigned)v << ((j & 3) * 8);
}

}  // namespace

__global__ __launch_bounds__(256) void rgb_to_nv12_kernel(const Nv12OutBatch pb, const Nv12OutCoef k, int bgr) {
  const int f = blockIdx.y;
  const int H = pb.f[f].H, W = pb.f[f].W;
  const size_t y_pitch = (size_t)pb.f[f].y_pitch, uv_pitch = (size_t)pb.f[f].uv_pitch;
  const uint8_t* __restrict__ src = pb.f[f].src;
  uint8_t* __restrict__ yp = pb.f[f].y;
  uint8_t* __restrict__ uvp = pb.f[f].uv;
  const bool wide = !(W & 7) && aligned8(src, 0) && aligned8(yp, pb.f[f].y_pitch) && aligned8(uvp, pb.f[f].uv_pitch);
  if (wide) {
    const int cw = W >> 3;
    const long units = (long)(H >> 1) * cw;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < units; i += (long)gridDim.x * 256) {
      const int cx = (int)(i % cw), by = (int)(i / cw);
      uint2 q[2][3];
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        const uint2* s = reinterpret_cast<const uint2*>(src + ((size_t)(2 * by + dy) * W + 8 * cx) * 3);
        q[dy][0] = s[0]; q[dy][1] = s[1]; q[dy][2] = s[2];
      }
      uint2 yw[2] = {make_uint2(0, 0), make_uint2(0, 0)}, uvw = make_uint2(0, 0);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        int rgb[4][3], y[4], U, V;
#pragma unroll
        for (int p = 0; p < 4; ++p) triple_of(q[p >> 1], 2 * b + (p & 1), bgr, rgb[p]);
        nv12_out_block(k, rgb, y, &U, &V);
#pragma unroll
        for (int p = 0; p < 4; ++p) put_byte(yw[p >> 1], 2 * b + (p & 1), y[p]);
        put_byte(uvw, 2 * b, U);
        put_byte(uvw, 2 * b + 1, V);
      }
      *reinterpret_cast<uint2*>(yp + (size_t)(2 * by) * y_pitch + 8 * cx) = yw[0];
      *reinterpret_cast<uint2*>(yp + (size_t)(2 * by + 1) * y_pitch + 8 * cx) = yw[1];
      *reinterpret_cast<uint2*>(uvp + (size_t)by * uv_pitch + 8 * cx) = uvw;
    }
    return;
  }
  const int bw = W >> 1;
  const long units = (long)(H >> 1) * bw;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < units; i += (long)gridDim.x * 256) {
    const int bx = (int)(i % bw), by = (int)(i / bw);
    int rgb[4][3], y[4], U, V;
#pragma unroll
    for (int p = 0; p < 4; ++p) triple_at(src + ((size_t)(2 * by + (p >> 1)) * W + 2 * bx + (p & 1)) * 3, bgr, rgb[p]);
    nv12_out_block(k, rgb, y, &U, &V);
#pragma unroll
    for (int p = 0; p < 4; ++p) yp[(size_t)(2 * by + (p >> 1)) * y_pitch + 2 * bx + (p & 1)] = (uint8_t)y[p];
    uint8_t* c = uvp + (size_t)by * uv_pitch + 2 * bx;
    c[0] = (uint8_t)U;
    c[1] = (uint8_t)V;
  }
}

// (no __restrict__ on the planes: the output may be the source surface)
__global__ __launch_bounds__(256) void nv12_compose_kernel(const Nv12ComposeBatch pb, const Nv12Coef k6, const Nv12OutCoef k, int bgr) {
  const int f = blockIdx.y;
  const int H = pb.f[f].H, W = pb.f[f].W;
  const size_t sy_pitch = (size_t)pb.f[f].src_y_pitch, suv_pitch = (size_t)pb.f[f].src_uv_pitch;
  const size_t y_pitch = (size_t)pb.f[f].y_pitch, uv_pitch = (size_t)pb.f[f].uv_pitch;
  const uint8_t* syp = pb.f[f].src_y;
  const uint8_t* suvp = pb.f[f].src_uv;
  const uint8_t* drawn = pb.f[f].drawn;
  uint8_t* yp = pb.f[f].y;
  uint8_t* uvp = pb.f[f].uv;
  const bool wide = !(W & 7) && aligned8(drawn, 0) && aligned8(syp, pb.f[f].src_y_pitch) && aligned8(suvp, pb.f[f].src_uv_pitch) &&
                    aligned8(yp, pb.f[f].y_pitch) && aligned8(uvp, pb.f[f].uv_pitch);
  if (wide) {
    const int cw = W >> 3;
    const long units = (long)(H >> 1) * cw;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < units; i += (long)gridDim.x * 256) {
      const int cx = (int)(i % cw), by = (int)(i / cw);
      uint2 q[2][3], sy[2];
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        const uint2* s = reinterpret_cast<const uint2*>(drawn + ((size_t)(2 * by + dy) * W + 8 * cx) * 3);
        q[dy][0] = s[0]; q[dy][1] = s[1]; q[dy][2] = s[2];
        sy[dy] = *reinterpret_cast<const uint2*>(syp + (size_t)(2 * by + dy) * sy_pitch + 8 * cx);
      }
      const uint2 suv = *reinterpret_cast<const uint2*>(suvp + (size_t)by * suv_pitch + 8 * cx);
      uint2 yw[2] = {make_uint2(0, 0), make_uint2(0, 0)}, uvw = make_uint2(0, 0);
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const unsigned pair = ((b & 2) ? suv.y : suv.x) >> ((b & 1) * 16);
        const int sU = (int)(pair & 255u), sV = (int)((pair >> 8) & 255u);
        int rgb[4][3], shown[4][3], srcy[4], y[4], U, V;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int px = 2 * b + (p & 1);
          triple_of(q[p >> 1], px, bgr, rgb[p]);
          const unsigned w = (px & 4) ? sy[p >> 1].y : sy[p >> 1].x;
          srcy[p] = (int)((w >> ((px & 3) * 8)) & 255u);
          nv12_pixel(k6, srcy[p], sU, sV, shown[p][0], shown[p][1], shown[p][2]);
        }
        nv12_out_compose_block(k, rgb, shown, srcy, sU, sV, y, &U, &V);
#pragma unroll
        for (int p = 0; p < 4; ++p) put_byte(yw[p >> 1], 2 * b + (p & 1), y[p]);
        put_byte(uvw, 2 * b, U);
        put_byte(uvw, 2 * b + 1, V);
      }
      *reinterpret_cast<uint2*>(yp + (size_t)(2 * by) * y_pitch + 8 * cx) = yw[0];
      *reinterpret_cast<uint2*>(yp + (size_t)(2 * by + 1) * y_pitch + 8 * cx) = yw[1];
      *reinterpret_cast<uint2*>(uvp + (size_t)by * uv_pitch + 8 * cx) = uvw;
    }
    return;
  }
  const int bw = W >> 1;
  const long units = (long)(H >> 1) * bw;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < units; i += (long)gridDim.x * 256) {
    const int bx = (int)(i % bw), by = (int)(i / bw);
    const uint8_t* sc = suvp + (size_t)by * suv_pitch + 2 * bx;
    const int sU = sc[0], sV = sc[1];
    int rgb[4][3], shown[4][3], srcy[4], y[4], U, V;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int row = 2 * by + (p >> 1), col = 2 * bx + (p & 1);
      triple_at(drawn + ((size_t)row * W + col) * 3, bgr, rgb[p]);
      srcy[p] = syp[(size_t)row * sy_pitch + col];
      nv12_pixel(k6, srcy[p], sU, sV, shown[p][0], shown[p][1], shown[p][2]);
    }
    nv12_out_compose_block(k, rgb, shown, srcy, sU, sV, y, &U, &V);      // (every source byte of the block has been read)
#pragma unroll
    for (int p = 0; p < 4; ++p) yp[(size_t)(2 * by + (p >> 1)) * y_pitch + 2 * bx + (p & 1)] = (uint8_t)y[p];
    uint8_t* c = uvp + (size_t)by * uv_pitch + 2 * bx;
    c[0] = (uint8_t)U;
    c[1] = (uint8_t)V;
  }
}

namespace {

// the grid of a launch: enough blocks for the frame with the most units, the rest of a frame in the grid-stride loop
template <class Batch>
unsigned grid_x(const Batch& pb, int n) {
  long most = 1;
  for (int i = 0; i < n; ++i) {
    const long u = (long)(pb.f[i].H >> 1) * ((pb.f[i].W & 7) ? pb.f[i].W >> 1 : pb.f[i].W >> 3);
    if (u > most) most = u;
  }
  const long g = (most + 255) / 256;
  return (unsigned)(g > 1024 ? 1024 : g);
}

}  // namespace

hipError_t launch_rgb_to_nv12(const Nv12OutBatch& pb, const Nv12OutCoef& k, int n, int bgr, hipStream_t s) {
  hipLaunchKernelGGL(rgb_to_nv12_kernel, dim3(grid_x(pb, n), (unsigned)n), dim3(256), 0, s, pb, k, bgr);
  return hipGetLastError();
}

hipError_t launch_nv12_compose(const Nv12ComposeBatch& pb, const Nv12Coef& k6, const Nv12OutCoef& k10, int n, int bgr, hipStream_t s) {
  hipLaunchKernelGGL(nv12_compose_kernel, dim3(grid_x(pb, n), (unsigned)n), dim3(256), 0, s, pb, k6, k10, bgr);
  return hipGetLastError();
}

}  // namespace acrmi
