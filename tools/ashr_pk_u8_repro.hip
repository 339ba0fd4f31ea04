// Why put_byte of csrc/nv12_out.hip hides its value behind an empty asm: a minimal reproducer.
//   hipcc --offload-arch=gfx950 -O3 tools/ashr_pk_u8_repro.hip -o ashr_pk_u8_repro && ./ashr_pk_u8_repro
//   hipcc --offload-arch=gfx950 -O3 -S --cuda-device-only tools/ashr_pk_u8_repro.hip -o - | grep -A8 v_ashr_pk_u8_i32
// With HIP 7.2.26015 / AMD clang 22.0.0git (roc-7.2.0) the kernel below becomes
//   v_ashr_pk_u8_i32 v2, v2, v3, 20      ; bytes 0 and 1: shift, clamp, pack
//   v_or3_b32 v1, v2, v3, v1             ; bytes 2 and 3 ORed over it, as if bits 31:16 of v2 were zero
// and on an MI355X the words the same pattern stored from nv12_out.hip had bytes 0 and 1 right and extra bits set in bytes 2
// and 3.  The program prints how many of its words differ from the host's; when it prints 0 with the compiler in use, the
// empty asm in put_byte may go.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

__host__ __device__ inline int c8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__host__ __device__ inline unsigned pack(const int* a) {
  return (unsigned)c8(a[0] >> 20) | (unsigned)c8(a[1] >> 20) << 8 | (unsigned)c8(a[2] >> 20) << 16 | (unsigned)c8(a[3] >> 20) << 24;
}

__global__ void pack4(const int* a, unsigned* o) { o[threadIdx.x] = pack(a + 4 * threadIdx.x); }

int main() {
  const int n = 256;
  std::vector<int> a(4 * n);
  unsigned x = 12345u;
  for (int& v : a) {
    x = x * 1664525u + 1013904223u;
    v = (int)(x >> 3) - (1 << 27);      // shifted by 20: about -128 .. 383, both clamps and the range between
  }
  int* da;
  unsigned* dout;
  if (hipMalloc(&da, a.size() * sizeof(int)) != hipSuccess || hipMalloc(&dout, n * sizeof(unsigned)) != hipSuccess) return 2;
  if (hipMemcpy(da, a.data(), a.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return 2;
  hipLaunchKernelGGL(pack4, dim3(1), dim3(n), 0, 0, da, dout);
  std::vector<unsigned> o(n);
  if (hipMemcpy(o.data(), dout, n * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) return 2;
  int wrong = 0, wrong_low = 0;
  for (int i = 0; i < n; ++i) {
    const unsigned want = pack(&a[4 * i]);
    wrong += o[i] != want;
    wrong_low += (o[i] & 0xffffu) != (want & 0xffffu);
  }
  std::printf("words that differ from the host's: %d of %d (of those, with a wrong low half: %d)\n", wrong, n, wrong_low);
  (void)hipFree(da);
  (void)hipFree(dout);
  return 0;
}
