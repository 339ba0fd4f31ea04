// 1x1 stride-1 convolution in fp32 on the four-wave streaming frame of conv_x3p.inc (same item shape, same register-staged
// loads one chunk ahead, same one barrier per chunk, same wave-private epilogue) - included by conv_mfma.hip.  The pointwise
// layers of the batch-64 program (HRNet layer1's bottlenecks outside the fused pairs, transition / fuse projections) are
// HBM-bound in fp32 as long as Cin, Cout <= 256; the eight-wave direct kernel streamed them at ~4 TB/s, this frame at ~5.
//
// Item = 256 consecutive pixels of a frame's flattened map x NT n-tiles of 32 couts; wave w owns pixels 64 w .. 64 w + 63 (two
// slots of 32: lane = pixel, lane >> 5 = which of the two channel quads of an 8-channel step).  A 32-channel chunk: the 256
// threads load 256 x 32 floats (8 x 16 bytes each, coalesced: 8 threads = one pixel's 128 bytes), write them as fp32 planes
// [channel quad 8][pixel] of 16-byte entries (plane stride 258 = 2 mod 16: the 16 lanes of a ds_write_b128 - 2 pixels x 8
// quads - hit 16 different bank quads; window reads are consecutive entries) and re-request each entry for the chunk after
// the next one.  Per 8-channel step 8 NT v_mfma_f32_32x32x2_f32 from NT weight-fragment loads and 2 ds_read_b128.
// Takes: 1x1 stride 1, Cin % 32 == 0, Cout % 32 == 0, H W % 256 == 0; weights = packer.pack_conv (the direct kernels' fragments).

template <int NT>
__global__ __launch_bounds__(256, 1) void conv_p1_kernel(const ConvArgs a, const ConvWork wk) {
  constexpr int CK = 32, NE = 8;                   // channels per chunk; entries (pixel, channel quad) per thread and chunk
  constexpr int PS = 258;                          // entries (16 bytes) per plane
  constexpr int BUF = 8 * PS * 4;                  // floats per plane buffer
  static_assert(PS >= 256 && PS % 16 == 2, "plane geometry");
  constexpr int PTILE = 32 * 32;                   // parked tile [32 pixels][32 couts], 16-byte columns XOR-swizzled by pixel & 7
  extern __shared__ f32x4 smem4[];
  float* lds = reinterpret_cast<float*>(smem4);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* part = lds + 2 * BUF + wave * 2 * PTILE;   // the wave's private transposition area: one tile per slot
  const int nchunks = a.Cin / CK;                  // >= 1
  const int vb = virtual_block(a);
  const int my_items = wk.total > vb ? (wk.total - 1 - vb) / (int)gridDim.x + 1 : 0;
  const int ktotal = my_items * nchunks;
  const int li = lane & 31, kg = lane >> 5;
  // byte address (plane buffer 0) of the lane's pixel in the wave's first slot, plane of quad kg (step 0)
  const unsigned raddr = (unsigned)((kg * PS + 64 * wave + li) * 16);
  // ... and of the thread's first entry: quad tid & 7 of item pixel tid >> 3 (entry i: 32 pixels = 512 bytes further)
  const unsigned paddr = (unsigned)(((tid & 7) * PS + (tid >> 3)) * 16);
  // store side: lane = (pixel p8 of a group of 8, cout quad q8), four pixel groups gq per slot
  const int p8 = lane >> 3, q8 = lane & 7;
  const int lane_pix = 64 * wave + p8;
  const int lane_out = lane_pix * a.out_cs + 4 * q8, lane_res = lane_pix * a.res_cs + 4 * q8;
  const bool has_res = a.res != nullptr;
  const float floor_ = a.relu ? 0.f : -__builtin_inff();
  f32x16 acc[2][NT];
  unsigned pk_addr[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    pk_addr[q] = (unsigned)((2 * BUF + wave * 2 * PTILE + li * 32 + 4 * ((2 * q + kg) ^ (li & 7))) * 4);

  // ---- weights: [cin / 8][n-tile][lane 64][4]: 1 KiB fragments (packer.pack_conv of a 1x1 filter)
  const int step_b = a.n_tiles * 1024, tap_b = a.cin8 * step_b;       // bytes
  const __amdgpu_buffer_rsrc_t wrsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.groups * tap_b, 0x00020000);
  const unsigned wlane = lane * 16;
  auto wbase = [&](int w_item) -> int {
    const ItemPos ip = item_pos(wk, w_item);
    return ip.g * tap_b + ip.rest * NT * 1024;
  };
  f32x4 Aq[2][NT];             // [set][n]
  f32x4 Bv[2][2];              // [set][slot]
  f32x4 stage[NE];             // the thread's entries of the chunk after the current one
  auto load_A = [&](auto set_tag, int base, int step) {
    constexpr int S = decltype(set_tag)::value;
    const int so = base + (step < a.cin8 ? step : a.cin8 - 1) * step_b;
#pragma unroll
    for (int n = 0; n < NT; ++n)
      Aq[S][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane + (unsigned)(n * 1024), so, 0));
  };
  // the lane's two slot windows of 8-channel step st (0 .. 3) of the plane buffer at byte offset boff
  auto read_B = [&](auto set_tag, unsigned boff, int st) {
    constexpr int S = decltype(set_tag)::value;
    const char* p = reinterpret_cast<const char*>(lds) + (raddr + boff);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) Bv[S][s2] = *reinterpret_cast<const f32x4*>(p + ((2 * st * PS + 32 * s2) * 16));
  };
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  auto pk_add4 = [](const f32x4& b, const f32x4& c) -> f32x4 {
    f32x2 lo, hi;
    const f32x2 b0 = {b[0], b[1]}, b1 = {b[2], b[3]}, c0 = {c[0], c[1]}, c1 = {c[2], c[3]};
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(lo) : "v"(b0), "v"(c0));
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(hi) : "v"(b1), "v"(c1));
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
  };

  // ---- the activations through registers: entry i of thread t = quad t & 7 of item pixel (t >> 3) + 32 i
  int doff[NE];
#pragma unroll
  for (int i = 0; i < NE; ++i) doff[i] = (((tid >> 3) + 32 * i) * a.in_cs + 4 * (tid & 7)) * 4;
  __amdgpu_buffer_rsrc_t drsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in), 0, 0, 0x00020000);
  int wd = vb, cd0 = 0, kd = 0;     // load cursor: item, first channel and index of the next chunk to request
  auto cursor_enter = [&]() {
    if (cd0 == 0) {                 // (uniform) the cursor enters an item: descriptor at its first pixel
      const bool valid = kd < ktotal;
      const ItemPos ip = item_pos(wk, valid ? wd : vb);
      const long long org = (((long long)ip.b * a.H * a.W) + (long long)ip.ty * 256) * (long long)a.in_cs + a.in_coff + ip.g * a.Cin;
      // past the last item: zero records, every entry reads zeros
      drsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in + org), 0, valid ? 0x7ffffff0 : 0, 0x00020000);
    }
  };
  auto cursor_leave = [&]() {
    cd0 += CK;
    if (cd0 >= a.Cin) { cd0 = 0; wd += (int)gridDim.x; }
    ++kd;
  };
  auto stage_entry = [&](int i) {
    stage[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(drsrc, doff[i], cd0 * 4, 0));
  };
  // entry i of the staged chunk into the plane buffer at byte offset boff
  auto plane_store = [&](int i, unsigned boff) {
    *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(lds) + (paddr + boff) + i * 512) = stage[i];
  };

  // ---- prologue: chunk 0 into plane buffer 0, chunk 1 staged, the first step's fragments and windows
  int w = vb, c0 = 0, k = 0;
  int wsc = wbase(w);
  cursor_enter();
#pragma unroll
  for (int i = 0; i < NE; ++i) stage_entry(i);
  cursor_leave();
  load_A(std::integral_constant<int, 0>(), wsc, 0);
#pragma unroll
  for (int i = 0; i < NE; ++i) plane_store(i, 0u);
  cursor_enter();
#pragma unroll
  for (int i = 0; i < NE; ++i) stage_entry(i);
  cursor_leave();
  __syncthreads();
  read_B(std::integral_constant<int, 0>(), 0u, 0);

  // One chunk = 4 steps of 8 channels; step j works on set j & 1 and prepares the other one.  Steps 0 .. 2 also move the staged
  // chunk k + 1 into the other plane buffer and re-request each entry (chunk k + 2) as soon as it is written; step 3 starts
  // with the chunk barrier (the planes of chunk k + 1 are complete, every wave has read the last window of chunk k).
  auto chunk = [&](auto first_tag, auto last_tag) {
    constexpr bool FIRST = decltype(first_tag)::value, LAST = decltype(last_tag)::value;
    const unsigned boff = (unsigned)((k & 1) * BUF * 4), boff_n = (unsigned)(((k + 1) & 1) * BUF * 4);
    const int nw = LAST ? w + (int)gridDim.x : w;
    const bool more = k + 1 < ktotal;
    const int wsn = (LAST && more) ? wbase(nw) : wsc;
    const int s0 = c0 / 8;
    auto mfmas = [&](auto set_tag, auto zero_tag) {
      constexpr int S = decltype(set_tag)::value;
      constexpr bool ZERO = decltype(zero_tag)::value;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            if (ZERO && j == 0) {
              const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
              acc[s2][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(Aq[S][n][j], Bv[S][s2][j], zero, 0, 0, 0);
            } else {
              acc[s2][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(Aq[S][n][j], Bv[S][s2][j], acc[s2][n], 0, 0, 0);
            }
          }
    };
    cursor_enter();
    // ---- step 0
    load_A(std::integral_constant<int, 1>(), wsc, s0 + 1);
    read_B(std::integral_constant<int, 1>(), boff, 1);
    if (FIRST) mfmas(std::integral_constant<int, 0>(), std::true_type());
    else mfmas(std::integral_constant<int, 0>(), std::false_type());
#pragma unroll
    for (int i = 0; i < 3; ++i) { plane_store(i, boff_n); stage_entry(i); }
    // ---- step 1
    load_A(std::integral_constant<int, 0>(), wsc, s0 + 2);
    read_B(std::integral_constant<int, 0>(), boff, 2);
    mfmas(std::integral_constant<int, 1>(), std::false_type());
#pragma unroll
    for (int i = 3; i < 6; ++i) { plane_store(i, boff_n); stage_entry(i); }
    // ---- step 2
    load_A(std::integral_constant<int, 1>(), wsc, s0 + 3);
    read_B(std::integral_constant<int, 1>(), boff, 3);
    mfmas(std::integral_constant<int, 0>(), std::false_type());
#pragma unroll
    for (int i = 6; i < NE; ++i) { plane_store(i, boff_n); stage_entry(i); }
    cursor_leave();
    // LAST: the first n-tile's bias and residual before the last step's MFMAs
    int rest = 0;
    float* out_tile = nullptr;
    __amdgpu_buffer_rsrc_t rrsrc = wrsrc, brsrc = wrsrc;
    f32x4 rv[NT][2][4], bvv[NT];
    auto request_res = [&](int n) {
      const int nt = rest * NT + n;
      bvv[n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(brsrc, 16 * q8, nt * 128, 0));
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
          rv[n][s2][gq] = __builtin_bit_cast(
              f32x4, __builtin_amdgcn_raw_buffer_load_b128(rrsrc, lane_res * 4, (nt * 32 + (32 * s2 + 8 * gq) * a.res_cs) * 4,
                                                           RES_CACHE_WINO));
    };
    if (LAST) {
      const ItemPos ip = item_pos(wk, w);
      const int g = ip.g, b = ip.b;
      rest = ip.rest;
      const float* bias = a.bias + (size_t)g * a.n_tiles * 32 + (size_t)b * a.bias_fstride;
      const int tile_pix = ip.ty * 256;
      out_tile = a.out + (size_t)b * a.Ho * a.Wo * a.out_cs + a.out_coff + g * a.Cout + (size_t)tile_pix * a.out_cs;
      const size_t res_off = (res_frame_off(a, b) + (size_t)tile_pix * a.res_cs) + a.res_coff + g * a.Cout;
      const size_t res_left = has_res ? (res_total(a) - res_off) * 4 : 0;
      rrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(has_res ? a.res + res_off : a.in), 0,
                                                (int)(unsigned)(res_left > 0xffffffffu ? 0xffffffffu : res_left), 0x00020000);
      brsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bias), 0, bias_row_left(a, g), 0x00020000);
      request_res(0);
    }
    // ---- step 3
    __syncthreads();
    load_A(std::integral_constant<int, 0>(), wsn, LAST ? 0 : s0 + 4);
    read_B(std::integral_constant<int, 0>(), boff_n, 0);
    mfmas(std::integral_constant<int, 1>(), std::false_type());

    if (LAST) {
      auto park = [&](auto ti_tag, const f32x16& x) {
        constexpr int TI = decltype(ti_tag)::value;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 v4 = {x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]};
          const unsigned ad = pk_addr[q];
          asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(ad), "a"(v4), "n"(TI * PTILE * 4) : "memory");
        }
      };
      // (the asm writes are invisible to hipcc's hazard recognizer: the last MFMA's passes drain here)
      asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
      if (NT == 2) request_res(NT - 1);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int nt = rest * NT + n;
        const f32x4 bv = bvv[n];
        __builtin_amdgcn_sched_barrier(0);
        park(std::integral_constant<int, 0>(), acc[0][n]);
        park(std::integral_constant<int, 1>(), acc[1][n]);
        asm volatile("s_nop 1" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        // (the wave's own LDS operations execute in order: the reads below see the tiles)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) {
            f32x4 o4 = *reinterpret_cast<const f32x4*>(part + s2 * PTILE + (8 * gq + p8) * 32 + 4 * (q8 ^ p8));
            o4 = pk_add4(pk_add4(o4, bv), rv[n][s2][gq]);
#pragma unroll
            for (int e = 0; e < 4; ++e) o4[e] = vmax1(o4[e], floor_);
            char* ub = reinterpret_cast<char*>(out_tile + nt * 32 + (32 * s2 + 8 * gq) * a.out_cs);   // uniform base
            __builtin_nontemporal_store(o4, reinterpret_cast<f32x4*>(ub + (unsigned)(lane_out * 4)));
          }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    wsc = wsn;
    c0 = LAST ? 0 : c0 + CK;
    w = nw;
    ++k;
  };
  if (nchunks == 1) {
    for (int item = 0; item < my_items; ++item) chunk(std::true_type(), std::true_type());
  } else {
    for (int item = 0; item < my_items; ++item) {
      chunk(std::true_type(), std::false_type());
      for (int ci = 2; ci < nchunks; ++ci) chunk(std::false_type(), std::false_type());
      chunk(std::false_type(), std::true_type());
    }
  }
}

static bool p1_ok(const ConvArgs& a) { return a.algo == 0 && takes_p1(conv_shape(a)); }

static hipError_t launch_p1_impl(const ConvArgs& a, hipStream_t s, int NT, const ConvKernel& k) {
  constexpr size_t lds = (2 * (size_t)8 * 258 * 4 + 4 * 2 * (size_t)32 * 32) * sizeof(float);
  return launch_conv_kernel(k, 256, lds, 1, (a.Ho * a.Wo) / 256, (a.Cout / 32) / NT, a, s);
}
static hipError_t launch_p1(const ConvArgs& a, hipStream_t s) {
  return a.Cout % 64 == 0 ? launch_p1_impl(a, s, 2, CONV_KERNEL(conv_p1_kernel<2>)) : launch_p1_impl(a, s, 1, CONV_KERNEL(conv_p1_kernel<1>));
}
