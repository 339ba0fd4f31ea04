// 1x1 stride-1 convolution with SPLIT fp32 operands on the 16-bit matrix pipe - included by conv_mfma.hip behind
// conv_x3.inc, whose scheme it shares (x = hi + lo in f16 / bf16, three products per MAC on v_mfma_f32_32x32x16, fp32
// accumulation, fp32 tensors in HBM, weights split and scaled by the packer, every activation split once by the loader threads).
// A pointwise convolution in fp32 is matrix-bound wherever Cin and Cout are large (ResNet-50's bottlenecks, HRNet's fuse
// projections: 2 Cin Cout / 157 TF per pixel against 4 (Cin + Cout) bytes / 5 TB/s); on the 16-bit pipe it is HBM-bound.
//
// Item = 256 consecutive pixels of the flattened [H W] map of one frame (H W % 256 == 0) x NT n-tiles of 32 couts; wave w
// owns pixels 64 w .. 64 w + 63 (two slots of 32: lane = pixel, k-group kg = lane >> 5 holds channels 8 kg .. 8 kg + 7 of a
// 16-channel step).  A 32-channel chunk: the 256 threads load its 256 x 32 fp32 values (4 x 2 buffer loads each, one chunk
// ahead, re-issued as soon as an entry is split), split them and write f16 planes [channel octet 4][hi | lo][pixel] of 16-byte
// entries (plane stride 258 = 2 mod 8: conflict-free 16-byte writes, window reads are consecutive entries); per 16-channel
// step 6 NT MFMAs from 2 NT weight-fragment loads and 4 ds_read_b128; one barrier per chunk; epilogue as conv_x3_kernel.
// Takes: 1x1 stride 1, Cin % 32 == 0, Cout % 32 == 0 (two n-tiles per wave when % 64), H W % 256 == 0, fp32 storage.

template <int NT, bool BF = false>
__global__ __launch_bounds__(256, 1) void conv_x3p_kernel(const ConvArgs a, const ConvWork wk) {
  using h16x8 = typename std::conditional<BF, bf16x8, acrmi::h16x8>::type;
  using h16x2 = typename std::conditional<BF, bf16x2, acrmi::h16x2>::type;
  constexpr int CK = 32, NE = 4;                   // channels per chunk; entries (pixel, channel octet) per thread and chunk
  constexpr int PS = 258, PS2 = 2 * PS;            // entries (16 bytes) per plane / per hi + lo pair of planes
  constexpr int BUF = 4 * PS2 * 4;                 // floats per plane buffer
  static_assert(PS >= 256 && PS % 8 == 2, "plane geometry");
  constexpr int PTILE = 32 * 32;                   // parked tile [32 pixels][32 couts], 16-byte columns XOR-swizzled by pixel & 7
  extern __shared__ f32x4 smem4[];
  float* lds = reinterpret_cast<float*>(smem4);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* part = lds + 2 * BUF + wave * 2 * PTILE;   // the wave's private transposition area: one tile per slot
  const int nchunks = a.Cin / CK;                  // >= 1
  const int ksteps = a.Cin / 16;
  const int vb = virtual_block(a);
  const int my_items = wk.total > vb ? (wk.total - 1 - vb) / (int)gridDim.x + 1 : 0;
  const int ktotal = my_items * nchunks;
  const int li = lane & 31, kg = lane >> 5;
  // byte address (plane buffer 0) of the lane's pixel in the wave's first slot, hi plane of octet kg (step 0)
  const unsigned raddr = (unsigned)((kg * PS2 + 64 * wave + li) * 16);
  // ... and of the thread's first entry: octet tid & 3 of item pixel tid >> 2 (entry i: 64 pixels = 1 KiB further)
  const unsigned paddr = (unsigned)(((tid & 3) * PS2 + (tid >> 2)) * 16);
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

  // ---- weights: [cin / 16][n-tile][hi | lo][lane 64][8 halves]: 1 KiB fragments (packer.pack_conv_x3 of a 1x1 filter)
  const int step_b = a.n_tiles * 2048, tap_b = ksteps * step_b;       // bytes
  const __amdgpu_buffer_rsrc_t wrsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.groups * tap_b, 0x00020000);
  const unsigned wlane = lane * 16;
  const float wscale = a.w[(size_t)a.groups * (tap_b / 4)];      // 2^-S of the packer's weight scale
  const float __attribute__((ext_vector_type(2))) wsp = {wscale, wscale};
  auto wbase = [&](int w_item) -> int {
    const ItemPos ip = item_pos(wk, w_item);
    return ip.g * tap_b + ip.rest * NT * 2048;
  };
  f32x4 Aq[2][NT][2];          // [set][n][hi | lo]
  h16x8 Bh[2][2], Bl[2][2];    // [set][slot]
  f32x4 stage[NE][2];          // the thread's entries of the chunk after the current one, fp32
  auto load_A = [&](auto set_tag, int base, int step) {
    constexpr int S = decltype(set_tag)::value;
    const int so = base + (step < ksteps ? step : ksteps - 1) * step_b;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int hl = 0; hl < 2; ++hl)
        Aq[S][n][hl] = __builtin_bit_cast(
            f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane + (unsigned)(n * 2048 + hl * 1024), so, 0));
  };
  auto read_B = [&](auto set_tag, unsigned boff, int st) {
    constexpr int S = decltype(set_tag)::value;
    const char* p = reinterpret_cast<const char*>(lds) + (raddr + boff);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      Bh[S][s2] = *reinterpret_cast<const h16x8*>(p + ((2 * st * PS2 + 32 * s2) * 16));
      Bl[S][s2] = *reinterpret_cast<const h16x8*>(p + ((2 * st * PS2 + PS + 32 * s2) * 16));
    }
  };
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  auto pk_fma4 = [](f32x2 m, const f32x4& b, const f32x4& c) -> f32x4 {   // m * b + c
    f32x2 lo, hi;
    const f32x2 b0 = {b[0], b[1]}, b1 = {b[2], b[3]}, c0 = {c[0], c[1]}, c1 = {c[2], c[3]};
    asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(lo) : "v"(m), "v"(b0), "v"(c0));
    asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(hi) : "v"(m), "v"(b1), "v"(c1));
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
  };
  auto pk_add4 = [](const f32x4& b, const f32x4& c) -> f32x4 {
    f32x2 lo, hi;
    const f32x2 b0 = {b[0], b[1]}, b1 = {b[2], b[3]}, c0 = {c[0], c[1]}, c1 = {c[2], c[3]};
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(lo) : "v"(b0), "v"(c0));
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(hi) : "v"(b1), "v"(c1));
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
  };

  // ---- the activations through registers: entry i of thread t = octet t & 3 of item pixel (t >> 2) + 64 i
  int doff[NE];
#pragma unroll
  for (int i = 0; i < NE; ++i) doff[i] = (((tid >> 2) + 64 * i) * a.in_cs + 8 * (tid & 3)) * 4;
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
#pragma unroll
    for (int h = 0; h < 2; ++h)
      stage[i][h] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(drsrc, doff[i], cd0 * 4 + h * 16, 0));
  };
  // entry i of the staged chunk: split into hi / lo, into the plane buffer at byte offset boff
  // range guard of the f16 split: see conv_x3.inc
  float range_max = 0.f;
  auto split_store = [&](int i, unsigned boff) {
    h16x8 hv, lv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x2 x = {stage[i][j >> 1][2 * (j & 1)], stage[i][j >> 1][2 * (j & 1) + 1]};
      if (!BF) asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(range_max) : "v"(x[0]), "v"(x[1]));      // (ONE instruction: conv_x3s2.inc)
      const h16x2 h = __builtin_convertvector(x, h16x2);
      const f32x2 rem = x - __builtin_convertvector(h, f32x2);
      const h16x2 l = __builtin_convertvector(rem, h16x2);
      hv[2 * j] = h[0]; hv[2 * j + 1] = h[1];
      lv[2 * j] = l[0]; lv[2 * j + 1] = l[1];
    }
    char* p = reinterpret_cast<char*>(lds) + (paddr + boff);
    *reinterpret_cast<h16x8*>(p + i * 1024) = hv;
    *reinterpret_cast<h16x8*>(p + i * 1024 + PS * 16) = lv;
  };

  // ---- prologue: chunk 0 split into plane buffer 0, chunk 1 staged, the first step's fragments and windows
  int w = vb, c0 = 0, k = 0;
  int wsc = wbase(w);
  cursor_enter();
#pragma unroll
  for (int i = 0; i < NE; ++i) stage_entry(i);
  cursor_leave();
  load_A(std::integral_constant<int, 0>(), wsc, 0);
#pragma unroll
  for (int i = 0; i < NE; ++i) split_store(i, 0u);
  cursor_enter();
#pragma unroll
  for (int i = 0; i < NE; ++i) stage_entry(i);
  cursor_leave();
  __syncthreads();
  read_B(std::integral_constant<int, 0>(), 0u, 0);

  // One chunk = 2 steps of 16 channels; step GI works on set GI and prepares the other one.  Step 0 also splits the staged
  // chunk k + 1 into the other plane buffer and re-requests each entry (chunk k + 2) as soon as it is split; step 1 starts
  // with the chunk barrier (the planes of chunk k + 1 are complete, every wave has read the last window of chunk k).
  auto chunk = [&](auto first_tag, auto last_tag) {
    constexpr bool FIRST = decltype(first_tag)::value, LAST = decltype(last_tag)::value;
    const unsigned boff = (unsigned)((k & 1) * BUF * 4), boff_n = (unsigned)(((k + 1) & 1) * BUF * 4);
    const int nw = LAST ? w + (int)gridDim.x : w;
    const bool more = k + 1 < ktotal;
    const int wsn = (LAST && more) ? wbase(nw) : wsc;
    const int s0 = c0 / 16;
    auto mfmas = [&](auto set_tag, auto zero_tag) {
      constexpr int S = decltype(set_tag)::value;
      constexpr bool ZERO = decltype(zero_tag)::value;
#pragma unroll
      for (int p = 0; p < 3; ++p)         // hi x lo, lo x hi, hi x hi
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            const h16x8 wf = __builtin_bit_cast(h16x8, Aq[S][n][p == 1 ? 1 : 0]);
            const h16x8 xf = p == 0 ? Bl[S][s2] : Bh[S][s2];
            if (ZERO && p == 0) {
              const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
              if constexpr (BF) acc[s2][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xf, zero, 0, 0, 0);
              else acc[s2][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, xf, zero, 0, 0, 0);
            } else {
              if constexpr (BF) acc[s2][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xf, acc[s2][n], 0, 0, 0);
              else acc[s2][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, xf, acc[s2][n], 0, 0, 0);
            }
          }
    };
    // ---- step 0
    load_A(std::integral_constant<int, 1>(), wsc, s0 + 1);
    read_B(std::integral_constant<int, 1>(), boff, 1);
    if (FIRST) mfmas(std::integral_constant<int, 0>(), std::true_type());
    else mfmas(std::integral_constant<int, 0>(), std::false_type());
    cursor_enter();
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      split_store(i, boff_n);
      stage_entry(i);            // chunk k + 2
    }
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
    // ---- step 1
    __syncthreads();
    load_A(std::integral_constant<int, 0>(), wsn, LAST ? 0 : s0 + 2);
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
            o4 = pk_add4(pk_fma4(wsp, o4, bv), rv[n][s2][gq]);      // (acc x 2^-S is exact: the fma rounds like the plain sum)
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
  if (!BF && a.range_flag && range_max > 65504.f) atomicOr(a.range_flag, 1u);
}

static hipError_t launch_x3p_impl(const ConvArgs& a, hipStream_t s, int NT, const ConvKernel& k) {
  constexpr size_t lds = (2 * (size_t)4 * 2 * 258 * 4 + 4 * 2 * (size_t)32 * 32) * sizeof(float);
  return launch_conv_kernel(k, 256, lds, 1, (a.Ho * a.Wo) / 256, (a.Cout / 32) / NT, a, s);
}
static hipError_t launch_x3p(const ConvArgs& a, bool bf, hipStream_t s) {
  if (!takes_x3p(conv_shape(a))) return hipErrorInvalidValue;
  if (bf) return a.Cout % 64 == 0 ? launch_x3p_impl(a, s, 2, CONV_KERNEL(conv_x3p_kernel<2, true>)) : launch_x3p_impl(a, s, 1, CONV_KERNEL(conv_x3p_kernel<1, true>));
  return a.Cout % 64 == 0 ? launch_x3p_impl(a, s, 2, CONV_KERNEL(conv_x3p_kernel<2>)) : launch_x3p_impl(a, s, 1, CONV_KERNEL(conv_x3p_kernel<1>));
}
