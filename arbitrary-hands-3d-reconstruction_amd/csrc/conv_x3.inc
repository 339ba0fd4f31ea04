// 3x3 stride-1 convolution on the 16-bit matrix pipe with SPLIT fp32 operands - included by conv_mfma.hip; frame =
// conv_wino24b_kernel's (four waves, 512 registers, LDS-DMA patches issued by the compute waves, one chunk barrier).
//
// Activations and weights stay fp32 in HBM.  Every operand x is split in registers into two f16 numbers hi = f16(x),
// lo = f16(x - hi) (round to nearest: x = hi + lo to 2^-22 |x|), and a product a * w is computed as the three f16 products
//     a_hi w_lo + a_lo w_hi + a_hi w_hi                (dropped: a_lo w_lo <= 2^-22 |a w|)
// on v_mfma_f32_32x32x16_f16 with fp32 accumulation: the round-off class of the fp32 kernels (the accumulation is fp32, the
// operands carry 22 bits instead of 24) at 3 x 32 cycles per 16 channels of a 32 x 32 tile - the fp32 pipe's
// v_mfma_f32_32x32x2_f32 needs 8 x 64 for the same tile (5.3x), its Winograd F(2x4,3x3) form 3 tap-equivalents instead of
// 9 taps: 1536 vs 864 cycles.  The direct form needs no transforms; the layers end up bound by HBM, not by the matrix pipe.
// The weights are split once by the packer (packer.pack_conv_x3: [tap][cin / 16][n-tile][hi | lo][lane 64][8 halves]), after
// a power-of-two scaling of the op's filters that keeps lo out of the f16 subnormals (the kernel multiplies the
// accumulators by the inverse, which is exact).
//
// Item = 8 x 32 output pixels x NT n-tiles of 32 couts; wave w owns output rows 2 w, 2 w + 1 (two slots of 32 pixels: lane
// = pixel n, k-group kg = lane >> 5 holds channels 8 kg .. 8 kg + 7 of a 16-channel step) and reads input rows 2 w .. 2 w + 3
// of the patch.  A step (16 channels) runs in three groups, one per filter column kx: the four row windows of column kx
// (8 ds_read_b128: hi and lo) feed 3 filter rows x 2 slots x NT n-tiles x 3 products = 18 NT MFMAs.  While a group's MFMAs
// run, the next group's weight fragments (6 NT buffer loads) and windows are fetched - the 16-bit pipe leaves about five
// issue slots per MFMA for that.
// Patch: every value of the 10 x 34-pixel x 32-channel patch is split ONCE (the first version split in the consumer: every
// lane its own windows, each value 4.8 times - 480 VALU per chunk and wave, 40 % of the MFMA issue rate): the 256 threads
// load the fp32 patch into registers (6 x 2 buffer loads each, one chunk ahead), split, and write f16 planes
// [channel octet 4][hi | lo][row][pixel] of 16-byte entries into LDS; plane stride 386 entries (2 mod 8: the 16 lanes of a
// ds_write_b128 - 4 pixels x 4 octets - hit 16 different bank quads; window reads are consecutive entries).  Two plane
// buffers of 48.25 KiB; one barrier per chunk.  Epilogue: each wave transposes its own tiles through a private 8 KiB (no
// barrier), bias + residual + ReLU, 16-byte stores.  LDS 128.5 KiB.
//
// Takes: 3x3 stride 1, Cin % 32 == 0, Cout % 32 == 0 (two n-tiles per wave when % 64), maps of 8 x 32-pixel tiles, fp32
// storage.  |x| must stay below 65504 (f16 range), like in the 16-bit programs.

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// BF: the same scheme on bf16 halves (v_mfma_f32_32x32x16_bf16): x = hi + lo carries 16 bits instead of 22 - fp32's exponent
// range (no 65504 limit, no subnormal lo) for 2^-16 relative round-off per product ('bf16x3' programs).
// TW = 16: items of 16 x 16 pixels for the maps narrower than 32 pixels (HRNet branch 3): a slot = 2 rows x 16 pixels, wave w
// owns rows 4 w .. 4 w + 3 and reads six patch rows (five windows per filter column instead of four).
// timing ablations (tools/exp_build.sh -DACRMI_X3_ABLATE=bits; WRONG results): 1 = every weight fragment from the same 1 KiB
// (the vector-memory path sees L1 hits only), 2 = no split arithmetic (raw bits stored), 4 = every window read from one
// address, 8 = no output stores, 16 = no residual / bias loads, 32 = no patch loads (staging registers keep their contents)
#ifndef ACRMI_X3_ABLATE
#define ACRMI_X3_ABLATE 0
#endif
// W22 (NT = 2, TW = 32; round 6): the four waves as 2 row groups x 2 n-tiles - wave (ph, wn) owns output rows 4 ph .. 4 ph + 3
// (FOUR slots) of n-tile wn instead of two rows of both n-tiles: 6 weight fragments per group and wave instead of 12 (the
// vector-memory path was the kernel's largest single cost: tools/x3exp.sh, ablation 1) for 12 window reads instead of 8.
template <int NT, bool BF = false, int TW = 32, bool W22 = false>
__global__ __launch_bounds__(256, 1) void conv_x3_kernel(const ConvArgs a, const ConvWork wk) {
  static_assert(!W22 || (NT == 2 && TW == 32), "2 x 2 wave layout: two n-tiles per item, 8 x 32-pixel items");
  constexpr int NTW = W22 ? 1 : NT, SL = W22 ? 4 : 2;      // n-tiles / slots per wave
  constexpr int X3_ABLATE = ACRMI_X3_ABLATE;
  using h16x8 = typename std::conditional<BF, bf16x8, acrmi::h16x8>::type;      // (the 16-bit operand types of this instantiation)
  using h16x2 = typename std::conditional<BF, bf16x2, acrmi::h16x2>::type;
  constexpr int CK = 32, TH = TW == 32 ? 8 : 16, PH = TH + 2, PWP = TW + 2;
  constexpr int NWIN = TW == 32 ? SL + 2 : 5;      // row windows of a wave per filter column
  constexpr int NE = 6;                            // patch entries (pixel, channel octet) per thread: 6 x 256 >= 10 x 34 x 4
  constexpr int PS = 386, PS2 = 2 * PS;            // entries (16 bytes) per plane / per hi + lo pair of planes
  constexpr int BUF = 4 * PS2 * 4;                 // floats per plane buffer
  static_assert(NE * 64 <= PS && PH * PWP <= PS && PS % 8 == 2, "plane geometry");
  constexpr int PTILE = 32 * 32;                   // parked tile [32 pixels][32 couts], 16-byte columns XOR-swizzled by pixel & 7
  extern __shared__ f32x4 smem4[];
  float* lds = reinterpret_cast<float*>(smem4);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = W22 ? 4 * (wave >> 1) : 2 * wave, nsel = W22 ? (wave & 1) : 0;      // first output row / n-tile of the wave (TW = 32)
  float* part = lds + 2 * BUF + wave * 2 * PTILE;   // the wave's private transposition area: one tile per slot
  const int nchunks = a.Cin / CK;                  // >= 1
  const int ksteps = a.Cin / 16;
  const int vb = virtual_block(a);
  const int my_items = wk.total > vb ? (wk.total - 1 - vb) / (int)gridDim.x + 1 : 0;
  const int ktotal = my_items * nchunks;
  const int li = lane & 31, kg = lane >> 5;
  // byte address (plane buffer 0) of the lane's pixel in the wave's first input row, hi plane of octet kg (step 0)
  const unsigned raddr = TW == 32 ? (unsigned)((kg * PS2 + row0 * PWP + li) * 16)
                                  : (unsigned)((kg * PS2 + (4 * wave + (li >> 4)) * PWP + (li & 15)) * 16);
  // ... and of the thread's first patch entry: octet tid & 3 of patch pixel tid >> 2 (entry i: 64 pixels = 1 KiB further)
  const unsigned paddr = (unsigned)(((tid & 3) * PS2 + (tid >> 2)) * 16);
  // store side: lane = (pixel p8 of a group of 8, cout quad q8), four pixel groups gq per slot
  const int p8 = lane >> 3, q8 = lane & 7;
  const int lane_pix = (TW == 32 ? row0 : 4 * wave) * a.Wo + p8;
  const int lane_out = lane_pix * a.out_cs + 4 * q8, lane_res = lane_pix * a.res_cs + 4 * q8;
  const bool has_res = a.res != nullptr;
  const float floor_ = a.relu ? 0.f : -__builtin_inff();
  f32x16 acc[SL][NTW];
  // pixel offset (within the wave's rows) of store group gq of slot s2: 8 pixels of a row
  auto pix_off = [&](int s2, int gq) -> int { return TW == 32 ? s2 * a.Wo + 8 * gq : (2 * s2 + (gq >> 1)) * a.Wo + 8 * (gq & 1); };
  // byte addresses of the lane's four 16-byte columns (couts 8 q + 4 kg ..) of its pixel's row in the wave's first parked tile
  unsigned pk_addr[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    pk_addr[q] = (unsigned)((2 * BUF + wave * 2 * PTILE + li * 32 + 4 * ((2 * q + kg) ^ (li & 7))) * 4);

  // ---- weights: [tap 9][cin / 16][n-tile][hi | lo][lane 64][8 halves]: 1 KiB fragments
  const int step_b = a.n_tiles * 2048, tap_b = ksteps * step_b;       // bytes
  const __amdgpu_buffer_rsrc_t wrsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.groups * 9 * tap_b, 0x00020000);
  const unsigned wlane = lane * 16;
  // 2^-S of the packer's power-of-two weight scale (packer.x3_weight_shift), the float behind the last fragment
  const float wscale = a.w[(size_t)a.groups * 9 * (tap_b / 4)];
  const float __attribute__((ext_vector_type(2))) wsp = {wscale, wscale};
  auto wbase = [&](int w_item) -> int {
    const ItemPos ip = item_pos(wk, w_item);
    return ip.g * 9 * tap_b + (ip.rest * NT + nsel) * 2048;
  };
  f32x4 Aq[2][3][NTW][2];      // [set][filter row ky][n][hi | lo]
  h16x8 Bh[2][NWIN], Bl[2][NWIN];    // [set][row window of the wave]
  f32x4 stage[NE][2];          // the thread's patch entries of the chunk after the current one, fp32
  // fragments of filter column kx, 16-channel step `step`, into set S
  auto load_A = [&](auto set_tag, int kx, int base, int step) {
    constexpr int S = decltype(set_tag)::value;
    const int so = (X3_ABLATE & 1) ? 0 : base + kx * tap_b + (step < ksteps ? step : ksteps - 1) * step_b;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int n = 0; n < NTW; ++n)
#pragma unroll
        for (int hl = 0; hl < 2; ++hl)
          Aq[S][ky][n][hl] = __builtin_bit_cast(
              f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane + ((X3_ABLATE & 1) ? 0u : (unsigned)(n * 2048 + hl * 1024)),
                                                           (X3_ABLATE & 1) ? so : so + ky * 3 * tap_b, 0));
  };
  // the lane's four row windows of filter column kx, 16-channel step st (0 / 1) of the plane buffer at byte offset boff
  auto read_B = [&](auto set_tag, unsigned boff, int st, int kx) {
    constexpr int S = decltype(set_tag)::value;
    const char* p = reinterpret_cast<const char*>(lds) + (raddr + boff);
#pragma unroll
    for (int r = 0; r < NWIN; ++r) {
      if (X3_ABLATE & 4) {
        if (r == 0) {
          Bh[S][r] = *reinterpret_cast<const h16x8*>(p);
          Bl[S][r] = *reinterpret_cast<const h16x8*>(p + PS * 16);
        }
        continue;
      }
      Bh[S][r] = *reinterpret_cast<const h16x8*>(p + ((2 * st * PS2 + r * PWP + kx) * 16));
      Bl[S][r] = *reinterpret_cast<const h16x8*>(p + ((2 * st * PS2 + PS + r * PWP + kx) * 16));
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
  // patch entry i of the staged chunk: split into hi / lo, into the plane buffer at byte offset boff
  // Range guard of the f16 split (not BF: bf16 halves have fp32's exponent range): the largest |x| this thread splits; a value
  // beyond 65504 becomes hi = inf, lo = -inf and the layer's output NaN - which the next ReLU would silently turn into 0.
  // One v_max3_f32 per two values here, one atomic OR into a.range_flag at the kernel's end if it ever happened: the
  // library then poisons the call's results with NaN and acrmi_check_range() reports ACRMI_ERANGE (VERDICT r4 / ADVICE r4).
  float range_max = 0.f;
  auto split_store = [&](int i, unsigned boff) {
    h16x8 hv, lv;
    if (X3_ABLATE & 2) {
      hv = __builtin_bit_cast(h16x8, stage[i][0]);
      lv = __builtin_bit_cast(h16x8, stage[i][1]);
    } else
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

  // ---- the patch through registers: entry i of thread t = octet t & 3 of patch pixel (t >> 2) + 64 i (row-major, 34 per row)
  int doff[NE], eff[NE];     // source byte offset relative to the patch origin pixel, first channel of a chunk / or out of range
  unsigned dhb[2] = {0u, 0u};   // 8 bits per entry: 1 top / 2 bottom / 4 left / 8 right ring of the patch, 16 = past the patch
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int pp = (tid >> 2) + 64 * i;
    const int row = pp / PWP, pix = pp - row * PWP;
    doff[i] = ((row * a.W + pix) * a.in_cs + 8 * (tid & 3)) * 4;
    const unsigned hb = (row == 0 ? 1u : 0u) | (row == PH - 1 ? 2u : 0u) | (pix == 0 ? 4u : 0u) | (pix == PWP - 1 ? 8u : 0u) |
                        (row < PH ? 0u : 16u);
    dhb[i >> 2] |= hb << (8 * (i & 3));
    eff[i] = (int)0x80000000;
  }
  const int tiles_y = wk.tiles_per_frame / wk.tiles_x;
  __amdgpu_buffer_rsrc_t drsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in), 0, 0, 0x00020000);
  int wd = vb, cd0 = 0, kd = 0;     // load cursor: item, first channel and index of the next chunk to request
  auto stage_load = [&]() {
    if (cd0 == 0) {                 // (uniform) the cursor enters an item: descriptor at its patch origin, halo entries
      const bool valid = kd < ktotal;
      const ItemPos ip = item_pos(wk, valid ? wd : vb);
      const unsigned edge = (ip.ty == 0 ? 1u : 0u) | (ip.ty == tiles_y - 1 ? 2u : 0u) | (ip.tx == 0 ? 4u : 0u) |
                            (ip.tx == wk.tiles_x - 1 ? 8u : 0u) | 16u;
      const long long org = (((long long)ip.b * a.H + (ip.ty * TH - 1)) * a.W + (ip.tx * TW - 1)) * (long long)a.in_cs +
                            a.in_coff + ip.g * a.Cin;
      // past the last item: zero records, every entry reads zeros
      drsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in + org), 0, valid ? 0x7ffffff0 : 0, 0x00020000);
#pragma unroll
      for (int i = 0; i < NE; ++i)
        eff[i] = ((dhb[i >> 2] >> (8 * (i & 3))) & edge) ? (int)0x80000000 : doff[i];
    }
    if (!(X3_ABLATE & 32) || kd < 2)
#pragma unroll
    for (int i = 0; i < NE; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        stage[i][h] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(drsrc, eff[i], cd0 * 4 + h * 16, 0));
    cd0 += CK;
    if (cd0 >= a.Cin) { cd0 = 0; wd += (int)gridDim.x; }
    ++kd;
  };

  const bool stamp = a.dbg && blockIdx.x == 0 && tid == 0;
  int ns_ = 0;
  if (stamp) a.dbg[ns_++] = clock64();
  // ---- prologue: chunk 0 split into plane buffer 0, chunk 1 staged, the first group's fragments and windows
  int w = vb, c0 = 0, k = 0;
  int wsc = wbase(w);
  stage_load();
  load_A(std::integral_constant<int, 0>(), 0, wsc, 0);
#pragma unroll
  for (int i = 0; i < NE; ++i) split_store(i, 0u);
  stage_load();
  __syncthreads();
  read_B(std::integral_constant<int, 0>(), 0u, 0, 0);

  // One chunk = 2 steps of 16 channels = 6 groups; group gi works on set gi & 1 and prepares set (gi + 1) & 1.
  auto chunk = [&](auto first_tag, auto last_tag) {
    constexpr bool FIRST = decltype(first_tag)::value, LAST = decltype(last_tag)::value;
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    const unsigned boff = (unsigned)((k & 1) * BUF * 4), boff_n = (unsigned)(((k + 1) & 1) * BUF * 4);
    const int nw = LAST ? w + (int)gridDim.x : w;
    const bool more = k + 1 < ktotal;
    const int wsn = (LAST && more) ? wbase(nw) : wsc;
    const int s0 = c0 / 16;
    // group GI of the chunk: filter column kx = GI % 3 of step GI / 3
    auto group = [&](auto gi_tag) {
      constexpr int GI = decltype(gi_tag)::value, KX = GI % 3, S = GI & 1, SN = S ^ 1;
      constexpr bool ZERO = FIRST && GI == 0;
      if (GI == 5)        // the chunk barrier, one group early: the planes of chunk k + 1 are complete, every wave has read
        __syncthreads();  // the last window of chunk k
      __builtin_amdgcn_sched_barrier(0);
      // the next group's fragments and windows
      if (GI < 2) {
        load_A(std::integral_constant<int, SN>(), KX + 1, wsc, s0);
        read_B(std::integral_constant<int, SN>(), boff, 0, KX + 1);
      } else if (GI == 2) {
        load_A(std::integral_constant<int, SN>(), 0, wsc, s0 + 1);
        read_B(std::integral_constant<int, SN>(), boff, 1, 0);
      } else if (GI < 5) {
        load_A(std::integral_constant<int, SN>(), KX + 1, wsc, s0 + 1);
        read_B(std::integral_constant<int, SN>(), boff, 1, KX + 1);
      } else {                             // the next chunk's (LAST: the next item's) first group, from the other buffer
        load_A(std::integral_constant<int, SN>(), 0, wsn, LAST ? 0 : s0 + 2);
        read_B(std::integral_constant<int, SN>(), boff_n, 0, 0);
      }
      if (GI == 5) stage_load();      // chunk k + 2 (the staging registers were emptied by groups 2 .. 4)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int p = 0; p < 3; ++p)         // hi x lo, lo x hi, hi x hi
#pragma unroll
          for (int s2 = 0; s2 < SL; ++s2)
#pragma unroll
            for (int n = 0; n < NTW; ++n) {
              const h16x8 wf = __builtin_bit_cast(h16x8, Aq[S][ky][n][p == 1 ? 1 : 0]);
              const h16x8 xf = p == 0 ? Bl[S][ky + (TW == 32 ? 1 : 2) * s2] : Bh[S][ky + (TW == 32 ? 1 : 2) * s2];
              if (ZERO && ky == 0 && p == 0) {
                const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if constexpr (BF) acc[s2][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xf, zero, 0, 0, 0);
                else acc[s2][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, xf, zero, 0, 0, 0);
              } else {
                if constexpr (BF) acc[s2][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xf, acc[s2][n], 0, 0, 0);
                else acc[s2][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, xf, acc[s2][n], 0, 0, 0);
              }
            }
      if (GI >= 2 && GI <= 4) {       // chunk k + 1: two of the thread's six entries per group, into the other plane buffer
        split_store(2 * (GI - 2), boff_n);
        split_store(2 * (GI - 2) + 1, boff_n);
      }
      // interleave: one MFMA, the fetches first, the split arithmetic behind them
      constexpr int NM = 9 * SL * NTW;      // MFMAs of the group
#pragma unroll
      for (int i = 0; i < NM; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (i < 3 * NTW) __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
        if (i < NWIN) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        if (GI >= 2 && GI <= 4 && i >= NM / 3) __builtin_amdgcn_sched_group_barrier(0x002, (40 + 2 * NM / 3 - 1) / (2 * NM / 3), 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    group(std::integral_constant<int, 0>());
    group(std::integral_constant<int, 1>());
    group(std::integral_constant<int, 2>());
    group(std::integral_constant<int, 3>());
    group(std::integral_constant<int, 4>());
    // LAST: the item's bias / residual descriptors, and the first n-tile's bias and residual requested BEFORE the last
    // group's MFMAs (their HBM latency then passes under them instead of in front of the epilogue)
    int rest = 0;
    float* out_tile = nullptr;
    __amdgpu_buffer_rsrc_t rrsrc = wrsrc, brsrc = wrsrc;
    f32x4 rv[NTW][SL][4], bvv[NTW];
    auto request_res = [&](int n) {
      const int nt = rest * NT + nsel + n;
      if (X3_ABLATE & 16) {
        bvv[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s2 = 0; s2 < SL; ++s2)
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) rv[n][s2][gq] = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
      }
      bvv[n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(brsrc, 16 * q8, nt * 128, 0));
#pragma unroll
      for (int s2 = 0; s2 < SL; ++s2)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
          rv[n][s2][gq] = __builtin_bit_cast(
              f32x4, __builtin_amdgcn_raw_buffer_load_b128(rrsrc, lane_res * 4, (nt * 32 + pix_off(s2, gq) * a.res_cs) * 4,
                                                           RES_CACHE_WINO));
    };
    if (LAST) {
      const ItemPos ip = item_pos(wk, w);
      const int g = ip.g, b = ip.b;
      rest = ip.rest;
      const float* bias = a.bias + (size_t)g * a.n_tiles * 32 + (size_t)b * a.bias_fstride;
      const int tile_pix = ip.ty * TH * a.Wo + ip.tx * TW;
      out_tile = a.out + (size_t)b * a.Ho * a.Wo * a.out_cs + a.out_coff + g * a.Cout + (size_t)tile_pix * a.out_cs;
      const size_t res_off = (res_frame_off(a, b) + (size_t)tile_pix * a.res_cs) + a.res_coff + g * a.Cout;
      const size_t res_left = has_res ? (res_total(a) - res_off) * 4 : 0;
      rrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(has_res ? a.res + res_off : a.in), 0,
                                                (int)(unsigned)(res_left > 0xffffffffu ? 0xffffffffu : res_left), 0x00020000);
      brsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bias), 0, bias_row_left(a, g), 0x00020000);
      request_res(0);
    }
    group(std::integral_constant<int, 5>());
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();

    if (LAST) {
      // accumulators -> the wave's tile TI, straight from the AGPRs (ds_write_b128 takes them as its data operand)
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
      if (NTW == 2) request_res(NTW - 1);      // (the second n-tile's: under the first one's transposition and stores)
#pragma unroll
      for (int n = 0; n < NTW; ++n) {
        const int nt = rest * NT + nsel + n;
        const f32x4 bv = bvv[n];
#pragma unroll
        for (int h2 = 0; h2 < SL / 2; ++h2) {      // two slots per round through the wave's two tiles (W22: two rounds)
          __builtin_amdgcn_sched_barrier(0);
          park(std::integral_constant<int, 0>(), acc[2 * h2][n]);
          park(std::integral_constant<int, 1>(), acc[2 * h2 + 1][n]);
          asm volatile("s_nop 1" ::: "memory");
          __builtin_amdgcn_sched_barrier(0);
          // (the wave's own LDS operations execute in order: the reads below see the tiles, the next round's writes come behind them)
#pragma unroll
          for (int sl = 0; sl < 2; ++sl)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
              const int s2 = 2 * h2 + sl;
              f32x4 o4 = *reinterpret_cast<const f32x4*>(part + sl * PTILE + (8 * gq + p8) * 32 + 4 * (q8 ^ p8));
              o4 = pk_add4(pk_fma4(wsp, o4, bv), rv[n][s2][gq]);      // (acc x 2^-S is exact: the fma rounds like the plain sum)
#pragma unroll
              for (int e = 0; e < 4; ++e) o4[e] = vmax1(o4[e], floor_);
              char* ub = reinterpret_cast<char*>(out_tile + nt * 32 + pix_off(s2, gq) * a.out_cs);   // uniform base
              if ((X3_ABLATE & 8) && o4[0] != 12345.678f) continue;
              __builtin_nontemporal_store(o4, reinterpret_cast<f32x4*>(ub + (unsigned)(lane_out * 4)));
            }
          if (SL > 2) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (the asm writes of the next round: not before these reads have returned)
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
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
  if (stamp) a.dbg[63] = ns_;
  if (!BF && a.range_flag && range_max > 65504.f) atomicOr(a.range_flag, 1u);
}

static hipError_t launch_x3_impl(const ConvArgs& a, hipStream_t s, int NT, int TW, const ConvKernel& k) {
  constexpr size_t lds = (2 * (size_t)4 * 2 * 386 * 4 + 4 * 2 * (size_t)32 * 32) * sizeof(float);
  return launch_conv_kernel(k, 256, lds, a.Wo / TW, a.Ho / (TW == 32 ? 8 : 16), (a.Cout / 32) / NT, a, s);
}
static hipError_t launch_x3(const ConvArgs& a, bool bf, hipStream_t s) {
  const int tw = takes_x3(conv_shape(a));      // 32 (8 x 32-pixel items), 16 (16 x 16-pixel items) or 0
  if (!tw) return hipErrorInvalidValue;
  const bool n2 = a.Cout % 64 == 0;
  if (tw == 32) {
    if (bf && n2 && g_force_cfg != 852) return launch_x3_impl(a, s, 2, 32, CONV_KERNEL(conv_x3_kernel<2, true, 32, true>));
    if (bf) return n2 ? launch_x3_impl(a, s, 2, 32, CONV_KERNEL(conv_x3_kernel<2, true>)) : launch_x3_impl(a, s, 1, 32, CONV_KERNEL(conv_x3_kernel<1, true>));
    if (n2 && g_force_cfg != 852) return launch_x3_impl(a, s, 2, 32, CONV_KERNEL(conv_x3_kernel<2, false, 32, true>));
    return n2 ? launch_x3_impl(a, s, 2, 32, CONV_KERNEL(conv_x3_kernel<2>)) : launch_x3_impl(a, s, 1, 32, CONV_KERNEL(conv_x3_kernel<1>));
  }
  if (bf) return n2 ? launch_x3_impl(a, s, 2, 16, CONV_KERNEL(conv_x3_kernel<2, true, 16>)) : launch_x3_impl(a, s, 1, 16, CONV_KERNEL(conv_x3_kernel<1, true, 16>));
  return n2 ? launch_x3_impl(a, s, 2, 16, CONV_KERNEL(conv_x3_kernel<2, false, 16>)) : launch_x3_impl(a, s, 1, 16, CONV_KERNEL(conv_x3_kernel<1, false, 16>));
}
