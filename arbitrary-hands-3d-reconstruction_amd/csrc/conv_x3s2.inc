// 3x3 STRIDE-2 convolution (padding 1, even H and W) with SPLIT fp32 operands on the 16-bit matrix pipe - included by
// conv_mfma.hip behind conv_x3.inc, whose scheme it shares (x = hi + lo in f16 / bf16, three products per MAC on
// v_mfma_f32_32x32x16, fp32 accumulation, fp32 tensors in HBM, weights split and scaled by the packer:
// packer.pack_conv_x3, the same nine-tap image).  HRNet's fuse-layer downsampling chains, transitions, stem conv2 and the
// tower entry (acr/model.py:620-686, 703-736, 288-313) in the 'fp16x3' / 'bf16x3' programs, which kept the fp32 polyphase
// kernel (conv_pp2.inc) for them until round 6 (VERDICT r5 "missing" 3): in the direct form on the 16-bit pipe a stride-2
// layer is 27 / 16 fp32-MFMA equivalents per output and tap set instead of the polyphase form's 6.25 - HBM-bound.
//
// Item = 8 x 32 OUTPUT pixels x NT n-tiles of 32 couts; wave w owns output rows 2 w, 2 w + 1 (two slots of 32 pixels: lane =
// output column, k-group kg = lane >> 5 holds channels 8 kg .. 8 kg + 7 of the 16-channel step) and reads input rows
// 4 w .. 4 w + 4 of the 17 x 65-pixel patch: slot s2, filter row ky -> patch row 4 w + 2 s2 + ky.  The patch columns are stored
// DE-INTERLEAVED ([33 even | 32 odd] entries per row), so that the window of filter column kx - input columns 2 c + kx - is
// 32 CONSECUTIVE 16-byte entries again (kx = 0: even c, 1: odd c, 2: even c + 1): conflict-free ds_read_b128 like the
// stride-1 kernel's.
// A 17 x 65 x 32-channel patch does not fit twice: the two plane buffers hold ONE 16-channel step each (2 channel octets x
// [hi | lo] x 1106 entries = 69.1 KiB), buffer 0 the even steps and buffer 1 the odd ones, a barrier per step.  A "chunk" of the
// code below = two steps = six groups (filter column kx of step 0 / 1), so that the fragment / window sets alternate at
// compile time like conv_x3_kernel's.  Per group: 5 row windows (10 ds_read_b128; ONE register set, each row replaced by the
// next group's window behind its last MFMA - the MFMAs run in the order of the rows they read), 6 NT weight fragments, 18 NT
// MFMAs.  The 256 threads move the fp32 patch through registers: 9 entries (pixel, channel octet) each per step, split into
// hi / lo while the MFMAs of groups 0 / 1 (3 / 4) run, every entry re-requested for the step after the next ONE GROUP after
// its split (two groups of latency; in the same group hipcc hoists the load over the split and the staging registers exist
// twice).  Epilogue as conv_x3_kernel with one 4 KiB transposition tile per wave.  LDS 154.3 KiB.
// Registers: the two-n-tile instantiation still keeps ~95 values in scratch in its single-chunk variant (every scratch access
// waits in the vmcnt queue behind the patch loads): Cin = 32 layers run one n-tile per item (launch_x3s2).
//
// Takes: 3x3 stride 2, H, W even, Ho % 8 == 0, Wo % 32 == 0, Cin % 32 == 0, Cout % 32 == 0 (two n-tiles per wave when % 64),
// no extra residual terms (the HR fuse hosts keep conv_pp2_kernel<.., true>), fp32 storage; |x| < 65504 for f16 halves.

template <int NT, bool BF = false>
__global__ __launch_bounds__(256, 1) void conv_x3s2_kernel(const ConvArgs a, const ConvWork wk) {
  using h16x8 = typename std::conditional<BF, bf16x8, acrmi::h16x8>::type;
  using h16x2 = typename std::conditional<BF, bf16x2, acrmi::h16x2>::type;
  constexpr int PH = 17, PWP = 65, PE = 33;        // patch rows, pixels per row, even-column entries per row
  constexpr int NPIX = PH * PWP;                   // 1105 live entries per plane; entry NPIX takes the dead lanes' writes
  constexpr int NE = 9;                            // entries per thread and step: 9 x 128 >= 1105
  constexpr int PS = 1106, PS2 = 2 * PS;           // entries (16 bytes) per plane / per hi + lo pair of planes
  constexpr int BUF = 2 * PS2 * 4;                 // floats per plane buffer (two channel octets)
  static_assert(NE * 128 >= NPIX && PS > NPIX && PS % 8 == 2, "plane geometry");
  constexpr int PTILE = 32 * 32;                   // parked tile [32 pixels][32 couts], 16-byte columns XOR-swizzled by pixel & 7
  extern __shared__ f32x4 smem4[];
  float* lds = reinterpret_cast<float*>(smem4);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* part = lds + 2 * BUF + wave * PTILE;      // the wave's private transposition tile
  const int nchunks = a.Cin / 32;                  // >= 1 (a chunk = two 16-channel steps)
  const int ksteps = a.Cin / 16;
  const int vb = virtual_block(a);
  const int my_items = wk.total > vb ? (wk.total - 1 - vb) / (int)gridDim.x + 1 : 0;
  const int ktotal = my_items * nchunks;           // chunks
  const int stotal = 2 * ktotal;                   // steps
  const int li = lane & 31, kg = lane >> 5;
  // byte address (within a plane buffer) of the lane's output column in the wave's first patch row, even columns, hi plane of
  // octet kg
  const unsigned raddr = (unsigned)((kg * PS2 + (4 * wave) * PWP + li) * 16);
  // store side: lane = (pixel p8 of a group of 8, cout quad q8), four pixel groups gq per slot (= output row)
  const int p8 = lane >> 3, q8 = lane & 7;
  const int lane_pix = 2 * wave * a.Wo + p8;
  const int lane_out = lane_pix * a.out_cs + 4 * q8, lane_res = lane_pix * a.res_cs + 4 * q8;
  const bool has_res = a.res != nullptr;
  const float floor_ = a.relu ? 0.f : -__builtin_inff();
  f32x16 acc[2][NT];
  unsigned pk_addr[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) pk_addr[q] = (unsigned)((2 * BUF + wave * PTILE + li * 32 + 4 * ((2 * q + kg) ^ (li & 7))) * 4);

  // ---- weights: [tap 9][cin / 16][n-tile][hi | lo][lane 64][8 halves]: 1 KiB fragments (packer.pack_conv_x3)
  const int step_b = a.n_tiles * 2048, tap_b = ksteps * step_b;       // bytes
  const __amdgpu_buffer_rsrc_t wrsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.groups * 9 * tap_b, 0x00020000);
  const unsigned wlane = lane * 16;
  const float wscale = a.w[(size_t)a.groups * 9 * (tap_b / 4)];      // 2^-S of the packer's weight scale
  const float __attribute__((ext_vector_type(2))) wsp = {wscale, wscale};
  auto wbase = [&](int w_item) -> int {
    const ItemPos ip = item_pos(wk, w_item);
    return ip.g * 9 * tap_b + ip.rest * NT * 2048;
  };
  f32x4 Aq[2][3][NT][2];       // [set][filter row ky][n][hi | lo]
  h16x8 Bh[5], Bl[5];          // [patch row 4 w + r]: ONE set, each row replaced by the next group's behind its last MFMA
  f32x4 stage[NE][2];          // the thread's entries of the step after the current one, fp32
  auto load_A = [&](auto set_tag, int kx, int base, int step) {
    constexpr int S = decltype(set_tag)::value;
    const int so = base + kx * tap_b + (step < ksteps ? step : ksteps - 1) * step_b;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int hl = 0; hl < 2; ++hl)
          Aq[S][ky][n][hl] = __builtin_bit_cast(
              f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane + (unsigned)(n * 2048 + hl * 1024), so + ky * 3 * tap_b, 0));
  };
  // row window r of filter column kx in the plane buffer at byte offset boff
  auto read_row = [&](int r, unsigned boff, int kx) {
    const int cofs = kx == 0 ? 0 : (kx == 1 ? PE : 1);
    const char* p = reinterpret_cast<const char*>(lds) + (raddr + boff);
    Bh[r] = *reinterpret_cast<const h16x8*>(p + ((r * PWP + cofs) * 16));
    Bl[r] = *reinterpret_cast<const h16x8*>(p + ((PS + r * PWP + cofs) * 16));
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

  // ---- the patch through registers: entry i of thread t = octet t & 1 of patch pixel (t >> 1) + 128 i (row-major, 65 per row)
  int doff[NE], eff[NE];       // source byte offset relative to the patch origin pixel / or out of range
  unsigned pad[NE];            // LDS byte address (plane buffer 0, hi plane) of the entry
  unsigned dhb[3] = {0u, 0u, 0u};   // 8 bits per entry: 1 top / 4 left ring of the patch, 16 = past the patch
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int pp = (tid >> 1) + 128 * i;
    const int row = pp / PWP, pix = pp - row * PWP;
    const bool live = pp < NPIX;
    doff[i] = ((row * a.W + pix) * a.in_cs + 8 * (tid & 1)) * 4;
    const int idx = live ? row * PWP + ((pix & 1) ? PE + (pix >> 1) : (pix >> 1)) : NPIX;
    pad[i] = (unsigned)(((tid & 1) * PS2 + idx) * 16);
    const unsigned hb = (row == 0 ? 1u : 0u) | (pix == 0 ? 4u : 0u) | (live ? 0u : 16u);
    dhb[i >> 2] |= hb << (8 * (i & 3));
    eff[i] = (int)0x80000000;
  }
  __amdgpu_buffer_rsrc_t drsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in), 0, 0, 0x00020000);
  int wd = vb, cd0 = 0, kd = 0;     // load cursor: item, first channel and index of the next STEP to request
  auto cursor_enter = [&]() {
    if (cd0 == 0) {                 // (uniform) the cursor enters an item: descriptor at its patch origin, halo entries
      const bool valid = kd < stotal;
      const ItemPos ip = item_pos(wk, valid ? wd : vb);
      const unsigned edge = (ip.ty == 0 ? 1u : 0u) | (ip.tx == 0 ? 4u : 0u) | 16u;      // (even H, W: no bottom / right ring)
      const long long org = (((long long)ip.b * a.H + (ip.ty * 16 - 1)) * a.W + (ip.tx * 64 - 1)) * (long long)a.in_cs +
                            a.in_coff + ip.g * a.Cin;
      // past the last item: zero records, every entry reads zeros
      drsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in + org), 0, valid ? 0x7ffffff0 : 0, 0x00020000);
#pragma unroll
      for (int i = 0; i < NE; ++i)
        eff[i] = ((dhb[i >> 2] >> (8 * (i & 3))) & edge) ? (int)0x80000000 : doff[i];
    }
  };
  auto cursor_leave = [&]() {
    cd0 += 16;
    if (cd0 >= a.Cin) { cd0 = 0; wd += (int)gridDim.x; }
    ++kd;
  };
  auto stage_entry = [&](int i) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
      stage[i][h] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(drsrc, eff[i], cd0 * 4 + h * 16, 0));
  };
  // entry i of the staged step: split into hi / lo, into the plane buffer at byte offset boff (range guard: conv_x3.inc)
  float range_max = 0.f;
  auto split_store = [&](int i, unsigned boff) {
    h16x8 hv, lv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x2 x = {stage[i][j >> 1][2 * (j & 1)], stage[i][j >> 1][2 * (j & 1) + 1]};
      if (!BF) asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(range_max) : "v"(x[0]), "v"(x[1]));      // (one instruction; as fmaxf / fabsf calls hipcc keeps a second copy of the staged values alive: scratch)
      const h16x2 h = __builtin_convertvector(x, h16x2);
      const f32x2 rem = x - __builtin_convertvector(h, f32x2);
      const h16x2 l = __builtin_convertvector(rem, h16x2);
      hv[2 * j] = h[0]; hv[2 * j + 1] = h[1];
      lv[2 * j] = l[0]; lv[2 * j + 1] = l[1];
    }
    char* p = reinterpret_cast<char*>(lds) + (pad[i] + boff);
    *reinterpret_cast<h16x8*>(p) = hv;
    *reinterpret_cast<h16x8*>(p + PS * 16) = lv;
  };

  const bool stamp = a.dbg && blockIdx.x == 0 && tid == 0;
  int ns_ = 0;
  if (stamp) a.dbg[ns_++] = clock64();
  // ---- prologue: step 0 split into plane buffer 0, step 1 staged, the first group's fragments and windows
  int w = vb, c0 = 0, k = 0;
  int wsc = wbase(w);
  cursor_enter();
#pragma unroll
  for (int i = 0; i < NE; ++i) stage_entry(i);
  cursor_leave();
  load_A(std::integral_constant<int, 0>(), 0, wsc, 0);
#pragma unroll
  for (int i = 0; i < NE; ++i) split_store(i, 0u);
  cursor_enter();
#pragma unroll
  for (int i = 0; i < NE; ++i) stage_entry(i);
  cursor_leave();
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 5; ++r) read_row(r, 0u, 0);

  constexpr unsigned BOFF1 = (unsigned)(BUF * 4);      // byte offset of plane buffer 1
  // One chunk = 2 steps of 16 channels = 6 groups; group gi works on set gi & 1 and prepares set (gi + 1) & 1.  Groups 0 - 2
  // read plane buffer 0 (step 0), groups 3 - 5 buffer 1; groups 0, 1 fill buffer 1 with the staged step, groups 3, 4 buffer 0.
  auto chunk = [&](auto first_tag, auto last_tag) {
    constexpr bool FIRST = decltype(first_tag)::value, LAST = decltype(last_tag)::value;
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    const int nw = LAST ? w + (int)gridDim.x : w;
    const bool more = k + 1 < ktotal;
    const int wsn = (LAST && more) ? wbase(nw) : wsc;
    const int s0 = c0 / 16;
    auto group = [&](auto gi_tag) {
      constexpr int GI = decltype(gi_tag)::value, KX = GI % 3, ST = GI / 3, S = GI & 1, SN = S ^ 1;
      constexpr bool ZERO = FIRST && GI == 0;
      constexpr bool SPLITS = KX < 2;                    // this group splits entries [E0, E1) of the staged step
      constexpr int E0 = KX == 0 ? 0 : 5, E1 = KX == 0 ? 5 : NE;
      constexpr int NLD = 6 * NT + (KX == 1 ? 10 : (KX == 2 ? 8 : 0));      // buffer loads of the group
      constexpr unsigned rb = ST ? BOFF1 : 0u, wb = ST ? 0u : BOFF1;      // buffer read by this step / filled for the next one
      if (KX == 2)        // the step barrier, one group early: the planes of the next step are complete, every wave has read the
        __syncthreads();  // last window of the step before this one
      __builtin_amdgcn_sched_barrier(0);
      // the next group's fragments; its windows replace this group's row by row (NKX / nb: its filter column / plane buffer)
      constexpr int NKX = (KX + 1) % 3;
      constexpr unsigned nb = KX < 2 ? rb : (ST ? 0u : BOFF1);
      if (KX < 2) load_A(std::integral_constant<int, SN>(), KX + 1, wsc, s0 + ST);
      else if (GI == 2) load_A(std::integral_constant<int, SN>(), 0, wsc, s0 + 1);
      else load_A(std::integral_constant<int, SN>(), 0, wsn, LAST ? 0 : s0 + 2);      // the next chunk's (LAST: the next item's) first group
      // MFMAs in the order of the patch rows they read: row r = 2 s2 + ky
#pragma unroll
      for (int r = 0; r < 5; ++r) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const int ky = r - 2 * s2;
          if (ky < 0 || ky > 2) continue;
#pragma unroll
          for (int p = 0; p < 3; ++p)         // hi x lo, lo x hi, hi x hi
#pragma unroll
            for (int n = 0; n < NT; ++n) {
              const h16x8 wf = __builtin_bit_cast(h16x8, Aq[S][ky][n][p == 1 ? 1 : 0]);
              const h16x8 xf = p == 0 ? Bl[r] : Bh[r];
              if (ZERO && ky == 0 && p == 0) {
                const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if constexpr (BF) acc[s2][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xf, zero, 0, 0, 0);
                else acc[s2][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, xf, zero, 0, 0, 0);
              } else {
                if constexpr (BF) acc[s2][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xf, acc[s2][n], 0, 0, 0);
                else acc[s2][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, xf, acc[s2][n], 0, 0, 0);
              }
            }
        }
        read_row(r, nb, NKX);
      }
      // the staged step into the other buffer: entries [0, 5) in the step's first group, [5, 9) in the second; an entry is
      // re-requested (the step after the next) ONE GROUP LATER - behind a scheduling boundary, so that the load can take the
      // registers the split has just emptied (requested in the same group hipcc hoists the loads over the split arithmetic
      // and the staging registers exist twice: scratch)
      if (KX == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) split_store(i, wb);
      } else if (KX == 1) {
#pragma unroll
        for (int i = 5; i < NE; ++i) split_store(i, wb);
        cursor_enter();
#pragma unroll
        for (int i = 0; i < 5; ++i) stage_entry(i);
      } else {
#pragma unroll
        for (int i = 5; i < NE; ++i) stage_entry(i);
        cursor_leave();
      }
      // interleave: one MFMA, the fetches first, the split arithmetic behind them
#pragma unroll
      for (int i = 0; i < 18 * NT; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (2 * i < NLD) __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
        if (i % (3 * NT) == 3 * NT - 1 || (i >= 6 * NT && i < 12 * NT && i % (3 * NT) == 0)) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        if (SPLITS && i >= 5) __builtin_amdgcn_sched_group_barrier(0x002, (24 * (E1 - E0) + 18 * NT - 6) / (18 * NT - 5), 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    group(std::integral_constant<int, 0>());
    group(std::integral_constant<int, 1>());
    group(std::integral_constant<int, 2>());
    group(std::integral_constant<int, 3>());
    group(std::integral_constant<int, 4>());
    // LAST: the item's bias / residual descriptors, the first n-tile's bias and residual requested BEFORE the last group's MFMAs
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
              f32x4, __builtin_amdgcn_raw_buffer_load_b128(rrsrc, lane_res * 4, (nt * 32 + (s2 * a.Wo + 8 * gq) * a.res_cs) * 4,
                                                           RES_CACHE_WINO));
    };
    if (LAST) {
      const ItemPos ip = item_pos(wk, w);
      const int g = ip.g, b = ip.b;
      rest = ip.rest;
      const float* bias = a.bias + (size_t)g * a.n_tiles * 32 + (size_t)b * a.bias_fstride;
      const int tile_pix = ip.ty * 8 * a.Wo + ip.tx * 32;
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
      // accumulators -> the wave's tile, straight from the AGPRs (ds_write_b128 takes them as its data operand)
      auto park = [&](const f32x16& x) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 v4 = {x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]};
          const unsigned ad = pk_addr[q];
          asm volatile("ds_write_b128 %0, %1" ::"v"(ad), "a"(v4) : "memory");
        }
      };
      // (the asm writes are invisible to hipcc's hazard recognizer: the last MFMA's passes drain here)
      asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
      if (NT == 2) request_res(NT - 1);      // (the second n-tile's: under the first one's transposition and stores)
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int nt = rest * NT + n;
        const f32x4 bv = bvv[n];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          __builtin_amdgcn_sched_barrier(0);
          park(acc[s2][n]);
          asm volatile("s_nop 1" ::: "memory");
          __builtin_amdgcn_sched_barrier(0);
          // (the wave's own LDS operations execute in order: the reads below see the tile, the next park comes behind them)
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) {
            f32x4 o4 = *reinterpret_cast<const f32x4*>(part + (8 * gq + p8) * 32 + 4 * (q8 ^ p8));
            o4 = pk_add4(pk_fma4(wsp, o4, bv), rv[n][s2][gq]);      // (acc x 2^-S is exact: the fma rounds like the plain sum)
#pragma unroll
            for (int e = 0; e < 4; ++e) o4[e] = vmax1(o4[e], floor_);
            char* ub = reinterpret_cast<char*>(out_tile + nt * 32 + (s2 * a.Wo + 8 * gq) * a.out_cs);   // uniform base
            __builtin_nontemporal_store(o4, reinterpret_cast<f32x4*>(ub + (unsigned)(lane_out * 4)));
          }
          // (WAR on the tile: the next park's ds_write_b128 are issued behind these ds_read_b128 of the same wave - in order)
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    }
    wsc = wsn;
    c0 = LAST ? 0 : c0 + 32;
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

static hipError_t launch_x3s2_impl(const ConvArgs& a, hipStream_t s, int NT, const ConvKernel& k) {
  constexpr size_t lds = (2 * (size_t)2 * 2 * 1106 * 4 + 4 * (size_t)32 * 32) * sizeof(float);
  static_assert(lds <= 160 * 1024, "two step buffers and the transposition tiles must fit the LDS");
  return launch_conv_kernel(k, 256, lds, a.Wo / 32, a.Ho / 8, (a.Cout / 32) / NT, a, s);
}
static hipError_t launch_x3s2(const ConvArgs& a, bool bf, hipStream_t s) {
  if (!takes_x3s2(conv_shape(a))) return hipErrorInvalidValue;
  // (single-chunk items, Cin = 32: the two-n-tile instantiation keeps ~100 values in scratch there and every scratch access
  //  waits behind the patch loads in flight - cfg 851 selects it anyway)
  const bool n2 = a.Cout % 64 == 0 && (a.Cin > 32 || g_force_cfg == 851);
  if (bf) return n2 ? launch_x3s2_impl(a, s, 2, CONV_KERNEL(conv_x3s2_kernel<2, true>)) : launch_x3s2_impl(a, s, 1, CONV_KERNEL(conv_x3s2_kernel<1, true>));
  return n2 ? launch_x3s2_impl(a, s, 2, CONV_KERNEL(conv_x3s2_kernel<2>)) : launch_x3s2_impl(a, s, 1, CONV_KERNEL(conv_x3s2_kernel<1>));
}
