// 3x3 stride-2 convolution (padding 1, even H and W) in polyphase form with F(2,2) on the two-tap phases - included by
// conv_mfma.hip; frame = conv_wino24b_kernel's (four waves, 512 registers, LDS-DMA patches issued by the compute waves, chunk
// barrier one step early, exchange through LDS).  HRNet's fuse-layer downsampling chains, transitions, stem conv2 and the tower
// entry (acr/model.py:620-686, 703-736, 288-313): 42 launches, 5.3 ms of the step in the direct form.
//
// Along one axis an output o reads input rows 2o-1, 2o, 2o+1.  The odd rows (phase 1) see the TWO taps (w0, w2), the even rows
// (phase 0) the single tap w1.  For a PAIR of outputs (o0, o1) with odd rows d0, d1, d2 and even rows e0, e1:
//     o0 = w0 d0 + w2 d1 + w1 e0          o1 = w0 d1 + w2 d2 + w1 e1
// F(2,2) on the two-tap part: m0 = (d0 - d1) w0, m1 = d1 (w0 + w2), m2 = (d2 - d1) w2; o0 = m0 + m1 (+ w1 e0), o1 = m1 + m2
// (+ w1 e1) - five 1-D terms {A0, A1, A2, B0, B1} instead of six products, each landing on output pattern e0 (A0, B0), e1
// (A2, B1) or both (A1).  In 2-D: 5 x 5 = 25 products per 2x2 output block instead of 36 (1.44x fewer MFMAs), and products
// with the same output pattern ACCUMULATE IN THE SAME MFMA ACCUMULATOR: 9 patterns = corner (e_oy, e_ox) x 4 with 4 products
// each, edge x 4 with 2 products each, centre (both, both) with 1.
//
// Work split (slot = one 2x2 output block, 32 slots = 8x16 output pixels per item): wave (oy, ox) owns corner (e_oy, e_ox)
// [acc 0], one edge pattern [acc 1: (e_oy, both) when oy == ox, (both, e_ox) otherwise] and - every wave, so that the four
// instruction streams stay identical and branch-free; only wave 0's copy is used - the centre [acc 2]: 7 products = 28 NT
// MFMAs per 8-channel step, 3 NT accumulator tiles.  All seven input combinations of a wave come from the 3x3 pixels
// {own row ia, centre row 2, phase-0 row iB} x {ja, 2, jB} of the slot's 5x5 window (ia = 4 oy, iB = 1 + 2 oy):
//     D[v] = P[a][v] - P[2][v];   k0 = D[a] - D[2], k1 = D[B], k2 = P[B][a] - P[B][2], k3 = P[B][B] (corner);
//     k4 = D[2], k5 = P[B][2] (edge);   k6 = P[2][2] (centre)
// = 9 ds_read_b128 + 5 float4 subtractions per step.  The waves with oy != ox read the TRANSPOSED pixel set (P[u][v] = pixel
// (row of v, column of u)), which turns k4 / k5 into their (both, e_ox) products and swaps k1 / k2 - the weights are packed
// per wave to match (packer.polyphase2_weights: 4 waves x 7 "taps").
// Epilogue: every wave parks its corner and edge tiles (wave 0 also the centre) as [slot][cout]; wave (oy, ox) then sums its
// own corner + the (e_oy, both) edge of wave 3 oy + the (both, e_ox) edge of wave 2 - ox + the centre for output parity
// (oy, ox): bias, residual, ReLU, 16-byte stores.  One exchange round per two n-tiles.
// Patch: 17 rows x 33 input pixels x 16 channels per chunk, layout [row][group of 4 pixels][pixel][4 quads] + 1 pad quad per
// group (17 = 1 mod 16), row stride 154 quads (four rows = 8 mod 16): conflict-free window reads.  LDS (NT >= 2): 2 x 41,984 B
// + 18 tiles x 4 KiB = 157,696 B.
//
// Takes: 3x3 stride 2, H, W even, Ho % 8 == 0, Wo % 16 == 0, Cin % 16 == 0, Cout % 32 == 0 (two n-tiles per wave when % 64),
// 16-byte aligned channel slices.  fp32 round-off: the F(2,2) transforms only add and subtract.

// XT: the item's epilogue also adds up to three extra residual terms at 1 / 2^shift of the output resolution (ConvArgs.xt: the
// HR-module fuse sum folded into the last convolution of the x0 downsampling chain): 3 x 4 more residual vectors per lane and n-tile in flight.
// Both n-tile counts are instantiated - <2, true> takes the hosts with Cout % 64 == 0 (506 of the 512 registers, no scratch:
// launch_pp2 below), <1, true> the others.
// ACRMI_PP2_HOIST (1): the DMA cursor's entry into the next item (item position by multiply-shift division, 64-bit origin,
// descriptor, the halo selects of the 11 pieces: ~90 scalar + ~55 vector instructions) runs in the chunk's FIRST step, between
// its MFMA groups, instead of behind the chunk barrier of the second one, where nothing covers it (0 = there: A/B builds)
#ifndef ACRMI_PP2_HOIST
#define ACRMI_PP2_HOIST 1
#endif
template <int NT, bool XT = false>
__global__ __launch_bounds__(256, 1) void conv_pp2_kernel(const ConvArgs a, const ConvWork wk) {

  constexpr int CK = 16, PH = 17, PWP = 33;
  constexpr int RS = 154, GQ = 17;                 // quads per patch row / per group of 4 pixels (4 x 4 + 1 pad)
  constexpr int NPIECE = (PH * RS + 63) / 64;      // 41 DMA pieces of 64 quads
  constexpr int NI = (NPIECE + 3) / 4;             // 11 per wave
  constexpr int BUF = NPIECE * 64 * 4;             // floats per patch buffer
  constexpr int PTILE = 32 * 32;                   // parked tile [32 slots][32 couts], 16-byte columns XOR-swizzled by slot & 7
  constexpr int NTR = NT >= 2 ? 2 : 1;             // n-tiles per exchange round
  constexpr int WTILES = 2 * NTR;                  // tiles a wave parks per round: [corner | edge][n]; the centre tiles follow
  extern __shared__ f32x4 smem4[];
  float* lds = reinterpret_cast<float*>(smem4);
  float* part = lds + 2 * BUF;
  float* part_c = part + 4 * WTILES * PTILE;       // wave 0's centre tiles [n]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nchunks = a.Cin / CK;                  // >= 1
  const int vb = virtual_block(a);
  const int my_items = wk.total > vb ? (wk.total - 1 - vb) / (int)gridDim.x + 1 : 0;
  const int ktotal = my_items * nchunks;
  const int li = lane & 31, lh = lane >> 5;
  const int oy = wave >> 1, ox = wave & 1;
  const bool transposed = oy != ox;
  // byte addresses (patch buffer 0) of the lane's 3x3 pixel set, channel quad lh of step 0
  unsigned paddr[3][3];
  {
    const int yi[3] = {4 * oy, 2, 1 + 2 * oy}, xj[3] = {4 * ox, 2, 1 + 2 * ox};
    const int R = li >> 3, C = li & 7;
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const int i = transposed ? yi[v] : yi[u], j = transposed ? xj[u] : xj[v];
        paddr[u][v] = (unsigned)(((4 * R + i) * RS + (C + (j >> 2)) * GQ + (j & 3) * 4 + lh) * 16);
      }
  }
  // store side: this wave writes output parity (oy, ox) of every 2x2 block; lane = (block column p8, cout quad q8), four
  // block rows gq per lane
  const int p8 = lane >> 3, q8 = lane & 7;
  const int lane_pix = oy * a.Wo + 2 * p8 + ox;
  const int lane_out = lane_pix * a.out_cs + 4 * q8, lane_res = lane_pix * a.res_cs + 4 * q8;
  const int gs_out = 2 * a.Wo * a.out_cs, gs_res = 2 * a.Wo * a.res_cs;
  const bool has_res = a.res != nullptr;
  const float floor_ = a.relu ? 0.f : -__builtin_inff();
  f32x16 acc[3][NT];
  // byte addresses of the lane's four 16-byte columns (couts 8 q + 4 lh ..) of its slot's row in the wave's first parked tile
  unsigned pk_addr[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    pk_addr[q] = (unsigned)((2 * BUF + wave * WTILES * PTILE + li * 32 + 4 * ((2 * q + lh) ^ (li & 7))) * 4);

  // ---- weights: 28 "taps" = wave x 7 products, [tap][cin / 8][n-tile][lane 64][4]
  const int tap_b = a.cin8 * a.n_tiles * 1024, step_b = a.n_tiles * 1024;
  const __amdgpu_buffer_rsrc_t wrsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.groups * 28 * tap_b, 0x00020000);
  const unsigned wlane = lane * 16;
  auto wbase = [&](int w_item) -> int {
    const ItemPos ip = item_pos(wk, w_item);
    return (ip.g * 28 + wave * 7) * tap_b + ip.rest * NT * 1024;
  };
  f32x4 bq[7][NT], v[2][7];
  auto load_frag = [&](int p, int base, int step) {
    const int so = base + p * tap_b + (step < a.cin8 ? step : a.cin8 - 1) * step_b;
#pragma unroll
    for (int n = 0; n < NT; ++n)
      bq[p][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane, so + n * 1024, 0));
  };
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const float one = a.ks == 3 ? 1.f : 2.f;   // always 1 (a runtime value: nothing is folded back into scalar ops)
  f32x2 m1p = {-one, -one};
  asm volatile("" : "+v"(m1p));
  auto pk_sub4 = [&](const f32x4& b, const f32x4& c) -> f32x4 {   // b - c  (as (-1) * c + b: exact)
    f32x2 lo, hi;
    const f32x2 b0 = {b[0], b[1]}, b1 = {b[2], b[3]}, c0 = {c[0], c[1]}, c1 = {c[2], c[3]};
    asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(lo) : "v"(m1p), "v"(c0), "v"(b0));
    asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(hi) : "v"(m1p), "v"(c1), "v"(b1));
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
  };
  auto pk_add4 = [](const f32x4& b, const f32x4& c) -> f32x4 {
    f32x2 lo, hi;
    const f32x2 b0 = {b[0], b[1]}, b1 = {b[2], b[3]}, c0 = {c[0], c[1]}, c1 = {c[2], c[3]};
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(lo) : "v"(b0), "v"(c0));
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(hi) : "v"(b1), "v"(c1));
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
  };
  f32x4 P[3][3];
  // the lane's 3x3 pixels of 8-channel step s (0 / 1) in the patch buffer at byte offset boff
  auto read_window = [&](unsigned boff, int s) {
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
      for (int vv = 0; vv < 3; ++vv)
        P[u][vv] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(lds) + (paddr[u][vv] + boff + (unsigned)(s * 32)));
  };
  auto transform = [&](f32x4 (&o)[7]) {
    const f32x4 Da = pk_sub4(P[0][0], P[1][0]), D2 = pk_sub4(P[0][1], P[1][1]), DB = pk_sub4(P[0][2], P[1][2]);
    o[0] = pk_sub4(Da, D2);
    o[1] = DB;
    o[2] = pk_sub4(P[2][0], P[2][1]);
    o[3] = P[2][2];
    o[4] = D2;
    o[5] = P[2][1];
    o[6] = P[1][1];
  };

  // ---- LDS-DMA of the patch (conv_wino24b.inc): piece jj[i] = 64 consecutive quads, lane l its quad 64 jj[i] + l
  int jj[NI], doff[NI], eff[NI];
  unsigned dhb[(NI + 3) / 4];      // 8 bits per piece: 1 top / 4 left ring of the patch, 16 = slot never fetched
#pragma unroll
  for (int i = 0; i < (NI + 3) / 4; ++i) dhb[i] = 0;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int j = i * 4 + wave;
    jj[i] = j < NPIECE ? j : NPIECE - 1;
    const int f = jj[i] * 64 + lane;
    const int row = f / RS, rem = f - row * RS;
    const int grp = rem / GQ, q = rem - grp * GQ;
    const int pix = grp * 4 + (q >> 2);
    const bool live = row < PH && q < 16 && pix < PWP;
    doff[i] = ((row * a.W + pix) * a.in_cs + 4 * (q & 3)) * 4;
    const unsigned hb = (row == 0 ? 1u : 0u) | (pix == 0 ? 4u : 0u) | (live ? 0u : 16u);
    dhb[i >> 2] |= hb << (8 * (i & 3));
    eff[i] = (int)0x80000000;
  }
  __amdgpu_buffer_rsrc_t drsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in), 0, 0, 0x00020000);
  int wd = vb, cd0 = 0, kd = 0;     // DMA cursor: item, first channel and index of the next chunk to request
  auto dma_begin = [&]() {
    if (cd0 == 0) {                 // (uniform) the cursor enters an item
      const bool valid = kd < ktotal;
      const ItemPos ip = item_pos(wk, valid ? wd : vb);
      const unsigned edge = (ip.ty == 0 ? 1u : 0u) | (ip.tx == 0 ? 4u : 0u) | 16u;      // (even H, W: no bottom / right ring)
      const long long org = (((long long)ip.b * a.H + (ip.ty * 16 - 1)) * a.W + (ip.tx * 32 - 1)) * (long long)a.in_cs +
                            a.in_coff + ip.g * a.Cin;
      drsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.in + org), 0, valid ? 0x7ffffff0 : 0, 0x00020000);
#pragma unroll
      for (int i = 0; i < NI; ++i)
        eff[i] = ((dhb[i >> 2] >> (8 * (i & 3))) & edge) ? (int)0x80000000 : doff[i];
    }
  };
  auto dma_piece = [&](int i, int bsel) {
    if (i < NI) lds_dma16(drsrc, lds + bsel * BUF + jj[i] * 256, eff[i], cd0 * 4);
  };
  auto dma_end = [&]() {
    cd0 += CK;
    if (cd0 >= a.Cin) { cd0 = 0; wd += (int)gridDim.x; }
    ++kd;
  };

  const bool stamp = a.dbg && blockIdx.x == 0 && tid == 0;
  int ns_ = 0;
  if (stamp) a.dbg[ns_++] = clock64();
  // ---- prologue: chunks 0 and 1 on their way, first weight fragments, first window
  int w = vb, c0 = 0, k = 0;
  int wsc = wbase(w);
  dma_begin();
#pragma unroll
  for (int i = 0; i < NI; ++i) dma_piece(i, 0);
  dma_end();
  dma_begin();
#pragma unroll
  for (int i = 0; i < NI; ++i) dma_piece(i, 1);
  dma_end();
#pragma unroll
  for (int p = 0; p < 7; ++p) load_frag(p, wsc, 0);
  __syncthreads();
  read_window(0u, 0);
  transform(v[0]);

  // One 8-channel step on fragment set SET: 7 groups of 4 NT MFMAs.  The next step's window (step rs of the buffer at byte
  // offset rboff) is requested behind group 0 and transformed into the OTHER set behind group 3; weights of the next step
  // replace each group's fragments behind its MFMAs.  BRIDGE = a chunk's second (last) step: the chunk barrier first, the
  // window is the first one of the next chunk in the other buffer, the pieces of the chunk after that go out, two per group.
  auto chunk = [&](auto first_tag, auto last_tag) {
    constexpr bool FIRST = decltype(first_tag)::value, LAST = decltype(last_tag)::value;
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    const unsigned boff = (unsigned)((k & 1) * BUF * 4), boff_n = (unsigned)(((k + 1) & 1) * BUF * 4);
    const int nw = LAST ? w + (int)gridDim.x : w;
    const bool more = k + 1 < ktotal;
    const int wsn = (LAST && more) ? wbase(nw) : wsc;
    auto step = [&](auto set_tag, auto zero_tag, auto bridge_tag, auto tail_tag, unsigned rboff, int rs, int wb, int ws) {
      constexpr int SET = decltype(set_tag)::value;
      constexpr bool ZERO = decltype(zero_tag)::value, BRIDGE = decltype(bridge_tag)::value, TAIL = decltype(tail_tag)::value;
      if (BRIDGE) {
        __syncthreads();
        if (!ACRMI_PP2_HOIST) dma_begin();
      }
#pragma unroll
      for (int p = 0; p < 7; ++p) {
        constexpr int amap[7] = {0, 0, 0, 0, 1, 1, 2};
        __builtin_amdgcn_sched_barrier(0);
        if (p == 0) read_window(rboff, rs);
        if (p == 3) transform(v[SET ^ 1]);
        if (ACRMI_PP2_HOIST && !BRIDGE && p == 5) dma_begin();      // (the cursor was advanced at the previous bridge)
        if (BRIDGE) {
          dma_piece(2 * p, k & 1);
          dma_piece(2 * p + 1, k & 1);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            if (ZERO && j == 0 && (p == 0 || p == 4 || p == 6)) {
              const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
              acc[amap[p]][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[p][n][j], v[SET][p][j], zero, 0, 0, 0);
            } else {
              acc[amap[p]][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[p][n][j], v[SET][p][j], acc[amap[p]][n], 0, 0, 0);
            }
          }
        __builtin_amdgcn_sched_barrier(0);
        if (!TAIL) load_frag(p, wb, ws);      // (TAIL: the next item's first fragments go out from the epilogue)
      }
      if (BRIDGE) dma_end();
    };
    const int s0 = c0 / 8;
    if (FIRST) step(std::integral_constant<int, 0>(), std::true_type(), std::false_type(), std::false_type(), boff, 1, wsc, s0 + 1);
    else step(std::integral_constant<int, 0>(), std::false_type(), std::false_type(), std::false_type(), boff, 1, wsc, s0 + 1);
    if (LAST) step(std::integral_constant<int, 1>(), std::false_type(), std::true_type(), std::true_type(), boff_n, 0, wsn, 0);
    else step(std::integral_constant<int, 1>(), std::false_type(), std::true_type(), std::false_type(), boff_n, 0, wsc, s0 + 2);
    __builtin_amdgcn_sched_barrier(0);
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();

    if (LAST) {
      const ItemPos ip = item_pos(wk, w);
      const int g = ip.g, b = ip.b, rest = ip.rest;
      const float* bias = a.bias + (size_t)g * a.n_tiles * 32 + (size_t)b * a.bias_fstride;
      const int tile_pix = ip.ty * 8 * a.Wo + ip.tx * 16;
      float* out_tile = a.out + (size_t)b * a.Ho * a.Wo * a.out_cs + a.out_coff + g * a.Cout + (size_t)tile_pix * a.out_cs;
      const size_t res_off = (res_frame_off(a, b) + (size_t)tile_pix * a.res_cs) + a.res_coff + g * a.Cout;
      const size_t res_left = has_res ? (res_total(a) - res_off) * 4 : 0;
      const __amdgpu_buffer_rsrc_t rrsrc = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(has_res ? a.res + res_off : a.in), 0,
          (int)(unsigned)(res_left > 0xffffffffu ? 0xffffffffu : res_left), 0x00020000);
      const __amdgpu_buffer_rsrc_t brsrc =
          __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bias), 0, bias_row_left(a, g), 0x00020000);
      // XT: descriptors of the extra terms at this frame / group, the lane's column offset; a missing term reads zeros
      // through a zero-record descriptor (branch-free: adding +0.0 changes no value)
      __amdgpu_buffer_rsrc_t xrs[3] = {brsrc, brsrc, brsrc};
      unsigned xvo[3] = {0u, 0u, 0u};
      int xsh[3] = {0, 0, 0}, xrow[3] = {0, 0, 0};
      if constexpr (XT) {
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const bool on = t < a.nxt;
          const int sh = on ? a.xt_shift[t] : 0, cs = on ? a.xt_cs[t] : 4;
          const int hs = a.Ho >> sh, wsx = a.Wo >> sh;
          const size_t off = (size_t)b * hs * wsx * cs + (on ? a.xt_coff[t] : 0) + g * a.Cout;
          const size_t left = on ? ((size_t)a.B * hs * wsx * cs - off) * 4 : 0;
          xrs[t] = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(on ? a.xt[t] + off : a.in), 0,
                                                     (int)(unsigned)(left > 0xffffffffu ? 0xffffffffu : left), 0x00020000);
          xvo[t] = (unsigned)((((ip.tx * 16 + 2 * p8 + ox) >> sh) * cs + 4 * q8) * 4);
          xsh[t] = sh;
          xrow[t] = wsx * cs * 4;      // bytes per row of the term's map
        }
      }
      // accumulators -> parked tile TI of the wave (the centre tiles: wave 0, behind every wave's), straight from the AGPRs:
      // ds_write_b128 takes them as its data operand
      auto park = [&](auto ti_tag, const f32x16& x) {
        constexpr int TI = decltype(ti_tag)::value % (4 * WTILES);
        constexpr bool CENTRE = decltype(ti_tag)::value >= 4 * WTILES;      // (immediate offsets end at 64 KiB)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 v4 = {x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]};
          const unsigned ad = pk_addr[q] + (CENTRE ? 4 * WTILES * PTILE * 4 : 0);
          asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(ad), "a"(v4), "n"(TI * PTILE * 4) : "memory");
        }
      };
      // (the asm writes are invisible to hipcc's hazard recognizer: the last MFMA's 16 passes drain here)
      asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
      for (int r0 = 0; r0 < NT; r0 += NTR) {
        f32x4 rv[NTR][4], bv[NTR];
        f32x4 xv[XT ? 3 : 1][NTR][4];
#pragma unroll
        for (int n = 0; n < NTR; ++n) {
          bv[n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(brsrc, 16 * q8, (rest * NT + r0 + n) * 128, 0));
#pragma unroll
          for (int gq = 0; gq < 4; ++gq)
            rv[n][gq] = __builtin_bit_cast(
                f32x4, __builtin_amdgcn_raw_buffer_load_b128(rrsrc, lane_res * 4, ((rest * NT + r0 + n) * 32 + gq * gs_res) * 4,
                                                             RES_CACHE_WINO));
          if constexpr (XT) {
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
              for (int gq = 0; gq < 4; ++gq) {      // output row ty * 8 + oy + 2 gq of the frame -> row >> shift of the term (scalar)
                const int so = ((ip.ty * 8 + oy + 2 * gq) >> xsh[t]) * xrow[t] + (rest * NT + r0 + n) * 128;
                xv[t][n][gq] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs[t], xvo[t], so, 0));
              }
          }
        }
        if (r0 > 0) __syncthreads();              // every wave has read the previous round's tiles
        __builtin_amdgcn_sched_barrier(0);
        park(std::integral_constant<int, 0>(), acc[0][r0]);
        park(std::integral_constant<int, NTR>(), acc[1][r0]);
        if (NTR == 2) {
          park(std::integral_constant<int, NTR - 1>(), acc[0][r0 + NTR - 1]);
          park(std::integral_constant<int, 2 * NTR - 1>(), acc[1][r0 + NTR - 1]);
        }
        if (wave == 0) {
          park(std::integral_constant<int, 4 * WTILES>(), acc[2][r0]);
          if (NTR == 2) park(std::integral_constant<int, 4 * WTILES + NTR - 1>(), acc[2][r0 + NTR - 1]);
        }
        asm volatile("s_nop 1" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (LAST && r0 + NTR >= NT) {             // the accumulators are dead: the next item's first weight fragments
#pragma unroll
          for (int p = 0; p < 7; ++p) load_frag(p, wsn, 0);
        }
        if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
        __syncthreads();                          // the round is parked
        if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
#pragma unroll
        for (int n = 0; n < NTR; ++n) {
          const int sw = p8 * 32 + 4 * (q8 ^ p8);
          const float* tc = part + (wave * WTILES + n) * PTILE + sw;               // own corner
          const float* ty_ = part + ((3 * oy) * WTILES + NTR + n) * PTILE + sw;     // (e_oy, both): wave (oy, oy)
          const float* tx_ = part + ((2 - ox) * WTILES + NTR + n) * PTILE + sw;     // (both, e_ox): wave (1 - ox, ox)
          const float* tm = part_c + n * PTILE + sw;                               // centre: wave 0
          f32x4 pp[4][4];
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) {
            pp[0][gq] = *reinterpret_cast<const f32x4*>(tc + 8 * gq * 32);
            pp[1][gq] = *reinterpret_cast<const f32x4*>(ty_ + 8 * gq * 32);
            pp[2][gq] = *reinterpret_cast<const f32x4*>(tx_ + 8 * gq * 32);
            pp[3][gq] = *reinterpret_cast<const f32x4*>(tm + 8 * gq * 32);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) {
            f32x4 o4 = pk_add4(pk_add4(pk_add4(pp[0][gq], pp[1][gq]), pp[2][gq]), pp[3][gq]);
            o4 = pk_add4(pk_add4(o4, bv[n]), rv[n][gq]);      // (no residual: zeros through a zero-record descriptor)
            if constexpr (XT) o4 = pk_add4(pk_add4(pk_add4(o4, xv[0][n][gq]), xv[1][n][gq]), xv[2][n][gq]);
            o4[0] = vmax1(o4[0], floor_); o4[1] = vmax1(o4[1], floor_); o4[2] = vmax1(o4[2], floor_); o4[3] = vmax1(o4[3], floor_);
            char* ub = reinterpret_cast<char*>(out_tile + (rest * NT + r0 + n) * 32 + gq * gs_out);   // uniform base
            __builtin_nontemporal_store(o4, reinterpret_cast<f32x4*>(ub + (unsigned)(lane_out * 4)));
          }
        }
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
}

static constexpr size_t pp2_lds(int NT) {      // two patches + the exchange area (nine tiles per n-tile)
  return (2 * (size_t)41 * 64 * 4 + 9 * (size_t)(NT >= 2 ? 2 : 1) * 32 * 32) * sizeof(float);
}
static_assert(pp2_lds(2) <= 160 * 1024, "patches + exchange area must fit the 160 KiB LDS");
static hipError_t launch_pp2_impl(const ConvArgs& a, hipStream_t s, int NT, const ConvKernel& k) {
  return launch_conv_kernel(k, 256, pp2_lds(NT), a.Wo / 16, a.Ho / 8, (a.Cout / 32) / NT, a, s);
}
static hipError_t launch_pp2(const ConvArgs& a, hipStream_t s) {
  if (!takes_pp2(conv_shape(a))) return hipErrorInvalidValue;
  if (a.nxt > 0)      // + extra residual terms (HR fuse)
    return a.Cout % 64 == 0 ? launch_pp2_impl(a, s, 2, CONV_KERNEL(conv_pp2_kernel<2, true>)) : launch_pp2_impl(a, s, 1, CONV_KERNEL(conv_pp2_kernel<1, true>));
  return a.Cout % 64 == 0 ? launch_pp2_impl(a, s, 2, CONV_KERNEL(conv_pp2_kernel<2, false>)) : launch_pp2_impl(a, s, 1, CONV_KERNEL(conv_pp2_kernel<1, false>));
}
