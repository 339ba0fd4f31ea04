// 3x3 stride-1 convolution as 2-D Winograd F(2x2,3x3) - included by conv_mfma.hip (uses its loader, work-item and
// epilogue helpers).  16 products per 2x2 output block instead of 36: 2.25x fewer MFMAs than the direct form.
//
// Work item = 8x16 output pixels (32 slots = 2x2 blocks) x 32*NT couts of one frame/group.
//  * loader waves (ws_loader) stream the raw halo'd patch [10][18][CK+4] HBM -> LDS, double buffered, one workgroup
//    barrier per Cin chunk - no arithmetic: on gfx950 a wave's VALU instructions cannot issue while the co-resident
//    wave streams MFMAs (tools/valu_beside_mfma.hip: a partner's v_add_f32 waits for the whole MFMA stream, at any
//    s_setprio), so every VALU instruction of this kernel sits in the MFMA waves' own instruction stream, where the
//    issue slots between two 64-cycle MFMAs hide it.
//  * the 16 Winograd positions are split over the 4 compute waves by row: wave py owns positions (py, 0..3), i.e.
//    4*NT accumulator tiles.  Per 8-channel step a lane reads the two window rows its position row needs
//    (t = d[ra] + sgn*d[rb]: B^T rows are (d0-d2, d1+d2, d2-d1, d1-d3)), 8 ds_read_b128, and forms its 4 activation
//    fragments with 32 VALU operations (v0=t0-t2, v1=t1+t2, v2=t2-t1, v3=t1-t3) for 16*NT MFMAs.
//  * MFMA operands are swapped (weight fragment as A, activation fragment as B): an accumulator tile is
//    D[cout][slot], the lane owns ONE slot and register quad g holds couts 8g+4*lh .. +3.
//  * weights: 16 "taps" U[py][px] = G g G^T (host, fp64), fragments fetched with raw buffer loads whose group /
//    position / step / n-tile offset is scalar (no VALU), refreshed in place right behind the MFMAs that used them.
//  * output transform: x-fold in registers, y-fold across the 4 waves through LDS - the parked tiles are laid out
//    [slot][cout], so the same round trip also turns "lane = slot" into "8 lanes = one pixel's 128-byte line" for
//    the store.  Wave (oy, ox) owns output parity (oy, ox) of every 2x2 block: bias, residual, ReLU, dwordx4 stores.
//  * the chunk body is instantiated per (first, last) chunk of an item: the first MFMA per accumulator takes C = 0
//    (inline constant, accumulators are never cleared by VALU moves), the last chunk carries the epilogue, and no
//    fragment register flows through a control-flow merge (a merge makes hipcc double the fragment buffers).

// ONE: every item is a single Cin chunk (Cin <= CK; NT = 1 only - the exchange area is then double-buffered).
// ODD (NT = 1, Cout = 33: the two segmentation convs): the 33rd output channel does not get a 32-cout tile of its own
// (31 rows of zeros at 64 cycles per MFMA) but rides on v_mfma_f32_4x4x1f32 (16 blocks of 4x4, 8 cycles): the block
// of lanes 4b..4b+3 multiplies its four slots' activations (the same B registers the 32x32x2 MFMAs use) with the
// channel's weight supplied in row 0 of the block (pack_conv replicates cout 32 into every 4th row of the second
// n-tile), so register 0 of a 4-register accumulator collects slot x channel-half partial sums; the two halves
// are added in the epilogue and the value travels through the x/y-fold in the pad column of the parked tiles.
// One eighth of the matrix-pipe time of a padded tile.
// SPLIT (NT = 1, small batches): split-K across CUs.  a.groups is the number of K-slices of ONE convolution: "group" s
// reads input channels [s*Cin, (s+1)*Cin) and its own packed filters (packer: one pack_conv per slice) exactly like a
// grouped convolution, but every slice belongs to the same Cout channels.  A slice's wave writes its folded tile
// (the y[gq] of the second half, before bias / residual / ReLU) to a.split_ws, fences, and counts itself in
// a.split_cnt[(tile, n-block), parity]; the wave that counts LAST re-reads all slices IN SLICE ORDER (also its own: the
// sum does not depend on who arrives last - results are bit-reproducible), adds bias and residual, stores, and re-arms
// the counter.  256->256 at 16x16, one frame: 16 items of 8 chunks become 64 items of 2 chunks (31 -> ~13 us).
template <int NT, int CK, int NLW, bool ONE, bool ODD = false, bool DMA = false, bool SPLIT = false>
__global__ __launch_bounds__((4 + NLW) * 64, 1) void conv_wino2_kernel(const ConvArgs a, const ConvWork wk) {
  static_assert(!ONE || NT == 1, "single-chunk items need the double-buffered exchange area");
  static_assert(!ODD || (NT == 1 && !ONE), "odd output channel: one regular tile, multi-chunk items");
  static_assert(!SPLIT || (NT == 1 && !ONE && !ODD), "split-K: one n-tile per item, >= 2 chunks per slice");
  constexpr int TH = 8, TW = 16, PH = TH + 2, PW = TW + 2, CP = CK + 4;
  constexpr int RAWBUF = PH * PW * CP;
  constexpr int PSTR = 36, PTILE = 32 * PSTR;   // parked tile: [32 slots][32 couts + 4 pad]
  constexpr int PART_W = 2 * NT * PTILE;        // floats one wave parks: [ox][nt] tiles
  extern __shared__ f32x4 smem4[];
  float* lds = reinterpret_cast<float*>(smem4);
  float* part = lds + 2 * RAWBUF;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: position row / output parity in SGPRs
  const int cin_pad = a.cin8 * 8;
  const int nchunks = (cin_pad + CK - 1) / CK;
  const int vb = virtual_block(a);
  const int my_items = wk.total > vb ? (wk.total - 1 - vb) / (int)gridDim.x + 1 : 0;
  const int ktotal = my_items * nchunks;
  if (wave >= 4) {
    // DMA: LDS-DMA loader waves (conv_mfma.hip dma_loader; Cin % 4 == 0) instead of the register-staged ones
    if constexpr (DMA) dma_loader<3, 1, TH, TW, CK, NLW>(a, wk, lds, tid - 256, my_items, nchunks, vb);
    else ws_loader<3, 1, TH, TW, CK, NLW, NoHook, false>(a, wk, lds, tid - 256, ktotal, cin_pad);
    return;
  }
  const int py = wave;
  const int li = lane & 31, lh = lane >> 5;
  // this position row's B^T combination t = d[ra] + sgn * d[rb] and the lane's window origin (block li>>3, li&7)
  const int ra = py == 0 ? 0 : (py == 2 ? 2 : 1);
  const int rb = py == 2 ? 1 : (py == 3 ? 3 : 2);
  const float sgn = py == 1 ? 1.f : -1.f;
  const int worg = (2 * (li >> 3) * PW + 2 * (li & 7)) * CP + 4 * lh;
  const int woff_a = worg + ra * PW * CP, woff_b = worg + rb * PW * CP;
  // store side: this wave writes output parity (oy, ox) of every 2x2 block; lane = (block column p8, cout quad q8),
  // four block rows gq per lane, so 8 lanes cover one pixel's 128-byte line
  const int oy = wave >> 1, ox = wave & 1;
  const int p8 = lane >> 3, q8 = lane & 7;
  const int lane_pix = oy * a.Wo + 2 * p8 + ox;
  const int lane_out = lane_pix * a.out_cs + 4 * q8, lane_res = lane_pix * a.res_cs + 4 * q8;
  const int gs_out = 2 * a.Wo * a.out_cs, gs_res = 2 * a.Wo * a.res_cs;   // block row +1 = two pixel rows down
  const float ysign = oy ? -1.f : 1.f;
  const bool has_res = a.res != nullptr;
  f32x16 acc[4][NT];

  const int tap_b = a.cin8 * a.n_tiles * 1024, step_b = a.n_tiles * 1024;   // weight bytes per position / per step
  const __amdgpu_buffer_rsrc_t wrsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.groups * 16 * tap_b, 0x00020000);
  const unsigned wlane = lane * 16;
  int w = vb, c0 = 0;
  struct WStream {          // weights of one item: byte offset of (group, position row py, n-block) + clamped n-tile offsets
    int base;
    int nto[NT];
  };
  auto wstream = [&](int w_item) -> WStream {
    const ItemPos ip = item_pos(wk, w_item);
    WStream ws;
    ws.base = (ip.g * 16 + py * 4) * tap_b + ip.rest * NT * 1024;
#pragma unroll
    for (int n = 0; n < NT; ++n) ws.nto[n] = (ip.rest * NT + n < a.n_tiles ? n : a.n_tiles - 1 - ip.rest * NT) * 1024;
    return ws;
  };
  // d: the two window rows (4 pixels each) of the NEXT step; v: this step's 4 activation fragments, each replaced
  // by the next step's as soon as its MFMAs are issued; bq: weight fragments, refreshed the same way.
  f32x4 d[2][4], v[4], bq[4][NT];
  f32x4 bo[4], acc33[4];   // ODD: weight fragments / accumulators of the 33rd channel
  auto load_frag = [&](int p, const WStream& ws, int step) {
    const int so = ws.base + p * tap_b + (step < a.cin8 ? step : a.cin8 - 1) * step_b;
#pragma unroll
    for (int n = 0; n < NT; ++n)
      bq[p][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane, so + ws.nto[n], 0));
    if (ODD) bo[p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane, so + 1024, 0));
  };
  auto read_rows = [&](const float* patch, int s) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      d[0][c] = *reinterpret_cast<const f32x4*>(patch + woff_a + c * CP + s * 8);
      d[1][c] = *reinterpret_cast<const f32x4*>(patch + woff_b + c * CP + s * 8);
    }
  };
  // VALU and MFMA instructions exclude each other on a SIMD (tools/valu_beside_mfma.hip: ~4.5 cycles per VALU
  // instruction next to the 64-cycle MFMAs, packed or not), so the transforms want v_pk_*_f32, two floats per issue
  // slot.  Add/subs are written as multiply-adds with a +-1 factor (x * (+-1) is exact, the results are those of the
  // plain form); the factor is a runtime value so that nothing is folded back into v_sub_f32.
  const float neg1f = a.ks == 3 ? -1.f : -2.f;   // always -1 here
  const f32x4 ysign4 = {ysign, ysign, ysign, ysign};
  const f32x16 neg16 = {neg1f, neg1f, neg1f, neg1f, neg1f, neg1f, neg1f, neg1f,
                        neg1f, neg1f, neg1f, neg1f, neg1f, neg1f, neg1f, neg1f};
  // hipcc scalarises these (a wave-uniform factor sits in an SGPR, which v_pk_fma_f32 cannot read for both halves;
  // a vector subtraction becomes v_sub_f32 x4), so the packed instructions are spelled out: (+-1, +-1) pairs pinned
  // in VGPRs, two v_pk_* per float4.
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  f32x2 neg1p = {neg1f, neg1f}, sgnp = {sgn, sgn};
  asm volatile("" : "+v"(neg1p), "+v"(sgnp));
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
  auto row_op = [&](f32x4 (&t)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) t[c] = pk_fma4(sgnp, d[1][c], d[0][c]);
  };
  auto col_op = [&](const f32x4 (&t)[4], int px) -> f32x4 {
    return px == 0   ? pk_fma4(neg1p, t[2], t[0])
           : px == 1 ? pk_add4(t[1], t[2])
           : px == 2 ? pk_fma4(neg1p, t[1], t[2])
                     : pk_fma4(neg1p, t[3], t[1]);
  };

  WStream wsc = wstream(w);
  if (ktotal > 0) {
#pragma unroll
    for (int p = 0; p < 4; ++p) load_frag(p, wsc, 0);
  }
  const bool stamp = a.dbg && blockIdx.x == 0 && tid == 0;   // per chunk: start, MFMAs done, (parked), barrier, (folded)
  int ns_ = 0;
  if (stamp) a.dbg[ns_++] = clock64();
  __syncthreads();   // barrier 0: chunk 0 is in buffer 0
  int k = 0, item_par = 0;
  auto chunk = [&](auto first_tag, auto last_tag) {
    constexpr bool FIRST = decltype(first_tag)::value, LAST = decltype(last_tag)::value;
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    const float* patch = lds + (k & 1) * RAWBUF;
    const int nc0 = LAST ? 0 : c0 + CK, nw = LAST ? w + (int)gridDim.x : w;
    const bool more = k + 1 < ktotal;
    const WStream wsn = (LAST && more) ? wstream(nw) : wsc;
    const int nsteps = (cin_pad - c0 < CK ? cin_pad - c0 : CK) / 8;
    // ---- an item's last chunk: where the item goes (scalar arithmetic), descriptors for its residual and bias
    int rest = 0, ty0 = 0, tx0 = 0;
    float* out_tile = nullptr;
    float* partb = part;
    EpiCtx e;
    f32x4 rv[NT][4], bv[NT];
    float rv33[4], bv33 = 0.f;
    bool vec[NT];
    bool full_tile_ = false;
    __amdgpu_buffer_rsrc_t rrsrc = wrsrc, brsrc = wrsrc;
    int split_grp = 0, split_s = 0;   // SPLIT: (tile, n-block) index and K-slice of this item
    auto s2p = [&](int p, bool& ok) -> int {
      int y = ty0 + 2 * (p >> 3) + oy, x = tx0 + 2 * (p & 7) + ox;
      ok = y < a.Ho && x < a.Wo;
      y = y < a.Ho ? y : a.Ho - 1;
      x = x < a.Wo ? x : a.Wo - 1;
      return y * a.Wo + x;
    };
    if (LAST) {
      const ItemPos ip = item_pos(wk, w);
      const int g = SPLIT ? 0 : ip.g, b = ip.b;      // SPLIT: the slices share bias, residual and output channels
      rest = ip.rest;
      ty0 = ip.ty * 8;
      tx0 = ip.tx * 16;
      if (SPLIT) {
        split_s = ip.g;
        split_grp = ((b * wk.tiles_per_frame + ip.ty * wk.tiles_x + ip.tx) * wk.nblk + ip.rest);
      }
      e.bias = a.bias + (size_t)g * a.n_tiles * 32 + (size_t)b * a.bias_fstride;
      e.outb = a.out + (size_t)b * a.Ho * a.Wo * a.out_cs + a.out_coff + g * a.Cout;
      e.resb = has_res ? a.res + res_frame_off(a, b) + a.res_coff + g * a.Cout : nullptr;
      e.res_cs = a.res_cs; e.out_cs = a.out_cs; e.Cout = a.Cout; e.relu = a.relu;
      e.vec_align = ((a.out_coff + g * a.Cout) % 4 == 0) && (a.out_cs % 4 == 0) &&
                    (!has_res || (((a.res_coff + g * a.Cout) % 4 == 0) && (a.res_cs % 4 == 0)));
      const bool full_tile = (ty0 + 8 <= a.Ho) && (tx0 + 16 <= a.Wo);
      full_tile_ = full_tile;
#pragma unroll
      for (int n = 0; n < NT; ++n) vec[n] = full_tile && e.vec_align && ((rest * NT + n + 1) * 32 <= a.Cout);
      // tile-relative descriptors: the lane part of an address is a kernel-constant VGPR, everything else a scalar
      // offset - no 64-bit address pairs in vector registers while the accumulators are live
      const int tile_pix = ty0 * a.Wo + tx0;
      out_tile = e.outb + (size_t)tile_pix * a.out_cs;
      // (records = what is left of the residual tensor behind the tile origin: a clamped n-tile of a ragged Cout may
      // point past a pixel's channels, never past the tensor)
      const size_t res_off = (res_frame_off(a, b) + (size_t)tile_pix * a.res_cs) + a.res_coff + g * a.Cout;
      const size_t res_left = (res_total(a) - res_off) * 4;
      rrsrc = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(has_res ? a.res + res_off : a.in), 0,
          (has_res && full_tile && e.vec_align) ? (int)(unsigned)(res_left > 0xffffffffu ? 0xffffffffu : res_left) : 0,
          0x00020000);
      brsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(e.bias), 0, bias_row_left(a, g), 0x00020000);
    }
    // the item's residual and bias: unconditional raw buffer loads (a zero-record descriptor returns 0 without
    // memory traffic when there is no residual or the tile takes the generic path).  With NT = 1 there are registers
    // to spare and the request goes out when the item's last chunk starts; with NT = 2 it waits for the last step,
    // whose d/t registers it takes over.
    constexpr bool EARLY_RES = NT == 1;
    auto request_res = [&]() {
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int ntc = rest * NT + n < a.n_tiles ? rest * NT + n : a.n_tiles - 1;
        bv[n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(brsrc, 16 * q8, ntc * 128, 0));
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
          rv[n][gq] = __builtin_bit_cast(
              f32x4, __builtin_amdgcn_raw_buffer_load_b128(rrsrc, lane_res * 4, (ntc * 32 + gq * gs_res) * 4, RES_CACHE_WINO));
      }
      if (ODD) {   // channel 32 of the same pixels (zero-record descriptor: 0 without a residual / on ragged tiles)
        bv33 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(brsrc, 0, 128, 0));
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
          rv33[gq] = __builtin_bit_cast(
              float, __builtin_amdgcn_raw_buffer_load_b32(rrsrc, (lane_res - 4 * q8) * 4, (32 + gq * gs_res) * 4, 0));
      }
    };
    if (LAST && EARLY_RES) request_res();
    // first fragments of the chunk (the patch only became visible at the barrier)
    read_rows(patch, 0);
    {
      f32x4 t[4];
      row_op(t);
#pragma unroll
      for (int px = 0; px < 4; ++px) v[px] = col_op(t, px);
    }
    // one 8-channel step: 4 groups of 4*NT MFMAs.  The next step's window rows are requested with group 0 and
    // row-combined with group 2 (d and t never live together); behind its group's MFMAs each fragment is replaced
    // by the next step's (activation: column combination; weights: buffer load).  A chunk's last step reads and
    // combines a defined but unused row.
    // TAIL: the last step of an item.  There is no next fragment to build, so (NT = 2) the registers of d and t take
    // the item's residual and bias instead, requested with group 0 - by the epilogue's second half they have had
    // the rest of the step, the x-fold and the barrier to arrive.
    auto step = [&](int s, auto zero_tag, auto tail_tag) {
      constexpr bool ZERO = decltype(zero_tag)::value, TAIL = decltype(tail_tag)::value;
      const bool last_step = s + 1 >= nsteps;
      f32x4 t[4];
#pragma unroll
      for (int px = 0; px < 4; ++px) {
        __builtin_amdgcn_sched_barrier(0);
        if (TAIL) {
          if (px == 0 && !EARLY_RES) request_res();
        } else {
          if (px == 0) read_rows(patch, s + 1);
          if (px == 2) row_op(t);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            if (ZERO && j == 0) {
              const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
              acc[px][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[px][n][j], v[px][j], zero, 0, 0, 0);
            } else {
              acc[px][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[px][n][j], v[px][j], acc[px][n], 0, 0, 0);
            }
          }
        if (ODD) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (ZERO && j == 0) {
              const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
              acc33[px] = __builtin_amdgcn_mfma_f32_4x4x1f32(bo[px][j], v[px][j], zero4, 0, 0, 0);
            } else {
              acc33[px] = __builtin_amdgcn_mfma_f32_4x4x1f32(bo[px][j], v[px][j], acc33[px], 0, 0, 0);
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (!TAIL) {
          if (px == 2) {
            v[0] = col_op(t, 0);
            v[1] = col_op(t, 1);
            v[2] = col_op(t, 2);
          }
          if (px == 3) v[3] = col_op(t, 3);
          // next step, or the first step of the same item's next chunk.  The load is unconditional - behind a
          // branch hipcc can no longer count the loads in flight and waits for vmcnt(0), i.e. for the fragments it
          // has just requested.  (The next item's first fragments go out from the epilogue, when the accumulator
          // registers are free.)
          const int nstep = last_step ? nc0 / 8 : c0 / 8 + s + 1;
          load_frag(px, wsc, nstep);
        }
      }
    };
    if (LAST) {
      if (FIRST && nsteps == 1) {
        step(0, std::true_type(), std::true_type());
      } else {
        int s = 0;
        if (FIRST) {
          step(0, std::true_type(), std::false_type());
          s = 1;
        }
        for (; s < nsteps - 1; ++s) step(s, std::false_type(), std::false_type());
        step(nsteps - 1, std::false_type(), std::true_type());
      }
    } else {
      int s = 0;
      if (FIRST) {
        step(0, std::true_type(), std::false_type());
        s = 1;
      }
      for (; s < nsteps; ++s) step(s, std::false_type(), std::false_type());
    }
    __builtin_amdgcn_sched_barrier(0);
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();

    // ---- item epilogue, first half (before the chunk barrier): x-fold, park for the y-fold
    if (LAST) {
      // with one chunk per item the next item parks before every wave has read this one's tiles: two areas
      if (NT == 1) partb = part + item_par * 4 * PART_W;
      // park the x-folded tiles as [slot][cout] (row stride 36 floats): the writer lane holds 4 consecutive couts
      // per register quad, the reader picks (pixel, cout quad) cells in NHWC store order
      float* pw = partb + wave * PART_W + li * PSTR + 4 * lh;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const f32x16 r0 = acc[0][n] + acc[1][n] + acc[2][n];
        const f32x16 r1 = __builtin_elementwise_fma(acc[2][n] + acc[3][n], neg16, acc[1][n]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          *reinterpret_cast<f32x4*>(pw + (0 * NT + n) * PTILE + 8 * q) = f32x4{r0[4 * q], r0[4 * q + 1], r0[4 * q + 2], r0[4 * q + 3]};
          *reinterpret_cast<f32x4*>(pw + (1 * NT + n) * PTILE + 8 * q) = f32x4{r1[4 * q], r1[4 * q + 1], r1[4 * q + 2], r1[4 * q + 3]};
        }
      }
      if (ODD) {   // x-fold, add the two channel halves (lanes l and l^32 hold the same slot), park in column 32
        float r0 = acc33[0][0] + acc33[1][0] + acc33[2][0];
        float r1 = __builtin_fmaf(acc33[2][0] + acc33[3][0], neg1f, acc33[1][0]);
        r0 += __shfl_xor(r0, 32, 64);
        r1 += __shfl_xor(r1, 32, 64);
        float* pw33 = partb + wave * PART_W + li * PSTR + 32;
        pw33[0 * NT * PTILE] = r0;     // (both halves write the same value)
        pw33[1 * NT * PTILE] = r1;
      }
      // the weight fragments of the next item's first step go out now that the accumulators are dead (the barrier
      // and the second half cover their L2 latency)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int p = 0; p < 4; ++p) load_frag(p, wsn, 0);
      if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    }
    __syncthreads();   // barrier k+1
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    // ---- second half: y-fold (oy = 0: R0+R1+R2, oy = 1: R1-R2-R3) of this wave's output parity, then store
    if (LAST) {
      const float* pr = partb + (ox * NT) * PTILE + p8 * PSTR + 4 * q8;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int n_tile = rest * NT + n;
        if (n_tile >= a.n_tiles) continue;
        f32x4 y[4];   // block row gq, block column p8, couts 4*q8 .. 4*q8+3
        {
          f32x4 pp[3][4];   // all 12 LDS reads of the tile in flight before the first add (one latency, not four)
#pragma unroll
          for (int gq = 0; gq < 4; ++gq)
#pragma unroll
            for (int j = 0; j < 3; ++j)
              pp[j][gq] = *reinterpret_cast<const f32x4*>(pr + (oy + j) * PART_W + n * PTILE + 8 * gq * PSTR);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) y[gq] = __builtin_elementwise_fma(pp[1][gq] + pp[2][gq], ysign4, pp[0][gq]);
        }
        if constexpr (SPLIT) {
          // The partial tiles and the counter live at the device's coherence point: sc0 sc1 stores write through the
          // (per-XCD, mutually incoherent) L2s, sc0 sc1 loads bypass them, the counter is an agent-scope atomic.  No
          // cache-wide fence: __threadfence() here means an L2 write-back + invalidate per wave (measured: batch-8 call
          // 6.9 -> 13.5 ms, every concurrent kernel pays).
          // (buffer builtins with the cache-policy operand rather than inline asm: hipcc does not know an asm store's data
          //  hazards and lets a VALU write follow it into the registers it is still reading - garbage tiles, measured)
          constexpr int SC01 = 1 | 16;                   // aux: sc0 (bit 0) + sc1 (bit 4) = system scope on gfx950
          const int S = a.groups;
          const __amdgpu_buffer_rsrc_t srsrc = __builtin_amdgcn_make_buffer_rsrc(
              a.split_ws + (size_t)split_grp * S * 4096, 0, S * 4096 * 4, 0x00020000);      // this (tile, n-block)'s S tiles
          const int my_off = ((split_s * 4 + wave) * 256 + lane) * 16;
#pragma unroll
          for (int gq = 0; gq < 4; ++gq)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, y[gq]), srsrc, my_off + gq * 1024, 0, SC01);
          __builtin_amdgcn_s_waitcnt(0x0f70);            // vmcnt(0) (gfx9 encoding; expcnt / lgkmcnt not waited for): the
                                                         // tile has reached memory before this wave is counted
          unsigned* cnt = a.split_cnt + (size_t)split_grp * 4 + wave;
          unsigned old = 0;
          if (lane == 0) old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          old = __builtin_amdgcn_readfirstlane(old);
          if (old + 1 != (unsigned)S) continue;          // another slice's wave finishes this (tile, n-block, parity)
          const int rd_off = (wave * 256 + lane) * 16;
#pragma unroll
          for (int gq = 0; gq < 4; ++gq)
            y[gq] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srsrc, rd_off + gq * 1024, 0, SC01));
          for (int sl = 1; sl < S; ++sl) {
            f32x4 t4[4];
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
              t4[gq] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srsrc, rd_off + gq * 1024, sl * 16384, SC01));
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) y[gq] += t4[gq];
          }
          // re-armed for the next launch (stream-ordered behind this one)
          if (lane == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        if (vec[n]) {   // full tile, aligned channel slices: bias, residual, ReLU, one full 128-byte line per 8 lanes
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) {
            f32x4 o4 = y[gq] + bv[n];
            if (has_res) o4 += rv[n][gq];
            if (a.relu) {
              o4[0] = vrelu1(o4[0]); o4[1] = vrelu1(o4[1]); o4[2] = vrelu1(o4[2]); o4[3] = vrelu1(o4[3]);
            }
            // global (not buffer) store: on gfx950 a buffer_store_dwordx4 with an SGPR soffset was observed to pick
            // up a VALU write to its data registers issued right behind it (hipcc inserts no wait state there)
            char* ub = reinterpret_cast<char*>(out_tile + n_tile * 32 + gq * gs_out);   // uniform base
            __builtin_nontemporal_store(o4, reinterpret_cast<f32x4*>(ub + (unsigned)(lane_out * 4)));
          }
        } else {        // ragged tile / ragged or unaligned channels: element-wise
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) {
            bool ok;
            const int pix = s2p(8 * gq + p8, ok);
#pragma unroll
            for (int e4 = 0; e4 < 4; ++e4) {
              const int co = n_tile * 32 + 4 * q8 + e4;
              if (ok && co < a.Cout) {
                float o1 = y[gq][e4] + e.bias[co];
                if (has_res) o1 += e.resb[(size_t)pix * a.res_cs + co];
                if (a.relu) o1 = vrelu1(o1);
                e.outb[(size_t)pix * a.out_cs + co] = o1;
              }
            }
          }
        }
      }
      if (ODD) {   // channel 32: the 8 lanes of a pixel hold (and store) the same value
        const float* pr33 = partb + (ox * NT) * PTILE + p8 * PSTR + 32;
        float o33[4];
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const float p0 = pr33[(oy + 0) * PART_W + 8 * gq * PSTR], p1 = pr33[(oy + 1) * PART_W + 8 * gq * PSTR],
                      p2 = pr33[(oy + 2) * PART_W + 8 * gq * PSTR];
          o33[gq] = __builtin_fmaf(p1 + p2, ysign, p0);
        }
        if (full_tile_ && e.vec_align) {
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) {
            float o1 = o33[gq] + bv33;
            if (has_res) o1 += rv33[gq];
            if (a.relu) o1 = vrelu1(o1);
            char* ub = reinterpret_cast<char*>(out_tile + 32 + gq * gs_out);
            *reinterpret_cast<float*>(ub + (unsigned)((lane_out - 4 * q8) * 4)) = o1;
          }
        } else {
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) {
            bool ok;
            const int pix = s2p(8 * gq + p8, ok);
            if (ok) {
              float o1 = o33[gq] + e.bias[32];
              if (has_res) o1 += e.resb[(size_t)pix * a.res_cs + 32];
              if (a.relu) o1 = vrelu1(o1);
              e.outb[(size_t)pix * a.out_cs + 32] = o1;
            }
          }
        }
      }
      if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
      item_par ^= 1;
    }
    wsc = wsn;
    c0 = nc0;
    w = nw;
    ++k;
  };
  for (int item = 0; item < my_items; ++item) {
    if constexpr (ONE) {
      chunk(std::true_type(), std::true_type());
    } else {   // nchunks >= 2 (checked by the host)
      chunk(std::true_type(), std::false_type());
      for (int ci = 2; ci < nchunks; ++ci) chunk(std::false_type(), std::false_type());
      chunk(std::false_type(), std::true_type());
    }
  }
  if (stamp) a.dbg[63] = ns_;
}

template <int NT, int CK, int NLW, bool ONE, bool ODD = false, bool DMA = false, bool SPLIT = false>
static hipError_t launch_wino2_impl(const ConvArgs& a, hipStream_t s) {
  constexpr size_t lds = (2 * (size_t)10 * 18 * (CK + 4) + (NT == 1 ? 2 : 1) * 4 * (size_t)2 * NT * 32 * 36) * sizeof(float);
  static_assert(lds <= 160 * 1024, "two patch buffers and the exchange area must fit the 160 KiB LDS");
  // ODD: the item's one regular tile carries the 33rd channel along
  return launch_conv_kernel(CONV_KERNEL(conv_wino2_kernel<NT, CK, NLW, ONE, ODD, DMA, SPLIT>), (4 + NLW) * 64, lds, (a.Wo + 15) / 16,
                            (a.Ho + 7) / 8, ODD ? 1 : (a.n_tiles + NT - 1) / NT, a, s);
}

// LDS-DMA loader waves where the input allows it (channel quads wholly inside / outside Cin); ACRMI_CONV_DMA=0 keeps the
// register-staged loader everywhere (A/B runs)
static bool conv_dma_ok(const ConvArgs& a) {
  static const char* env = experiment_env("ACRMI_CONV_DMA");
  return (!env || atoi(env) != 0) && takes_dma(conv_shape(a));
}
// conv_wino2_kernel: measured 23.3 ms (LDS-DMA) vs 22.2 ms (register loader) over the network's 157 launches - with
// two LDS buffers only one chunk is in flight, the register loader runs two ahead.  ACRMI_CONV_DMA=2 selects it anyway.
static bool conv_dma_wino2(const ConvArgs& a) {
  static const char* env = experiment_env("ACRMI_CONV_DMA");
  return env && atoi(env) >= 2 && conv_dma_ok(a);
}

template <int NT, int CK, int NLW>
static hipError_t launch_wino2(const ConvArgs& a, hipStream_t s) {
  const bool one = (a.cin8 * 8 + CK - 1) / CK < 2;
  const bool dma = conv_dma_wino2(a);
  if constexpr (NT == 1) {
    if (a.splitk) {      // K-slices as groups (conv_wino2_kernel SPLIT): >= 2 chunks per slice, workspace from the caller
      if (one || !a.split_ws || !a.split_cnt || a.groups < 2) return hipErrorInvalidValue;
      return launch_wino2_impl<1, CK, NLW, false, false, false, true>(a, s);
    }
    if (!one && a.Cout == 33 && a.groups == 1 && g_force_cfg != 804)
      return dma ? launch_wino2_impl<1, CK, NLW, false, true, true>(a, s) : launch_wino2_impl<1, CK, NLW, false, true>(a, s);
    if (one) return dma ? launch_wino2_impl<1, CK, NLW, true, false, true>(a, s) : launch_wino2_impl<1, CK, NLW, true>(a, s);
    return dma ? launch_wino2_impl<1, CK, NLW, false, false, true>(a, s) : launch_wino2_impl<1, CK, NLW, false>(a, s);
  } else {
    if (one || a.splitk) return hipErrorInvalidValue;   // single-buffered exchange area: an item needs >= 2 chunks
    return dma ? launch_wino2_impl<NT, CK, NLW, false, false, true>(a, s) : launch_wino2_impl<NT, CK, NLW, false>(a, s);
  }
}
