// 3x3 stride-1 convolution with Cin <= 32 and Cout = 32 (HRNet branch 0: 72 of the network's 222 Winograd launches,
// the least efficient ones of round 1 at 42 % matrix-pipe occupancy) as 2-D Winograd F(2x2,3x3) on
// v_mfma_f32_16x16x4_f32 - included by conv_mfma.hip (uses its loader and work-item helpers).
//
// conv_wino2_kernel splits the 16 Winograd positions over four waves, so every item ends with an exchange of the
// x-folded tiles through LDS, a workgroup barrier and a second half that reads them back: with one Cin chunk per item
// nothing overlaps that tail (r01 stamps: 6.4k cycles of MFMA phase + 0.7k park + 2.2k store per 4.1k of MFMAs).  Here
// a wave owns ALL 16 positions of a 16-slot x 16-cout tile (16 accumulators of 4 registers - the same 64 registers
// as 4 tiles of 32x32), so
//  * the output transform A^T M A happens in registers (24 float4 operations), no exchange, no second barrier: the
//    only workgroup barrier of an item is the patch hand-over with the loader waves, and it sits in the MIDDLE of
//    the item (after the last window read), so it never has a wave's epilogue behind it;
//  * the layer's transformed weights (16 positions x 32 x 32 floats = 64 KiB) live in LDS for the whole launch:
//    weight fragments are ds_read_b128 (+1 cycle beside an MFMA) instead of global loads (+16), through a ring that
//    runs continuously over the cyclic (position, step) sequence - it never restarts at an item boundary;
//  * lane (slot j = lane & 15, channel quad kq = lane >> 4) reads the 4x4 window of its slot as 16 ds_read_b128 per
//    16-channel step and forms all 16 position fragments with 32 float4 add/subs (v_pk_add_f32 with neg modifiers:
//    exact, no multiplier register).  The slot -> (block row, block column) map is chosen so that the 16 lanes of
//    every ds_read_b128 lane group hit 16 different bank quads with the patch's 36-float pixel stride.
// MFMA operands: A = weights W[pos][cout = 16*ch + (lane & 15)][cin = 16 s + 4 kq + e], B = activations
// V[pos][slot][cin]; D[cout = 4*(lane >> 4) + r][slot = lane & 15]: a lane ends up with 4 consecutive couts of its
// slot's 2x2 output block = one 16-byte store per output pixel (4 lanes = one 64-byte segment).
//
// Workgroup = NCW compute waves + NLW loader waves; NCW = TH / 2: (slot group sg = 2 block rows) x (cout half ch).
//  * TH = 8  (4 compute waves, one per SIMD, <= 256 registers): the next step's fragments are built in the gaps of the
//    current step's MFMA stream (PIPE).
//  * TH = 16 (8 compute waves, two per SIMD, <= 168 registers): fragments are built between the MFMA streams and the
//    SIMD's other wave fills the gap.
// Store waves of conv_wino3_kernel (NSW = 2).  A compute wave's epilogue store writes 64 bytes per pixel (4 lanes x 16
// bytes - the other cout half of the pixel's 128-byte line belongs to another wave) and costs it ~250 cycles per
// instruction, 4 per item.  With store waves the epilogue ends in ds_write_b128 to a staging tile [pixel][32 couts]
// (double buffered) and two VALU-free waves write the tile out behind the next item's barrier: ds_read_b128 +
// non-temporal global_store_dwordx4, 8 lanes = one pixel's full 128-byte line, addresses = per-item scalar base +
// constant lane offset.  (The weights of these layers come from LDS, so - unlike in conv_wino2_kernel, where the same
// idea lost - the flush does not compete with any global load of the compute waves.)
// DUAL (ConvArgs.out2): the store waves also write relu(((tile + up(xt0)) + up(xt1)) + up(xt2)) - the HR-module fuse sum of the
// full resolution (acr/model.py:672-686, i = 0: this conv's output + the 1x1-projected lower branches, nearest-upsampled by
// 2^shift) - to a second map.  The store waves are VALU-free otherwise and have a whole item's time per tile: per octet three
// 16-byte loads (neighbouring pixels share their low-resolution source: L1 / L2 hits), three float4 adds, a max, one more store.
template <int TH, bool DUAL = false>
__device__ __forceinline__ void wino3_store_waves(const ConvArgs& a, const ConvWork& wk, const float* stage, int sw, int lane,
                                                  int my_items, int vb) {
  constexpr int TW = 16, STILE = TH * TW * 32, NI = TH * TW / 8 / 2;   // 8-pixel octets per wave and item
  const int pin = lane >> 3, q = lane & 7;
  const unsigned lane_out = (unsigned)(pin * a.out_cs + 4 * q) * 4u;
  const unsigned lane_out2 = (unsigned)(pin * a.out2_cs + 4 * q) * 4u;
  // octet t of the tile = pixel row t / 2, columns 8 (t & 1) + pin: key of the pixel's column swizzle
  int soff[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int t = sw * NI + i, row = t >> 1, col = 8 * (t & 1) + pin;
    soff[i] = (row * TW + col) * 32 + 4 * (q ^ (((col >> 1) + 4 * ((row >> 1) & 1)) & 7));
  }
  // DUAL: the terms of item kk are REQUESTED one item ahead (they depend on the item's position only, not on the staged tile):
  // their latency runs beside the compute waves' next item instead of inside the flush, whose budget is one item's time
  f32x4 tv[DUAL ? 3 : 1][NI];
  auto request_terms = [&](int kk) {
    if constexpr (DUAL) {
      const ItemPos ip = item_pos(wk, vb + kk * (int)gridDim.x);
#pragma unroll
      for (int tt = 0; tt < 3; ++tt) {
        // term tt at this frame: descriptor (zero records when the term does not exist: the loads return 0), the lane's
        // column part per octet parity, the row part on the scalar unit
        const bool on = tt < a.nxt;
        const int sh = on ? a.xt_shift[tt] : 0, cs = on ? a.xt_cs[tt] : 4;
        const int hs = a.Ho >> sh, wsx = a.Wo >> sh;
        const size_t off = (size_t)ip.b * hs * wsx * cs + (on ? a.xt_coff[tt] : 0);
        const size_t left = on ? ((size_t)a.B * hs * wsx * cs - off) * 4 : 0;
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(on ? a.xt[tt] + off : a.in), 0, (int)(unsigned)(left > 0xffffffffu ? 0xffffffffu : left), 0x00020000);
        unsigned xo[2];
#pragma unroll
        for (int hp = 0; hp < 2; ++hp) xo[hp] = (unsigned)((((ip.tx * TW + 8 * hp + pin) >> sh) * cs + 4 * q) * 4);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int t = sw * NI + i;
          const int so = (((ip.ty * TH + (t >> 1)) >> sh) * wsx) * cs * 4;
          tv[tt][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, xo[t & 1], so, 0));
        }
      }
    }
  };
  auto flush = [&](int kk) {
    const ItemPos ip = item_pos(wk, vb + kk * (int)gridDim.x);
    const size_t tile_pix = ((size_t)ip.b * a.Ho + (size_t)ip.ty * TH) * a.Wo + (size_t)ip.tx * TW;
    float* out_tile = a.out + tile_pix * a.out_cs + a.out_coff;
    const float* st = stage + (kk & 1) * STILE;
    f32x4 v[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) v[i] = *reinterpret_cast<const f32x4*>(st + soff[i]);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int t = sw * NI + i;
      char* ub = reinterpret_cast<char*>(out_tile + ((t >> 1) * a.Wo + 8 * (t & 1)) * a.out_cs);   // uniform
      __builtin_nontemporal_store(v[i], reinterpret_cast<f32x4*>(ub + lane_out));
    }
    if constexpr (DUAL) {
      float* out2_tile = a.out2 + tile_pix * a.out2_cs + a.out2_coff;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int t = sw * NI + i;
        f32x4 y = ((v[i] + tv[0][i]) + tv[1][i]) + tv[2][i];
        y[0] = vrelu1(y[0]); y[1] = vrelu1(y[1]); y[2] = vrelu1(y[2]); y[3] = vrelu1(y[3]);
        char* ub = reinterpret_cast<char*>(out2_tile + ((t >> 1) * a.Wo + 8 * (t & 1)) * a.out2_cs);   // uniform
        __builtin_nontemporal_store(y, reinterpret_cast<f32x4*>(ub + lane_out2));
      }
    }
  };
  if (my_items >= 1) request_terms(0);
  __syncthreads();   // barrier 0
  for (int k = 0; k < my_items; ++k) {
    __syncthreads();   // barrier k + 1: every compute wave is past item k - 1's epilogue
    if (k >= 1) {
      flush(k - 1);
      request_terms(k);      // (the registers of item k - 1's terms are free now)
    }
  }
  __syncthreads();     // the last item is staged
  if (my_items >= 1) flush(my_items - 1);
}

// timing ablations (tools/exp_build.sh -DACRMI_W3_ABLATE=bits; WRONG results): 1 = no input-transform VALU, 2 = no window
// reads, 4 = no weight-ring reads, 8 = no epilogue arithmetic / staging writes
#ifndef ACRMI_W3_ABLATE
#define ACRMI_W3_ABLATE 0
#endif
template <int TH, int NLW, bool PIPE, int LPRIO = 0, bool DMA = false, int NSW = 0, bool DUAL = false>
__global__ __launch_bounds__((TH / 2 + NLW + NSW) * 64, 1) void conv_wino3_kernel(const ConvArgs a, const ConvWork wk) {
  constexpr int W3_ABLATE = ACRMI_W3_ABLATE;
  static_assert(!DUAL || NSW == 2, "the second output is written by the store waves");
  constexpr int TW = 16, PH = TH + 2, PW = TW + 2, CK = 32, CP = CK + 4;
  constexpr int NCW = TH / 2;
  constexpr int RAWBUF = PH * PW * CP;
  constexpr int WFLOATS = 16 * 2 * 2 * 256;        // [pos][step][cout half][lane][4]
  constexpr int STILE = TH * TW * 32;              // NSW: output staging tile [pixel][32 couts], two of them
  static_assert(NSW == 0 || (NSW == 2 && TH == 8), "store waves: two, 8x16-pixel items");
  extern __shared__ f32x4 smem4[];
  float* lds = reinterpret_cast<float*>(smem4);
  float* wlds = lds + 2 * RAWBUF;
  float* stage = wlds + WFLOATS;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cin_pad = a.cin8 * 8;
  const int vb = virtual_block(a);
  const int my_items = wk.total > vb ? (wk.total - 1 - vb) / (int)gridDim.x + 1 : 0;
  if constexpr (NSW > 0) {
    if (wave >= NCW + NLW) {
      wino3_store_waves<TH, DUAL>(a, wk, stage, wave - NCW - NLW, lane, my_items, vb);
      return;
    }
  }
  if (wave >= NCW) {
    if constexpr (DMA) dma_loader<3, 1, TH, TW, CK, NLW>(a, wk, lds, tid - NCW * 64, my_items, 1, vb);   // (conv_mfma.hip)
    else ws_loader<3, 1, TH, TW, CK, NLW, NoHook, false, LPRIO>(a, wk, lds, tid - NCW * 64, my_items, cin_pad);
    if constexpr (NSW > 0) __syncthreads();   // the store waves' last hand-over
    return;
  }
  // ---- the layer's weights -> LDS (64 KiB, once per workgroup; visible after barrier 0)
  {
    const f32x4* src = reinterpret_cast<const f32x4*>(a.w);
    f32x4* dst = reinterpret_cast<f32x4*>(wlds);
    constexpr int PER = WFLOATS / 4 / (NCW * 64);
    f32x4 tmp[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) tmp[i] = src[tid + i * NCW * 64];
#pragma unroll
    for (int i = 0; i < PER; ++i) dst[tid + i * NCW * 64] = tmp[i];
  }
  const int ch = wave & 1, sg = wave >> 1;
  const int j = lane & 15, kq = lane >> 4;
  // slot j -> block (brow, bcol) of this wave's two block rows: lanes {0-3, 12-15} take block row 0, lanes {4-11}
  // block row 1 - the ds_read_b128 lane groups ({0-3,12-15,20-27}, {4-11,16-19,28-31}, +32) then see 8 block
  // columns of one row (even bank quads) next to 8 of the other row's kq+1 lanes (odd quads): conflict free
  const int in_a = (j < 4) || (j >= 12);
  const int brow = in_a ? 0 : 1;
  const int bcol = in_a ? (j < 4 ? j : j - 8) : j - 4;
  const int by = 2 * sg + brow;                                      // block row inside the tile
  const int worg = ((2 * by) * PW + 2 * bcol) * CP + 4 * kq;         // window origin (floats) inside a patch
  const float* wfrag = wlds + ch * 256 + lane * 4;                   // + (pos * 2 + step) * 512
  const bool has_res = a.res != nullptr;
  // output: pixel (oy, ox) of the block = tile pixel (2 by + oy, 2 bcol + ox), couts 16 ch + 4 kq .. +3
  const int lane_pix = (2 * by) * a.Wo + 2 * bcol;
  // (byte offsets: addresses are "uniform base + 32-bit lane offset", no 64-bit pointer pairs in vector registers)
  const unsigned lane_out = (unsigned)(lane_pix * a.out_cs + 16 * ch + 4 * kq) * 4u;
  const unsigned lane_res = (unsigned)(lane_pix * a.res_cs + 16 * ch + 4 * kq) * 4u;
  const f32x4 bias4 = *reinterpret_cast<const f32x4*>(a.bias + 16 * ch + 4 * kq);
  // NSW: staging cell of the block's pixel (0, 0): [pixel][8 x 16 bytes], 16-byte column XOR (bcol + 4 brow) & 7 -
  // the 8 lanes of a ds_write_b128 lane group (8 slots, one channel quad) land on 8 different columns
  const int stage_off = ((2 * by) * TW + 2 * bcol) * 32 + 4 * ((4 * ch + kq) ^ ((bcol + 4 * brow) & 7));

  typedef float f32x2 __attribute__((ext_vector_type(2)));
  auto pk_add4 = [](const f32x4& b, const f32x4& c) -> f32x4 {
    f32x2 lo, hi;
    const f32x2 b0 = {b[0], b[1]}, b1 = {b[2], b[3]}, c0 = {c[0], c[1]}, c1 = {c[2], c[3]};
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(lo) : "v"(b0), "v"(c0));
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(hi) : "v"(b1), "v"(c1));
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
  };
  auto pk_sub4 = [](const f32x4& b, const f32x4& c) -> f32x4 {   // b - c (negation is exact)
    f32x2 lo, hi;
    const f32x2 b0 = {b[0], b[1]}, b1 = {b[2], b[3]}, c0 = {c[0], c[1]}, c1 = {c[2], c[3]};
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(lo) : "v"(b0), "v"(c0));
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(hi) : "v"(b1), "v"(c1));
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
  };
  // B^T d B in two passes over a 4x4 array of float4 (rows first, then columns), in place:
  // (x0, x1, x2, x3) -> (x0 - x2, x1 + x2, x2 - x1, x1 - x3)
  auto bt4 = [&](f32x4& x0, f32x4& x1, f32x4& x2, f32x4& x3) {   // (one temporary: the 8-wave variant is register bound)
    x0 = pk_sub4(x0, x2);
    x3 = pk_sub4(x1, x3);
    const f32x4 t = pk_add4(x1, x2);
    x2 = pk_sub4(x2, x1);
    x1 = t;
  };
  f32x4 acc[16];
  // fragments V[pos = py*4 + px] of the two 16-channel steps of an item: while one set feeds the MFMAs the other is
  // built in place from a window [wy*4 + wx] (row pass, then column pass) - the sets swap roles every step
  f32x4 va[16], vb_[16];
  f32x4 wr[4];        // weight-fragment ring: two position pairs
  f32x4 rv[4];        // residual of the lane's 4 output pixels

  auto read_column = [&](f32x4 (&d)[16], const float* patch, int s, int wx) {
    if (W3_ABLATE & 2) return;
#pragma unroll
    for (int wy = 0; wy < 4; ++wy)
      d[wy * 4 + wx] = *reinterpret_cast<const f32x4*>(patch + worg + (wy * PW + wx) * CP + 16 * s);
  };
  auto read_window = [&](f32x4 (&d)[16], const float* patch, int s) {
#pragma unroll
    for (int wx = 0; wx < 4; ++wx) read_column(d, patch, s, wx);
  };
  // transform work is cut into 8 pieces (4 window columns for the row pass, 4 position rows for the column pass)
  auto transform_piece = [&](f32x4 (&d)[16], int piece) {
    if (W3_ABLATE & 1) return;
    if (piece < 4) bt4(d[piece], d[4 + piece], d[8 + piece], d[12 + piece]);                  // rows: per window column
    else bt4(d[(piece - 4) * 4], d[(piece - 4) * 4 + 1], d[(piece - 4) * 4 + 2], d[(piece - 4) * 4 + 3]);
  };
  // weight fragments of position pair g (cyclic, step-major: g = s*8 + pair) -> ring slots 2*(g & 1), +1
  auto ring_load = [&](int g) {
    if ((W3_ABLATE & 4) && g > 1) return;
    const int gg = g & 15, s = gg >> 3, p0 = (gg & 7) * 2;
    wr[(g & 1) * 2] = *reinterpret_cast<const f32x4*>(wfrag + (p0 * 2 + s) * 512);
    wr[(g & 1) * 2 + 1] = *reinterpret_cast<const f32x4*>(wfrag + ((p0 + 1) * 2 + s) * 512);
  };
  // one 16-channel step: 8 position pairs x (2 x 4) MFMAs.  The two positions of a pair alternate, so consecutive
  // MFMAs never depend on each other (v_mfma_f32_16x16x4_f32: 32 cycles issue, 40 dependent).  In FRONT of pair g's
  // MFMAs the ring slots of pair g-1 are refilled with pair g+1: those MFMAs were issued >= 256 cycles ago (no wait
  // states) and the fragments have pair g's 256 cycles to arrive.  `between(pair)` is issued behind the pair's MFMAs.
  auto mfma_step = [&](int s, const f32x4 (&v)[16], auto zero_tag, auto between) {
    constexpr bool ZERO = decltype(zero_tag)::value;
#pragma unroll
    for (int pr = 0; pr < 8; ++pr) {
      __builtin_amdgcn_sched_barrier(0);
      const int g = s * 8 + pr;
      ring_load(g + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int pos = 2 * pr + h;
          const float wv = wr[(g & 1) * 2 + h][e];
          if (ZERO && e == 0) {
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            acc[pos] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, v[pos][e], zero, 0, 0, 0);
          } else {
            acc[pos] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, v[pos][e], acc[pos], 0, 0, 0);
          }
        }
      __builtin_amdgcn_sched_barrier(0);
      between(pr);
    }
  };

  const bool stamp = a.dbg && blockIdx.x == 0 && tid == 0;
  int ns_ = 0;
  if (stamp) a.dbg[ns_++] = clock64();
  __syncthreads();   // barrier 0: patch 0 is in buffer 0, the weights are in LDS
  if (my_items > 0) {
    ring_load(0);
    read_window(va, lds, 0);
#pragma unroll
    for (int p = 0; p < 8; ++p) transform_piece(va, p);
    if (PIPE) read_column(vb_, lds, 1, 0);
  }
  int w = vb;
  for (int k = 0; k < my_items; ++k, w += (int)gridDim.x) {
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    const float* patch = lds + (k & 1) * RAWBUF;
    // (the last item re-reads its own patch instead of a next one: the reads stay unconditional)
    const float* patch_next = k + 1 < my_items ? lds + ((k + 1) & 1) * RAWBUF : patch;
    // ---- where the item goes; its residual is requested now and read in the epilogue
    const ItemPos ip = item_pos(wk, w);
    const size_t tile_pix = ((size_t)ip.b * a.Ho + (size_t)ip.ty * TH) * a.Wo + (size_t)ip.tx * TW;
    float* out_tile = a.out + tile_pix * a.out_cs + a.out_coff;
    // PIPE (registers to spare): requested now, read in the epilogue.  Two waves per SIMD: requested when the
    // epilogue starts (the fragment registers are dead by then) - the SIMD's other wave covers the latency.
    auto request_res = [&]() {
      if (has_res) {
        const float* res_tile = a.res + tile_pix * a.res_cs + a.res_coff;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const char* ub = reinterpret_cast<const char*>(res_tile + ((q >> 1) * a.Wo + (q & 1)) * a.res_cs);   // uniform
          rv[q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ub + lane_res));
        }
      }
    };
    if (PIPE) request_res();
    // ---- step 0 (channels 0..15) on va; the window of step 1 becomes vb_ beside it (PIPE) or after it
    if (PIPE) {
      // the window of the next step arrives column by column: column c is requested behind pair c-1 (column 0 behind
      // the previous step's pair 7 or, for a new patch, right behind the barrier), row-combined behind pair c, and the
      // column pass runs behind pairs 4..7 - 4 LDS reads and 8 packed adds per pair, never a burst in front of the
      // weight-fragment ring
      mfma_step(0, va, std::true_type(), [&](int pr) {
        if (pr < 3) read_column(vb_, patch, 1, pr + 1);
        transform_piece(vb_, pr);
      });
    } else {
      mfma_step(0, va, std::true_type(), [&](int) {});
      read_window(vb_, patch, 1);
#pragma unroll
      for (int p = 0; p < 8; ++p) transform_piece(vb_, p);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    // barrier k+1: every wave has read its last window of patch k (the loader may refill that buffer with patch
    // k+2), and patch k+1 is complete
    __syncthreads();
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    // ---- step 1 (channels 16..31) on vb_; the next item's first window becomes va beside it (PIPE)
    if (PIPE) {
      read_column(va, patch_next, 0, 0);     // (patch k+1 only became visible at the barrier)
      mfma_step(1, vb_, std::false_type(), [&](int pr) {
        if (pr < 3) read_column(va, patch_next, 0, pr + 1);
        transform_piece(va, pr);
        if (pr == 7) read_column(vb_, patch_next, 1, 0);
      });
    } else {
      mfma_step(1, vb_, std::false_type(), [&](int) {});
    }
    __builtin_amdgcn_sched_barrier(0);
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    // ---- epilogue in registers: Y = A^T M A (x-fold, then y-fold), bias, residual, ReLU, 16-byte stores
    {
      if (!PIPE) request_res();
      f32x4 r0[4], r1[4];
#pragma unroll
      for (int py = 0; py < 4; ++py) {
        r0[py] = pk_add4(pk_add4(acc[py * 4], acc[py * 4 + 1]), acc[py * 4 + 2]);
        r1[py] = pk_sub4(pk_sub4(acc[py * 4 + 1], acc[py * 4 + 2]), acc[py * 4 + 3]);
      }
      f32x4 y[4];     // [oy*2 + ox]
      y[0] = pk_add4(pk_add4(r0[0], r0[1]), r0[2]);
      y[1] = pk_add4(pk_add4(r1[0], r1[1]), r1[2]);
      y[2] = pk_sub4(pk_sub4(r0[1], r0[2]), r0[3]);
      y[3] = pk_sub4(pk_sub4(r1[1], r1[2]), r1[3]);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 o4 = pk_add4(y[q], bias4);
        if (has_res) o4 = pk_add4(o4, rv[q]);
        if (a.relu) {
          o4[0] = vrelu1(o4[0]); o4[1] = vrelu1(o4[1]); o4[2] = vrelu1(o4[2]); o4[3] = vrelu1(o4[3]);
        }
        if constexpr (NSW > 0) {
          *reinterpret_cast<f32x4*>(stage + (k & 1) * STILE + stage_off + ((q >> 1) * TW + (q & 1)) * 32) = o4;
        } else {
          char* ub = reinterpret_cast<char*>(out_tile + ((q >> 1) * a.Wo + (q & 1)) * a.out_cs);                // uniform
          __builtin_nontemporal_store(o4, reinterpret_cast<f32x4*>(ub + lane_out));
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);     // (keeps the next window's reads - 64 registers - behind the epilogue)
    if (!PIPE) {
      read_window(va, patch_next, 0);
#pragma unroll
      for (int p = 0; p < 8; ++p) transform_piece(va, p);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
  }
  if constexpr (NSW > 0) __syncthreads();   // the last item is staged: the store waves flush it
  if (stamp) a.dbg[63] = ns_;
}

// conv_wino3b_kernel: the same layers with a wave tile of 16 slots x 32 couts (all 16 positions, 32 accumulators of 4
// registers).  conv_wino3_kernel's two cout-half waves of a slot group both build the same position fragments; here a
// slot group's fragments are built once and feed both cout halves - the input-transform VALU and the window reads per
// MFMA halve (the same amortisation over 32 couts that conv_wino2_kernel's NT = 1 tiles have), which is what the
// 32-cycle MFMA stream is most sensitive to (tools/mfma16_stream.hip: 8 packed adds + 2 LDS reads in front of 8 MFMAs
// cost 321 cycles instead of 256).  Item = 16x16 output pixels on 4 compute waves (slot groups).  With 128 accumulator
// registers there is no room for a second fragment set: the next step's window is read into the registers of the
// fragments the step has already consumed (column 0/1 behind pair 3, column 2 behind pair 5, column 3 behind pair 7),
// the row pass follows two pairs later, the column pass runs between the steps.
// RES (a residual is added): its 8 float4 per lane are requested behind pairs 2 and 4 of the item's last step and take
// the registers the next window would otherwise be read into - that window is then read behind the epilogue.
template <int NLW, bool DMA, bool RES>
__global__ __launch_bounds__((4 + NLW) * 64, 1) void conv_wino3b_kernel(const ConvArgs a, const ConvWork wk) {
  constexpr int TH = 16, TW = 16, PH = TH + 2, PW = TW + 2, CK = 32, CP = CK + 4, NCW = 4;
  constexpr int RAWBUF = PH * PW * CP;
  constexpr int WFLOATS = 16 * 2 * 2 * 256;        // [pos][step][cout half][lane][4]
  extern __shared__ f32x4 smem4[];
  float* lds = reinterpret_cast<float*>(smem4);
  float* wlds = lds + 2 * RAWBUF;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cin_pad = a.cin8 * 8;
  const int vb = virtual_block(a);
  const int my_items = wk.total > vb ? (wk.total - 1 - vb) / (int)gridDim.x + 1 : 0;
  if (wave >= NCW) {
    if constexpr (DMA) dma_loader<3, 1, TH, TW, CK, NLW>(a, wk, lds, tid - NCW * 64, my_items, 1, vb);
    else ws_loader<3, 1, TH, TW, CK, NLW, NoHook, false, 3>(a, wk, lds, tid - NCW * 64, my_items, cin_pad);
    return;
  }
  {   // the layer's weights -> LDS (64 KiB, once per workgroup; visible after barrier 0)
    const f32x4* src = reinterpret_cast<const f32x4*>(a.w);
    f32x4* dst = reinterpret_cast<f32x4*>(wlds);
    constexpr int PER = WFLOATS / 4 / (NCW * 64);
    f32x4 tmp[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) tmp[i] = src[tid + i * NCW * 64];
#pragma unroll
    for (int i = 0; i < PER; ++i) dst[tid + i * NCW * 64] = tmp[i];
  }
  const int sg = wave;
  const int j = lane & 15, kq = lane >> 4;
  const int in_a = (j < 4) || (j >= 12);             // slot -> block map: see conv_wino3_kernel (conflict-free reads)
  const int brow = in_a ? 0 : 1;
  const int bcol = in_a ? (j < 4 ? j : j - 8) : j - 4;
  const int by = 2 * sg + brow;
  const int worg = ((2 * by) * PW + 2 * bcol) * CP + 4 * kq;
  const float* wfrag = wlds + lane * 4;                               // + ((pos * 2 + step) * 2 + half) * 256
  constexpr bool has_res = RES;
  const int lane_pix = (2 * by) * a.Wo + 2 * bcol;
  const unsigned lane_out = (unsigned)(lane_pix * a.out_cs + 4 * kq) * 4u;     // + 64 bytes for the second cout half
  const unsigned lane_res = (unsigned)(lane_pix * a.res_cs + 4 * kq) * 4u;

  typedef float f32x2 __attribute__((ext_vector_type(2)));
  auto pk_add4 = [](const f32x4& b, const f32x4& c) -> f32x4 {
    f32x2 lo, hi;
    const f32x2 b0 = {b[0], b[1]}, b1 = {b[2], b[3]}, c0 = {c[0], c[1]}, c1 = {c[2], c[3]};
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(lo) : "v"(b0), "v"(c0));
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(hi) : "v"(b1), "v"(c1));
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
  };
  auto pk_sub4 = [](const f32x4& b, const f32x4& c) -> f32x4 {   // b - c (negation is exact)
    f32x2 lo, hi;
    const f32x2 b0 = {b[0], b[1]}, b1 = {b[2], b[3]}, c0 = {c[0], c[1]}, c1 = {c[2], c[3]};
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(lo) : "v"(b0), "v"(c0));
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(hi) : "v"(b1), "v"(c1));
    return f32x4{lo[0], lo[1], hi[0], hi[1]};
  };
  auto bt4 = [&](f32x4& x0, f32x4& x1, f32x4& x2, f32x4& x3) {   // (x0, x1, x2, x3) -> (x0 - x2, x1 + x2, x2 - x1, x1 - x3)
    x0 = pk_sub4(x0, x2);
    x3 = pk_sub4(x1, x3);
    const f32x4 t = pk_add4(x1, x2);
    x2 = pk_sub4(x2, x1);
    x1 = t;
  };
  f32x4 acc[16][2];
  f32x4 va[16], vb_[16];   // fragment sets of consecutive steps (their live ranges barely overlap: one register set)
  f32x4 wr[8];             // weight ring: two position pairs x 2 positions x 2 cout halves

  auto read_column = [&](f32x4 (&d)[16], const float* patch, int s, int wx) {
#pragma unroll
    for (int wy = 0; wy < 4; ++wy)
      d[wy * 4 + wx] = *reinterpret_cast<const f32x4*>(patch + worg + (wy * PW + wx) * CP + 16 * s);
  };
  auto transform_piece = [&](f32x4 (&d)[16], int piece) {   // 0..3: row pass of window column, 4..7: column pass of row
    if (piece < 4) bt4(d[piece], d[4 + piece], d[8 + piece], d[12 + piece]);
    else bt4(d[(piece - 4) * 4], d[(piece - 4) * 4 + 1], d[(piece - 4) * 4 + 2], d[(piece - 4) * 4 + 3]);
  };
  auto ring_load = [&](int g) {   // cyclic pair index g = s*8 + pair -> ring slots 4*(g & 1) ..
    const int gg = g & 15, s = gg >> 3, p0 = (gg & 7) * 2;
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        wr[(g & 1) * 4 + h2 * 2 + h] = *reinterpret_cast<const f32x4*>(wfrag + (((p0 + h2) * 2 + s) * 2 + h) * 256);
  };
  // one 16-channel step: 8 pairs x (2 positions x 2 cout halves x 4) MFMAs; `between(pair)` behind each pair
  auto mfma_step = [&](int s, const f32x4 (&v)[16], auto zero_tag, auto between) {
    constexpr bool ZERO = decltype(zero_tag)::value;
#pragma unroll
    for (int pr = 0; pr < 8; ++pr) {
      __builtin_amdgcn_sched_barrier(0);
      const int g = s * 8 + pr;
      ring_load(g + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int pos = 2 * pr + h2;
            const float wv = wr[(g & 1) * 4 + h2 * 2 + h][e];
            if (ZERO && e == 0) {
              const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
              acc[pos][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, v[pos][e], zero, 0, 0, 0);
            } else {
              acc[pos][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv, v[pos][e], acc[pos][h], 0, 0, 0);
            }
          }
      __builtin_amdgcn_sched_barrier(0);
      between(pr);
    }
  };
  // the next step's window into the registers of fragments this step has consumed, row pass two pairs later
  auto refill = [&](f32x4 (&nx)[16], const float* patch, int s, int pr) {
    if (pr == 3) { read_column(nx, patch, s, 0); read_column(nx, patch, s, 1); }
    if (pr == 5) { read_column(nx, patch, s, 2); transform_piece(nx, 0); transform_piece(nx, 1); }
    if (pr == 7) { read_column(nx, patch, s, 3); transform_piece(nx, 2); }
  };
  auto finish = [&](f32x4 (&nx)[16]) {
    transform_piece(nx, 3);
#pragma unroll
    for (int p = 4; p < 8; ++p) transform_piece(nx, p);
  };

  const bool stamp = a.dbg && blockIdx.x == 0 && tid == 0;
  int ns_ = 0;
  if (stamp) a.dbg[ns_++] = clock64();
  __syncthreads();   // barrier 0: patch 0 is in buffer 0, the weights are in LDS
  if (my_items > 0) {
    ring_load(0);
#pragma unroll
    for (int wx = 0; wx < 4; ++wx) read_column(va, lds, 0, wx);
#pragma unroll
    for (int p = 0; p < 8; ++p) transform_piece(va, p);
  }
  int w = vb;
  for (int k = 0; k < my_items; ++k, w += (int)gridDim.x) {
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    const float* patch = lds + (k & 1) * RAWBUF;
    const float* patch_next = k + 1 < my_items ? lds + ((k + 1) & 1) * RAWBUF : patch;   // (reads stay unconditional)
    const ItemPos ip = item_pos(wk, w);
    const size_t tile_pix = ((size_t)ip.b * a.Ho + (size_t)ip.ty * TH) * a.Wo + (size_t)ip.tx * TW;
    float* out_tile = a.out + tile_pix * a.out_cs + a.out_coff;
    // ---- step 0 (channels 0..15) on va, building vb_ = window (patch k, channels 16..31)
    mfma_step(0, va, std::true_type(), [&](int pr) { refill(vb_, patch, 1, pr); });
    finish(vb_);
    __builtin_amdgcn_sched_barrier(0);
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    __syncthreads();   // barrier k+1: patch k has been read for the last time; patch k+1 is complete
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    // ---- step 1 (channels 16..31) on vb_, building va = window (patch k+1, channels 0..15)
    // (only window columns 0 and 1 now: the epilogue needs the registers of the other two)
    f32x4 rv[2][4];     // residual of the lane's 4 output pixels, per cout half
    auto request_res = [&](int h) {
      if (has_res) {
        const float* res_tile = a.res + tile_pix * a.res_cs + a.res_coff;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const char* ub = reinterpret_cast<const char*>(res_tile + ((q >> 1) * a.Wo + (q & 1)) * a.res_cs + 16 * h);   // uniform
          rv[h][q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ub + lane_res));
        }
      }
    };
    mfma_step(1, vb_, std::false_type(), [&](int pr) {
      if (RES) {     // behind pairs 2 and 4: by then 4 / 8 fragments of this step are dead, 16 registers per half
        if (pr == 2) request_res(0);
        if (pr == 4) request_res(1);
      } else {
        if (pr == 3) { read_column(va, patch_next, 0, 0); read_column(va, patch_next, 0, 1); }
        if (pr == 5) { transform_piece(va, 0); transform_piece(va, 1); }
      }
    });
    __builtin_amdgcn_sched_barrier(0);
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    // ---- epilogue in registers, one cout half after the other: Y = A^T M A, bias, residual, ReLU, 16-byte stores
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // x-fold one position row at a time and fold it straight into the four outputs: 6 live temporaries, and a row's
      // accumulators are dead as soon as it is folded
      f32x4 y[4];     // [oy*2 + ox]
#pragma unroll
      for (int py = 0; py < 4; ++py) {
        const f32x4 r0 = pk_add4(pk_add4(acc[py * 4][h], acc[py * 4 + 1][h]), acc[py * 4 + 2][h]);
        const f32x4 r1 = pk_sub4(pk_sub4(acc[py * 4 + 1][h], acc[py * 4 + 2][h]), acc[py * 4 + 3][h]);
        if (py == 0) { y[0] = r0; y[1] = r1; }
        if (py == 1) { y[0] = pk_add4(y[0], r0); y[1] = pk_add4(y[1], r1); y[2] = r0; y[3] = r1; }
        if (py == 2) { y[0] = pk_add4(y[0], r0); y[1] = pk_add4(y[1], r1); y[2] = pk_sub4(y[2], r0); y[3] = pk_sub4(y[3], r1); }
        if (py == 3) { y[2] = pk_sub4(y[2], r0); y[3] = pk_sub4(y[3], r1); }
      }
      const f32x4 bias4 = *reinterpret_cast<const f32x4*>(a.bias + 16 * h + 4 * kq);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 o4 = pk_add4(y[q], bias4);
        if (has_res) o4 = pk_add4(o4, rv[h][q]);
        if (a.relu) {
          o4[0] = vrelu1(o4[0]); o4[1] = vrelu1(o4[1]); o4[2] = vrelu1(o4[2]); o4[3] = vrelu1(o4[3]);
        }
        char* ub = reinterpret_cast<char*>(out_tile + ((q >> 1) * a.Wo + (q & 1)) * a.out_cs + 16 * h);                  // uniform
        __builtin_nontemporal_store(o4, reinterpret_cast<f32x4*>(ub + lane_out));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (RES) {
      read_column(va, patch_next, 0, 0);
      read_column(va, patch_next, 0, 1);
    }
    read_column(va, patch_next, 0, 2);
    read_column(va, patch_next, 0, 3);
    if (RES) { transform_piece(va, 0); transform_piece(va, 1); }
    transform_piece(va, 2);
    finish(va);
    __builtin_amdgcn_sched_barrier(0);
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
  }
  if (stamp) a.dbg[63] = ns_;
}

template <int NLW, bool DMA, bool RES>
static hipError_t launch_wino3b_impl(const ConvArgs& a, hipStream_t s) {
  constexpr size_t lds = (2 * (size_t)18 * 18 * 36 + 16 * 2 * 2 * 256) * sizeof(float);
  static_assert(lds <= 160 * 1024, "two patch buffers and the layer's weights must fit the 160 KiB LDS");
  return launch_conv_kernel(CONV_KERNEL(conv_wino3b_kernel<NLW, DMA, RES>), (4 + NLW) * 64, lds, a.Wo / 16, a.Ho / 16, 1, a, s);
}

template <int TH, int NLW, bool PIPE, int LPRIO = 0, bool DMA = false, int NSW = 0, bool DUAL = false>
static hipError_t launch_wino3_impl(const ConvArgs& a, hipStream_t s) {
  constexpr size_t lds = (2 * (size_t)(TH + 2) * 18 * 36 + 16 * 2 * 2 * 256 + (NSW > 0 ? 2 * TH * 16 * 32 : 0)) * sizeof(float);
  static_assert(lds <= 160 * 1024, "two patch buffers, the layer's weights and the staging tiles must fit the 160 KiB LDS");
  return launch_conv_kernel(CONV_KERNEL(conv_wino3_kernel<TH, NLW, PIPE, LPRIO, DMA, NSW, DUAL>), (TH / 2 + NLW + NSW) * 64, lds,
                            a.Wo / 16, a.Ho / TH, 1, a, s);
}

static hipError_t launch_wino3(const ConvArgs& a, hipStream_t s) {
  if (!takes_wino3(conv_shape(a))) return hipErrorInvalidValue;
  const bool dma_ok = conv_dma_ok(a);
  if (a.out2) {      // + the full-resolution HR fuse sum as a second output (store waves)
    if (!dma_ok || a.nxt < 1 || a.nxt > 3 || a.out2_cs % 4 || a.out2_coff % 4) return hipErrorInvalidValue;
    return launch_wino3_impl<8, 2, true, 0, true, 2, true>(a, s);
  }
  // tuning variants (tools/conv_bench.py --cfg): register-staged loader at priority 0 / 3 / 1, one LDS-DMA loader
  // wave, 16x16-pixel items on 8 compute waves (two per SIMD, 168 registers: spills)
  if (g_force_cfg == 831) return launch_wino3_impl<8, 2, true, 0>(a, s);
  if (g_force_cfg == 833) return launch_wino3_impl<8, 2, true, 3>(a, s);
  if (g_force_cfg == 834) return launch_wino3_impl<8, 2, true, 1>(a, s);
  if (dma_ok && g_force_cfg == 836) return launch_wino3_impl<8, 1, true, 0, true>(a, s);
  if (g_force_cfg == 832 && a.Ho % 16 == 0) return launch_wino3_impl<16, 4, false>(a, s);
  if (g_force_cfg == 837 && a.Ho % 16 == 0) {
    if (a.res) return dma_ok ? launch_wino3b_impl<2, true, true>(a, s) : launch_wino3b_impl<2, false, true>(a, s);
    return dma_ok ? launch_wino3b_impl<2, true, false>(a, s) : launch_wino3b_impl<2, false, false>(a, s);
  }
  // measured (batch 64, 32->32 @128x128, with / without residual; conv_wino2_kernel: 0.159 / 0.149 ms):
  //   register loader prio 3: 0.144 / 0.129    prio 0: 0.146 / 0.134 (patch 1.8k cycles late)
  //   LDS-DMA loader, 2 waves: 0.138 / 0.119   1 wave: 0.154 / 0.134    8 compute waves: 0.190 / 0.114
  //   16 slots x 32 couts per wave (conv_wino3b_kernel, 16x16-pixel items): 0.123 / 0.109
  // inside the network (input fresh from the previous kernel): 8x16 items 0.121 / 0.104, 16x32 wave tile 0.116 / 0.112
  // -> the 16x32 wave tile took the residual layers until the 8x16-item kernel got its store waves: over the network's
  // 65 launches 7.24 ms with the 16x32 tile on the residual layers, 6.77 ms with the 8x16 items + store waves everywhere
  // (tools/ab_cfg.py, former default vs this one).  conv_wino3b_kernel stays reachable as --cfg 837.
  // store waves (conv_bench --cfg 839: without): the epilogue's stores leave the compute waves
  if (dma_ok && g_force_cfg != 839) return launch_wino3_impl<8, 2, true, 0, true, 2>(a, s);
  if (dma_ok) return launch_wino3_impl<8, 2, true, 0, true>(a, s);
  return launch_wino3_impl<8, 2, true, 3>(a, s);
}
