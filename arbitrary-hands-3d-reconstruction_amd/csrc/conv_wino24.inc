// 3x3 stride-1 convolution as 2-D Winograd F(2x4,3x3): F(2,3) along y, F(4,3) along x - included by conv_mfma.hip.
// 24 products per 2x4 output block (3 per output) instead of F(2x2,3x3)'s 16 per 2x2 (4 per output): 1.33x fewer
// MFMAs again, 3x fewer than the direct form.
//
// Why this shape and not F(4x4,3x3) (36 products per 16 outputs): conv_wino2_kernel's frame gives every compute wave ONE
// position row, whose x-fold completes in registers and whose y-fold is the exchange through LDS.  F(2,3) along y keeps
// the four position rows = four waves; F(4,3) along x only lengthens a row from 4 to 6 positions (6 accumulator tiles =
// 96 registers with one n-tile per wave).  Six position rows (F(4,3) along y) would not map onto four SIMDs, and with all
// 36 positions in one wave (conv_wino3_kernel's frame on 16x16x4 MFMAs) 36 accumulators + 36 fragment vectors do not
// fit the 256 registers a wave has next to the loader waves.
//
// Frame = conv_wino2_kernel's (conv_wino2.inc), NT = 1, items of at least two Cin chunks:
//  * work item = 8x32 output pixels = 32 slots (2x4 blocks: 4 block rows x 8 block columns) x 32 couts; the loader waves
//    stream the raw patch [10][34][CK+4] (CK = 32), double buffered, one workgroup barrier per chunk.  Two such
//    patches (96 KiB) leave room for 8 parked tiles, not 16: the exchange runs in TWO rounds (output columns 0/1, then
//    2/3) with two extra workgroup barriers per item, which the loader waves join (ws_loader EXTRA = 2).  (First
//    version: CK = 16 and one round - a chunk was then 2 steps behind a ~1.7k-cycle prologue + barrier, 44 % of an
//    item's cycles in MFMAs, no faster than conv_wino2_kernel.);
//  * wave py owns positions (py, 0..5): per 8-channel step it reads the two window rows its B2^T row combines, 2 x 6
//    ds_read_b128, forms t[c] = d[ra][c] + sgn d[rb][c] and the six fragments of B4^T:
//      v0 = 4 t0 - 5 t2 + t4,   v1 = (t4 - 4 t2) + (t3 - 4 t1),   v2 = (t4 - 4 t2) - (t3 - 4 t1),
//      v5 = 4 t1 - 5 t3 + t5,   v3 = (t4 - t2) + 2 (t3 - t1),     v4 = (t4 - t2) - 2 (t3 - t1)
//    (12 float4 multiply-adds as v_pk_fma_f32 / v_pk_add_f32 with constant pairs pinned in VGPRs) for 24 MFMAs;
//  * weights: 24 taps U[py][px] = G2 g G4^T (packer.winograd24_weights, fp64 on the host);
//  * x-fold in registers with A4^T: o0 = m0+m1+m2+m3+m4, o1 = m1-m2+2(m3-m4), o2 = m1+m2+4(m3+m4),
//    o3 = m1-m2+8(m3-m4)+m5 - four tiles per wave parked as [slot][cout]; y-fold across the waves through LDS exactly as
//    in conv_wino2_kernel; wave (oy, oh) stores output row parity oy and output columns 2 oh, 2 oh + 1 of every block.
// Round-off: F(4,3) carries ~10x the round-off of F(2,3) in fp32 (constants up to 8 instead of 1) - measured per layer in
// tests/test_gpu_hardening.py, gated per layer by the packer (conv_algo).

template <int NLW>
__global__ __launch_bounds__((4 + NLW) * 64, 1) void conv_wino24_kernel(const ConvArgs a, const ConvWork wk) {
  constexpr int CK = 32, TH = 8, TW = 32, PH = TH + 2, PW = TW + 2, CP = CK + 4;
  constexpr int RAWBUF = PH * PW * CP;
  constexpr int PSTR = 36, PTILE = 32 * PSTR;   // parked tile: [32 slots][32 couts + 4 pad]
  constexpr int PART_W = 2 * PTILE;             // floats one wave parks per round: two output-column tiles
  extern __shared__ f32x4 smem4[];
  float* lds = reinterpret_cast<float*>(smem4);
  float* part = lds + 2 * RAWBUF;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cin_pad = a.cin8 * 8;
  const int nchunks = (cin_pad + CK - 1) / CK;            // >= 2 (checked by the host)
  const int vb = virtual_block(a);
  const int my_items = wk.total > vb ? (wk.total - 1 - vb) / (int)gridDim.x + 1 : 0;
  const int ktotal = my_items * nchunks;
  if (wave >= 4) {
    ws_loader<3, 1, TH, TW, CK, NLW, NoHook, false, 3, 2>(a, wk, lds, tid - 256, ktotal, cin_pad);
    return;
  }
  const int py = wave;
  const int li = lane & 31, lh = lane >> 5;
  // this position row's B2^T combination t = d[ra] + sgn * d[rb]; the lane's window origin (block row li>>3, column li&7)
  const int ra = py == 0 ? 0 : (py == 2 ? 2 : 1);
  const int rb = py == 2 ? 1 : (py == 3 ? 3 : 2);
  const float sgn = py == 1 ? 1.f : -1.f;
  const int worg = (2 * (li >> 3) * PW + 4 * (li & 7)) * CP + 4 * lh;
  const int woff_a = worg + ra * PW * CP, woff_b = worg + rb * PW * CP;
  // store side: this wave writes output row parity oy and columns oh (round A), 2 + oh (round B) of every 2x4 block; lane
  // = (block column p8, cout quad q8), four block rows gq per lane, so 8 lanes cover one pixel's 128-byte line
  const int oy = wave >> 1, oh = wave & 1;
  const int p8 = lane >> 3, q8 = lane & 7;
  const int lane_pix = oy * a.Wo + 4 * p8 + oh;          // (+ 2 for the wave's round-B column)
  const int lane_out = lane_pix * a.out_cs + 4 * q8, lane_res = lane_pix * a.res_cs + 4 * q8;
  const int gs_out = 2 * a.Wo * a.out_cs, gs_res = 2 * a.Wo * a.res_cs;   // block row +1 = two pixel rows down
  const float ysign = oy ? -1.f : 1.f;
  const bool has_res = a.res != nullptr;
  f32x16 acc[6];

  const int tap_b = a.cin8 * a.n_tiles * 1024, step_b = a.n_tiles * 1024;   // weight bytes per position / per step
  const __amdgpu_buffer_rsrc_t wrsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.groups * 24 * tap_b, 0x00020000);
  const unsigned wlane = lane * 16;
  int w = vb, c0 = 0;
  auto wbase = [&](int w_item) -> int {      // byte offset of (group, position row py, n-tile of the item)
    const ItemPos ip = item_pos(wk, w_item);
    return (ip.g * 24 + py * 6) * tap_b + ip.rest * 1024;
  };
  f32x4 d[2][6], v[6], bq[6];
  auto load_frag = [&](int p, int base, int step) {
    const int so = base + p * tap_b + (step < a.cin8 ? step : a.cin8 - 1) * step_b;
    bq[p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane, so, 0));
  };
  auto read_rows = [&](const float* patch, int s) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      d[0][c] = *reinterpret_cast<const f32x4*>(patch + woff_a + c * CP + s * 8);
      d[1][c] = *reinterpret_cast<const f32x4*>(patch + woff_b + c * CP + s * 8);
    }
  };
  // packed multiply-adds with constant pairs pinned in VGPRs (see conv_wino2.inc: hipcc scalarises the plain forms)
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const float one = a.ks == 3 ? 1.f : 2.f;   // always 1 here (a runtime value: nothing is folded back into scalar ops)
  f32x2 sgnp = {sgn * one, sgn * one}, m1p = {-one, -one}, p4p = {4.f * one, 4.f * one}, m4p = {-4.f * one, -4.f * one},
        m5p = {-5.f * one, -5.f * one}, p2p = {2.f * one, 2.f * one}, m2p = {-2.f * one, -2.f * one};
  asm volatile("" : "+v"(sgnp), "+v"(m1p), "+v"(p4p), "+v"(m4p), "+v"(m5p), "+v"(p2p), "+v"(m2p));
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
  auto row_op = [&](f32x4 (&t)[6]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) t[c] = pk_fma4(sgnp, d[1][c], d[0][c]);
  };
  // B4^T in three pieces, each issued behind MFMAs whose fragments it replaces
  auto col_a = [&](const f32x4 (&t)[6]) {      // v0, v1, v2
    v[0] = pk_fma4(p4p, t[0], pk_fma4(m5p, t[2], t[4]));
    const f32x4 e = pk_fma4(m4p, t[2], t[4]), f = pk_fma4(m4p, t[1], t[3]);
    v[1] = pk_add4(e, f);
    v[2] = pk_fma4(m1p, f, e);
  };
  auto col_b = [&](const f32x4 (&t)[6]) {      // v3, v4
    const f32x4 e = pk_fma4(m1p, t[2], t[4]), f = pk_fma4(m1p, t[1], t[3]);
    v[3] = pk_fma4(p2p, f, e);
    v[4] = pk_fma4(m2p, f, e);
  };
  auto col_c = [&](const f32x4 (&t)[6]) {      // v5
    v[5] = pk_fma4(p4p, t[1], pk_fma4(m5p, t[3], t[5]));
  };

  int wsc = wbase(w);
  if (ktotal > 0) {
#pragma unroll
    for (int p = 0; p < 6; ++p) load_frag(p, wsc, 0);
  }
  const bool stamp = a.dbg && blockIdx.x == 0 && tid == 0;
  int ns_ = 0;
  if (stamp) a.dbg[ns_++] = clock64();
  __syncthreads();   // barrier 0: chunk 0 is in buffer 0
  int k = 0;
  auto chunk = [&](auto first_tag, auto last_tag) {
    constexpr bool FIRST = decltype(first_tag)::value, LAST = decltype(last_tag)::value;
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    const float* patch = lds + (k & 1) * RAWBUF;
    const int nc0 = LAST ? 0 : c0 + CK, nw = LAST ? w + (int)gridDim.x : w;
    const bool more = k + 1 < ktotal;
    const int wsn = (LAST && more) ? wbase(nw) : wsc;
    const int nsteps = (cin_pad - c0 < CK ? cin_pad - c0 : CK) / 8;
    int rest = 0, ty0 = 0, tx0 = 0;
    float* out_tile = nullptr;
    EpiCtx e;
    f32x4 rv[2][4], bv;
    bool vec = false;
    __amdgpu_buffer_rsrc_t rrsrc = wrsrc, brsrc = wrsrc;
    auto s2p = [&](int p, int oc, bool& ok) -> int {     // slot p, output column oc of the block -> pixel
      int y = ty0 + 2 * (p >> 3) + oy, x = tx0 + 4 * (p & 7) + oc;
      ok = y < a.Ho && x < a.Wo;
      y = y < a.Ho ? y : a.Ho - 1;
      x = x < a.Wo ? x : a.Wo - 1;
      return y * a.Wo + x;
    };
    if (LAST) {
      const ItemPos ip = item_pos(wk, w);
      const int g = ip.g, b = ip.b;
      rest = ip.rest;
      ty0 = ip.ty * TH;
      tx0 = ip.tx * TW;
      e.bias = a.bias + (size_t)g * a.n_tiles * 32 + (size_t)b * a.bias_fstride;
      e.outb = a.out + (size_t)b * a.Ho * a.Wo * a.out_cs + a.out_coff + g * a.Cout;
      e.resb = has_res ? a.res + res_frame_off(a, b) + a.res_coff + g * a.Cout : nullptr;
      e.res_cs = a.res_cs; e.out_cs = a.out_cs; e.Cout = a.Cout; e.relu = a.relu;
      e.vec_align = ((a.out_coff + g * a.Cout) % 4 == 0) && (a.out_cs % 4 == 0) &&
                    (!has_res || (((a.res_coff + g * a.Cout) % 4 == 0) && (a.res_cs % 4 == 0)));
      const bool full_tile = (ty0 + TH <= a.Ho) && (tx0 + TW <= a.Wo);
      vec = full_tile && e.vec_align && ((rest + 1) * 32 <= a.Cout);
      const int tile_pix = ty0 * a.Wo + tx0;
      out_tile = e.outb + (size_t)tile_pix * a.out_cs;
      const size_t res_off = (res_frame_off(a, b) + (size_t)tile_pix * a.res_cs) + a.res_coff + g * a.Cout;
      const size_t res_left = (res_total(a) - res_off) * 4;
      rrsrc = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(has_res ? a.res + res_off : a.in), 0,
          (has_res && full_tile && e.vec_align) ? (int)(unsigned)(res_left > 0xffffffffu ? 0xffffffffu : res_left) : 0,
          0x00020000);
      brsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(e.bias), 0, bias_row_left(a, g), 0x00020000);
    }
    // the item's residual and bias: unconditional raw buffer loads (a zero-record descriptor returns 0 without memory
    // traffic when there is no residual or the tile takes the generic path), requested with the item's last step, whose
    // window / row-combination registers they take over
    auto request_res = [&]() {
      const int ntc = rest < a.n_tiles ? rest : a.n_tiles - 1;
      bv = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(brsrc, 16 * q8, ntc * 128, 0));
#pragma unroll
      for (int oc = 0; oc < 2; ++oc)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
          rv[oc][gq] = __builtin_bit_cast(
              f32x4, __builtin_amdgcn_raw_buffer_load_b128(rrsrc, (lane_res + 2 * oc * a.res_cs) * 4,
                                                           (ntc * 32 + gq * gs_res) * 4, RES_CACHE_WINO));
    };
    // first fragments of the chunk (the patch only became visible at the barrier)
    read_rows(patch, 0);
    {
      f32x4 t[6];
      row_op(t);
      col_a(t);
      col_b(t);
      col_c(t);
    }
    // one 8-channel step: 6 groups of 4 MFMAs.  The next step's window rows are requested with group 0 and row-combined
    // with group 2; behind its group's MFMAs each fragment is replaced by the next step's (activations: B4^T pieces
    // behind groups 2, 4 and 5; weights: buffer load).  A chunk's last step reads and combines a defined but unused row.
    auto step = [&](int s, auto zero_tag, auto tail_tag) {
      constexpr bool ZERO = decltype(zero_tag)::value, TAIL = decltype(tail_tag)::value;
      const bool last_step = s + 1 >= nsteps;
      f32x4 t[6];
#pragma unroll
      for (int px = 0; px < 6; ++px) {
        __builtin_amdgcn_sched_barrier(0);
        if (TAIL) {
          if (px == 0) request_res();
        } else {
          if (px == 0) read_rows(patch, s + 1);
          if (px == 2) row_op(t);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (ZERO && j == 0) {
            const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            acc[px] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[px][j], v[px][j], zero, 0, 0, 0);
          } else {
            acc[px] = __builtin_amdgcn_mfma_f32_32x32x2f32(bq[px][j], v[px][j], acc[px], 0, 0, 0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (!TAIL) {
          if (px == 2) col_a(t);      // v0..v2: their MFMAs have been issued
          if (px == 4) col_b(t);      // v3, v4
          if (px == 5) col_c(t);      // v5
          const int nstep = last_step ? nc0 / 8 : c0 / 8 + s + 1;
          load_frag(px, wsc, nstep);
        }
      }
    };
    if (LAST) {
      int s = 0;
      if (FIRST) {      // (never the item's only step: an item has >= 2 chunks)
        step(0, std::true_type(), std::false_type());
        s = 1;
      }
      for (; s < nsteps - 1; ++s) step(s, std::false_type(), std::false_type());
      step(nsteps - 1, std::false_type(), std::true_type());
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

    // ---- item epilogue: x-fold with A4^T in registers; the exchange for the y-fold runs in two rounds of two output
    // columns (the area holds 4 waves x 2 tiles).  Round A is parked before the chunk barrier, round B between the two
    // extra barriers.
    f32x16 o2, o3;
    float* pw = part + wave * PART_W + li * PSTR + 4 * lh;
    auto park = [&](int slot, const f32x16& o) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<f32x4*>(pw + slot * PTILE + 8 * q) = f32x4{o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
    };
    // y-fold (oy = 0: R0+R1+R2, oy = 1: R1-R2-R3) of parked tile `oh` = output column oc of the blocks, then store
    auto fold_store = [&](int oc, const f32x4 (&rvc)[4]) {
      const f32x4 ysign4 = {ysign, ysign, ysign, ysign};
      const float* pr = part + oh * PTILE + p8 * PSTR + 4 * q8;
      f32x4 y[4];   // block row gq, block column p8, couts 4*q8 .. 4*q8+3
      {
        f32x4 pp[3][4];
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
#pragma unroll
          for (int j = 0; j < 3; ++j)
            pp[j][gq] = *reinterpret_cast<const f32x4*>(pr + (oy + j) * PART_W + 8 * gq * PSTR);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) y[gq] = __builtin_elementwise_fma(pp[1][gq] + pp[2][gq], ysign4, pp[0][gq]);
      }
      if (vec) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          f32x4 o4 = y[gq] + bv;
          if (has_res) o4 += rvc[gq];
          if (a.relu) {
            o4[0] = vrelu1(o4[0]); o4[1] = vrelu1(o4[1]); o4[2] = vrelu1(o4[2]); o4[3] = vrelu1(o4[3]);
          }
          char* ub = reinterpret_cast<char*>(out_tile + rest * 32 + gq * gs_out + (oc - oh) * a.out_cs);   // uniform base
          __builtin_nontemporal_store(o4, reinterpret_cast<f32x4*>(ub + (unsigned)(lane_out * 4)));
        }
      } else {        // ragged tile / ragged or unaligned channels: element-wise
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          bool ok;
          const int pix = s2p(8 * gq + p8, oc, ok);
#pragma unroll
          for (int e4 = 0; e4 < 4; ++e4) {
            const int co = rest * 32 + 4 * q8 + e4;
            if (ok && co < a.Cout) {
              float o1 = y[gq][e4] + e.bias[co];
              if (has_res) o1 += e.resb[(size_t)pix * a.res_cs + co];
              if (a.relu) o1 = vrelu1(o1);
              e.outb[(size_t)pix * a.out_cs + co] = o1;
            }
          }
        }
      }
    };
    if (LAST) {
      {   // even output columns from the sums, odd ones from the differences
        const f32x16 s12 = acc[1] + acc[2], s34 = acc[3] + acc[4];
        park(0, acc[0] + s12 + s34);          // o0
        o2 = s12 + 4.f * s34;
      }
      __builtin_amdgcn_sched_barrier(0);
      {
        const f32x16 d12 = acc[1] - acc[2], d34 = acc[3] - acc[4];
        park(1, d12 + 2.f * d34);             // o1
        o3 = d12 + 8.f * d34 + acc[5];
      }
      // the weight fragments of the next item's first step go out now that the accumulators are dead
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int p = 0; p < 6; ++p) load_frag(p, wsn, 0);
      if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    }
    __syncthreads();   // barrier k+1
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    if (LAST) {
      const bool active = rest < a.n_tiles;
      if (active) fold_store(oh, rv[0]);              // round A: output columns 0 / 1
      __syncthreads();                                // extra barrier 1: every wave has read round A's tiles
      park(0, o2);
      park(1, o3);
      __syncthreads();                                // extra barrier 2: round B is parked
      if (active) fold_store(2 + oh, rv[1]);          // round B: output columns 2 / 3
      if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    }
    wsc = wsn;
    c0 = nc0;
    w = nw;
    ++k;
  };
  for (int item = 0; item < my_items; ++item) {
    chunk(std::true_type(), std::false_type());
    for (int ci = 2; ci < nchunks; ++ci) chunk(std::false_type(), std::false_type());
    chunk(std::false_type(), std::true_type());
  }
  if (stamp) a.dbg[63] = ns_;
}

// F(2x4,3x3): 3x3 stride 1, Cin >= 33 (two 32-channel chunks per item); any Cout / groups / map size (ragged tiles take the
// element-wise epilogue; maps narrower than 32 pixels waste slots - the packer keeps those on F(2x2,3x3)).
static hipError_t launch_wino24(const ConvArgs& a, hipStream_t s) {
  constexpr int NLW = 4;
  constexpr size_t lds = (2 * (size_t)10 * 34 * 36 + 4 * (size_t)2 * 32 * 36) * sizeof(float);
  static_assert(lds <= 160 * 1024, "two patch buffers and the exchange area must fit the 160 KiB LDS");
  if (a.ks != 3 || a.stride != 1 || (a.cin8 * 8 + 31) / 32 < 2) return hipErrorInvalidValue;
  return launch_conv_kernel(CONV_KERNEL(conv_wino24_kernel<NLW>), (4 + NLW) * 64, lds, (a.Wo + 31) / 32, (a.Ho + 7) / 8, a.n_tiles, a, s);
}
