// Direct convolution (3x3 stride 2, 1x1, and the 3x3 stride-1 fallback) - included by conv_mfma.hip.
//
// Same workgroup shape as the Winograd kernel: NCW = WAVES_M x WAVES_N compute waves (one per SIMD) + NLW loader
// waves streaming the raw halo'd patch [PH][PW][CK+4] HBM -> LDS (ws_loader), one workgroup barrier per Cin chunk.
// Per compute wave MT x NTW accumulator tiles (32 output pixels x 32 couts each).  What the inner loop is built
// around (tools/valu_beside_mfma.hip): next to a 64-cycle fp32 MFMA a ds_read_b128 costs ~1 cycle, a VALU
// instruction ~4.5 (+9 for switching), a 16-byte global load ~16, and a load behind a branch turns every later
// wait into vmcnt(0).  So:
//  * the (8-channel step, tap) units of a chunk are unrolled statically, UNITS per pass, over a ring of R fragment
//    sets: behind the MFMAs of unit u the fragments of unit u+R are requested into the same registers (prefetch
//    distance R-1 units, no register copies, no double buffer);
//  * weight fragments: raw buffer loads, lane part in the vector offset, (tap, step, n-tile) in the SCALAR offset:
//    no address VALU; always issued (clamped past the end), and the stream simply runs on into the item's next
//    chunk (steps are contiguous in the packed weights);
//  * activation fragments: ds_read_b128 with immediate tap offsets from one address register per M-tile;
//  * MFMA operands are swapped (weights as A, activations as B): an accumulator tile is D[cout][pixel], the lane
//    owns one pixel and register quad g holds couts 8g+4*lh .. +3; the epilogue sends each tile through a
//    wave-private LDS tile [32 pixels][36] (4 ds_write_b128 + 4 ds_read_b128, no barrier) to get 8 lanes per
//    pixel = one 128-byte line per 8 lanes for residual loads and non-temporal stores - instead of ~120 VALU
//    instructions of cross-lane transposes per tile;
//  * the first MFMA per accumulator of an item takes C = 0 (inline constant).
// The chunk body is instantiated per (first, last) chunk of an item so that no fragment register flows through a
// control-flow merge.

// ONE: every item is a single Cin chunk (Cin <= CK).
// XT: the epilogue adds ConvArgs.xt, up to three extra residual terms at 1 / 2^shift of the output resolution (the HR-module
// fuse sum folded into the last convolution of the x0 downsampling chain; small-batch programs: 3x3 stride 2, 32-cout items).
template <int KS, int S, int TH, int TW, int WAVES_M, int MT, int WAVES_N, int NTW, int CK, int NLW, bool ONE, bool XT = false>
__global__ __launch_bounds__((WAVES_M * WAVES_N + NLW) * 64, 1) void conv_ws2_kernel(const ConvArgs a, const ConvWork wk) {
  static_assert(!XT || (!ONE && NTW == 1), "extra residual terms: multi-chunk items of one n-tile per wave");
  constexpr int PH = (TH - 1) * S + KS, PW = (TW - 1) * S + KS, CP = CK + 4;
  constexpr int NCW = WAVES_M * WAVES_N;
  constexpr int TAPS = KS * KS;
  constexpr int BUF = PH * PW * CP;
  constexpr int SPC = CK / 8;                       // 8-channel steps per full chunk
  constexpr int R = TAPS == 1 ? 4 : 3;              // weight-fragment ring (L2 latency)
  constexpr int RA = TAPS == 1 ? 2 : 3;             // activation-fragment ring (LDS latency)
  constexpr int SU = TAPS == 1 ? 4 : 1;             // steps per statically unrolled pass
  constexpr int UNITS = SU * TAPS;                  // (step, tap) units per pass
  constexpr int PSTR = 36, PTILE = 32 * PSTR;       // epilogue tile: [32 pixels][32 couts + 4 pad]
  static_assert(UNITS % R == 0 && UNITS % RA == 0, "the rings must divide a pass");
  static_assert(SPC % SU == 0, "a full chunk is a whole number of passes");
  static_assert(TH * TW == 32 * MT * WAVES_M, "tile pixels must equal 32*MT*WAVES_M");
  static_assert(TW == 16, "epilogue pixel mapping assumes 16-pixel tile rows");
  extern __shared__ f32x4 smem4[];
  float* lds = reinterpret_cast<float*>(smem4);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cin_pad = a.cin8 * 8;
  const int nchunks = (cin_pad + CK - 1) / CK;
  const int vb = virtual_block(a);
  const int my_items = wk.total > vb ? (wk.total - 1 - vb) / (int)gridDim.x + 1 : 0;
  const int ktotal = my_items * nchunks;
  if (wave >= NCW) {
    ws_loader<KS, S, TH, TW, CK, NLW>(a, wk, lds, tid - NCW * 64, ktotal, cin_pad);
    return;
  }
  const int wm = wave % WAVES_M, wn = wave / WAVES_M;
  const int li = lane & 31, lh = lane >> 5;
  float* epi = lds + 2 * BUF + wave * PTILE;
  int aoff[MT];   // patch offset (floats) of this lane's pixel in M-tile m, tap (0,0), channel 4*lh
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int p = (wm * MT + m) * 32 + li;
    aoff[m] = ((p / TW) * S * PW + (p % TW) * S) * CP + 4 * lh;
  }
  // store side: lane = (pixel p8 of a half row, cout quad q8), 4 half rows gq per tile
  const int p8 = lane >> 3, q8 = lane & 7;
  const bool has_res = a.res != nullptr;

  const int tap_b = a.cin8 * a.n_tiles * 1024, step_b = a.n_tiles * 1024;   // weight bytes per tap / per step
  const __amdgpu_buffer_rsrc_t wrsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.groups * TAPS * tap_b, 0x00020000);
  const unsigned wlane = lane * 16;
  f32x16 acc[MT][NTW];
  f32x4 act[RA][MT], wgt[R][NTW];
  int w = vb, c0 = 0;
  struct WStream {   // weights of one item: byte offset of (group, n-block of this wave) + clamped n-tile offsets
    int base;
    int nto[NTW];
    int active;      // this wave's first n-tile exists (int: a bool member sends the struct copies through scratch)
  };
  auto wstream = [&](int w_item, int nb) -> WStream {   // nb < 0: the item's own n-block
    const ItemPos ip = item_pos(wk, w_item);
    const int nt0 = ((nb < 0 ? ip.rest : nb) * WAVES_N + wn) * NTW;
    WStream ws;
    ws.active = nt0 < a.n_tiles;
    const int nt0c = ws.active ? nt0 : 0;
    ws.base = ip.g * TAPS * tap_b + nt0c * 1024;
#pragma unroll
    for (int n = 0; n < NTW; ++n) ws.nto[n] = (nt0c + n < a.n_tiles ? n : a.n_tiles - 1 - nt0c) * 1024;
    return ws;
  };
  auto load_w = [&](int r, const WStream& ws, int tap, int step) {
    const int so = ws.base + tap * tap_b + (step < a.cin8 ? step : a.cin8 - 1) * step_b;
#pragma unroll
    for (int n = 0; n < NTW; ++n)
      wgt[r][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane, so + ws.nto[n], 0));
  };
  // ONE-chunk items can run all their n-blocks from the one LDS patch (wk.nb_inner > 1, the work list then has one
  // item per tile): the input tile is read once instead of once per n-block
  const int nbn = ONE ? wk.nb_inner : 1;
  WStream wsc = wstream(w, nbn > 1 ? 0 : -1);
  if (ktotal > 0) {
#pragma unroll
    for (int u = 0; u < R; ++u) load_w(u, wsc, u % TAPS, u / TAPS);
  }
  const bool stamp = a.dbg && blockIdx.x == 0 && tid == 0;   // per chunk: start, MFMAs done, barrier, (stored)
  int ns_ = 0;
  if (stamp) a.dbg[ns_++] = clock64();
  __syncthreads();   // barrier 0: chunk 0 is in buffer 0
  int k = 0;
  auto chunk = [&](auto first_tag, auto last_tag) {
    constexpr bool FIRST = decltype(first_tag)::value, LAST = decltype(last_tag)::value;
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    const float* patch = lds + (k & 1) * BUF;
    const int nc0 = LAST ? 0 : c0 + CK, nw = LAST ? w + (int)gridDim.x : w;
    const bool more = k + 1 < ktotal;
    const WStream wsn = (LAST && more) ? wstream(nw, nbn > 1 ? 0 : -1) : wsc;
    const int nsteps = (cin_pad - c0 < CK ? cin_pad - c0 : CK) / 8;
    // ---- an item's last chunk first requests the item's residual and bias: by the epilogue they are there, and
    // the fragment waits in between do not see them (the weight ring is requested R units ahead of its use).
    // Raw buffer loads, always issued (a branch would make hipcc wait for vmcnt(0) in the MFMA loop): without a
    // residual the descriptor has zero records and the loads return 0 without touching memory.
    int nt0 = 0, item_rest = 0;
    float* outb = nullptr;
    const float* bias = nullptr;
    const float* resb = nullptr;
    bool vec_align = false;
    f32x4 rv[MT][NTW][4], bv[NTW];
    f32x4 xv[XT ? 3 : 1][MT][4];
    int pix[MT][4];
    bool pok[MT][4];
    __amdgpu_buffer_rsrc_t rrsrc = wrsrc, brsrc = wrsrc;
    __amdgpu_buffer_rsrc_t xrs[3] = {wrsrc, wrsrc, wrsrc};
    int xvo[XT ? 3 : 1][MT][4];
    if (LAST) {
      const ItemPos ip = item_pos(wk, w);
      const int g = ip.g, b = ip.b;
      const int ty0 = ip.ty * TH, tx0 = ip.tx * TW;
      item_rest = ip.rest;
      bias = a.bias + (size_t)g * a.n_tiles * 32 + (size_t)b * a.bias_fstride;
      outb = a.out + (size_t)b * a.Ho * a.Wo * a.out_cs + a.out_coff + g * a.Cout;
      resb = has_res ? a.res + res_frame_off(a, b) + a.res_coff + g * a.Cout : nullptr;
      vec_align = ((a.out_coff + g * a.Cout) % 4 == 0) && (a.out_cs % 4 == 0) &&
                  (!has_res || (((a.res_coff + g * a.Cout) % 4 == 0) && (a.res_cs % 4 == 0)));
      const bool full_tile = (ty0 + TH <= a.Ho) && (tx0 + TW <= a.Wo);
      // pixel of (M-tile m, half row gq, lane): tile-relative p = (wm*MT + m)*32 + 8*gq + p8 -> row p/16, col p%16
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int p = (wm * MT + m) * 32 + 8 * gq + p8;
          int y = ty0 + p / TW, x = tx0 + p % TW;
          pok[m][gq] = full_tile || (y < a.Ho && x < a.Wo);
          y = y < a.Ho ? y : a.Ho - 1;
          x = x < a.Wo ? x : a.Wo - 1;
          pix[m][gq] = y * a.Wo + x;
        }
      // (records = what is left of the residual tensor behind this frame/group origin: a clamped n-tile of a ragged
      // Cout may point past a pixel's channels, never past the tensor)
      const size_t res_off = res_frame_off(a, b) + a.res_coff + g * a.Cout;
      const size_t res_left = (res_total(a) - res_off) * 4;
      rrsrc = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(has_res ? resb : a.in), 0,
          (has_res && vec_align) ? (int)(unsigned)(res_left > 0xffffffffu ? 0xffffffffu : res_left) : 0, 0x00020000);
      brsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bias), 0, bias_row_left(a, g), 0x00020000);
      if constexpr (XT) {
        // the extra terms at this frame / group; the lane's pixel (y >> shift, x >> shift) of term t.  A missing term reads
        // zeros through a zero-record descriptor (branch-free).
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const bool on = t < a.nxt;
          const int sh = on ? a.xt_shift[t] : 0, cs = on ? a.xt_cs[t] : 4;
          const int hs = a.Ho >> sh, wsx = a.Wo >> sh;
          const size_t off = (size_t)b * hs * wsx * cs + (on ? a.xt_coff[t] : 0) + g * a.Cout;
          const size_t left = on ? ((size_t)a.B * hs * wsx * cs - off) * 4 : 0;
          xrs[t] = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(on ? a.xt[t] + off : a.in), 0,
                                                     (int)(unsigned)(left > 0xffffffffu ? 0xffffffffu : left), 0x00020000);
#pragma unroll
          for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
              const int pp = (wm * MT + m) * 32 + 8 * gq + p8;
              int y = ty0 + pp / TW, x = tx0 + pp % TW;
              y = y < a.Ho ? y : a.Ho - 1;
              x = x < a.Wo ? x : a.Wo - 1;
              xvo[t][m][gq] = (((y >> sh) * wsx + (x >> sh)) * cs + 4 * q8) * 4;
            }
        }
      }
    }
    for (int nb = 0; nb < nbn; ++nb) {
    if (LAST) {
      nt0 = ((nbn > 1 ? nb : item_rest) * WAVES_N + wn) * NTW;
#pragma unroll
      for (int n = 0; n < NTW; ++n) {
        const int ntc = nt0 + n < a.n_tiles ? nt0 + n : a.n_tiles - 1;
        bv[n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(brsrc, 16 * q8, ntc * 128, 0));
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int gq = 0; gq < 4; ++gq)
            rv[m][n][gq] = __builtin_bit_cast(
                f32x4, __builtin_amdgcn_raw_buffer_load_b128(rrsrc, (pix[m][gq] * a.res_cs + 4 * q8) * 4, ntc * 128, RES_CACHE_DIRECT));
        if constexpr (XT) {      // (NTW == 1)
#pragma unroll
          for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
              for (int gq = 0; gq < 4; ++gq)
                xv[t][m][gq] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs[t], xvo[t][m][gq], ntc * 128, 0));
        }
      }
    }
    // activation fragments of the first RA units (the patch only became visible at the barrier)
#pragma unroll
    for (int u = 0; u < RA; ++u)
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int t = u % TAPS;
        act[u][m] = *reinterpret_cast<const f32x4*>(patch + aoff[m] + ((t / KS) * PW + t % KS) * CP + (u / TAPS) * 8);
      }
    // one pass = UNITS statically unrolled (step, tap) units starting at step s
    auto pass = [&](int s, auto zero_tag) {
      constexpr bool ZERO = decltype(zero_tag)::value;
      const float* ps = patch + s * 8;
#pragma unroll
      for (int u = 0; u < UNITS; ++u) {
        const int r = u % R, ra = u % RA;
        __builtin_amdgcn_sched_barrier(0);
        if (SU == 1 || s + u / TAPS < nsteps) {   // (ragged chunk: uniform branch around the MFMAs only)
          // a ragged last step with <= 4 channels inside Cin (34: the coordinate channels): MFMA j multiplies channels
          // j and 4 + j of the step, the ones past `left` would add exact zeros
          const int left = a.Cin - c0 - 8 * (s + u / TAPS);
          const int jn = (left >= 5 || a.phase_delay == 5) ? 4 : (left < 1 ? 1 : left);   // (conv_bench --phase 5: all four)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j > 0 && j >= jn) continue;     // (uniform)
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
              for (int n = 0; n < NTW; ++n) {
                if (ZERO && u == 0 && j == 0) {
                  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                  acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(wgt[r][n][j], act[ra][m][j], zero, 0, 0, 0);
                } else {
                  acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(wgt[r][n][j], act[ra][m][j], acc[m][n], 0, 0, 0);
                }
              }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        // units u + RA (activations, LDS) and u + R (weights, L2) into the registers unit u just released
        const int ua = u + RA, ta = ua % TAPS, sa = ua / TAPS;   // static tap, static step offset
#pragma unroll
        for (int m = 0; m < MT; ++m)
          act[ra][m] = *reinterpret_cast<const f32x4*>(ps + aoff[m] + ((ta / KS) * PW + ta % KS) * CP + sa * 8);
        const int un = u + R, tn = un % TAPS, sn = un / TAPS;
        load_w(r, wsc, tn, c0 / 8 + s + sn);
      }
    };
    // the first pass of every chunk is peeled: a wait at the head of the pass loop has to hold for the back edge
    // too, so hipcc would make the chunk's first fragment wait (vmcnt = ring loads in flight) also wait for the
    // residual loads just requested above
    if (FIRST) pass(0, std::true_type());
    else pass(0, std::false_type());
    for (int s = SU; s < nsteps; s += SU) pass(s, std::false_type());
    __builtin_amdgcn_sched_barrier(0);
    if (nb + 1 == nbn) {   // the patch is free once the item's last n-block has read it
      if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
      __syncthreads();   // barrier k+1
      if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    }
    if (LAST) {
      // ---- epilogue: bias, residual, ReLU, store; each tile goes through the wave's LDS tile
      if (wsc.active) {
        bool vec[NTW];
#pragma unroll
        for (int n = 0; n < NTW; ++n) vec[n] = vec_align && ((nt0 + n + 1) * 32 <= a.Cout);
#pragma unroll
        for (int n = 0; n < NTW; ++n) {
          if (nt0 + n >= a.n_tiles) continue;
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            // D[cout][pixel]: lane (li, lh) holds pixel li, couts 8q+4lh..+3 in register quad q
#pragma unroll
            for (int q = 0; q < 4; ++q)
              *reinterpret_cast<f32x4*>(epi + li * PSTR + 8 * q + 4 * lh) =
                  f32x4{acc[m][n][4 * q], acc[m][n][4 * q + 1], acc[m][n][4 * q + 2], acc[m][n][4 * q + 3]};
            f32x4 y[4];
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) y[gq] = *reinterpret_cast<const f32x4*>(epi + (8 * gq + p8) * PSTR + 4 * q8);
            if (vec[n]) {
#pragma unroll
              for (int gq = 0; gq < 4; ++gq) {
                f32x4 o4 = y[gq] + bv[n] + rv[m][n][gq];   // (rv is 0 without a residual)
                if constexpr (XT) o4 = ((o4 + xv[0][m][gq]) + xv[1][m][gq]) + xv[2][m][gq];
                if (a.relu) {
                  o4[0] = vrelu1(o4[0]); o4[1] = vrelu1(o4[1]); o4[2] = vrelu1(o4[2]); o4[3] = vrelu1(o4[3]);
                }
                if (pok[m][gq])
                {   // uniform base + 32-bit lane offset: one address register per store
                  char* ub = reinterpret_cast<char*>(outb + (nt0 + n) * 32);
                  __builtin_nontemporal_store(
                      o4, reinterpret_cast<f32x4*>(ub + (unsigned)((pix[m][gq] * a.out_cs + 4 * q8) * 4)));
                }
              }
            } else {   // ragged or unaligned channels: element-wise
#pragma unroll
              for (int gq = 0; gq < 4; ++gq)
#pragma unroll
                for (int e4 = 0; e4 < 4; ++e4) {
                  const int co = (nt0 + n) * 32 + 4 * q8 + e4;
                  if (pok[m][gq] && co < a.Cout) {
                    float o1 = y[gq][e4] + bias[co];
                    if (has_res) o1 += resb[(size_t)pix[m][gq] * a.res_cs + co];
                    if (a.relu) o1 = vrelu1(o1);
                    outb[(size_t)pix[m][gq] * a.out_cs + co] = o1;
                  }
                }
            }
          }
        }
      }
      // weight fragments of the first units of the item's next n-block / of the next item
      __builtin_amdgcn_sched_barrier(0);
      const WStream wnext = nb + 1 < nbn ? wstream(w, nb + 1) : wsn;
#pragma unroll
      for (int u = 0; u < R; ++u) load_w(u, wnext, u % TAPS, u / TAPS);
      wsc = wnext;
      if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    }
    }   // n-blocks of the item
    if (!LAST) wsc = wsn;
    c0 = nc0;
    w = nw;
    ++k;
  };
  for (int item = 0; item < my_items; ++item) {
    if constexpr (ONE) {
      chunk(std::true_type(), std::true_type());
    } else {
      chunk(std::true_type(), std::false_type());
      for (int ci = 2; ci < nchunks; ++ci) chunk(std::false_type(), std::false_type());
      chunk(std::false_type(), std::true_type());
    }
  }
  if (stamp) a.dbg[63] = ns_;
}

template <int KS, int S, int TH, int TW, int WAVES_M, int MT, int WAVES_N, int NTW, int CK, int NLW, bool ONE, bool XT = false>
static hipError_t launch_ws2_impl(const ConvArgs& a, hipStream_t s) {
  constexpr int PH = (TH - 1) * S + KS, PW = (TW - 1) * S + KS;
  constexpr size_t lds = (2 * (size_t)PH * PW * (CK + 4) + (size_t)WAVES_M * WAVES_N * 32 * 36) * sizeof(float);
  static_assert(lds <= 160 * 1024, "two patch buffers and the epilogue tiles must fit the 160 KiB LDS");
  // (XT: the vector epilogue only - Cout % 32 == 0, 16-byte aligned output channels: conv_rules.h conv_algo_reject)
  int nblk = (a.n_tiles + WAVES_N * NTW - 1) / (WAVES_N * NTW), nb_inner = 1;
  if (ONE && nblk > 1 && g_force_cfg != 901) {   // all n-blocks of a tile from one patch
    nb_inner = nblk;
    nblk = 1;
  }
  return launch_conv_kernel(CONV_KERNEL(conv_ws2_kernel<KS, S, TH, TW, WAVES_M, MT, WAVES_N, NTW, CK, NLW, ONE, XT>),
                            (WAVES_M * WAVES_N + NLW) * 64, lds, (a.Wo + TW - 1) / TW, (a.Ho + TH - 1) / TH, nblk, a, s, nb_inner);
}

template <int KS, int S, int TH, int TW, int WAVES_M, int MT, int WAVES_N, int NTW, int CK, int NLW>
static hipError_t launch_ws2(const ConvArgs& a, hipStream_t s) {
  if ((a.cin8 * 8 + CK - 1) / CK < 2)
    return launch_ws2_impl<KS, S, TH, TW, WAVES_M, MT, WAVES_N, NTW, CK, NLW, true>(a, s);
  return launch_ws2_impl<KS, S, TH, TW, WAVES_M, MT, WAVES_N, NTW, CK, NLW, false>(a, s);
}
