// F(2x4,3x3) with ALL 24 Winograd positions of a tile in ONE wave (round 6) - included by conv_mfma.hip behind
// conv_wino24b.inc; same packed weights (algo 4: 4x6 taps through packer.pack_conv), same LDS-DMA patches, same input
// transform, a different ownership of the products.
//
// Why.  conv_wino24b_kernel gives wave py the six positions of position ROW py for two 32-cout tiles; the output transform
// needs all four rows, so an item ends with an exchange through LDS: x-fold in registers, park, barrier, y-fold of three
// waves' tiles, again for the odd columns - 770 VALU instructions, 32 ds_write_b128 per wave on the 13-cycle LDS store path
// and three barriers: 8.4k of the 38.6k cycles of a two-chunk item (DESIGN.md section 2 "Where an item's cycles go"), none of
// it hideable beside fp32 MFMAs (tools/coissue).  Here wave w owns 16 COUTS (of the item's 64) x all 24 positions x 32 slots:
// 48 accumulator tiles of v_mfma_f32_16x16x4_f32 (16 couts x 16 slots, 4 registers: 192 registers as before), so the whole
// output transform A2^T M A4 is a per-lane affair: no park, no exchange, no epilogue barrier, ~500 VALU.
//
// The price is on the input side: every wave now needs the transformed fragments of ALL positions.  Wave w still transforms
// position row w only (the same 12 window reads + 36 packed VALU per 8-channel step as conv_wino24b) and the four waves
// exchange the results through LDS once per step: 6 KiB written per wave (12 ds_write_b64, conflict-free up to 2-way), 24 KiB
// read (24 ds_read_b128, conflict-free), double-buffered (2 x 24 KiB), ONE workgroup barrier per step.  In-step order:
//   group 0 (positions 0-3): window rows of the NEXT step are requested;   group 1: row combination;
//   group 2: columns 0-2 of the next step's fragments are formed and stored;   group 3: columns 3-5;
//   group 4: barrier behind its MFMAs - the next step's fragments are complete, this step's have all been read;
//   group 5: the next step's first four fragments are fetched.
// Weight fragments: lane (cout m = lane & 15, k = lane >> 4) needs W[pos][16 w + m][channels c(g, k)], g = 0, 1, for the two
// K = 4 MFMAs of a position and step.  With c(g, k) = 4 (k & 1) + 2 (k >> 1) + g they are the two floats at byte 8 (k >> 1) of
// the 16-byte quad of lane 32 (k & 1) + 16 (w & 1) + m in conv_wino24's packed layout: one 8-byte buffer load per position
// and step, refreshed in place behind the position's MFMAs like conv_wino24b's.
// B fragments in LDS, per position 1 KiB: float 64 k + 4 s16 + 2 h + g = V[slot 16 h + s16][channel c(g, k)]: the reader's
// ds_read_b128 at quad 16 k + s16 returns {h0 g0, h0 g1, h1 g0, h1 g1}; the writer lane (slot li, channel quad lh) holds
// channels 4 lh .. 4 lh + 3 = (k = lh: g 0, 1), (k = lh + 2: g 0, 1): two 8-byte stores.
// Results: the products are conv_wino24_kernel's, summed over the channels in a different order (0, 4, 2, 6 | 1, 5, 3, 7 per
// step instead of 0, 4, 1, 5, 2, 6, 3, 7) and folded y first, then x: same arithmetic up to fp32 round-off.
// LDS: 2 x 48,128 B patches + 2 x 24,576 B fragments = 145,408 B.
//
// Takes: 3x3 stride 1, Cin % 32 == 0, Cin >= 64, Cout % 64 == 0, maps tiled exactly by 8x32-pixel items, 16-byte aligned
// channel slices, groups, per-frame bias, residual (incl. the broadcast map).
//
// STATUS (round 6): correct (tests/test_gpu_kernels.py::test_conv2d_winograd24_all_positions_frame), measured, NOT the default -
// see wino24c_ok below.
typedef float f32x2_w24c __attribute__((ext_vector_type(2)));
typedef int i32x4_w24c __attribute__((ext_vector_type(4)));

// One LDS-DMA piece as conv_wino24b's lds_dma16, but spelled in asm so that hipcc does NOT track it: this kernel reads LDS in
// every MFMA group (the exchanged fragments), and a tracked LDS-DMA makes every later ds_read that may alias it (same
// dynamic array: all of them) wait for the piece - HBM latency on the critical path of every chunk.  Ordering instead: a piece
// is complete before its issuing wave's next-but-one step (loads return in order and the wave waits for weight fragments it
// requested AFTER the piece before every MFMA group), and the chunk is first read two steps and two workgroup barriers later.
__device__ __forceinline__ void lds_dma16_raw(i32x4_w24c rsrc, unsigned lds_byte, int voff, int soff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
               :
               : "s"(lds_byte), "v"(voff), "s"(rsrc), "s"(soff)
               : "memory");
}

// timing ablations (tools/exp_build.sh -DACRMI_W24C_ABLATE=bits; WRONG results): 1 = no input-transform VALU, 2 = no weight
// loads in the steps, 4 = no fragment reads, 8 = no fragment stores, 16 = no step barrier, 32 = no window reads, 64 = no DMA
#ifndef ACRMI_W24C_ABLATE
#define ACRMI_W24C_ABLATE 0
#endif
__global__ __launch_bounds__(256, 1) void conv_wino24c_kernel(const ConvArgs a, const ConvWork wk) {
  constexpr int ABL = ACRMI_W24C_ABLATE;
  constexpr int CK = 32, TW = 32, TH = 8, PH = TH + 2, PWP = TW + 2;
  constexpr int RS = 300, GQ = 33, BCOLS = 8;
  constexpr int NPIECE = (PH * RS + 63) / 64;      // 47 DMA pieces of 64 quads
  constexpr int NI = (NPIECE + 3) / 4;             // 12 per wave
  constexpr int BUF = NPIECE * 64 * 4;             // floats per patch buffer
  constexpr int VPOS = 256, VBUF = 24 * VPOS;      // floats per position / per fragment buffer
  typedef f32x2_w24c f32x2;
  extern __shared__ f32x4 smem4[];
  float* lds = reinterpret_cast<float*>(smem4);
  float* vlds = lds + 2 * BUF;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nchunks = a.Cin / CK;                  // >= 2
  const int vb = virtual_block(a);
  const int my_items = wk.total > vb ? (wk.total - 1 - vb) / (int)gridDim.x + 1 : 0;
  const int ktotal = my_items * nchunks;
  // ---- transform side (as conv_wino24b_kernel): wave = position row py, lane = (slot li, channel quad lh)
  const int py = wave;
  const int li = lane & 31, lh = lane >> 5;
  const int ra = py == 0 ? 0 : (py == 2 ? 2 : 1);
  const int rb = py == 2 ? 1 : (py == 3 ? 3 : 2);
  const float sgn = py == 1 ? 1.f : -1.f;
  const int worg = ((2 * (li / BCOLS)) * RS + (li % BCOLS) * GQ) * 4 + 4 * lh;
  const int woff_a = worg + ra * RS * 4, woff_b = worg + rb * RS * 4;
  const int vw = (py * 6) * VPOS + 64 * lh + 4 * (li & 15) + 2 * (li >> 4);      // fragment store offset (floats), + px * VPOS, + 128
  // ---- product side: lane = (cout / slot m16, k index kq)
  const int m16 = lane & 15, kq = lane >> 4;
  const int vr = 64 * kq + 4 * m16;                                               // fragment load offset (floats), + pos * VPOS
  const bool has_res = a.res != nullptr;
  const float floor_ = a.relu ? 0.f : -__builtin_inff();
  f32x4 acc[24][2];

  // ---- weights: 8 bytes per position and step (see the file comment)
  const int tap_b = __builtin_amdgcn_readfirstlane(a.cin8 * a.n_tiles * 1024), step_b = __builtin_amdgcn_readfirstlane(a.n_tiles * 1024);
  const __amdgpu_buffer_rsrc_t wrsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, a.groups * 24 * tap_b, 0x00020000);
  const unsigned wlane = (unsigned)((32 * (kq & 1) + 16 * (wave & 1) + m16) * 16 + 8 * (kq >> 1));
  auto wbase = [&](int w_item) -> int {
    const ItemPos ip = item_pos(wk, w_item);
    return ip.g * 24 * tap_b + (ip.rest * 2 + (wave >> 1)) * 1024;
  };
  f32x2 A[24];
  auto load_A = [&](int p, int base, int step) {
    const int so = base + p * tap_b + (step < a.cin8 ? step : a.cin8 - 1) * step_b;
    A[p] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(wrsrc, wlane, so, 0));
  };

  // ---- input transform of the wave's position row (conv_wino24b_kernel's, verbatim)
  f32x4 d[2][3], v[6];
  // (in halves of three window columns: the raw rows of a half are 24 registers, row-combined into t before the other half
  //  is requested)
  auto read_rows = [&](const float* patch, int s, int half) {
#pragma unroll
    for (int c = 3 * half; c < 3 * half + 3; ++c) {
      const int cq = ((c >> 2) * GQ + (c & 3) * 8) * 4;
      d[0][c - 3 * half] = *reinterpret_cast<const f32x4*>(patch + woff_a + cq + s * 8);
      d[1][c - 3 * half] = *reinterpret_cast<const f32x4*>(patch + woff_b + cq + s * 8);
    }
  };
  const float one = a.ks == 3 ? 1.f : 2.f;   // always 1 (a runtime value: nothing is folded back into scalar ops)
  f32x2 sgnp = {sgn * one, sgn * one}, m1p = {-one, -one}, p4p = {4.f * one, 4.f * one}, m4p = {-4.f * one, -4.f * one},
        m5p = {-5.f * one, -5.f * one}, p2p = {2.f * one, 2.f * one}, m2p = {-2.f * one, -2.f * one}, p8p = {8.f * one, 8.f * one};
  asm volatile("" : "+v"(sgnp), "+v"(m1p), "+v"(p4p), "+v"(m4p), "+v"(m5p), "+v"(p2p), "+v"(m2p), "+v"(p8p));
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
  auto row_op = [&](f32x4 (&t)[6], int half) {
#pragma unroll
    for (int c = 0; c < 3; ++c) t[3 * half + c] = pk_fma4(sgnp, d[1][c], d[0][c]);
  };
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
  auto write_V = [&](float* vbuf, int px) {
    *reinterpret_cast<f32x2*>(vbuf + vw + px * VPOS) = f32x2{v[px][0], v[px][1]};
    *reinterpret_cast<f32x2*>(vbuf + vw + px * VPOS + 128) = f32x2{v[px][2], v[px][3]};
  };
  f32x4 Bf[2][2];                               // B fragments of the position pair being multiplied / of the next pair
  auto read_B = [&](const float* vbuf, int P, int set) {
#pragma unroll
    for (int q = 0; q < 2; ++q) Bf[set][q] = *reinterpret_cast<const f32x4*>(vbuf + (2 * P + q) * VPOS + vr);
  };

  // ---- LDS-DMA of the raw patches (conv_wino24b_kernel's)
  int jj[NI], doff[NI], eff[NI];
  unsigned dhb[NI / 4];
#pragma unroll
  for (int i = 0; i < NI / 4; ++i) dhb[i] = 0;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int j = i * 4 + wave;
    jj[i] = j < NPIECE ? j : NPIECE - 1;
    const int f = jj[i] * 64 + lane;
    const int row = f / RS, rem = f - row * RS;
    const int grp = rem / GQ, q = rem - grp * GQ;
    const int pix = grp * 4 + (q >> 3);
    const bool live = row < PH && q < 32 && pix < PWP;
    doff[i] = ((row * a.W + pix) * a.in_cs + 4 * (q & 7)) * 4;
    const unsigned hb = (row == 0 ? 1u : 0u) | (row == PH - 1 ? 2u : 0u) | (pix == 0 ? 4u : 0u) | (pix == PWP - 1 ? 8u : 0u) |
                        (live ? 0u : 16u);
    dhb[i >> 2] |= hb << (8 * (i & 3));
    eff[i] = (int)0x80000000;
  }
  const int tiles_y = wk.tiles_per_frame / wk.tiles_x;
  auto make_rsrc = [](const float* p, int records) -> i32x4_w24c {
    const unsigned long long u = (unsigned long long)p;
    return i32x4_w24c{__builtin_amdgcn_readfirstlane((int)(unsigned)u), __builtin_amdgcn_readfirstlane((int)((u >> 32) & 0xffffu)),
                      __builtin_amdgcn_readfirstlane(records), __builtin_amdgcn_readfirstlane(0x00020000)};
  };
  i32x4_w24c drsrc = make_rsrc(a.in, 0);
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) float*)lds;      // LDS byte address of the patches
  int wd = vb, cd0 = 0, kd = 0;     // DMA cursor: item, first channel and index of the next chunk to request
  auto dma_begin = [&]() {
    if (cd0 == 0) {                 // (uniform) the cursor enters an item: descriptor at its patch origin, halo lanes
      const bool valid = kd < ktotal;
      const ItemPos ip = item_pos(wk, valid ? wd : vb);
      const unsigned edge = (ip.ty == 0 ? 1u : 0u) | (ip.ty == tiles_y - 1 ? 2u : 0u) | (ip.tx == 0 ? 4u : 0u) |
                            (ip.tx == wk.tiles_x - 1 ? 8u : 0u) | 16u;
      const long long org = (((long long)ip.b * a.H + (ip.ty * TH - 1)) * a.W + (ip.tx * TW - 1)) * (long long)a.in_cs +
                            a.in_coff + ip.g * a.Cin;
      drsrc = make_rsrc(a.in + org, valid ? 0x7ffffff0 : 0);
#pragma unroll
      for (int i = 0; i < NI; ++i)
        eff[i] = ((dhb[i >> 2] >> (8 * (i & 3))) & edge) ? (int)0x80000000 : doff[i];
    }
  };
  auto dma_piece = [&](int i, int bsel) {
    lds_dma16_raw(drsrc, __builtin_amdgcn_readfirstlane(lds_base + (unsigned)(bsel * BUF + jj[i] * 256) * 4u), eff[i],
                  __builtin_amdgcn_readfirstlane(cd0 * 4));
  };
  auto dma_end = [&]() {
    cd0 += CK;
    if (cd0 >= a.Cin) { cd0 = 0; wd += (int)gridDim.x; }
    ++kd;
  };

  const bool stamp = a.dbg && blockIdx.x == 0 && tid == 0;
  int ns_ = 0;
  if (stamp) a.dbg[ns_++] = clock64();
  // ---- prologue: chunks 0 and 1 on their way, the first step's weights, the first step's fragments exchanged
  int w = vb, c0 = 0, k = 0, sg = 0;      // item, first channel of the chunk, chunk index, global step index
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
  for (int p = 0; p < 24; ++p) load_A(p, wsc, 0);
  // (the asm pieces are not tracked by hipcc: in the steady state they are ordered by the weight loads behind them - see
  //  lds_dma16_raw - but nothing younger is waited for before this first barrier, so the wait is explicit here)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  {
    f32x4 t[6];
    read_rows(lds, 0, 0);
    row_op(t, 0);
    read_rows(lds, 0, 1);
    row_op(t, 1);
    col_a(t);
    col_b(t);
    col_c(t);
#pragma unroll
    for (int px = 0; px < 6; ++px) write_V(vlds, px);
  }
  __syncthreads();
  read_B(vlds, 0, 0);

  // One 8-channel step: twelve pairs of positions x 4 MFMAs each (h0 g0, h1 g0, h0 g1, h1 g1: the two accumulators of a
  // position alternate, the 40-cycle dependent latency never shows).  rp / rs: patch and 8-channel step of the NEXT step's
  // window; wb / ws: weights of the next step.  BRIDGE = a chunk's last step (the window is the next chunk's first, the
  // pieces of the chunk after that go out, one per pair).  Behind pair 10 the workgroup barrier: the next step's fragments
  // are complete (stored behind pairs 4 and 6), this step's have all been read (pair 11's were requested in front of pair 10).
  auto step = [&](auto zero_tag, auto bridge_tag, const float* rp, int rs, int wb, int ws) __attribute__((always_inline)) {
    constexpr bool ZERO = decltype(zero_tag)::value, BRIDGE = decltype(bridge_tag)::value;
    const float* vcur = vlds + (sg & 1) * VBUF;
    float* vnext = vlds + ((sg + 1) & 1) * VBUF;
    int wso = __builtin_amdgcn_readfirstlane(wb + (ws < a.cin8 ? ws : a.cin8 - 1) * step_b);      // the next step's weights, position by position
    f32x4 t[6];
    if (BRIDGE) dma_begin();
#pragma unroll
    for (int P = 0; P < 12; ++P) {
      __builtin_amdgcn_sched_barrier(0);
#ifdef ACRMI_W24_STEPSTAMPS
      if (P == 0 && stamp && ns_ < 60) a.dbg[ns_++] = clock64();
#endif
      if (P == 0 && !(ABL & 32)) read_rows(rp, rs, 0);
      if (P == 1) { if (!(ABL & 1)) row_op(t, 0); if (!(ABL & 32)) read_rows(rp, rs, 1); }
      if (P == 2 && !(ABL & 1)) row_op(t, 1);
      if (!(ABL & 4)) {
        if (P < 11) read_B(vcur, P + 1, (P + 1) & 1);
        else read_B(vnext, 0, 0);                    // (behind the barrier: the next step's fragments are complete)
      }
      if (BRIDGE && !(ABL & 64)) dma_piece(P, k & 1);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int p = 2 * P + q;
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            // (spelled in asm with the accumulator tied in place: through the builtin hipcc renames every accumulator on
            //  every MFMA - up to 256 AGPRs in flight for 192 live ones, nothing left to spill VGPRs into, 700 B of scratch)
            if (ZERO && g == 0)
              asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, 0" : "=a"(acc[p][h]) : "v"(A[p][g]), "v"(Bf[P & 1][q][2 * h + g]));
            else
              asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+a"(acc[p][h]) : "v"(A[p][g]), "v"(Bf[P & 1][q][2 * h + g]));
          }
      }
      __builtin_amdgcn_sched_barrier(0);
      // (staggering the stores over the waves - wave w behind pair 3 + w / 6 + w - was tried: slower, the uniform branches cost
      //  more than the shared store path; profiles/r06_wino24c_ablation.txt)
      if (P == 4) {
        if (!(ABL & 1)) col_a(t);
        if (!(ABL & 8)) {
          write_V(vnext, 0);
          write_V(vnext, 1);
          write_V(vnext, 2);
        }
      }
      if (P == 6) {
        if (!(ABL & 1)) {
          col_b(t);
          col_c(t);
        }
        if (!(ABL & 8)) {
          write_V(vnext, 3);
          write_V(vnext, 4);
          write_V(vnext, 5);
        }
      }
      if (P == 10 && !(ABL & 16)) __syncthreads();
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (!(ABL & 2)) A[2 * P + q] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(wrsrc, wlane, wso, 0));
        wso = __builtin_amdgcn_readfirstlane(wso + tap_b);
        asm volatile("" : "+s"(wso));      // (pins the running offset: hipcc otherwise forms all 24 at the top of the step - 24 SGPRs)
      }
    }
    if (BRIDGE) dma_end();
    ++sg;
  };

  for (int item = 0; item < my_items; ++item) {
    const int nw = w + (int)gridDim.x;
    const bool more = item + 1 < my_items;
    const int wsn = more ? wbase(nw) : wsc;
    // what the epilogue needs (scalar): item position, output tile, residual / bias descriptors
    const ItemPos ip = item_pos(wk, w);
    const int cch = ip.rest * 64 + 16 * wave + 4 * kq;          // the lane's first cout inside the group
    const float* bias = a.bias + (size_t)ip.g * a.n_tiles * 32 + (size_t)ip.b * a.bias_fstride;
    const int tile_pix = ip.ty * TH * a.Wo + ip.tx * TW;
    float* out_tile = a.out + (size_t)ip.b * a.Ho * a.Wo * a.out_cs + a.out_coff + ip.g * a.Cout + (size_t)tile_pix * a.out_cs;
    const size_t res_off = (res_frame_off(a, ip.b) + (size_t)tile_pix * a.res_cs) + a.res_coff + ip.g * a.Cout;
    const size_t res_left = has_res ? (res_total(a) - res_off) * 4 : 0;
    const __amdgpu_buffer_rsrc_t rrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(has_res ? a.res + res_off : a.in), 0, (int)(unsigned)(res_left > 0xffffffffu ? 0xffffffffu : res_left), 0x00020000);
    const __amdgpu_buffer_rsrc_t brsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bias), 0, bias_row_left(a, ip.g), 0x00020000);
    // (first / middle / last chunk spelled out, as in conv_wino24b_kernel: one zero-initialising chunk, a plain loop, one chunk
    //  whose last step fetches the next item's weights - no run-time choice between step variants inside the loop)
    auto chunk = [&](auto first_tag, auto last_tag) __attribute__((always_inline)) {
      constexpr bool FIRST = decltype(first_tag)::value, LAST = decltype(last_tag)::value;
      if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
      const float* patch = lds + (k & 1) * BUF;
      const float* patch_n = lds + ((k + 1) & 1) * BUF;
      const int s0 = c0 / 8;
      if (FIRST) step(std::true_type(), std::false_type(), patch, 1, wsc, s0 + 1);
      else step(std::false_type(), std::false_type(), patch, 1, wsc, s0 + 1);
      step(std::false_type(), std::false_type(), patch, 2, wsc, s0 + 2);
      step(std::false_type(), std::false_type(), patch, 3, wsc, s0 + 3);
      if (LAST) step(std::false_type(), std::true_type(), patch_n, 0, wsn, 0);
      else step(std::false_type(), std::true_type(), patch_n, 0, wsc, s0 + 4);
      c0 = LAST ? 0 : c0 + CK;
      ++k;
    };
    chunk(std::true_type(), std::false_type());
    for (int ci = 2; ci < nchunks; ++ci) chunk(std::false_type(), std::false_type());
    chunk(std::false_type(), std::true_type());
    __builtin_amdgcn_sched_barrier(0);
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    // ---- item epilogue, all in registers: Y = A2^T M (y first: two rows of six), then the x-fold with A4^T, bias, residual,
    // ReLU, 16-byte stores (the lane's 4 couts of one pixel).  Residual rows are requested one row ahead.
    {
      const f32x4 bias4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(brsrc, (unsigned)(cch * 4), 0, 0));
      f32x4 R[2][4];
      auto lane_pix = [&](int h) -> int {        // pixel (row 2 br, column 4 bc) of the lane's slot in half h
        const int slot = 16 * h + m16;
        return (2 * (slot >> 3)) * a.Wo + 4 * (slot & 7);
      };
      auto request_res = [&](int h, int oy) {
        const int base = (lane_pix(h) + oy * a.Wo) * a.res_cs + cch;
#pragma unroll
        for (int ox = 0; ox < 4; ++ox)
          R[oy][ox] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rrsrc, (unsigned)((base + ox * a.res_cs) * 4), 0, RES_CACHE_WINO));
      };
      request_res(0, 0);
      request_res(0, 1);
      // (the asm MFMAs and the asm accumulator reads below are invisible to hipcc's hazard recognizer: the last MFMA's 8
      //  passes drain here)
      asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        __builtin_amdgcn_sched_barrier(0);
        f32x4 Y[2][6];
        // (the accumulators live in AGPRs; read with explicit v_accvgpr_read_b32, one window column at a time: left to itself
        //  hipcc copies all 192 of them to VGPRs at the top of the epilogue and spills - conv_wino24b.inc has the same note)
        auto rd = [](const f32x4& x) -> f32x4 {
          f32x4 r;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float t;
            asm("v_accvgpr_read_b32 %0, %1" : "=v"(t) : "a"(x[e]));
            r[e] = t;
          }
          return r;
        };
#pragma unroll
        for (int px = 0; px < 6; ++px) {
          __builtin_amdgcn_sched_barrier(0);
          const f32x4 a0 = rd(acc[px][h]), a1 = rd(acc[6 + px][h]), a2 = rd(acc[12 + px][h]), a3 = rd(acc[18 + px][h]);
          const f32x4 t12 = pk_add4(a1, a2), t23 = pk_add4(a2, a3);
          Y[0][px] = pk_add4(a0, t12);                 // R0 + (R1 + R2)
          Y[1][px] = pk_fma4(m1p, t23, a1);            // R1 - (R2 + R3)
        }
#pragma unroll
        for (int oy = 0; oy < 2; ++oy) {
          __builtin_amdgcn_sched_barrier(0);
          const f32x4(&m)[6] = Y[oy];
          f32x4 o[4];
          const f32x4 s12 = pk_add4(m[1], m[2]), s34 = pk_add4(m[3], m[4]);
          o[0] = pk_add4(pk_add4(m[0], s12), s34);
          o[2] = pk_fma4(p4p, s34, s12);
          const f32x4 d12 = pk_fma4(m1p, m[2], m[1]), d34 = pk_fma4(m1p, m[4], m[3]);
          o[1] = pk_fma4(p2p, d34, d12);
          o[3] = pk_add4(pk_fma4(p8p, d34, d12), m[5]);
          char* ub = reinterpret_cast<char*>(out_tile);         // uniform
          const unsigned lo = (unsigned)(((lane_pix(h) + oy * a.Wo) * a.out_cs + cch) * 4);
#pragma unroll
          for (int ox = 0; ox < 4; ++ox) {
            f32x4 o4 = pk_add4(pk_add4(o[ox], bias4), R[oy][ox]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {      // (one v_max_f32 per float: fmaxf canonicalises its operand first - two per float)
              float r;
              asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(o4[e]), "v"(floor_));
              o4[e] = r;
            }
            __builtin_nontemporal_store(o4, reinterpret_cast<f32x4*>(ub + lo + (unsigned)(ox * a.out_cs * 4)));
          }
          if (h == 0) request_res(1, oy);                       // the other half's row takes this row's registers
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    wsc = wsn;
    w = nw;
  }
  if (stamp) a.dbg[63] = ns_;
}

// conv_wino24c_kernel for the shapes it takes (conv_rules.h takes_wino24c).  NOT routed by default: measured 7 % SLOWER than conv_wino24b_kernel on the two-chunk
// layers (item 41.2k vs 38.6k cycles: the epilogue drops from 8.4k to 5.9k, but the per-step fragment exchange - 24 reads,
// 12 stores, a barrier, 24 instead of 12 weight loads - adds ~600 cycles to each of the 8 steps; profiles/r06_wino24c_ablation.txt,
// DESIGN.md section 7).  conv_bench --cfg 842 / acrmi_tune(0, 842) selects it (A/B runs, tests/test_gpu_kernels.py).
static bool wino24c_ok(const ConvArgs& a) { return g_force_cfg == 842 && takes_wino24c(conv_shape(a)); }

static hipError_t launch_wino24c(const ConvArgs& a, hipStream_t s) {
  constexpr size_t lds = (2 * (size_t)47 * 64 * 4 + 2 * (size_t)24 * 256) * sizeof(float);
  static_assert(lds <= 160 * 1024, "patches + fragment buffers must fit the 160 KiB LDS");
  return launch_conv_kernel(CONV_KERNEL(conv_wino24c_kernel), 256, lds, a.Wo / 32, a.Ho / 8, a.Cout / 64, a, s);
}
