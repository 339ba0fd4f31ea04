// F(2x4,3x3) on a four-wave, 512-register frame - included by conv_mfma.hip behind conv_wino24.inc (same packed weights,
// same arithmetic, same item order; launch_wino24 sends the shapes this kernel takes here and keeps the rest).
//
// Why a second frame.  conv_wino24_kernel runs 4 compute + 4 loader waves, i.e. two waves per SIMD and 256 registers per
// wave: 96 accumulator registers (6 positions x ONE 32-cout tile) are all that fits next to the fragment buffers, so the
// input transform (36 packed VALU + 12 window reads per 8-channel step) is paid per 24 MFMAs, a chunk starts with a
// ~1.6k-cycle prologue (the patch only becomes readable at the chunk barrier) and the matrix pipe is 0.48 busy
// (profiles/r03_pmc_mfma.txt).  fp32 MFMAs run at the vector rate on gfx950: every VALU / LDS / VMEM instruction of the
// wave is issue time the matrix pipe does not get back, so the lever is fewer of them per MFMA.
//
// This frame: 256 threads = one wave per SIMD, up to 512 registers per wave, no loader waves.
//  * NT = 2: wave py owns positions (py, 0..5) of TWO 32-cout tiles (192 accumulator registers): transform and window
//    reads per MFMA halve, the patch is fetched once per 64 couts;
//  * the patch comes in through LDS-DMA (buffer_load_dwordx4 ... lds) issued by the compute waves themselves: 47 pieces
//    of 1 KiB per 32-channel chunk, 12 per wave, no VGPR stop-over, no ds_write; halo pixels outside the map and the pad
//    slots are lanes whose offset is forced out of the descriptor's range (they land as zeros);
//  * the chunk barrier sits one step EARLY: at the start of a chunk's last step every wave has finished reading the
//    chunk's buffer (window reads run one step ahead of the MFMAs) and chunk k+1 has long landed, so the last step
//    reads and transforms the first window of chunk k+1 (or of the next item) while its own MFMAs run - no prologue -
//    and the DMA of chunk k+2 goes out behind that barrier with a whole chunk to arrive;
//  * patch layout [row 10][group 9][pixel 4][quad 8] with one pad quad per 4-pixel group (group stride 33 quads = 1
//    mod 16) and a row stride of 300 quads (two rows = 8 mod 16): the 16 lanes a ds_read_b128 serves per LDS cycle
//    (8 block columns x 2 block rows) hit 16 different bank quads.  conv_wino24_kernel's [pixel][36 floats] layout puts
//    the lanes' 4-pixel stride on 4 bank quads: a 4-way conflict on every window read;
//  * exchange for the y-fold as in conv_wino24_kernel, two rounds, but round A carries the EVEN output columns (both
//    are sums: o0 = m0 + s12 + s34, o2 = s12 + 4 s34) and round B the odd ones (differences), so nothing is held in
//    registers across a round; parked tiles are [32 slots][32 couts] without padding, 16-byte columns XOR-swizzled by
//    slot & 7 (conflict free for the writer's 8-lane and the reader's 16-lane groups).
// LDS: 2 x 48,128 B patches + 4 waves x 4 tiles x 4 KiB = 161,792 B.
//
// Takes: 3x3 stride 1, Cin % 32 == 0, Cout % 32 == 0, exactly tiled maps (8x32- or 16x16-pixel items), 16-byte aligned channel
// slices; tensors of any size (the descriptor starts at the item's patch, offsets are patch-relative).  Results are those of
// conv_wino24_kernel (same products, same order).

// One LDS-DMA piece: 64 lanes x 16 bytes, lane l from rsrc + voff(l) + soff to dst + 16 l.  (A plain function, not spelled
// inside the kernel template: with a template-dependent address expression hipcc's HOST pass silently drops the whole
// kernel instantiation - no diagnostic, the kernel handle just stays an undefined symbol in the .so.)
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t rsrc, float* dst, int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)dst, 16, voff, soff, 0, 0);
}

// TW = 32: items of 8 x 32 pixels (4 x 8 blocks); TW = 16: items of 16 x 16 pixels (8 x 4 blocks) for the maps narrower
// than 32 pixels (HRNet branch 3: 256 -> 256 at 16 x 16, one item per frame and n-block).  Same 32 slots, same exchange;
// what changes is the slot -> pixel map, the patch (18 rows of 5 groups, row stride 170 quads = 2 mod 8: a ds_read_b128's
// 16 lanes are then 4 block columns x 4 block rows on 16 different bank quads) and the store addresses.
// ONE: every item is a single 32-channel chunk (Cin = 32) - its own instantiation, so that the chunk body with both the
// zero-initialising first step and the epilogue does not cost the multi-chunk kernels registers (with one kernel for both
// hipcc spilled 6 VGPRs and 41 more SGPRs).
// timing ablations (tools/exp_build.sh -DACRMI_W24_ABLATE=bits; WRONG results): 1 = no input-transform VALU, 2 = no weight
// loads in the steps, 4 = no LDS-DMA pieces, 8 = no window reads, 16 = no global stores, 32 = no parking writes, 64 = no
// bias / residual requests, 128 = the epilogue's y-fold reads no parked tiles
#ifndef ACRMI_W24_ABLATE
#define ACRMI_W24_ABLATE 0
#endif
//
// GROUP (conv_wino24b_group_kernel): one launch walks the items of TWO independent problems of this instantiation, problem 0's
// [0, total0) then problem 1's [total0, total0 + total1), dealt to the workgroups like one problem's.  Everything the body reads
// from a problem is wave-uniform and belongs to one of three cursors, each with the index of its problem:
//   ix_d  the DMA cursor (input map; enters the next problem up to two chunks ahead of the MFMAs: dma_begin_scalar),
//   ix_c  the weights and the chunk count (switches in the epilogue of problem 0's last item, in front of the next item's
//         first fragments),
//   ix_e  the epilogue (output, residual, bias; switches behind that item's last store).
// A switch is scalar loads and moves, plus once per launch the per-lane offsets that hold a map width (doff, lane_out,
// lane_res); the steps between two switches are those of the ungrouped kernel, and so is every sum.  The workgroups never
// wait for each other: the two problems are independent by construction (csrc/group_plan.h).
// Registers of the <2, 32> group form: 256 VGPRs + 201 AGPRs, no scratch (ungrouped: 240 + 192) - nine values are parked in
// AGPRs; measured per chunk and per epilogue it runs at the ungrouped kernel's pace (profiles/group_launch_ab.txt, stamps).
template <int NT, int TW, bool ONE, bool GROUP>
__device__ __forceinline__ void wino24b_body(const ConvArgs* ga, const ConvWork* gw) {
  const ConvArgs& a = ga[0];      // the launch-wide fields (tuning state) and, ungrouped, the problem
  const ConvWork& wk = gw[0];

  constexpr int CK = 32, TH = TW == 32 ? 8 : 16, PH = TH + 2, PWP = TW + 2;
  constexpr int W24_ABLATE = ACRMI_W24_ABLATE;
  constexpr int RS = TW == 32 ? 300 : 170, GQ = 33;   // quads (16 bytes) per patch row / per group of 4 pixels
  constexpr int BCOLS = TW / 4;                    // block columns of an item (8 / 4); slot = block row * BCOLS + block column
  constexpr int NPIECE = (PH * RS + 63) / 64;      // 47 / 48 DMA pieces of 64 quads
  constexpr int NI = (NPIECE + 3) / 4;             // 12 per wave
  constexpr int BUF = NPIECE * 64 * 4;             // floats per patch buffer
  constexpr int PTILE = 32 * 32;                   // parked tile [32 slots][32 couts]
  constexpr int PART_W = 2 * NT * PTILE;           // floats one wave parks per round: [column of the round][nt]
  extern __shared__ f32x4 smem4[];
  float* lds = reinterpret_cast<float*>(smem4);
  float* part = lds + 2 * BUF;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int vb = virtual_block(a);
  // GROUP: the cursors' problems (0 / 1).  A cursor reads its problem's fields from the kernel arguments where it needs them
  // - once per item, next to scalar work that is there anyway - and not from registers held across the steps: the frame has
  // no scalar register to spare, and a copy of both problems would live in VGPR lanes (v_readlane in every step).  What the
  // STEPS read (cin8_c, cin_d, tap_b, step_b, the descriptors) is kept in variables that a switch renews.
  // A workgroup whose first item lies in problem 1 starts there.
  const int total0 = wk.total;
  int ix_d = (GROUP && vb >= total0) ? 1 : 0, ix_c = ix_d, ix_e = ix_d;
  auto AD = [&]() -> const ConvArgs& { return ga[GROUP ? ix_d : 0]; };
  auto AC = [&]() -> const ConvArgs& { return ga[GROUP ? ix_c : 0]; };
  auto AE = [&]() -> const ConvArgs& { return ga[GROUP ? ix_e : 0]; };
  auto WD = [&]() -> const ConvWork& { return gw[GROUP ? ix_d : 0]; };
  auto WC = [&]() -> const ConvWork& { return gw[GROUP ? ix_c : 0]; };
  auto WE = [&]() -> const ConvWork& { return gw[GROUP ? ix_e : 0]; };
  auto base = [&](int ix) -> int { return (GROUP && ix) ? total0 : 0; };      // first item of the cursor's problem
  bool doff_stale = false;                         // the DMA cursor changed problem: dma_begin_vector renews doff
  int nchunks = AC().Cin / CK;                       // >= 1 (GROUP: of the problem the MFMAs are in)
  int cin8_c = AC().cin8, cin_d = AD().Cin;
  const int total = GROUP ? total0 + gw[GROUP ? 1 : 0].total : total0;
  const int my_items = total > vb ? (total - 1 - vb) / (int)gridDim.x + 1 : 0;
  int ktotal = my_items * nchunks;
  if constexpr (GROUP) {
    const int items0 = total0 > vb ? (total0 - 1 - vb) / (int)gridDim.x + 1 : 0;
    ktotal = items0 * (ga[0].Cin / CK) + (my_items - items0) * (ga[1].Cin / CK);
  }
  const int py = wave;
  const int li = lane & 31, lh = lane >> 5;
  const int ra = py == 0 ? 0 : (py == 2 ? 2 : 1);
  const int rb = py == 2 ? 1 : (py == 3 ? 3 : 2);
  const float sgn = py == 1 ? 1.f : -1.f;
  // window origin of the lane's slot (block row li / BCOLS, block column li % BCOLS), floats
  const int worg = ((2 * (li / BCOLS)) * RS + (li % BCOLS) * GQ) * 4 + 4 * lh;
  const int woff_a = worg + ra * RS * 4, woff_b = worg + rb * RS * 4;
  // store side: wave (oy, oh) writes output row parity oy and output column 2 oh (round A) / 2 oh + 1 (round B) of every
  // 2x4 block; lane = (block column p8, cout quad q8), four block rows gq per lane
  const int oy = wave >> 1, oh = wave & 1;
  const int p8 = lane >> 3, q8 = lane & 7;
  // (reader slot 8 gq + p8 = block row (8 gq + p8) / BCOLS, block column p8 % BCOLS)
  int lane_pix = (2 * (p8 / BCOLS) + oy) * AE().Wo + 4 * (p8 % BCOLS) + 2 * oh;
  int lane_out = lane_pix * AE().out_cs + 4 * q8, lane_res = lane_pix * AE().res_cs + 4 * q8;
  int gs_out = (16 / BCOLS) * AE().Wo * AE().out_cs, gs_res = (16 / BCOLS) * AE().Wo * AE().res_cs;   // gq + 1 = 8 slots on = 2 / 4 pixel rows
  const float ysign = oy ? -1.f : 1.f;
  bool has_res = AE().res != nullptr;
  float floor_ = AE().relu ? 0.f : -__builtin_inff();
  f32x16 acc[6][NT];

  // ---- weights: as conv_wino24_kernel, NT n-tiles per position
  int tap_b = cin8_c * AC().n_tiles * 1024, step_b = AC().n_tiles * 1024;
  __amdgpu_buffer_rsrc_t wrsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(AC().w), 0, AC().groups * 24 * tap_b, 0x00020000);
  const unsigned wlane = lane * 16;
  auto wbase = [&](int w_item) -> int {
    const ItemPos ip = item_pos(WC(), w_item - base(ix_c));
    return (ip.g * 24 + py * 6) * tap_b + ip.rest * NT * 1024;
  };
  f32x4 d[2][6], v[6], bq[6][NT];
  auto load_frag = [&](int p, int base, int step) {
    const int so = base + p * tap_b + (step < cin8_c ? step : cin8_c - 1) * step_b;
#pragma unroll
    for (int n = 0; n < NT; ++n)
      bq[p][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane, so + n * 1024, 0));
  };
  // window column c of the slot: pixel 4 bc + c (bc = the slot's block column) -> group bc + (c >> 2), pixel c & 3 of it
  auto read_rows = [&](const float* patch, int s) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const int cq = ((c >> 2) * GQ + (c & 3) * 8) * 4;
      d[0][c] = *reinterpret_cast<const f32x4*>(patch + woff_a + cq + s * 8);
      d[1][c] = *reinterpret_cast<const f32x4*>(patch + woff_b + cq + s * 8);
    }
  };
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const float one = a.ks == 3 ? 1.f : 2.f;   // always 1 (a runtime value: nothing is folded back into scalar ops)
  f32x2 sgnp = {sgn * one, sgn * one}, m1p = {-one, -one}, p4p = {4.f * one, 4.f * one}, m4p = {-4.f * one, -4.f * one},
        m5p = {-5.f * one, -5.f * one}, p2p = {2.f * one, 2.f * one}, m2p = {-2.f * one, -2.f * one};
  f32x2 ysignp = {ysign * one, ysign * one};
  asm volatile("" : "+v"(sgnp), "+v"(m1p), "+v"(p4p), "+v"(m4p), "+v"(m5p), "+v"(p2p), "+v"(m2p), "+v"(ysignp));
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

  // ---- LDS-DMA: piece jj[i] = 64 consecutive quads of the patch buffer, lane l its quad 64 jj[i] + l
  int jj[NI];           // (uniform) piece index; the 48th slot repeats piece 46 (same data to the same place)
  int doff[NI];         // source byte offset of the lane's quad relative to the patch origin pixel, first channel of a chunk
  unsigned dhb[NI / 4]; // 8 bits per piece: 1 top / 2 bottom / 4 left / 8 right ring of the patch, 16 = slot never fetched
  int eff[NI];          // doff, or out of range where the item's tile touches the map border
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
    doff[i] = ((row * AD().W + pix) * AD().in_cs + 4 * (q & 7)) * 4;
    const unsigned hb = (row == 0 ? 1u : 0u) | (row == PH - 1 ? 2u : 0u) | (pix == 0 ? 4u : 0u) | (pix == PWP - 1 ? 8u : 0u) |
                        (live ? 0u : 16u);
    dhb[i >> 2] |= hb << (8 * (i & 3));
    eff[i] = (int)0x80000000;
  }
  int tiles_y = WD().tiles_per_frame / WD().tiles_x;
  __amdgpu_buffer_rsrc_t drsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(AD().in), 0, 0, 0x00020000);
  int wd = vb, cd0 = 0, kd = 0;     // DMA cursor: item, first channel and index of the next chunk to request
  // The cursor enters an item (cd0 == 0, uniform): descriptor at its patch origin, halo lanes.  In two halves since round 6:
  // the SCALAR half (item position by multiply-shift division, the 64-bit origin, the descriptor: ~100 dependent scalar
  // instructions) runs in the step BEFORE the bridge, the VECTOR half (3 VALU per piece) behind that step's fourth MFMA group
  // as one burst.  Measured (profiles/r06_wino24b_ablation_mainloop.txt + r06_wino24b_hoists.txt): at the head of the bridge
  // step the two cost ~750 cycles of an idle matrix pipe per item; moved, the bridge step lost 710 and the step before it
  // gained 640 - hipcc keeps the chain as ONE clump of scalar instructions between two MFMAs (a dependent scalar chain is
  // issue time like anything else; only independent scalar instructions ride along for free), and forcing it apart with
  // sched_group_barrier / a branch-free form was slower (it recomputes per chunk).  Net of this and prep_last: -0.5 % per item.
  unsigned dma_edge = 0;
  auto dma_begin_scalar = [&]() {
    if (cd0 == 0) {
      const bool valid = kd < ktotal;
      if constexpr (GROUP) {
        if (valid && ix_d == 0 && wd >= total0) {   // the cursor's first item of problem 1
          ix_d = 1;
          tiles_y = WD().tiles_per_frame / WD().tiles_x;
          cin_d = AD().Cin;
          doff_stale = true;
        }
      }
      const ItemPos ip = item_pos(WD(), (valid ? wd : vb) - base(ix_d));
      dma_edge = (ip.ty == 0 ? 1u : 0u) | (ip.ty == tiles_y - 1 ? 2u : 0u) | (ip.tx == 0 ? 4u : 0u) |
                 (ip.tx == WD().tiles_x - 1 ? 8u : 0u) | 16u;
      const long long org = (((long long)ip.b * AD().H + (ip.ty * TH - 1)) * AD().W + (ip.tx * TW - 1)) * (long long)AD().in_cs +
                            AD().in_coff + ip.g * AD().Cin;
      // past the last item: zero records, every lane out of range (the pieces then write zeros into a buffer nobody reads)
      drsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(AD().in + org), 0, valid ? 0x7ffffff0 : 0, 0x00020000);
    }
  };
  auto dma_begin_vector = [&]() {
    if (cd0 == 0) {
      if constexpr (GROUP) {
        if (doff_stale) {      // (uniform; once per launch) the lanes' source offsets on problem 1's map
          doff_stale = false;
#pragma unroll
          for (int i = 0; i < NI; ++i) {
            const int f = jj[i] * 64 + lane;
            const int row = f / RS, rem = f - row * RS;
            const int grp = rem / GQ, q = rem - grp * GQ;
            doff[i] = ((row * AD().W + grp * 4 + (q >> 3)) * AD().in_cs + 4 * (q & 7)) * 4;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < NI; ++i)
        eff[i] = ((dhb[i >> 2] >> (8 * (i & 3))) & dma_edge) ? (int)0x80000000 : doff[i];
    }
  };
  auto dma_begin = [&]() {
    dma_begin_scalar();
    dma_begin_vector();
  };
  auto dma_piece = [&](int i, int bsel) {
    lds_dma16(drsrc, lds + bsel * BUF + jj[i] * 256, eff[i], cd0 * 4);
  };
  auto dma_end = [&]() {
    cd0 += CK;
    if (cd0 >= cin_d) { cd0 = 0; wd += (int)gridDim.x; }
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
  for (int p = 0; p < 6; ++p) load_frag(p, wsc, 0);
  __syncthreads();
  read_rows(lds, 0);
  {
    f32x4 t[6];
    row_op(t);
    col_a(t);
    col_b(t);
    col_c(t);
  }

  auto chunk = [&](auto first_tag, auto last_tag) {
    constexpr bool FIRST = decltype(first_tag)::value, LAST = decltype(last_tag)::value;
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    const float* patch = lds + (k & 1) * BUF;
    const float* patch_n = lds + ((k + 1) & 1) * BUF;
    const int nw = LAST ? w + (int)gridDim.x : w;
    const bool more = k + 1 < ktotal;
    // the next item's weights (GROUP: named in the epilogue, behind the switch of ac - the steps below still read this item's)
    int wsn = (!GROUP && LAST && more) ? wbase(nw) : wsc;
    int rest = 0;
    float* out_tile = nullptr;
    f32x4 rv[NT][4], bv[NT];
    __amdgpu_buffer_rsrc_t rrsrc = wrsrc, brsrc = wrsrc;
    // what the item's epilogue needs (all scalar: item position, output tile, residual / bias descriptors).  Round 6: runs
    // inside the LAST chunk's second step, interleaved with its MFMAs - at the top of the chunk its ~500 cycles of dependent
    // scalar arithmetic ran with the matrix pipe idle (profiles/r06_wino24b_ablation_epilogue.txt: 696 vs 200 cycles)
    auto prep_last = [&]() {
      const ItemPos ip = item_pos(WE(), w - base(ix_e));
      const int g = ip.g, b = ip.b;
      rest = ip.rest;
      const float* bias = AE().bias + (size_t)g * AE().n_tiles * 32 + (size_t)b * AE().bias_fstride;
      const int tile_pix = ip.ty * TH * AE().Wo + ip.tx * TW;
      out_tile = AE().out + (size_t)b * AE().Ho * AE().Wo * AE().out_cs + AE().out_coff + g * AE().Cout + (size_t)tile_pix * AE().out_cs;
      const size_t res_off = (res_frame_off(AE(), b) + (size_t)tile_pix * AE().res_cs) + AE().res_coff + g * AE().Cout;
      const size_t res_left = has_res ? (res_total(AE()) - res_off) * 4 : 0;
      rrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(has_res ? AE().res + res_off : AE().in), 0,
                                                (int)(unsigned)(res_left > 0xffffffffu ? 0xffffffffu : res_left), 0x00020000);
      brsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bias), 0, bias_row_left(AE(), g), 0x00020000);
    };
    // residual of one round (column offset oc pixels) and the bias: unconditional raw buffer loads (zero records: 0)
    auto request_res = [&](int oc) {
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
          rv[n][gq] = __builtin_bit_cast(
              f32x4, __builtin_amdgcn_raw_buffer_load_b128(rrsrc, (lane_res + oc * AE().res_cs) * 4,
                                                           ((rest * NT + n) * 32 + gq * gs_res) * 4, RES_CACHE_WINO));
    };
    auto request_bias = [&]() {
#pragma unroll
      for (int n = 0; n < NT; ++n)
        bv[n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(brsrc, 16 * q8, (rest * NT + n) * 128, 0));
    };
    // One 8-channel step: 6 groups of 4 NT MFMAs.  Behind group 0 the window rows of the NEXT step are requested (rows of
    // step rs in rp), row-combined with group 2; behind its group's MFMAs each fragment is replaced by the next step's
    // (activations: B4^T pieces behind groups 2, 4 and 5; weights: buffer loads from wb at 8-channel step ws).
    // BRIDGE = a chunk's last step: the chunk barrier comes first (see the file comment), the window is the first one of
    // the next chunk in the other buffer, and the pieces of the chunk after that go out, two per group.
    // TAIL = an item's last step (a BRIDGE whose weights are the next item's).
    // HOOK: scalar work hidden under this step's MFMAs - 1 = the epilogue's scalars (prep_last), 2 = the DMA cursor's next
    // item (dma_begin_scalar, its vector half behind the same MFMA group)
    auto step = [&](auto zero_tag, auto bridge_tag, auto tail_tag, auto hook_tag, const float* rp, int rs, int wb, int ws) {
      constexpr bool ZERO = decltype(zero_tag)::value, BRIDGE = decltype(bridge_tag)::value, TAIL = decltype(tail_tag)::value;
      constexpr int HOOK = decltype(hook_tag)::value;
      (void)BRIDGE;
      f32x4 t[6];
#ifdef ACRMI_W24_STEPSTAMPS
      if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
#endif
      if (BRIDGE) __syncthreads();
#pragma unroll
      for (int px = 0; px < 6; ++px) {
        __builtin_amdgcn_sched_barrier(0);
        if (HOOK == 1 && px == 1) prep_last();
        if (HOOK == 2 && px == 3) dma_begin_scalar();
        if (px == 0 && !(W24_ABLATE & 8)) read_rows(rp, rs);
        if (px == 2 && !(W24_ABLATE & 1)) row_op(t);
        if (BRIDGE && !(W24_ABLATE & 4)) {
          dma_piece(2 * px, k & 1);
          dma_piece(2 * px + 1, k & 1);
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
        __builtin_amdgcn_sched_barrier(0);
        if (HOOK == 2 && px == 3) dma_begin_vector();
        if (!(W24_ABLATE & 1)) {
          if (px == 2) col_a(t);      // v0..v2: their MFMAs have been issued
          if (px == 4) col_b(t);      // v3, v4
          if (px == 5) col_c(t);      // v5
        }
        // (TAIL: the next item's first weight fragments go out from the epilogue - 48 registers it needs for the x-fold)
        if (!TAIL && !(W24_ABLATE & 2)) load_frag(px, wb, ws);
      }
      if (BRIDGE) dma_end();
    };
    const int s0 = c0 / 8;
    typedef std::integral_constant<int, 0> H0;
    typedef std::integral_constant<int, LAST ? 1 : 0> H1;
    typedef std::integral_constant<int, 2> H2;
    if (FIRST) step(std::true_type(), std::false_type(), std::false_type(), H0(), patch, 1, wsc, s0 + 1);
    else step(std::false_type(), std::false_type(), std::false_type(), H0(), patch, 1, wsc, s0 + 1);
    step(std::false_type(), std::false_type(), std::false_type(), H1(), patch, 2, wsc, s0 + 2);
    step(std::false_type(), std::false_type(), std::false_type(), H2(), patch, 3, wsc, s0 + 3);
    if (LAST) step(std::false_type(), std::true_type(), std::true_type(), H0(), patch_n, 0, wsn, 0);
    else step(std::false_type(), std::true_type(), std::false_type(), H0(), patch_n, 0, wsc, s0 + 4);
    __builtin_amdgcn_sched_barrier(0);
    if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
    bool to1 = false;      // GROUP: this item is the workgroup's last of problem 0 and one of problem 1 follows
    if constexpr (GROUP && LAST) to1 = more && ix_c == 0 && nw >= total0;

    // ---- item epilogue: x-fold with A4^T in registers (even output columns from the sums, odd ones from the
    // differences), y-fold across the waves through LDS in two rounds
    if (LAST) {
      // x-fold and park in halves of 8 accumulator registers (couts 16 h .. 16 h + 15 of the tile): the accumulators live
      // in AGPRs and every operand of the fold is first copied to a VGPR - on whole tiles the copies of one n-tile (80
      // registers) next to the next item's fragments and the residual pushed loop constants out to scratch, and their
      // reloads (12 x scratch_load + vmcnt(0)) cost the first chunk of every item ~6k cycles
      typedef float f32x8 __attribute__((ext_vector_type(8)));
      // (spelled as v_accvgpr_read_b32: left to itself hipcc copies all twelve accumulator tiles to VGPRs at the top of
      //  the epilogue - 192 registers)
      auto half = [](const f32x16& x, int h) -> f32x8 {
        f32x8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float t;
          asm("v_accvgpr_read_b32 %0, %1" : "=v"(t) : "a"(x[8 * h + e]));   // (not volatile: hipcc interleaves the 40 reads
                                                                           //  of a group with its arithmetic)
          r[e] = t;
        }
        return r;
      };
      // packed arithmetic on 8 registers (4 x v_pk_*): x +- y as 1 * x + (+-1) * y, c * x + y with c = 2, 4, 8 (exact
      // products: the results are those of conv_wino24_kernel's plain multiply + add)
      f32x2 p8p = {8.f * one, 8.f * one};
      asm volatile("" : "+v"(p8p));
      auto pk_add8 = [](const f32x8& b, const f32x8& c) -> f32x8 {
        f32x8 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          f32x2 o;
          const f32x2 b2 = {b[2 * e], b[2 * e + 1]}, c2 = {c[2 * e], c[2 * e + 1]};
          asm("v_pk_add_f32 %0, %1, %2" : "=v"(o) : "v"(b2), "v"(c2));
          r[2 * e] = o[0];
          r[2 * e + 1] = o[1];
        }
        return r;
      };
      auto pk_fma8 = [](f32x2 m, const f32x8& b, const f32x8& c) -> f32x8 {   // m * b + c
        f32x8 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          f32x2 o;
          const f32x2 b2 = {b[2 * e], b[2 * e + 1]}, c2 = {c[2 * e], c[2 * e + 1]};
          asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(o) : "v"(m), "v"(b2), "v"(c2));
          r[2 * e] = o[0];
          r[2 * e + 1] = o[1];
        }
        return r;
      };
      auto park8 = [&](int t2, int n, int h, const f32x8& o) {
        float* pw = part + wave * PART_W + (t2 * NT + n) * PTILE + li * 32;
        if (W24_ABLATE & 32) return;
#pragma unroll
        for (int q = 0; q < 2; ++q)
          *reinterpret_cast<f32x4*>(pw + 4 * ((2 * (2 * h + q) + lh) ^ (li & 7))) = f32x4{o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
      };
      // y-fold (oy = 0: R0+R1+R2, oy = 1: R1-R2-R3) of parked tile oh of the round, then bias, residual, ReLU, store;
      // oc = the round's column offset in pixels (0 / 1) on top of the wave's 2 oh
      auto fold_store = [&](int oc) {
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          const float* pr = part + (oh * NT + n) * PTILE + p8 * 32 + 4 * (q8 ^ p8);
          f32x4 y[4];
          {
            f32x4 pp[3][4];
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
#pragma unroll
              for (int j = 0; j < 3; ++j)
                if (W24_ABLATE & 128) pp[j][gq] = f32x4{one, one, one, one};
                else pp[j][gq] = *reinterpret_cast<const f32x4*>(pr + (oy + j) * PART_W + 8 * gq * 32);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) y[gq] = pk_fma4(ysignp, pk_add4(pp[1][gq], pp[2][gq]), pp[0][gq]);
          }
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) {
            // no branches: without a residual rv is 0 (zero-record descriptor), without ReLU the floor is -inf
            f32x4 o4 = pk_add4(pk_add4(y[gq], bv[n]), rv[n][gq]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {      // (one v_max_f32 per float: fmaxf canonicalises its operand first - two VALU per float)
              float r;
              asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(o4[e]), "v"(floor_));
              o4[e] = r;
            }
            char* ub = reinterpret_cast<char*>(out_tile + (rest * NT + n) * 32 + gq * gs_out + oc * AE().out_cs);   // uniform
            if (!(W24_ABLATE & 16)) __builtin_nontemporal_store(o4, reinterpret_cast<f32x4*>(ub + (unsigned)(lane_out * 4)));
            else asm volatile("" :: "v"(o4));
          }
        }
      };
      // round A's residual and the bias: the x-fold below (~400 VALU) covers their latency
      if (!(W24_ABLATE & 64)) {
        request_bias();
        request_res(0);
      } else {
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          bv[n] = f32x4{one, one, one, one};
#pragma unroll
          for (int gq = 0; gq < 4; ++gq) rv[n][gq] = f32x4{one, one, one, one};
        }
      }
      // (the asm reads below are invisible to hipcc's hazard recognizer: the last MFMA's 16 passes drain here)
      asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          __builtin_amdgcn_sched_barrier(0);
          const f32x8 s12 = pk_add8(half(acc[1][n], h), half(acc[2][n], h)), s34 = pk_add8(half(acc[3][n], h), half(acc[4][n], h));
          park8(0, n, h, pk_add8(pk_add8(half(acc[0][n], h), s12), s34));    // o0 = (m0 + s12) + s34
          park8(1, n, h, pk_fma8(p4p, s34, s12));                            // o2 = s12 + 4 s34
        }
      __builtin_amdgcn_sched_barrier(0);
      if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
      __syncthreads();                        // round A is parked
      if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
      fold_store(0);
      if (!(W24_ABLATE & 64)) request_res(1);   // round B's residual takes round A's registers
      __syncthreads();                        // every wave has read round A's tiles
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          __builtin_amdgcn_sched_barrier(0);
          const f32x8 d12 = pk_fma8(m1p, half(acc[2][n], h), half(acc[1][n], h)), d34 = pk_fma8(m1p, half(acc[4][n], h), half(acc[3][n], h));
          park8(0, n, h, pk_fma8(p2p, d34, d12));                                  // o1 = d12 + 2 d34
          park8(1, n, h, pk_add8(pk_fma8(p8p, d34, d12), half(acc[5][n], h)));     // o3 = (d12 + 8 d34) + m5
        }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (GROUP) {
        if (to1) {      // the weights' cursor enters problem 1 (scalar)
          ix_c = 1;
          nchunks = AC().Cin / CK;
          cin8_c = AC().cin8;
          tap_b = cin8_c * AC().n_tiles * 1024;
          step_b = AC().n_tiles * 1024;
          wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(AC().w), 0, AC().groups * 24 * tap_b, 0x00020000);
        }
        if (more) wsn = wbase(nw);
      }
#pragma unroll
      for (int p = 0; p < 6; ++p) load_frag(p, wsn, 0);   // the next item's first step: round B's fold covers their latency
      __syncthreads();                        // round B is parked
      fold_store(1);
      if (stamp && ns_ < 60) a.dbg[ns_++] = clock64();
      if constexpr (GROUP) {
        if (to1) {      // ... and the epilogue's: once per launch, the store and residual offsets of the lanes on problem 1's map
          ix_e = 1;
          lane_pix = (2 * (p8 / BCOLS) + oy) * AE().Wo + 4 * (p8 % BCOLS) + 2 * oh;
          lane_out = lane_pix * AE().out_cs + 4 * q8;
          lane_res = lane_pix * AE().res_cs + 4 * q8;
          gs_out = (16 / BCOLS) * AE().Wo * AE().out_cs;
          gs_res = (16 / BCOLS) * AE().Wo * AE().res_cs;
          has_res = AE().res != nullptr;
          floor_ = AE().relu ? 0.f : -__builtin_inff();
        }
      }
    }
    wsc = wsn;
    c0 = LAST ? 0 : c0 + CK;
    w = nw;
    ++k;
  };
  if constexpr (ONE) {     // Cin = 32: every item is one chunk - zero-initialising first step, bridge + epilogue behind it
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

template <int NT, int TW, bool ONE = false>
__global__ __launch_bounds__(256, 1) void conv_wino24b_kernel(const ConvArgs a, const ConvWork wk) {
  wino24b_body<NT, TW, ONE, false>(&a, &wk);
}
// two problems of the <NT, TW, false> instantiation in one launch (launch_conv_group)
template <int NT, int TW>
__global__ __launch_bounds__(256, 1) void conv_wino24b_group_kernel(const ConvGroup g) {
  wino24b_body<NT, TW, false, true>(g.a, g.wk);
}

// item width of conv_wino24b_kernel for the shapes it takes (conv_rules.h takes_wino24b), else 0: everything else stays on
// conv_wino24_kernel; ACRMI_WINO24B=0 / cfg 840 keep the old frame
static int wino24b_ok(const ConvArgs& a) {
  static const char* env = experiment_env("ACRMI_WINO24B");
  return ((env && atoi(env) == 0) || g_force_cfg == 840) ? 0 : takes_wino24b(conv_shape(a));
}

static constexpr int wino24b_th(int TW) { return TW == 32 ? 8 : 16; }
static constexpr size_t wino24b_lds(int NT, int TW) {      // two patches (row stride 300 / 170 floats) + the exchange area
  return (2 * (size_t)(((wino24b_th(TW) + 2) * (TW == 32 ? 300 : 170) + 63) / 64) * 64 * 4 + 4 * (size_t)2 * NT * 32 * 32) * sizeof(float);
}
static_assert(wino24b_lds(2, 32) <= 160 * 1024 && wino24b_lds(2, 16) <= 160 * 1024, "patches + exchange area must fit the 160 KiB LDS");
// (plain functions, not a template over NT / TW: referenced only from a function template, hipcc left the host-side handles
//  of the kernel instantiations undefined)
// the instantiation that takes `a` (tw = wino24b_ok(a)), with its n-tiles per wave and item width; false: none
struct Wino24bPick {
  ConvKernel k;
  int NT, TW;
};
static bool wino24b_pick(const ConvArgs& a, int tw, Wino24bPick& p) {
  const bool one = a.Cin == 32;
  if (a.Cout % 64 == 0) {
    if (tw == 16) {
      if (one) return false;
      p = Wino24bPick{CONV_KERNEL(conv_wino24b_kernel<2, 16>), 2, 16};
    } else if (one) {
      p = Wino24bPick{CONV_KERNEL(conv_wino24b_kernel<2, 32, true>), 2, 32};
    } else {      // HRNet branches 1 and 2 at large batches: the instantiation with a group form
      p = Wino24bPick{CONV_KERNEL_GROUPED((conv_wino24b_kernel<2, 32>), (conv_wino24b_group_kernel<2, 32>)), 2, 32};
    }
    return true;
  }
  p = one ? Wino24bPick{CONV_KERNEL(conv_wino24b_kernel<1, 32, true>), 1, 32} : Wino24bPick{CONV_KERNEL(conv_wino24b_kernel<1, 32>), 1, 32};
  return true;
}
static ConvProblem wino24b_problem(const ConvArgs& a, const Wino24bPick& p) {
  // (the packed weights pad Cout to whole 64-cout blocks: a.n_tiles may count a tile of zeros)
  return ConvProblem{a, a.Wo / p.TW, a.Ho / wino24b_th(p.TW), (a.Cout / 32) / p.NT};
}
static hipError_t launch_wino24b(const ConvArgs& a, int tw, hipStream_t s) {
  Wino24bPick p;
  if (!wino24b_pick(a, tw, p)) return hipErrorInvalidValue;
  const ConvProblem pr = wino24b_problem(a, p);
  return launch_conv_kernel(p.k, 256, wino24b_lds(p.NT, p.TW), &pr, 1, s);
}
// n problems that wino24b_pick sends to ONE instantiation with a group form, as one launch
static hipError_t launch_wino24b_group(const ConvArgs* a, const int* tw, int n, hipStream_t s) {
  Wino24bPick p0;
  ConvProblem pr[CONV_GROUP_MAX];
  if (n < 1 || n > CONV_GROUP_MAX || !wino24b_pick(a[0], tw[0], p0)) return hipErrorInvalidValue;
  for (int i = 0; i < n; ++i) {
    Wino24bPick p;
    if (!wino24b_pick(a[i], tw[i], p) || p.k.fn != p0.k.fn) return hipErrorInvalidValue;
    pr[i] = wino24b_problem(a[i], p);
  }
  return launch_conv_kernel(p0.k, 256, wino24b_lds(p0.NT, p0.TW), pr, n, s);
}
