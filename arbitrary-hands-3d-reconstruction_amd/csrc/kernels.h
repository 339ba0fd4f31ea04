// Internal launch interface between the C ABI (acrmi.hip) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

#include <stdlib.h>

#include "conv_rules.h"
#include "nv12_out_plan.h"
#include "smooth_plan.h"
#include "assoc_plan.h"
#include "point_plan.h"

namespace acrmi {

// Environment switches of timing experiments / A-B runs (lane-sync ablation, event flags, loader and kernel-frame A/B) exist
// only in a library built with -DACRMI_EXPERIMENTS (`python -m <package>.build --experiments`); the production library does
// not read them.  Diagnostics (ACRMI_DEBUG*) and configuration (ACRMI_RCCL_LIB) are plain getenv.
inline const char* experiment_env(const char* name) {
#ifdef ACRMI_EXPERIMENTS
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

struct ConvArgs {
  const float* in;
  const float* w;      // packed [group][tap][cin8][ntile][lane64][4]
  const float* bias;   // [group][coutP] or per frame
  const float* res;    // may be null
  float* out;
  int B, H, W, Ho, Wo;
  int in_cs, in_coff, Cin;
  int out_cs, out_coff, Cout;
  int res_cs, res_coff;
  int ks, stride, relu, groups;
  int n_tiles;          // 32-cout tiles per group in the packed weights (CoutP/32)
  int cin8;             // ceil(Cin/8)
  int bias_fstride;     // floats between frames' bias rows (0 = shared)
  int algo;             // 0 direct, 1..7 the other kernels: which shapes each takes, its taps and the size of its packed
                        // weights are stated in conv_rules.h (conv_algo_reject, conv_taps, conv_weight_floats)
  long long* dbg;       // optional device buffer for cycle stamps (tuning only)
  int phase_delay;      // tuning switches of the loader waves (acrmi_tune key 3): 8 = idle loader (timing ablation, wrong
                        // results), 9 = loader at priority 0; 0 = off
  int xcd_swizzle;      // 1: work items are dealt to the XCDs in contiguous bands (see virtual_block, conv_mfma.hip)
  const float* zeros;   // >= 16 bytes of device zeros (source of halo / pad-channel lanes of conv_wino3's LDS-DMA loader)
  // Storage type of the activations (ACRMI_DT_*).  F16 / BF16: in, w (and out / res unless out_f32) point at 16-bit
  // data, channel strides / offsets / counts are in elements of their tensor, cin8 = ceil(Cin / 16), the weights are
  // packer.pack_conv_h16 fragments and algo must be 0 (conv_h16.hip).
  int dtype;
  int out_f32;          // 16-bit input, fp32 output and fp32 residual (the head exits)
  int res_bcast;        // 1: res is ONE [Ho][Wo][res_cs] map added to every frame (not conv_wino3 / the 16-bit kernels)
  // Split-K (algo 2, small batches; conv_wino2.inc SPLIT): groups = K-slices of one convolution (slice s reads input
  // channels [s*Cin, (s+1)*Cin), all slices produce the same Cout channels).  split_ws: conv_splitk_ws_floats() floats,
  // split_cnt: conv_splitk_counters() zeroed unsigned, both private to the launches of one stream.
  int in_sub;           // 2: the loader reads every other input row / column (a 1x1 stride-2 convolution runs as the 1x1
                        // stride-1 kernel on the subsampled map; H, W stay the input's, Ho, Wo the output's); 0 / 1: dense
  int splitk;
  float* split_ws;
  unsigned* split_cnt;
  // Extra residual terms (the HR-module fuse, acr/model.py:672-686, folded into the epilogue of the downsampling chain's
  // last convolution): out = [relu]((conv + bias + res) + up(xt[0]) + up(xt[1]) + up(xt[2])), summed in this order; term t
  // is a [B][Ho >> shift][Wo >> shift][xt_cs] map read at pixel (y >> shift, x >> shift) = nearest-neighbour upsampling,
  // channels [xt_coff, xt_coff + groups * Cout).  3x3 stride-2 convolutions only (conv_pp2_kernel<1, true> / <2, true>, the 32-cout
  // conv_ws2_kernel), Cout % 32 == 0, 16-byte aligned channel slices.
  int nxt;
  const float* xt[3];
  int xt_cs[3], xt_coff[3], xt_shift[3];
  // ACRMI_CONV_DUAL (conv_wino3_kernel with store waves only): `out` stays the convolution's own output (bias, residual, ReLU);
  // the xt terms are NOT added to it but to a SECOND output, out2 = relu(((out + up(xt[0])) + up(xt[1])) + up(xt[2])) - the
  // full-resolution HR fuse sum, whose first term (branch 0's last conv2) is also read by the downsampling chains
  float* out2;
  int out2_cs, out2_coff;
  unsigned* range_flag;   // conv_x3 / conv_x3p with f16 halves: set to 1 when an activation beyond the f16 range was split
                          // (null: not tracked - the stand-alone operator calls)
};
// The derived fields (Ho, Wo, cin8, n_tiles) from the primary ones (H, W, ks, stride, Cin, Cout, dtype): every ConvArgs is
// completed here.
inline void conv_derive(ConvArgs& a) {
  a.Ho = conv_out_size(a.H, a.ks, a.stride);
  a.Wo = conv_out_size(a.W, a.ks, a.stride);
  a.cin8 = conv_ksteps(a.Cin, a.dtype);
  a.n_tiles = conv_n_tiles(a.Cout);
}
// workspace of a split-K launch: (8x16-pixel tiles) x (32-cout blocks) groups of `splits` partial tiles of 4096 floats
inline size_t conv_splitk_groups(int B, int Ho, int Wo, int cout) {
  return (size_t)B * ((Ho + 7) / 8) * ((Wo + 15) / 16) * conv_n_tiles(cout);
}
inline size_t conv_splitk_ws_floats(int B, int Ho, int Wo, int cout, int splits) { return conv_splitk_groups(B, Ho, Wo, cout) * splits * 4096; }
inline size_t conv_splitk_counters(int B, int Ho, int Wo, int cout) { return conv_splitk_groups(B, Ho, Wo, cout) * 4; }

// one-time per-DEVICE kernel setup (dynamic LDS attribute): true the first time `flags` (one static array per kernel
// instantiation) is asked about the current device
constexpr int MAX_DEVICES = 64;
bool first_use_on_device(unsigned char* flags);
// held by a launcher from the first_use_on_device() test until the attribute is set (and by launch_conv throughout)
std::recursive_mutex& launch_mutex();

// returns hipSuccess or the launch error; cout tiles etc. derived inside
hipError_t launch_conv(ConvArgs a, hipStream_t s);
hipError_t launch_conv_h16(ConvArgs a, hipStream_t s);   // called by launch_conv when a.dtype != ACRMI_DT_F32
// Two INDEPENDENT convolutions that launch_conv routes to one kernel instantiation with a group form (conv_frame.h ConvGroup;
// today conv_wino24b_kernel<2, 32>) as ONE launch: the second's work items follow the first's inside the persistent
// workgroups, so its start-up and one launch boundary are not paid.  Each output is bit-identical to its own launch's.
// conv_can_group asks the routing; launch_conv_group with n = 1 is launch_conv, with a pair that cannot share a launch an error.
bool conv_can_group(const ConvArgs& a, const ConvArgs& b);
hipError_t launch_conv_group(const ConvArgs* a, int n, hipStream_t s);
const char* conv_kernel_name(const ConvArgs& a);
void conv_force_cfg(int cfg);
void conv_set_debug(long long* dbg);
void conv_set_phase_delay(int cycles);
void conv_set_xcd_swizzle(int on);

hipError_t launch_u8norm(const uint8_t* img, long n_pixels, float* out, hipStream_t s);
// stem.hip: uint8 RGB [B,H,W,3] -> relu(conv3x3 s2 (x/255*2-1) + b) [B,H/2,W/2,64 of out_cs]; wpk = packer.pack_stem
bool stem_shape_ok(int H, int W, int out_cs, int out_coff);
hipError_t launch_stem(const uint8_t* img, int B, int H, int W, const float* wpk, const float* bias, float* out,
                       int out_cs, int out_coff, int relu, hipStream_t s);
// the same with the output rounded to f16 / bf16 (out_cs / out_coff in elements, multiples of 8)
// layer1's conv3 (64 -> 256, + residual, ReLU) chained with the next block's conv1 (256 -> 64, ReLU) in one kernel
// (csrc/pair1x1.hip); wpk = packer.pack_pair1x1 (33088 floats); npix = B * H * W
hipError_t launch_pair1x1(const float* t2, int t2_cs, int t2_coff, const float* x, int x_cs, int x_coff, float* y, int y_cs,
                          int y_coff, float* t, int t_cs, int t_coff, const float* wpk, long npix, hipStream_t s);
constexpr long PAIR1X1_FLOATS = 256 * 64 + 64 * 256 + 256 + 64;
// ResNet stem (7x7 stride 2 pad 3, csrc/stem7.hip): wpk = packer.pack_stem7 fragments [74][2][64]
bool stem7_shape_ok(int H, int W, int out_cs, int out_coff);
hipError_t launch_stem7(const uint8_t* img, int B, int H, int W, const float* wpk, const float* bias, float* out,
                        int out_cs, int out_coff, int relu, hipStream_t s);
hipError_t launch_stem7_h16(const uint8_t* img, int B, int H, int W, const float* wpk, const float* bias, void* out,
                            int out_cs, int out_coff, int relu, int dtype, hipStream_t s);
hipError_t launch_stem_h16(const uint8_t* img, int B, int H, int W, const float* wpk, const float* bias, void* out,
                           int out_cs, int out_coff, int relu, int dtype, hipStream_t s);
hipError_t launch_bilinear2x(const float* in, int B, int H, int W, int in_cs, int in_coff, int C, float* out,
                             int out_cs, int out_coff, hipStream_t s);
struct FuseArgs {
  const float* term[4];
  int cs[4], shift[4];
  int nterms, B, H, W, C, out_cs, relu;
  float* out;
};
hipError_t launch_fuse_sum(const FuseArgs& a, hipStream_t s);
// One axis of OpenCV's uint8 INTER_CUBIC (csrc/preprocess.hip states the rule): destination index d -> source origin s0 and
// the four 11-bit fixed-point coefficients.
__device__ inline void cv_cubic_taps(int d, double scale, int& s0, int (&c)[4]) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  const float fl = floorf(f);
  s0 = (int)fl;
  f -= fl;
  const float A = -0.75f;
  float k[4];
  k[0] = ((A * (f + 1.f) - 5.f * A) * (f + 1.f) + 8.f * A) * (f + 1.f) - 4.f * A;
  k[1] = ((A + 2.f) * f - (A + 3.f)) * f * f + 1.f;
  k[2] = ((A + 2.f) * (1.f - f) - (A + 3.f)) * (1.f - f) * (1.f - f) + 1.f;
  k[3] = 1.f - k[0] - k[1] - k[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int v = (int)rintf(k[i] * 2048.f);            // saturate_cast<short>(float): cvRound, then clamp
    c[i] = v < -32768 ? -32768 : (v > 32767 ? 32767 : v);
  }
}
// n BGR frames of one size H x W in one allocation (csrc/preprocess.hip; acrmi_preprocess)
hipError_t launch_preprocess(const uint8_t* bgr, int n, int H, int W, int out_size, uint8_t* out, hipStream_t s);
// NV12 surfaces at full resolution (csrc/nv12.hip; acrmi_nv12_to_rgb): geometry by value, NV12_FRAMES_PER_LAUNCH per launch
constexpr int NV12_FRAMES_PER_LAUNCH = 64;
struct Nv12Coef {
  int cy, cub, cug, cvg, cvr, y_off;
};
struct Nv12DstFrame {   // 40 bytes: 64 of them + the coefficient row are 2.6 KB of the 4 KB argument block
  const uint8_t* y;
  const uint8_t* uv;
  uint8_t* dst;
  int H, W, y_pitch, uv_pitch;
};
struct Nv12DstBatch {
  Nv12DstFrame f[NV12_FRAMES_PER_LAUNCH];
};
static_assert(sizeof(Nv12DstBatch) + sizeof(Nv12Coef) + 8 <= 4096, "NV12 kernel arguments must fit the 4 KB argument block");
hipError_t launch_nv12_to_rgb(const Nv12DstBatch& pb, const Nv12Coef& k, int n, int bgr, hipStream_t s);
// The NV12 colour rule of one pixel (csrc/nv12.hip states it).  Shared by nv12_to_rgb_kernel and the NV12 window kernel.
__device__ inline int nv12_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ inline void nv12_pixel(const Nv12Coef& k, int Y, int U, int V, int& R, int& G, int& B) {
  int yy = Y - k.y_off;
  yy = (yy < 0 ? 0 : yy) * k.cy;
  const int u = U - 128, v = V - 128, r = 1 << 19;
  R = nv12_clamp8((yy + k.cvr * v + r) >> 20);
  G = nv12_clamp8((yy + k.cug * u + k.cvg * v + r) >> 20);
  B = nv12_clamp8((yy + k.cub * u + r) >> 20);
}
// NV12 surfaces as the OUTPUT (csrc/nv12_out.hip, csrc/nv12_out_plan.h; acrmi_rgb_to_nv12, acrmi_nv12_compose): geometry by
// value again.  A compose frame names five planes and six sizes, 64 bytes: 58 of them (3712 bytes), the two coefficient rows and
// the flag (68 bytes) and the 256 bytes of hidden arguments hipcc appends to the kernel-argument segment make 4040 of the 4096
// bytes; 59 would not fit.
struct Nv12OutFrame {   // 40 bytes
  const uint8_t* src;   // tight [H, W, 3]
  uint8_t* y;
  uint8_t* uv;
  int H, W, y_pitch, uv_pitch;
};
struct Nv12OutBatch {
  Nv12OutFrame f[NV12_FRAMES_PER_LAUNCH];
};
constexpr int NV12_COMPOSE_FRAMES_PER_LAUNCH = 58;
struct Nv12ComposeFrame {   // 64 bytes
  const uint8_t* src_y;
  const uint8_t* src_uv;
  const uint8_t* drawn;     // tight [H, W, 3]
  uint8_t* y;               // may be src_y (then uv is src_uv and the pitches agree): a thread reads and writes its own blocks only
  uint8_t* uv;
  int H, W, src_y_pitch, src_uv_pitch, y_pitch, uv_pitch;
};
struct Nv12ComposeBatch {
  Nv12ComposeFrame f[NV12_COMPOSE_FRAMES_PER_LAUNCH];
};
static_assert(sizeof(Nv12OutBatch) + sizeof(Nv12OutCoef) + 8 + 256 <= 4096 &&
                  sizeof(Nv12ComposeBatch) + sizeof(Nv12Coef) + sizeof(Nv12OutCoef) + 8 + 256 <= 4096,
              "NV12 output kernel arguments must fit the 4 KB argument block");
hipError_t launch_rgb_to_nv12(const Nv12OutBatch& pb, const Nv12OutCoef& k, int n, int bgr, hipStream_t s);
hipError_t launch_nv12_compose(const Nv12ComposeBatch& pb, const Nv12Coef& k6, const Nv12OutCoef& k10, int n, int bgr, hipStream_t s);
// Windows of frames (csrc/preprocess.hip): a window of a frame pre-processed as a frame of its own size - a region of
// interest (acrmi_preprocess_rois / acrmi_preprocess_rois_nv12) or the whole frame (acrmi_preprocess_frames /
// acrmi_preprocess_nv12).  Geometry by value, ROIS_PER_LAUNCH per launch; the windows are already clamped to their frames
// (csrc/roi_plan.h) and the kernels trust them.
constexpr int ROIS_PER_LAUNCH = 64;
struct RoiBgr {         // 24 bytes
  const uint8_t* src;   // the window's first pixel: frame + (t * W + l) * 3
  size_t pitch;         // bytes per row of the FRAME (W * 3)
  int h, w;             // the window
};
struct RoiBgrBatch {
  RoiBgr r[ROIS_PER_LAUNCH];
};
struct RoiNv12 {        // 40 bytes
  const uint8_t* y;     // the planes of the FRAME: chroma is addressed in frame coordinates, so odd l and t are legal
  const uint8_t* uv;
  int y_pitch, uv_pitch;
  int l, t, h, w;       // the window: rows [t, t + h), columns [l, l + w) of the frame
};
struct RoiNv12Batch {
  RoiNv12 r[ROIS_PER_LAUNCH];
};
static_assert(sizeof(RoiBgrBatch) + 24 <= 4096 && sizeof(RoiNv12Batch) + sizeof(Nv12Coef) + 24 <= 4096,
              "window kernel arguments must fit the 4 KB argument block");
hipError_t launch_preprocess_rois(const RoiBgrBatch& rb, int n, int out_size, uint8_t* out, hipStream_t s);
hipError_t launch_preprocess_rois_nv12(const RoiNv12Batch& rb, const Nv12Coef& k, int n, int out_size, uint8_t* out, hipStream_t s);
// The same windows with the BOXES in device memory (acrmi_preprocess_rois_dev / acrmi_preprocess_rois_nv12_dev; DESIGN.md
// "Tracking on the device"): what the host knows travels by value - the frame, its size and the index of the region's box -
// and the kernel reads boxes[box], clamps it to the frame itself (roi_plan_or_frame, csrc/roi_plan.h: a box without pixels
// becomes the whole frame) and writes the region's `offsets` row and status word.
struct RoiBgrDev {      // 24 bytes
  const uint8_t* frame; // the FRAME's first pixel
  int H, W;             // the frame
  int box;              // the region: row of boxes / offsets, element of status
};
struct RoiBgrDevBatch {
  RoiBgrDev r[ROIS_PER_LAUNCH];
};
struct RoiNv12Dev {     // 40 bytes
  const uint8_t* y;     // the planes of the FRAME
  const uint8_t* uv;
  int y_pitch, uv_pitch;
  int H, W;             // the frame
  int box;
};
struct RoiNv12DevBatch {
  RoiNv12Dev r[ROIS_PER_LAUNCH];
};
static_assert(sizeof(RoiBgrDevBatch) + 48 <= 4096 && sizeof(RoiNv12DevBatch) + sizeof(Nv12Coef) + 48 <= 4096,
              "window kernel arguments must fit the 4 KB argument block");
hipError_t launch_preprocess_rois_dev(const RoiBgrDevBatch& rb, const int32_t* boxes, int n, int out_size, uint8_t* out,
                                      float* offsets, int32_t* status, hipStream_t s);
hipError_t launch_preprocess_rois_nv12_dev(const RoiNv12DevBatch& rb, const Nv12Coef& k, const int32_t* boxes, int n, int out_size,
                                           uint8_t* out, float* offsets, int32_t* status, hipStream_t s);
// csrc/track.hip (acrmi_track_boxes): pj2d_org [n,2,21,2], slots [n,2,slot_floats] with the flag at flag_at, frame_hw int32
// [n,2] = (H, W) -> boxes int32 [n,4], the rule of csrc/track_plan.h; one wave per region, one launch for any n
hipError_t launch_track_boxes(const float* pj2d_org, const float* slots, const int32_t* frame_hw, int n, int slot_floats,
                              int flag_at, double scale, int min_size, int32_t* boxes, hipStream_t s);
hipError_t launch_pow11(float* buf, long n_pixels, int cs, int ch, hipStream_t s);
// fp32 NCHW [B,C,H,W] -> channels [coff, coff + C) of an NHWC buffer with channel stride cs (acrmi_heads: backbone features a
// caller hands to head_forward, acr/model.py:47-53)
hipError_t launch_nchw_to_nhwc(const float* in, int B, int C, int H, int W, float* out, int cs, int coff, hipStream_t s);
hipError_t launch_coordfill(float* buf, int B, int H, int W, int cs, int coff, hipStream_t s);
// 16-bit storage variants (dtype = ACRMI_DT_F16 / ACRMI_DT_BF16; strides and offsets in elements, C % 8 == 0)
hipError_t launch_maxpool3s2(const float* in, int B, int H, int W, int in_cs, int in_coff, int C, float* out, int out_cs,
                             int out_coff, hipStream_t s);
hipError_t launch_maxpool3s2_h16(const void* in, int B, int H, int W, int in_cs, int in_coff, int C, void* out, int out_cs,
                                 int out_coff, int dtype, hipStream_t s);
hipError_t launch_bilinear2x_h16(const void* in, int B, int H, int W, int in_cs, int in_coff, int C, void* out, int out_cs,
                                 int out_coff, int dtype, hipStream_t s);
hipError_t launch_fuse_sum_h16(const FuseArgs& a, int dtype, hipStream_t s);   // a.term / a.out carry 16-bit pointers
hipError_t launch_pow11_h16(void* buf, long n_pixels, int cs, int ch, int dtype, hipStream_t s);
hipError_t launch_coordfill_h16(void* buf, int B, int H, int W, int cs, int coff, int dtype, hipStream_t s);

// attention pooling: segm [B,2H,2W,segm_cs] logits (channels 1..32 at even pixels), feat [B,H,W,feat_cs] (C ch)
// stats_ws: [B,32,2] (max, 1/sumexp); pooled [B,32,C]
hipError_t launch_attpool(const float* segm, int segm_cs, const float* feat, int feat_cs, int C, int B, int H, int W,
                          float* ws, float* pooled, hipStream_t s, int feat_dtype = 0);   // feat may be f16 / bf16 (ACRMI_DT_*)
size_t attpool_ws_floats(int B, int C);

// pare bias: pooled [B,32,320] -> per-frame bias row [B, biasP] for the 109->109 mix conv
struct PareArgs {
  const float* pooled;   // [B,32,C] (C = 320: 256 contact + 64 shape; C = 256: contact only, shape conv folded into lin_w)
  const float* lc_w;     // LocallyConnected2d weight [6][256][16]
  const float* lin_w;    // [10][(C == 320 ? 64 : 256) * 16]
  const float* lin_b;    // [10]
  const float* mix_wp;   // [109][106] columns of the mix conv that multiply pare
  const float* mix_b;    // [109]
  float* out;            // [B, out_stride]
  int B, C, part0, out_stride;
};
hipError_t launch_parebias(const PareArgs& a, hipStream_t s);

struct DecodeArgs {
  const float* center[2];
  const float* params[2];
  const float* prior[2];
  int center_cs, params_cs, prior_cs;
  int B;
  float* slots;
  float thresh;          // centermap_conf_thresh (acr/result_parser.py:241), strict >
  const unsigned* poison; // non-null and != 0 on the device: the program's results are invalid (fp16x3 range overflow) - every
                         // slot is written as NaN, so that MANO's meshes are NaN too instead of plausible numbers
  const int* prior_gate; // null: the cross-hand prior is decided per frame (both hands found, centers <= 32 px apart);
                         // else [B]: < 0 = per frame, 0 = no prior, 1 = prior whenever the frame has both hands (the caller
                         // has applied the reference's batch-wide rules, acr/result_parser.py:42-47,131)
};
hipError_t launch_decode(const DecodeArgs& a, hipStream_t s);
// The max_hand (1..ACRMI_MAX_HAND) best centers of each map per frame: slots [B,max_hand,2,ACRMI_SLOT], pair k = (left rank
// k, right rank k), the prior of a hand from its nearest flagged partner of the other side.  prior_gate
// is not read; max_hand = 1 writes what launch_decode writes.
hipError_t launch_decode_multi(const DecodeArgs& a, int max_hand, hipStream_t s);
// The reference's BATCH-WIDE prior decision (acr/result_parser.py:42-47, 102-145) from a first decode's slots [B,2,ACRMI_SLOT]:
// gate[b] = 1 when frame b has both hands AND the batch has a left and a right detection AND the left center of the FIRST
// left-detected frame and the right center of the FIRST right-detected frame are <= 32 map pixels apart; else 0.  One workgroup.
hipError_t launch_prior_gate(const float* slots, int B, int* gate, hipStream_t s);

// One-Euro smoothing of the decoded (poses, betas) between decode and MANO (acr/utils.py:1466-1527), filter state per video
// stream in a table: one workgroup per stream present in the launch, that stream's frames in batch order (smooth_plan.h)
struct SmoothArgs {
  float* slots;          // [n frames of the launch,2,ACRMI_SLOT], smoothed in place where the flag is set
  float* state;          // [capacity][2 hands][x_raw | x_filt | dx_filt][64]
  int* init;             // [capacity][2]
  float mincutoff, mincutoff_betas, beta, freq;
  float alpha_d, one_minus_alpha_d;   // derivative filter: compute_alpha(dcutoff) in double, rounded once
  float two_pi, te;
  SmoothBatch b;         // which frames belong to which stream, by value
};
hipError_t launch_smooth(const SmoothArgs& a, int n_streams, hipStream_t s);
// the n <= SMOOTH_FRAMES_PER_LAUNCH listed streams start a new sequence (their init flags are cleared)
struct SmoothIds {
  int32_t id[SMOOTH_FRAMES_PER_LAUNCH];
};
hipError_t launch_smooth_reset(const SmoothIds& ids, int n, int* init, hipStream_t s);

// Association of the hands of [n frames,K,2,ACRMI_SLOT] with the tracks of their streams, the reordering of the rows into track
// order and (smooth) the One-Euro step of every slot that has a detection (assoc_plan.h): one workgroup
// of 128 * K threads per stream present in the launch, plus one for the frames that belong to no stream when there are any.
struct AssocArgs {
  SmoothArgs s;          // slots [n,K,2,ACRMI_SLOT]; state [capacity][K][2][x_raw | x_filt | dx_filt][64]; init [capacity][K][2]
  AssocSide* meta;       // [capacity][2]
  int32_t* track_ids;    // [n,K,2]
  int32_t* perm;         // [n,K,2] or null
  int K, gate, max_miss, smooth, m;       // m: frames of the launch
  uint32_t loose[SMOOTH_FRAMES_PER_LAUNCH / 32];      // bit f: frame f belongs to no stream (track_ids -1, perm identity)
};
hipError_t launch_associate(const AssocArgs& a, int n_streams, bool any_loose, hipStream_t s);
// the n <= SMOOTH_FRAMES_PER_LAUNCH listed streams free every slot and restart their ids at 0
hipError_t launch_assoc_reset(const SmoothIds& ids, int n, int K, AssocSide* meta, int* init, hipStream_t s);

// Point heads: the six non-center head towers evaluated only at the pixels the decode reads (heads.hip).
// Per tower (floats): entry W [9 taps][9 cin/4][64 cout][4] + b[64]; 4 x (conv W [9][16][64][4] + b[64]);
// exit W [64][112] + b[112].  Three towers per side in the order params (k=1), cam (k=3), prior (k=4).
constexpr int TP_ENTRY_W = 9 * 9 * 64 * 4;
constexpr int TP_CONV_W = 9 * 16 * 64 * 4;
constexpr int TP_EXIT_N = 112;
constexpr int TP_TOWER_FLOATS = TP_ENTRY_W + 64 + 4 * (TP_CONV_W + 64) + 64 * TP_EXIT_N + TP_EXIT_N;
struct PointArgs {
  const float* x34; int x_cs;              // [B,128,128,x_cs] backbone features + coord maps (34 channels)
  const float* center[2]; int center_cs;   // [B,64,64,center_cs] channel 0
  const float* w;                          // 3 x TP_TOWER_FLOATS (this side)
  const float* mix_w;                      // [109 cin][TP_EXIT_N] mix conv (cam3 columns merged)
  const float* bias; int bias_stride;      // per-frame pare bias rows
  float* p109; int p109_cs;                // [B,64,64,cs] cam(3) | params(106) before the mix
  float* prior; int prior_cs;              // [B,64,64,cs] 106-ch prior map
  float* final_; int final_cs;             // [B,64,64,cs] 109-ch params map after the mix
  int* picks;                              // workspace of max_batch * POINT_PLAN_INTS ints: [B,4] flat_l, flat_r, prior gate
                                           // (launch_point_heads) or [B] PointPlan (launch_point_heads_multi)
  int side, B;
  float thresh;                            // centermap_conf_thresh
  int prior_when_both;                     // ACRMI_OPT_BATCH_PRIOR: evaluate the prior point whenever the frame has BOTH hands - the
                                           // batch-wide rule (acrmi_prior_gate) may open the gate for a frame whose own centers are
                                           // more than 32 px apart; the gated decode then decides whether the value is added
};
hipError_t launch_point_heads(const PointArgs& a, hipStream_t s);
// the same towers at the max_hand (1..ACRMI_MAX_HAND) best centres of each side: the pixels of point_plan.h, which are the ones
// decode_multi_kernel reads.  prior_when_both is not read (the batch-wide prior rule knows one hand per side).
hipError_t launch_point_heads_multi(const PointArgs& a, int max_hand, hipStream_t s);

struct ManoTables {   // device pointers
  const float* v_template;   // [778*3]
  const float* shapedirs_t;  // [10][2334]   (transposed for coalesced reads)
  const float* posedirs_t;   // [135][2334]
  const float* jreg;         // [16][778]
  const float* weights;      // [778][16]
  const float* hands_mean;   // [45]
  // f16 copies for ACRMI_OPT_MANO_FP16 (same layouts)
  const unsigned short* shapedirs_h;
  const unsigned short* posedirs_h;
  const unsigned short* weights_h;
  // round 6: the two SMALL tables as f16 pairs - lo = f16(x - float(hi)); value = float(hi) + float(lo), ~22 bits - the
  // skinning weights (a plain-f16 weight near 0.5 is off by 2.4e-4: x a ~0.1 m joint offset = the 6e-5 m of r5's configs[4]) and
  // the shape blend shapes.  The pose blend table (1.26 of the 1.46 MB per side: what "fp16 MANO LBS" halves) stays plain f16.
  const unsigned short* shapedirs_l;
  const unsigned short* weights_l;
};
struct ManoArgs {
  ManoTables t[2];
  const float* poses; int pose_stride;
  const float* betas; int beta_stride;
  const int32_t* side;
  int H, center_idx;
  float *verts, *joints, *center;
  const float* cam; int cam_stride;
  const float* offsets; int off_div;   // offsets row = hand row / off_div
  float *verts_camed, *pj2d, *pj2d_org;
  int lbs_f16;                         // blend-shape tables and skinning weights from their f16 copies
  int slices;                          // workgroups per hand (launch_mano sets it): slice s computes pose blend, skinning and
                                       // outputs of vertices [s * ceil(778 / slices), ...) - everything before the pose blend
                                       // (rotations, shape blend, joint regression, chain) is cheap and repeated per slice
  int pose_rotmat;                     // 1: `poses` rows are 16 row-major 3x3 rotation matrices (joint_rot_mode='rotmat',
                                       // mano/manolayer.py:151-162): no Rodrigues, no hands_mean
};
hipError_t launch_mano(const ManoArgs& a, hipStream_t s);
// The backward of the axis-angle mode (csrc/mano_grad.hip): cotangents in, gradients of poses and betas out.  Always the fp32
// tables of t[].
struct ManoGradArgs {
  ManoTables t[2];
  const float* poses; int pose_stride;
  const float* betas; int beta_stride;
  const int32_t* side;
  int H, center_idx;
  const float *g_verts, *g_joints, *g_center;   // [H,778,3], [H,21,3], [H,3]; each may be null = zeros
  float *g_poses, *g_betas;                     // [H,48], [H,10]
};
hipError_t launch_mano_backward(const ManoGradArgs& a, hipStream_t s);
// The fused fitter (csrc/mano_fit.hip; the rule is csrc/mano_fit_plan.h): `steps` Adam iterations per hand in one launch.
struct ManoFitArgs {
  ManoTables t[2];
  float* state;                                 // [H, FIT_STATE]: read, and written when steps > 0
  const int32_t* side;
  int H, center_idx;
  const float *y3, *w3;                         // [H,21,3], [H,21]; y3 null = no 3-D term, w3 null = ones
  const float *y2, *w2;                         // [H,21,2], [H,21]
  const float *yv, *wv;                         // [H,778,3], [H]; yv non-null selects the dense vertex level
  const float* prior;                           // [H,58] or null = zeros
  double lam_pose, lam_beta, lr[5], b1, b2, eps;
  int steps, dense;                             // dense: the dense vertex level also without yv
  float *poses, *betas, *trans, *cam, *loss;    // [H,48], [H,10], [H,3], [H,3], [H,2]
  float* grad;                                  // [H,64] or null: the gradient of the last evaluated step
};
hipError_t launch_mano_fit(const ManoFitArgs& a, hipStream_t s);
hipError_t launch_cam_trans(const float* joints, const float* pj2d, int n, float focal, float img, float* out, hipStream_t s);

// Mesh overlay (csrc/render.hip; DESIGN.md "Rendering"): M meshes of one vertex / face count drawn into N equal-sized frames.
struct RenderArgs {
  const float* verts;            // [M, n_verts, 3]
  const float* trans;            // [M, 3] or null
  const int32_t* topo[2];        // mesh topology blobs (build_mesh_topology) on the device; [1] may be null
  const int32_t* mesh_topo;      // [M] 0 / 1 = which blob, or null (all 0)
  const int32_t* mesh_frame;     // [M] frame the mesh is drawn into, < 0 = not drawn
  const float* rgb;              // [M, 3] base colour, channel order of the image
  const float* view;             // [N, 4] scale x, scale y, shift x, shift y of the 512 canvas, or null (identity)
  const float* mesh_view;        // [M, 4] the same per MESH (views over regions), exclusive with `view`: the depth value is then
                                 // sx / Z, one virtual camera per frame (csrc/region_view_plan.h)
  float focal, visible_weight;
  const uint8_t* img_in;         // [N, H, W, 3]
  uint8_t* img_out;              // may be img_in
  int32_t* ids_out;              // [N, H, W] or null
  char* ws;                      // render_workspace_bytes(M, n_faces)
  size_t ws_box_off, ws_rec_off; // (launch_render fills these)
  int n_meshes, n_verts, n_faces, n_frames, H, W;
  const float* vcol;             // [M, n_verts, 3] base colour per VERTEX in [0,1], channel order of the image, or null: `rgb`.
                                 // Last, so that the flat kernels read every other field where they always did.
};
constexpr int RENDER_MAX_VERTS = 4000;      // 16 bytes of LDS per vertex in the setup kernel
long long mesh_topology_ints(int n_faces, int n_verts);
bool build_mesh_topology(const int32_t* faces, int n_faces, int n_verts, int32_t* blob);
size_t render_workspace_bytes(int n_meshes, int n_faces);
hipError_t launch_render(const RenderArgs& a, hipStream_t s);
hipError_t launch_render_prep(const float* slots, const float* offsets, int B, int slot_stride, int flag_at, const float* colors,
                              int32_t* mesh_frame, int32_t* mesh_topo, float* rgb, float* view, hipStream_t s);
// views over regions: slots [n,2,slot_stride], offsets [n,10] and region_frame [n] on the device -> mesh_frame [2n] (-1: not
// drawn), and where not null mesh_topo [2n], rgb [2n,3], mesh_view [2n,4]; colors may be null when rgb is
hipError_t launch_render_region_prep(const float* slots, const float* offsets, const int32_t* region_frame, int n, int n_frames,
                                     int H, int W, int slot_stride, int flag_at, const float* colors, int32_t* mesh_frame,
                                     int32_t* mesh_topo, float* rgb, float* mesh_view, hipStream_t s);

// Per-vertex colours (csrc/vertex_color.hip; the rule: csrc/vertex_color_plan.h).
struct VertexColorArgs {
  const float* values;           // [M, V]
  const int32_t* flags;          // [M, V] or null
  const float* base_rgb;         // [M, 3]
  float* vcol;                   // [M, V, 3]
  float lo, hi;
  float flag_rgb[3];
  int reverse, M, V;
  uint8_t lut[768];              // [256][3] in the image's channel order
};
hipError_t launch_vertex_colors(const VertexColorArgs& a, hipStream_t s);
struct ContactValuesArgs {
  const float* d2;               // [B*K*K, 2, V]
  const float* s;                // the same shape (nearest-vertex measure), or null
  const int32_t* cross;          // the same shape (surface measure), or null: exactly one of the two
  float max_depth;
  float* value;                  // [B, K, 2, V]
  int32_t* flag;                 // [B, K, 2, V]
  int B, K, V;
};
hipError_t launch_contact_values(const ContactValuesArgs& a, hipStream_t s);

// The two contact measures between meshes (csrc/contact.hip): what both read and write, then what each adds.
struct ContactFrame {
  const float* verts;            // [M, n_verts, 3]
  const float* trans;            // [M, 3] or null
  const int32_t* topo[2];        // mesh topology blobs on the device; [1] may be null
  const int32_t* mesh_topo;      // [M] 0 / 1 = which blob, or null (all 0)
  const int32_t* pairs;          // [n_pairs, 2] mesh indices; outside [0, M): the pair is skipped
  float contact_dist, max_depth;
  float* d2;                     // [n_pairs, 2, n_verts]
  float4* ws;                    // contact_workspace_bytes / surface_workspace_bytes of the sizes, 16-byte aligned
  float* sum_f;                  // [n_pairs, CONTACT_SUM_F or SURFACE_SUM_F]
  int32_t* sum_i;                // [n_pairs, CONTACT_SUM_I or SURFACE_SUM_I]
  int n_meshes, n_verts, n_faces, n_pairs;
};
// Contact and interpenetration by the nearest vertex (csrc/contact_plan.h).
struct ContactArgs : ContactFrame {
  const int32_t* sign;           // [M] +1 / -1 orientation of the mesh's topology, or null (all +1)
  int32_t* nn;                   // [n_pairs, 2, n_verts]
  float* side;                   // [n_pairs, 2, n_verts]
};
hipError_t launch_contact(const ContactArgs& a, hipStream_t s);
// acrmi_contact: slots [B,K,2,ACRMI_SLOT] on the device -> pairs [B*K*K,2], mesh_topo and sign [2*B*K]
hipError_t launch_contact_prep(const float* slots, int B, int K, int sign_left, int sign_right, int32_t* pairs, int32_t* mesh_topo,
                               int32_t* sign, hipStream_t s);
// The surface contact measure (csrc/surface_contact_plan.h).
struct SurfaceContactArgs : ContactFrame {
  int32_t *face, *cross;         // [n_pairs, 2, n_verts]
  float* point;                  // [n_pairs, 2, n_verts, 3]
};
hipError_t launch_surface_contact(const SurfaceContactArgs& a, hipStream_t s);

// Scoring against ground truth (csrc/score.hip; the rule: csrc/score_plan.h).
struct ScoreSet {                // one point set of a pose-errors launch
  const float *P, *G;            // [N, n, 3] prediction, truth
  const uint8_t* valid;          // [N, n] or null
  const float *oP, *oG;          // origin rows (row stride o_stride floats) read when root < 0, or null
  const uint8_t* o_valid;        // with them: the origins of row r are good only when o_valid[r * o_valid_stride] != 0; or null
  const float* trans;            // [N, 3] or null
  float *e_ra, *e_pa;            // [N, n]
  float* row_f;                  // [N, SCORE_ROW_F]
  int32_t* row_i;                // [N, SCORE_ROW_I]
  float* xform;                  // [N, SCORE_XFORM] or null
  float* pair_err;               // [N / 2] or null
  int n, root, o_stride, o_valid_stride;
};
struct ScoreArgs {
  ScoreSet set[2];
  int n_sets;
  const int32_t* group;          // [N] or null: group_side ? row & 1 : 0
  int group_side;
  const float* flags;            // flag of row r at flags[r * flag_stride], or null
  int flag_stride;
  int N, n_groups;
};
hipError_t launch_pose_errors(const ScoreArgs& a, hipStream_t s);
struct ScoreAccArgs {
  const float *e_ra, *e_pa;      // [N, n]
  const int32_t* group;
  int group_side;
  const float* flags;
  int flag_stride;
  const float* pair_err;         // [N / 2] or null
  int N, n, n_groups, n_bins;
  double bin_width;
  int64_t* board;                // score_board_bytes
  int64_t* pair_board;           // score_pair_bytes, or null
};
hipError_t launch_score_accumulate(const ScoreAccArgs& a, hipStream_t s);

// Matching decoded hands to ground truth (csrc/match.hip; the rule: csrc/match_plan.h).
struct MatchArgs {
  const float* pred;             // [B, K, 2, n, D]
  const float* truth;            // [B, G, 2, n, D]
  const uint8_t* valid;          // [B, G, 2, n] or null
  const uint8_t* truth_valid;    // [B, G, 2] or null
  const float* flags;            // flag of prediction row r = (b * K + i) * 2 + s at flags[r * flag_stride], or null
  size_t flag_stride;
  const float* trans;            // [B, K, 2, D] or null
  const int32_t* group;          // [B, G, 2] or null = the side
  int B, K, G, n, D;
  float gate;
  int min_points;
  int32_t* match;                // [B, K, 2]
  int32_t* pred_of;              // [B, G, 2]
  float* cost;                   // [B, K, 2]
  int32_t* counts;               // [B, 2, 3]
  int32_t* group_out;            // [B, G, 2]
};
hipError_t launch_match(const MatchArgs& a, hipStream_t s);
struct MatchGatherArgs {
  const float* src;              // [B, Ks, 2, W]
  const int32_t* index;          // [B, Kd, 2]
  float* dst;                    // [B, Kd, 2, W]
  long long rows, W;             // rows = B * Kd * 2
  int Ks, Kd;
};
hipError_t launch_match_gather(const MatchGatherArgs& a, hipStream_t s);
struct MatchAccArgs {
  const int32_t* counts;         // [B, 2, 3]
  const float* cost;             // [B, K, 2]
  int B, K;
  int64_t* board;                // match_board_bytes
};
hipError_t launch_match_accumulate(const MatchAccArgs& a, hipStream_t s);

// Key-point skeleton and heat-map views (csrc/overlay.hip; DESIGN.md "Key-point and heat-map views").
struct SkeletonArgs {
  const float* kps;              // [n_hands, 21, 2] MANO joint order; pixels of the image, or (normalized) [-1, 1] of the 512 canvas
  const int32_t* hand_frame;     // [n_hands] frame a hand is drawn into, < 0 = not drawn - or null with `slots`:
  const float* slots;            // [n_hands, slot_stride]: hand h belongs to frame h / 2, drawn when its flag_at > 0.5
  int slot_stride, flag_at, normalized;
  int n_hands, n_frames, H, W, line_width, circle_rad;
  const uint8_t* img_in;         // [n_frames, H, W, 3]
  uint8_t* img_out;              // may be img_in
  int wide;                      // (launch_skeleton fills this)
  uint8_t colors[64];            // [21][3] in the image's channel order
};
struct HeatmapBase {             // what the heat maps over frames and over regions share
  const void* maps[2];           // left / right, one pair per frame or region; [1] null = one view
  long long frame_stride;        // elements between the maps of two frames (regions)
  int pix_stride;                // elements between two cells of a row (1; the channel stride of a head buffer)
  int dtype;                     // 0 fp32, 1 f16, 2 bf16 (ACRMI_DT_*)
  int n, h, w, H, W;             // frames (regions), map size, frame size
  const float* offsets;          // [n, 10]
  float weight;
  const uint8_t* img_in;         // [frames, H, W, 3]
  uint8_t* out[2];
  int wide;                      // (the launcher fills this)
  uint8_t lut[768];              // [256][3] in the image's channel order
};
struct HeatmapArgs : HeatmapBase {
  const float* view;             // [n, 4] scale x, scale y, shift x, shift y; null: the view is taken from `offsets`, or none
};
constexpr int OVERLAY_MAX_DIM = 16384, OVERLAY_MAX_FRAMES = 65535, OVERLAY_MAX_WIDTH = 11, OVERLAY_MAX_RAD = 255;
extern const uint8_t kSkeletonRGB[21][3];
void skeleton_default_colors(bool bgr, uint8_t* out63);
void heatmap_default_lut(bool bgr, uint8_t* out768);
hipError_t launch_skeleton(const SkeletonArgs& a, hipStream_t s);
hipError_t launch_heatmap(const HeatmapArgs& a, hipStream_t s);
// Heat maps of REGIONS composed over their frames (DESIGN.md "Views over regions"): region i's maps tint the pixels of its
// window in frame region_frame[i]; where windows overlap the larger colour index wins.
struct RegionHeatmapArgs : HeatmapBase {
  const int32_t* region_frame;   // [n]
  int n_frames;
};
hipError_t launch_region_heatmap(const RegionHeatmapArgs& a, hipStream_t s);

// The part segmentation as an output (csrc/segm.hip; csrc/segm_plan.h).
struct SegmArgs {
  const float* logits;           // [n, h, w, pix_stride] fp32, C classes per cell
  long long frame_stride;        // floats between the maps of two frames
  int pix_stride, C;
  int n, h, w, H, W;
  const float* view;             // [n, 4] or null
  const float* offsets;          // [n, 10]: the view is taken from these rows instead (null: `view`, or none)
  float weight;
  const uint8_t* img_in;         // [n, H, W, 3], with `out`
  uint8_t* out;                  // the drawn view, may be img_in; or null
  uint8_t* labels;               // [n, H, W]; or null
  int wide, wide_labels, vec;    // (launch_segm fills these)
  uint8_t colors[192];           // [C][3] in the image's channel order
};
hipError_t launch_segm(const SegmArgs& a, hipStream_t s);
struct SegmStatsArgs {
  const uint8_t* labels;         // [n, H, W]
  const int32_t* ids;            // [n, H, W] of the rasteriser, or null
  int n_faces, n, H, W, C;
  int32_t *counts, *boxes, *agree;      // [n, C], [n, 2, 4], [n, 2, 3] (null without ids)
  int32_t* ws;                   // segm_stats_ws_ints(n, H, W)
};
hipError_t launch_segm_stats(const SegmStatsArgs& a, hipStream_t s);

}  // namespace acrmi
