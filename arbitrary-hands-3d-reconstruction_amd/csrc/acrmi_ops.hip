// libacrmi.so: the stand-alone operators of the C ABI (unit tests / callers with their own tensors; no context).
#include "acrmi_ctx.h"
#include "contact_plan.h"
#include "surface_contact_plan.h"
#include "conv_frame.h"   // conv_shape
#include "match_plan.h"
#include "roi_plan.h"
#include "score_plan.h"
#include "segm_plan.h"
#include "track_plan.h"
#include "vertex_color_plan.h"

#include <initializer_list>
#include <vector>

// (poison: acrmi_decode_gated's range flag of an 'fp16x3' program; null for the stand-alone operator)
int decode_maps_impl(const float* l_center, const float* r_center, int center_cs, const float* l_params,
                     const float* r_params, int params_cs, const float* l_prior, const float* r_prior, int prior_cs,
                     int B, float conf_thresh, const int32_t* prior_gate, const unsigned* poison, float* slots, void* stream,
                     int max_hand) {
  if (!l_center || !r_center || !l_params || !r_params || !l_prior || !r_prior || !slots || B <= 0 || params_cs < 109 ||
      prior_cs < 106 || center_cs < 1 || !(conf_thresh == conf_thresh))
    return fail(nullptr, ACRMI_EINVAL, "acrmi_decode_maps: bad arguments");
  DecodeArgs d{};
  d.center[0] = l_center; d.center[1] = r_center; d.center_cs = center_cs;
  d.params[0] = l_params; d.params[1] = r_params; d.params_cs = params_cs;
  d.prior[0] = l_prior; d.prior[1] = r_prior; d.prior_cs = prior_cs;
  d.B = B; d.slots = slots; d.thresh = conf_thresh;
  d.prior_gate = prior_gate;
  d.poison = poison;
  hipError_t e = max_hand > 0 ? launch_decode_multi(d, max_hand, (hipStream_t)stream) : launch_decode(d, (hipStream_t)stream);
  if (e != hipSuccess) return fail(nullptr, ACRMI_EHIP, "decode launch: %s", hipGetErrorString(e));
  return ACRMI_OK;
}

extern "C" {

int acrmi_decode_maps_gated(const float* l_center, const float* r_center, int center_cs, const float* l_params,
                            const float* r_params, int params_cs, const float* l_prior, const float* r_prior, int prior_cs,
                            int B, float conf_thresh, const int32_t* prior_gate, float* slots, void* stream) {
  return decode_maps_impl(l_center, r_center, center_cs, l_params, r_params, params_cs, l_prior, r_prior, prior_cs, B, conf_thresh,
                          prior_gate, nullptr, slots, stream);
}

int acrmi_decode_maps(const float* l_center, const float* r_center, int center_cs, const float* l_params,
                      const float* r_params, int params_cs, const float* l_prior, const float* r_prior, int prior_cs,
                      int B, float conf_thresh, float* slots, void* stream) {
  return acrmi_decode_maps_gated(l_center, r_center, center_cs, l_params, r_params, params_cs, l_prior, r_prior, prior_cs, B,
                                 conf_thresh, nullptr, slots, stream);
}

int acrmi_decode_maps_multi(const float* l_center, const float* r_center, int center_cs, const float* l_params,
                            const float* r_params, int params_cs, const float* l_prior, const float* r_prior, int prior_cs,
                            int B, int max_hand, float conf_thresh, float* slots, void* stream) {
  if (max_hand < 1 || max_hand > ACRMI_MAX_HAND)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_decode_maps_multi: max_hand %d outside 1..%d", max_hand, ACRMI_MAX_HAND);
  return decode_maps_impl(l_center, r_center, center_cs, l_params, r_params, params_cs, l_prior, r_prior, prior_cs, B, conf_thresh,
                          nullptr, nullptr, slots, stream, max_hand);
}

// ---- stand-alone operators -------------------------------------------------------------------------
}  // extern "C"

// the tail of the convolution entry points: channel ranges, derived fields, the shape rules (csrc/conv_rules.h); then the launch
static int conv_check(const char* who, ConvArgs& a) {
  if ((a.ks != 1 && a.ks != 3) || (a.stride != 1 && a.stride != 2))
    return fail(nullptr, ACRMI_EINVAL, "%s: only 3x3 and 1x1 at stride 1 / 2 are implemented (got k%d s%d)", who, a.ks, a.stride);
  const int og = a.splitk ? 1 : a.groups;      // the slices of a split-K conv share the output channels
  if (a.in_coff < 0 || a.out_coff < 0 || a.res_coff < 0 || a.in_coff + a.groups * a.Cin > a.in_cs || a.out_coff + og * a.Cout > a.out_cs ||
      (a.res && a.res_coff + og * a.Cout > a.res_cs) || a.bias_fstride < 0 || (a.bias_fstride > 0 && a.bias_fstride < a.groups * a.Cout))
    return fail(nullptr, ACRMI_EINVAL, "%s: channel slice outside its tensor's channel stride", who);
  conv_derive(a);
  if (const char* why = conv_algo_reject(a.algo, conv_shape(a))) return fail(nullptr, ACRMI_EINVAL, "%s: %s", who, why);
  return ACRMI_OK;
}
static int conv_check_and_launch(const char* who, ConvArgs& a, void* stream) {
  if (int r = conv_check(who, a)) return r;
  hipError_t e = launch_conv(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "conv launch: %s", hipGetErrorString(e));
}

extern "C" {

int acrmi_conv2d(const float* in, int B, int H, int W, int in_cs, int in_coff, int cin, const float* w_packed,
                 const float* bias, int bias_frame_stride, const float* res, int res_cs, int res_coff, float* out,
                 int out_cs, int out_coff, int cout, int ksize, int stride, int relu, int groups, int algo,
                 void* stream) {
  if (!in || !w_packed || !bias || !out || B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || groups <= 0)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_conv2d: bad arguments");
  const int bias_map = algo >= 0 ? (algo & ACRMI_CONV_BIAS_MAP) : 0;      // res = ONE map [Ho][Wo][res_cs] for all frames
  if (algo >= 0) algo &= ~ACRMI_CONV_BIAS_MAP;
  if (bias_map && !res) return fail(nullptr, ACRMI_EINVAL, "acrmi_conv2d: ACRMI_CONV_BIAS_MAP needs res (the map)");
  ConvArgs a{};
  a.in = in; a.w = w_packed; a.bias = bias; a.res = res; a.out = out;
  a.B = B; a.H = H; a.W = W;
  a.in_cs = in_cs; a.in_coff = in_coff; a.Cin = cin;
  a.out_cs = out_cs; a.out_coff = out_coff; a.Cout = cout;
  a.res_cs = res_cs; a.res_coff = res_coff;
  a.ks = ksize; a.stride = stride; a.relu = relu; a.groups = groups;
  a.bias_fstride = bias_frame_stride;
  a.algo = algo;
  a.res_bcast = bias_map ? 1 : 0;
  return conv_check_and_launch("acrmi_conv2d", a, stream);
}

int acrmi_conv2d_group(const acrmi_conv_problem* p, int n, void* stream) {
  if (!p || n < 1 || n > 2) return fail(nullptr, ACRMI_EINVAL, "acrmi_conv2d_group: 1 or 2 problems");
  if (n == 1)
    return acrmi_conv2d(p->in, p->B, p->H, p->W, p->in_cs, p->in_coff, p->cin, p->w_packed, p->bias, p->bias_frame_stride, p->res, p->res_cs,
                        p->res_coff, p->out, p->out_cs, p->out_coff, p->cout, p->ksize, p->stride, p->relu, p->groups, p->algo, stream);
  ConvArgs a[2];
  for (int i = 0; i < n; ++i) {
    const acrmi_conv_problem& q = p[i];
    if (!q.in || !q.w_packed || !q.bias || !q.out || q.B <= 0 || q.H <= 0 || q.W <= 0 || q.cin <= 0 || q.cout <= 0 || q.groups <= 0 ||
        q.algo < 0 || (q.algo & ACRMI_CONV_BIAS_MAP))
      return fail(nullptr, ACRMI_EINVAL, "acrmi_conv2d_group: bad arguments (problem %d)", i);
    a[i] = ConvArgs{};
    a[i].in = q.in; a[i].w = q.w_packed; a[i].bias = q.bias; a[i].res = q.res; a[i].out = q.out;
    a[i].B = q.B; a[i].H = q.H; a[i].W = q.W;
    a[i].in_cs = q.in_cs; a[i].in_coff = q.in_coff; a[i].Cin = q.cin;
    a[i].out_cs = q.out_cs; a[i].out_coff = q.out_coff; a[i].Cout = q.cout;
    a[i].res_cs = q.res_cs; a[i].res_coff = q.res_coff;
    a[i].ks = q.ksize; a[i].stride = q.stride; a[i].relu = q.relu; a[i].groups = q.groups;
    a[i].bias_fstride = q.bias_frame_stride;
    a[i].algo = q.algo;
    if (int r = conv_check("acrmi_conv2d_group", a[i])) return r;
  }
  if (!conv_can_group(a[0], a[1]))
    return fail(nullptr, ACRMI_EINVAL, "acrmi_conv2d_group: the two problems do not run on one kernel instantiation with a group form");
  hipError_t e = launch_conv_group(a, n, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "conv group launch: %s", hipGetErrorString(e));
}

size_t acrmi_conv2d_splitk_workspace(int B, int H, int W, int cout, int splits) {
  if (B <= 0 || H <= 0 || W <= 0 || cout <= 0 || splits < 2) return 0;
  const size_t cnt = (conv_splitk_counters(B, H, W, cout) * sizeof(unsigned) + 255) / 256 * 256;
  return cnt + conv_splitk_ws_floats(B, H, W, cout, splits) * sizeof(float);
}

int acrmi_conv2d_splitk(const float* in, int B, int H, int W, int in_cs, int in_coff, int cin_slice, int splits,
                        const float* w_packed, const float* bias, const float* res, int res_cs, int res_coff, float* out,
                        int out_cs, int out_coff, int cout, int relu, void* workspace, size_t workspace_bytes, void* stream) {
  if (!in || !w_packed || !bias || !out || !workspace || B <= 0 || H <= 0 || W <= 0 || cout <= 0)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_conv2d_splitk: bad arguments");
  if (workspace_bytes < acrmi_conv2d_splitk_workspace(B, H, W, cout, splits) || ((uintptr_t)workspace & 15))
    return fail(nullptr, ACRMI_EINVAL, "acrmi_conv2d_splitk: workspace too small (acrmi_conv2d_splitk_workspace) or unaligned");
  ConvArgs a{};      // (2..8 slices of >= 64 channels, a multiple of 32, each; Cout != 33: conv_rules.h)
  a.in = in; a.w = w_packed; a.bias = bias; a.res = res; a.out = out;
  a.B = B; a.H = H; a.W = W;
  a.in_cs = in_cs; a.in_coff = in_coff; a.Cin = cin_slice;
  a.out_cs = out_cs; a.out_coff = out_coff; a.Cout = cout;
  a.res_cs = res_cs; a.res_coff = res_coff;
  a.ks = 3; a.stride = 1; a.relu = relu; a.groups = splits;
  a.algo = 2;
  a.splitk = 1;
  a.split_cnt = reinterpret_cast<unsigned*>(workspace);
  a.split_ws = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) +
                                        (conv_splitk_counters(B, H, W, cout) * sizeof(unsigned) + 255) / 256 * 256);
  return conv_check_and_launch("acrmi_conv2d_splitk", a, stream);
}

int acrmi_conv2d_h16(const void* in, int B, int H, int W, int in_cs, int in_coff, int cin, const void* w_packed,
                     const float* bias, int bias_frame_stride, const void* res, int res_cs, int res_coff, void* out,
                     int out_cs, int out_coff, int cout, int ksize, int stride, int relu, int groups, int dtype,
                     int out_f32, void* stream) {
  if (!in || !w_packed || !bias || !out || B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || groups <= 0 ||
      (dtype != ACRMI_DT_F16 && dtype != ACRMI_DT_BF16))
    return fail(nullptr, ACRMI_EINVAL, "acrmi_conv2d_h16: bad arguments");
  ConvArgs a{};
  a.in = reinterpret_cast<const float*>(in); a.w = reinterpret_cast<const float*>(w_packed); a.bias = bias;
  a.res = reinterpret_cast<const float*>(res); a.out = reinterpret_cast<float*>(out);
  a.B = B; a.H = H; a.W = W;
  a.in_cs = in_cs; a.in_coff = in_coff; a.Cin = cin;
  a.out_cs = out_cs; a.out_coff = out_coff; a.Cout = cout;
  a.res_cs = res_cs; a.res_coff = res_coff;
  a.ks = ksize; a.stride = stride; a.relu = relu; a.groups = groups;
  a.bias_fstride = bias_frame_stride;
  a.algo = 0; a.dtype = dtype; a.out_f32 = out_f32 ? 1 : 0;
  return conv_check_and_launch("acrmi_conv2d_h16", a, stream);
}

// ---- input pre-processing (csrc/preprocess.hip, csrc/nv12.hip, csrc/roi_plan.h; DESIGN.md "NV12 input", "Regions of interest")
}  // extern "C"

namespace {

// (cy, cub, cug, cvg, cvr, y_off) by ACRMI_NV12_*: OpenCV's literal ITUR_BT_601 integers, then round(x * 2^20) of the
// textbook Kr / Kb forms (limited range: 255/219 luma and 255/224 chroma gains; full range: none)
const int32_t kNv12Matrix[5][6] = {
    {1220542, 2116026, -409993, -852492, 1673527, 16},     // cv601
    {1220945, 2115221, -410793, -852458, 1673555, 16},     // bt601
    {1048576, 1858077, -360853, -748826, 1470104, 0},      // bt601-full
    {1220945, 2215014, -223607, -558796, 1879825, 16},     // bt709
    {1048576, 1945738, -196424, -490864, 1651297, 0},      // bt709-full
};

// Null row = cv601.  Refused: y_off outside 0..255, or a row whose int32 sums could overflow:
// 255 |cy| + 128 max(|cub|, |cvr|, |cug| + |cvg|) + 2^19 >= 2^31.
int nv12_coef(const char* who, const int32_t* coef6, Nv12Coef& k) {
  const int32_t* c = coef6 ? coef6 : kNv12Matrix[0];
  auto mag = [](int32_t v) { return v < 0 ? -(long long)v : (long long)v; };
  long long m = mag(c[1]);
  if (mag(c[4]) > m) m = mag(c[4]);
  if (mag(c[2]) + mag(c[3]) > m) m = mag(c[2]) + mag(c[3]);
  if (c[5] < 0 || c[5] > 255)
    return fail(nullptr, ACRMI_EINVAL, "%s: y_off %d outside 0..255", who, (int)c[5]);
  if (255 * mag(c[0]) + 128 * m + (1LL << 19) >= (1LL << 31))
    return fail(nullptr, ACRMI_EINVAL, "%s: coefficient row (%d, %d, %d, %d, %d) could overflow the int32 sums", who, (int)c[0],
                (int)c[1], (int)c[2], (int)c[3], (int)c[4]);
  k.cy = c[0]; k.cub = c[1]; k.cug = c[2]; k.cvg = c[3]; k.cvr = c[4]; k.y_off = c[5];
  return ACRMI_OK;
}

int nv12_check_frames(const char* who, const acrmi_nv12_frame* fr, int n) {
  for (int i = 0; i < n; ++i) {
    const acrmi_nv12_frame& f = fr[i];
    if (!f.y_dev || !f.uv_dev) return fail(nullptr, ACRMI_EINVAL, "%s: frame %d: null plane", who, i);
    if (f.H < 2 || f.W < 2 || (f.H & 1) || (f.W & 1))
      return fail(nullptr, ACRMI_EINVAL, "%s: frame %d: size %d x %d (H x W) must be even and >= 2", who, i, f.H, f.W);
    if (f.y_pitch < f.W || f.uv_pitch < f.W)
      return fail(nullptr, ACRMI_EINVAL, "%s: frame %d: pitch (y %d, uv %d) below the width %d", who, i, f.y_pitch, f.uv_pitch, f.W);
  }
  return ACRMI_OK;
}

// Regions of interest: every region's frame index and window, before anything is queued; sizes(frame, H, W) says how large a
// frame is.  plans[i] = the clamped window, pad and crop of region i (csrc/roi_plan.h).
template <class Sizes>
int roi_plans(const char* who, const acrmi_roi* rois, int n, int n_frames, const Sizes& sizes, std::vector<RoiPlan>& plans) {
  plans.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    const acrmi_roi& q = rois[i];
    if (q.frame < 0 || q.frame >= n_frames)
      return fail(nullptr, ACRMI_EINVAL, "%s: region %d: frame index %d outside [0, %d)", who, i, (int)q.frame, n_frames);
    int H, W;
    sizes(q.frame, H, W);
    if (!roi_plan(H, W, q.l, q.t, q.r, q.b, &plans[(size_t)i]))
      return fail(nullptr, ACRMI_EINVAL, "%s: region %d: box (l %d, t %d, r %d, b %d) leaves no pixel of frame %d (%d x %d, H x W)",
                  who, i, (int)q.l, (int)q.t, (int)q.r, (int)q.b, (int)q.frame, H, W);
  }
  return ACRMI_OK;
}

// The plan of the whole frame, the window (0, 0, W, H): what the frame entry points hand to the window path.  The sizes have
// been checked, so every frame has a plan.
template <class Frame>
std::vector<RoiPlan> full_frame_plans(const Frame* frames, int n) {
  std::vector<RoiPlan> plans((size_t)n);
  for (int i = 0; i < n; ++i)      // (void): H, W > 0 has been checked, and the whole frame of such a size is never empty
    (void)roi_plan(frames[i].H, frames[i].W, 0, 0, frames[i].W, frames[i].H, &plans[(size_t)i]);
  return plans;
}

// The window path, one helper per pixel format: output image i is the window plans[i] of frames[frame_of(i)] and gets the
// `offsets` row of its plan.  ROIS_PER_LAUNCH records per launch.  Everything has been validated by the caller.
template <class FrameOf>
int preprocess_windows_bgr(const char* what, const acrmi_frame* frames, const std::vector<RoiPlan>& plans, const FrameOf& frame_of,
                           uint8_t* out_rgb_dev, float* offsets_host, void* stream) {
  const int n = (int)plans.size();
  for (int i0 = 0; i0 < n; i0 += ROIS_PER_LAUNCH) {
    const int m = n - i0 < ROIS_PER_LAUNCH ? n - i0 : ROIS_PER_LAUNCH;
    RoiBgrBatch rb{};
    for (int i = 0; i < m; ++i) {
      const acrmi_frame& fr = frames[frame_of(i0 + i)];
      const RoiPlan& p = plans[(size_t)(i0 + i)];
      rb.r[i].pitch = (size_t)fr.W * 3;
      rb.r[i].src = fr.bgr_dev + (size_t)p.t * rb.r[i].pitch + (size_t)p.l * 3;
      rb.r[i].h = p.b - p.t; rb.r[i].w = p.r - p.l;
      if (offsets_host) roi_offsets_row(p, offsets_host + (size_t)(i0 + i) * 10);
    }
    hipError_t e = launch_preprocess_rois(rb, m, 512, out_rgb_dev + (size_t)i0 * 512 * 512 * 3, (hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, ACRMI_EHIP, "%s: %s", what, hipGetErrorString(e));
  }
  return ACRMI_OK;
}

template <class FrameOf>
int preprocess_windows_nv12(const char* what, const acrmi_nv12_frame* frames, const std::vector<RoiPlan>& plans,
                            const FrameOf& frame_of, const Nv12Coef& k, uint8_t* out_rgb_dev, float* offsets_host, void* stream) {
  const int n = (int)plans.size();
  for (int i0 = 0; i0 < n; i0 += ROIS_PER_LAUNCH) {
    const int m = n - i0 < ROIS_PER_LAUNCH ? n - i0 : ROIS_PER_LAUNCH;
    RoiNv12Batch rb{};
    for (int i = 0; i < m; ++i) {
      const acrmi_nv12_frame& fr = frames[frame_of(i0 + i)];
      const RoiPlan& p = plans[(size_t)(i0 + i)];
      rb.r[i].y = fr.y_dev; rb.r[i].uv = fr.uv_dev; rb.r[i].y_pitch = fr.y_pitch; rb.r[i].uv_pitch = fr.uv_pitch;
      rb.r[i].l = p.l; rb.r[i].t = p.t; rb.r[i].h = p.b - p.t; rb.r[i].w = p.r - p.l;
      if (offsets_host) roi_offsets_row(p, offsets_host + (size_t)(i0 + i) * 10);
    }
    hipError_t e = launch_preprocess_rois_nv12(rb, k, m, 512, out_rgb_dev + (size_t)i0 * 512 * 512 * 3, (hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, ACRMI_EHIP, "%s: %s", what, hipGetErrorString(e));
  }
  return ACRMI_OK;
}

// The window path with the boxes in device memory (DESIGN.md "Tracking on the device"): the loop of the helpers above, but a
// record holds the frame and the index of its region's box, and the kernel makes the plan.  Nothing is copied, awaited or
// allocated.  Everything has been validated by the caller.
template <class FrameOf>
int preprocess_windows_bgr_dev(const char* what, const acrmi_frame* frames, const FrameOf& frame_of, const int32_t* boxes_dev, int n,
                               uint8_t* out_rgb_dev, float* offsets_dev, int32_t* status_dev, void* stream) {
  for (int i0 = 0; i0 < n; i0 += ROIS_PER_LAUNCH) {
    const int m = n - i0 < ROIS_PER_LAUNCH ? n - i0 : ROIS_PER_LAUNCH;
    RoiBgrDevBatch rb{};
    for (int i = 0; i < m; ++i) {
      const acrmi_frame& fr = frames[frame_of(i0 + i)];
      rb.r[i].frame = fr.bgr_dev; rb.r[i].H = fr.H; rb.r[i].W = fr.W; rb.r[i].box = i0 + i;
    }
    hipError_t e = launch_preprocess_rois_dev(rb, boxes_dev, m, 512, out_rgb_dev + (size_t)i0 * 512 * 512 * 3, offsets_dev, status_dev,
                                              (hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, ACRMI_EHIP, "%s: %s", what, hipGetErrorString(e));
  }
  return ACRMI_OK;
}

template <class FrameOf>
int preprocess_windows_nv12_dev(const char* what, const acrmi_nv12_frame* frames, const FrameOf& frame_of, const Nv12Coef& k,
                                const int32_t* boxes_dev, int n, uint8_t* out_rgb_dev, float* offsets_dev, int32_t* status_dev,
                                void* stream) {
  for (int i0 = 0; i0 < n; i0 += ROIS_PER_LAUNCH) {
    const int m = n - i0 < ROIS_PER_LAUNCH ? n - i0 : ROIS_PER_LAUNCH;
    RoiNv12DevBatch rb{};
    for (int i = 0; i < m; ++i) {
      const acrmi_nv12_frame& fr = frames[frame_of(i0 + i)];
      rb.r[i].y = fr.y_dev; rb.r[i].uv = fr.uv_dev; rb.r[i].y_pitch = fr.y_pitch; rb.r[i].uv_pitch = fr.uv_pitch;
      rb.r[i].H = fr.H; rb.r[i].W = fr.W; rb.r[i].box = i0 + i;
    }
    hipError_t e = launch_preprocess_rois_nv12_dev(rb, k, boxes_dev, m, 512, out_rgb_dev + (size_t)i0 * 512 * 512 * 3, offsets_dev,
                                                   status_dev, (hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, ACRMI_EHIP, "%s: %s", what, hipGetErrorString(e));
  }
  return ACRMI_OK;
}

// the frame of every region, before anything is queued: roi_frame_host[i] in [0, n_frames), or - NULL - frame i of n frames
int roi_frames_check(const char* who, const int32_t* roi_frame_host, int n, int n_frames) {
  if (!roi_frame_host) {
    if (n != n_frames)
      return fail(nullptr, ACRMI_EINVAL, "%s: %d regions of %d frames: without roi_frame_host there is one region per frame", who, n,
                  n_frames);
    return ACRMI_OK;
  }
  for (int i = 0; i < n; ++i)
    if (roi_frame_host[i] < 0 || roi_frame_host[i] >= n_frames)
      return fail(nullptr, ACRMI_EINVAL, "%s: region %d: frame index %d outside [0, %d)", who, i, (int)roi_frame_host[i], n_frames);
  return ACRMI_OK;
}

bool track_args_ok(double scale, int min_size) { return scale > 0 && scale <= DBL_MAX && min_size >= 1; }

// NV12 output (csrc/nv12_out_plan.h).  Null row = cv601; a refused row names its reason.
int nv12_out_coef(const char* who, const int32_t* coef10, Nv12OutCoef& k) {
  const int32_t* c = coef10 ? coef10 : kNv12OutMatrix[0];
  const char* why = nullptr;
  if (!nv12_out_row(c, &k, &why))
    return fail(nullptr, ACRMI_EINVAL, "%s: output row (%d, %d, %d, %d, %d, %d, %d, %d, %d, y_off %d): %s", who, (int)c[0], (int)c[1],
                (int)c[2], (int)c[3], (int)c[4], (int)c[5], (int)c[6], (int)c[7], (int)c[8], (int)c[9], why);
  return ACRMI_OK;
}

int nv12_check_surfaces(const char* who, const acrmi_nv12_surface* su, int n) {
  for (int i = 0; i < n; ++i) {
    const acrmi_nv12_surface& f = su[i];
    if (!f.y_dev || !f.uv_dev) return fail(nullptr, ACRMI_EINVAL, "%s: surface %d: null plane", who, i);
    if (f.H < 2 || f.W < 2 || (f.H & 1) || (f.W & 1))
      return fail(nullptr, ACRMI_EINVAL, "%s: surface %d: size %d x %d (H x W) must be even and >= 2", who, i, f.H, f.W);
    if (f.y_pitch < f.W || f.uv_pitch < f.W)
      return fail(nullptr, ACRMI_EINVAL, "%s: surface %d: pitch (y %d, uv %d) below the width %d", who, i, f.y_pitch, f.uv_pitch, f.W);
  }
  return ACRMI_OK;
}

}  // namespace

extern "C" {

int acrmi_nv12_matrix(int which, int32_t coef6[6]) {
  if (!coef6 || which < 0 || which > ACRMI_NV12_BT709_FULL)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_nv12_matrix: bad arguments (matrix %d)", which);
  for (int i = 0; i < 6; ++i) coef6[i] = kNv12Matrix[which][i];
  return ACRMI_OK;
}

int acrmi_preprocess(const uint8_t* bgr_dev, int n, int H, int W, uint8_t* out_rgb_dev, float* offsets_host,
                     void* stream) {
  if (!bgr_dev || !out_rgb_dev || n <= 0 || H <= 0 || W <= 0)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_preprocess: bad arguments");
  if (offsets_host) {     // the reference's `offsets` row (acr/utils.py:1276-1313): that of the whole frame's plan
    RoiPlan p{};
    (void)roi_plan(H, W, 0, 0, W, H, &p);      // H, W > 0: never empty
    for (int i = 0; i < n; ++i) roi_offsets_row(p, offsets_host + (size_t)i * 10);
  }
  hipError_t e = launch_preprocess(bgr_dev, n, H, W, 512, out_rgb_dev, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "preprocess: %s", hipGetErrorString(e));
}

int acrmi_preprocess_frames(const acrmi_frame* frames_host, int n, uint8_t* out_rgb_dev, float* offsets_host, void* stream) {
  if (!frames_host || !out_rgb_dev || n <= 0) return fail(nullptr, ACRMI_EINVAL, "acrmi_preprocess_frames: bad arguments");
  for (int i = 0; i < n; ++i)
    if (!frames_host[i].bgr_dev || frames_host[i].H <= 0 || frames_host[i].W <= 0)
      return fail(nullptr, ACRMI_EINVAL, "acrmi_preprocess_frames: frame %d: null pointer or empty size (%d x %d)", i,
                  frames_host[i].H, frames_host[i].W);
  return preprocess_windows_bgr("preprocess_frames", frames_host, full_frame_plans(frames_host, n), [](int i) { return i; },
                                out_rgb_dev, offsets_host, stream);
}

int acrmi_preprocess_nv12(const acrmi_nv12_frame* frames_host, int n, const int32_t* coef6_host, uint8_t* out_rgb_dev,
                          float* offsets_host, void* stream) {
  if (!frames_host || !out_rgb_dev || n <= 0) return fail(nullptr, ACRMI_EINVAL, "acrmi_preprocess_nv12: bad arguments");
  Nv12Coef k{};
  int rc = nv12_coef("acrmi_preprocess_nv12", coef6_host, k);
  if (rc == ACRMI_OK) rc = nv12_check_frames("acrmi_preprocess_nv12", frames_host, n);
  if (rc != ACRMI_OK) return rc;
  return preprocess_windows_nv12("preprocess_nv12", frames_host, full_frame_plans(frames_host, n), [](int i) { return i; }, k,
                                 out_rgb_dev, offsets_host, stream);
}

int acrmi_nv12_to_rgb(const acrmi_nv12_frame* frames_host, int n, const int32_t* coef6_host, int bgr,
                      uint8_t* const* dst_dev_host, void* stream) {
  if (!frames_host || !dst_dev_host || n <= 0) return fail(nullptr, ACRMI_EINVAL, "acrmi_nv12_to_rgb: bad arguments");
  Nv12Coef k{};
  int rc = nv12_coef("acrmi_nv12_to_rgb", coef6_host, k);
  if (rc == ACRMI_OK) rc = nv12_check_frames("acrmi_nv12_to_rgb", frames_host, n);
  if (rc != ACRMI_OK) return rc;
  for (int i = 0; i < n; ++i)
    if (!dst_dev_host[i]) return fail(nullptr, ACRMI_EINVAL, "acrmi_nv12_to_rgb: frame %d: null destination", i);
  for (int i0 = 0; i0 < n; i0 += NV12_FRAMES_PER_LAUNCH) {
    const int m = n - i0 < NV12_FRAMES_PER_LAUNCH ? n - i0 : NV12_FRAMES_PER_LAUNCH;
    Nv12DstBatch pb{};
    for (int i = 0; i < m; ++i) {
      const acrmi_nv12_frame& fr = frames_host[i0 + i];
      pb.f[i].y = fr.y_dev; pb.f[i].uv = fr.uv_dev; pb.f[i].dst = dst_dev_host[i0 + i]; pb.f[i].H = fr.H; pb.f[i].W = fr.W;
      pb.f[i].y_pitch = fr.y_pitch; pb.f[i].uv_pitch = fr.uv_pitch;
    }
    hipError_t e = launch_nv12_to_rgb(pb, k, m, bgr ? 1 : 0, (hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, ACRMI_EHIP, "nv12_to_rgb: %s", hipGetErrorString(e));
  }
  return ACRMI_OK;
}

// ---- NV12 output (csrc/nv12_out.hip, csrc/nv12_out_plan.h; DESIGN.md "NV12 output") -----------------------------------------
int acrmi_nv12_out_matrix(int which, int32_t coef10[10]) {
  if (!coef10 || which < 0 || which > ACRMI_NV12_BT709_FULL)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_nv12_out_matrix: bad arguments (matrix %d)", which);
  for (int i = 0; i < 10; ++i) coef10[i] = kNv12OutMatrix[which][i];
  return ACRMI_OK;
}

int acrmi_rgb_to_nv12(const uint8_t* const* src_dev_host, const acrmi_nv12_surface* surfaces_host, int n,
                      const int32_t* coef10_host, int bgr, void* stream) {
  if (!src_dev_host || !surfaces_host || n <= 0) return fail(nullptr, ACRMI_EINVAL, "acrmi_rgb_to_nv12: bad arguments");
  Nv12OutCoef k{};
  int rc = nv12_out_coef("acrmi_rgb_to_nv12", coef10_host, k);
  if (rc == ACRMI_OK) rc = nv12_check_surfaces("acrmi_rgb_to_nv12", surfaces_host, n);
  if (rc != ACRMI_OK) return rc;
  for (int i = 0; i < n; ++i)
    if (!src_dev_host[i]) return fail(nullptr, ACRMI_EINVAL, "acrmi_rgb_to_nv12: frame %d: null source", i);
  for (int i0 = 0; i0 < n; i0 += NV12_FRAMES_PER_LAUNCH) {
    const int m = n - i0 < NV12_FRAMES_PER_LAUNCH ? n - i0 : NV12_FRAMES_PER_LAUNCH;
    Nv12OutBatch pb{};
    for (int i = 0; i < m; ++i) {
      const acrmi_nv12_surface& su = surfaces_host[i0 + i];
      pb.f[i].src = src_dev_host[i0 + i]; pb.f[i].y = su.y_dev; pb.f[i].uv = su.uv_dev; pb.f[i].H = su.H; pb.f[i].W = su.W;
      pb.f[i].y_pitch = su.y_pitch; pb.f[i].uv_pitch = su.uv_pitch;
    }
    hipError_t e = launch_rgb_to_nv12(pb, k, m, bgr ? 1 : 0, (hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, ACRMI_EHIP, "rgb_to_nv12: %s", hipGetErrorString(e));
  }
  return ACRMI_OK;
}

int acrmi_nv12_compose(const acrmi_nv12_frame* src_frames_host, const uint8_t* const* drawn_dev_host,
                       const acrmi_nv12_surface* out_surfaces_host, int n, const int32_t* coef6_host, const int32_t* coef10_host,
                       int bgr, void* stream) {
  if (!src_frames_host || !drawn_dev_host || !out_surfaces_host || n <= 0)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_nv12_compose: bad arguments");
  Nv12Coef k6{};
  Nv12OutCoef k10{};
  int rc = nv12_coef("acrmi_nv12_compose", coef6_host, k6);
  if (rc == ACRMI_OK) rc = nv12_out_coef("acrmi_nv12_compose", coef10_host, k10);
  if (rc == ACRMI_OK) rc = nv12_check_frames("acrmi_nv12_compose", src_frames_host, n);
  if (rc == ACRMI_OK) rc = nv12_check_surfaces("acrmi_nv12_compose", out_surfaces_host, n);
  if (rc != ACRMI_OK) return rc;
  for (int i = 0; i < n; ++i) {
    if (!drawn_dev_host[i]) return fail(nullptr, ACRMI_EINVAL, "acrmi_nv12_compose: frame %d: null drawn frame", i);
    if (out_surfaces_host[i].H != src_frames_host[i].H || out_surfaces_host[i].W != src_frames_host[i].W)
      return fail(nullptr, ACRMI_EINVAL, "acrmi_nv12_compose: frame %d: the output surface is %d x %d, the source %d x %d (H x W)", i,
                  out_surfaces_host[i].H, out_surfaces_host[i].W, src_frames_host[i].H, src_frames_host[i].W);
  }
  for (int i0 = 0; i0 < n; i0 += NV12_COMPOSE_FRAMES_PER_LAUNCH) {
    const int m = n - i0 < NV12_COMPOSE_FRAMES_PER_LAUNCH ? n - i0 : NV12_COMPOSE_FRAMES_PER_LAUNCH;
    Nv12ComposeBatch pb{};
    for (int i = 0; i < m; ++i) {
      const acrmi_nv12_frame& fr = src_frames_host[i0 + i];
      const acrmi_nv12_surface& su = out_surfaces_host[i0 + i];
      Nv12ComposeFrame& c = pb.f[i];
      c.src_y = fr.y_dev; c.src_uv = fr.uv_dev; c.drawn = drawn_dev_host[i0 + i]; c.y = su.y_dev; c.uv = su.uv_dev;
      c.H = fr.H; c.W = fr.W; c.src_y_pitch = fr.y_pitch; c.src_uv_pitch = fr.uv_pitch; c.y_pitch = su.y_pitch; c.uv_pitch = su.uv_pitch;
    }
    hipError_t e = launch_nv12_compose(pb, k6, k10, m, bgr ? 1 : 0, (hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, ACRMI_EHIP, "nv12_compose: %s", hipGetErrorString(e));
  }
  return ACRMI_OK;
}

// ---- regions of interest (DESIGN.md "Regions of interest") ----------------------------------------------------------
int acrmi_roi_offsets(int H, int W, const acrmi_roi* roi, int32_t window_ltrb[4], float offsets10[10]) {
  if (!roi || H <= 0 || W <= 0) return fail(nullptr, ACRMI_EINVAL, "acrmi_roi_offsets: bad arguments");
  RoiPlan p;
  if (!roi_plan(H, W, roi->l, roi->t, roi->r, roi->b, &p))
    return fail(nullptr, ACRMI_EINVAL, "acrmi_roi_offsets: box (l %d, t %d, r %d, b %d) leaves no pixel of a %d x %d (H x W) frame",
                (int)roi->l, (int)roi->t, (int)roi->r, (int)roi->b, H, W);
  if (window_ltrb) { window_ltrb[0] = p.l; window_ltrb[1] = p.t; window_ltrb[2] = p.r; window_ltrb[3] = p.b; }
  if (offsets10) roi_offsets_row(p, offsets10);
  return ACRMI_OK;
}

int acrmi_preprocess_rois(const acrmi_frame* frames_host, int n_frames, const acrmi_roi* rois_host, int n,
                          uint8_t* out_rgb_dev, float* offsets_host, void* stream) {
  if (!frames_host || !rois_host || !out_rgb_dev || n <= 0 || n_frames <= 0)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_preprocess_rois: bad arguments");
  for (int i = 0; i < n_frames; ++i)
    if (!frames_host[i].bgr_dev || frames_host[i].H <= 0 || frames_host[i].W <= 0)
      return fail(nullptr, ACRMI_EINVAL, "acrmi_preprocess_rois: frame %d: null pointer or empty size (%d x %d)", i,
                  frames_host[i].H, frames_host[i].W);
  std::vector<RoiPlan> plans;
  int rc = roi_plans("acrmi_preprocess_rois", rois_host, n, n_frames,
                     [&](int f, int& H, int& W) { H = frames_host[f].H; W = frames_host[f].W; }, plans);
  if (rc != ACRMI_OK) return rc;
  return preprocess_windows_bgr("preprocess_rois", frames_host, plans, [&](int i) { return rois_host[i].frame; }, out_rgb_dev,
                                offsets_host, stream);
}

int acrmi_preprocess_rois_nv12(const acrmi_nv12_frame* frames_host, int n_frames, const acrmi_roi* rois_host, int n,
                               const int32_t* coef6_host, uint8_t* out_rgb_dev, float* offsets_host, void* stream) {
  if (!frames_host || !rois_host || !out_rgb_dev || n <= 0 || n_frames <= 0)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_preprocess_rois_nv12: bad arguments");
  Nv12Coef k{};
  int rc = nv12_coef("acrmi_preprocess_rois_nv12", coef6_host, k);
  if (rc == ACRMI_OK) rc = nv12_check_frames("acrmi_preprocess_rois_nv12", frames_host, n_frames);
  std::vector<RoiPlan> plans;
  if (rc == ACRMI_OK)
    rc = roi_plans("acrmi_preprocess_rois_nv12", rois_host, n, n_frames,
                   [&](int f, int& H, int& W) { H = frames_host[f].H; W = frames_host[f].W; }, plans);
  if (rc != ACRMI_OK) return rc;
  return preprocess_windows_nv12("preprocess_rois_nv12", frames_host, plans, [&](int i) { return rois_host[i].frame; }, k,
                                 out_rgb_dev, offsets_host, stream);
}

// ---- tracking on the device (csrc/track_plan.h, csrc/track.hip; DESIGN.md "Tracking on the device") ------------------
int acrmi_track_box(const float* pts_host, int n_pts, int H, int W, double scale, int min_size, int32_t box_ltrb[4]) {
  if (!box_ltrb || n_pts < 0 || (n_pts > 0 && !pts_host) || H <= 0 || W <= 0)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_track_box: bad arguments");
  if (!track_args_ok(scale, min_size))
    return fail(nullptr, ACRMI_EINVAL, "acrmi_track_box: scale %g must be finite and > 0, min_size %d must be >= 1", scale, min_size);
  track_box_of_points(pts_host, n_pts, H, W, scale, min_size, box_ltrb);
  return ACRMI_OK;
}

int acrmi_assoc_step(int max_hand, int gate, int max_miss, const float* rows_host, int row_stride, int32_t* state,
                     int32_t* track_ids, int32_t* perm, int32_t* born) {
  static_assert(ACRMI_ASSOC_STATE == ASSOC_STATE_INTS, "the header states the size of AssocSide");
  if (!rows_host || !state || !track_ids || !perm || row_stride < 2)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_assoc_step: bad arguments");
  if (!assoc_params_ok(max_hand, gate, max_miss))
    return fail(nullptr, ACRMI_EINVAL, "acrmi_assoc_step: max_hand %d outside 1..%d, gate %d outside 0..%d or max_miss %d < -1",
                max_hand, ASSOC_MAX_HAND, gate, ASSOC_GATE_ANY, max_miss);
  AssocSide s;
  memcpy(&s, state, sizeof s);
  AssocStep o;
  assoc_step(s, max_hand, gate, max_miss, rows_host, row_stride, o);
  memcpy(state, &s, sizeof s);
  for (int k = 0; k < max_hand; ++k) {
    track_ids[k] = o.track_id[k];
    perm[k] = o.perm[k];
    if (born) born[k] = o.born[k];
  }
  return ACRMI_OK;
}

int acrmi_track_boxes(const float* pj2d_org_dev, const float* slots_dev, const int32_t* frame_hw_dev, int n, double scale,
                      int min_size, int32_t* boxes_dev, void* stream) {
  if (!pj2d_org_dev || !slots_dev || !frame_hw_dev || !boxes_dev || n <= 0)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_track_boxes: bad arguments");
  if (!track_args_ok(scale, min_size))
    return fail(nullptr, ACRMI_EINVAL, "acrmi_track_boxes: scale %g must be finite and > 0, min_size %d must be >= 1", scale, min_size);
  hipError_t e = launch_track_boxes(pj2d_org_dev, slots_dev, frame_hw_dev, n, ACRMI_SLOT, ACRMI_SLOT_FLAG, scale, min_size, boxes_dev,
                                    (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "track_boxes: %s", hipGetErrorString(e));
}

int acrmi_preprocess_rois_dev(const acrmi_frame* frames_host, int n_frames, const int32_t* roi_frame_host, const int32_t* boxes_dev,
                              int n, uint8_t* out_rgb_dev, float* offsets_dev, int32_t* status_dev, void* stream) {
  if (!frames_host || !boxes_dev || !out_rgb_dev || n <= 0 || n_frames <= 0)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_preprocess_rois_dev: bad arguments");
  for (int i = 0; i < n_frames; ++i)
    if (!frames_host[i].bgr_dev || frames_host[i].H <= 0 || frames_host[i].W <= 0)
      return fail(nullptr, ACRMI_EINVAL, "acrmi_preprocess_rois_dev: frame %d: null pointer or empty size (%d x %d)", i,
                  frames_host[i].H, frames_host[i].W);
  int rc = roi_frames_check("acrmi_preprocess_rois_dev", roi_frame_host, n, n_frames);
  if (rc != ACRMI_OK) return rc;
  return preprocess_windows_bgr_dev("preprocess_rois_dev", frames_host, [&](int i) { return roi_frame_host ? roi_frame_host[i] : i; },
                                    boxes_dev, n, out_rgb_dev, offsets_dev, status_dev, stream);
}

int acrmi_preprocess_rois_nv12_dev(const acrmi_nv12_frame* frames_host, int n_frames, const int32_t* roi_frame_host,
                                   const int32_t* boxes_dev, int n, const int32_t* coef6_host, uint8_t* out_rgb_dev,
                                   float* offsets_dev, int32_t* status_dev, void* stream) {
  if (!frames_host || !boxes_dev || !out_rgb_dev || n <= 0 || n_frames <= 0)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_preprocess_rois_nv12_dev: bad arguments");
  Nv12Coef k{};
  int rc = nv12_coef("acrmi_preprocess_rois_nv12_dev", coef6_host, k);
  if (rc == ACRMI_OK) rc = nv12_check_frames("acrmi_preprocess_rois_nv12_dev", frames_host, n_frames);
  if (rc == ACRMI_OK) rc = roi_frames_check("acrmi_preprocess_rois_nv12_dev", roi_frame_host, n, n_frames);
  if (rc != ACRMI_OK) return rc;
  return preprocess_windows_nv12_dev("preprocess_rois_nv12_dev", frames_host,
                                     [&](int i) { return roi_frame_host ? roi_frame_host[i] : i; }, k, boxes_dev, n, out_rgb_dev,
                                     offsets_dev, status_dev, stream);
}

int acrmi_u8norm(const uint8_t* img, int n_pixels, float* out, void* stream) {
  if (!img || !out || n_pixels <= 0) return fail(nullptr, ACRMI_EINVAL, "acrmi_u8norm: bad arguments");
  hipError_t e = launch_u8norm(img, n_pixels, out, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "u8norm: %s", hipGetErrorString(e));
}

int acrmi_bilinear2x(const float* in, int B, int H, int W, int in_cs, int C, float* out, int out_cs, void* stream) {
  if (!in || !out || B <= 0 || H < 2 || W < 2 || C % 4 || in_cs % 4 || out_cs % 4)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_bilinear2x: bad arguments");
  hipError_t e = launch_bilinear2x(in, B, H, W, in_cs, 0, C, out, out_cs, 0, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "bilinear2x: %s", hipGetErrorString(e));
}

int acrmi_fuse_sum(int nterms, const float* const* terms, const int* term_cs, const int* term_shift, int B, int H,
                   int W, int C, float* out, int out_cs, int relu, void* stream) {
  if (nterms < 1 || nterms > 4 || !terms || !term_cs || !term_shift || !out || C % 4)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_fuse_sum: bad arguments");
  FuseArgs f{};
  f.nterms = nterms; f.B = B; f.H = H; f.W = W; f.C = C; f.out = out; f.out_cs = out_cs; f.relu = relu;
  for (int t = 0; t < nterms; ++t) { f.term[t] = terms[t]; f.cs[t] = term_cs[t]; f.shift[t] = term_shift[t]; }
  hipError_t e = launch_fuse_sum(f, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "fuse_sum: %s", hipGetErrorString(e));
}

int acrmi_stem_conv(const uint8_t* img, int B, int H, int W, const float* w_packed, const float* bias, float* out,
                    int out_cs, int out_coff, int relu, void* stream) {
  if (!img || !w_packed || !bias || !out || B <= 0 || !stem_shape_ok(H, W, out_cs, out_coff))
    return fail(nullptr, ACRMI_EINVAL, "acrmi_stem_conv: bad arguments (H %% 16, W %% 128, 64 channels inside out_cs)");
  hipError_t e = launch_stem(img, B, H, W, w_packed, bias, out, out_cs, out_coff, relu, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "stem: %s", hipGetErrorString(e));
}

size_t acrmi_attpool_ws_floats(int B, int C) { return B > 0 && C > 0 ? attpool_ws_floats(B, C) : 0; }

int acrmi_attpool(const float* segm, int segm_cs, const float* feat, int feat_cs, int C, int B, float* ws,
                  float* pooled, void* stream) {
  if (!segm || !feat || !ws || !pooled || B <= 0) return fail(nullptr, ACRMI_EINVAL, "acrmi_attpool: bad arguments");
  hipError_t e = launch_attpool(segm, segm_cs, feat, feat_cs, C, B, 128, 128, ws, pooled, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "attpool: %s", hipGetErrorString(e));
}

int acrmi_parebias(const float* pooled, int C, int part0, const float* lc_w, const float* lin_w, const float* lin_b,
                   const float* mix_wp, const float* mix_b, int B, float* out, int out_stride, void* stream) {
  if (!pooled || !lc_w || !lin_w || !lin_b || !mix_wp || !mix_b || !out || B <= 0 || (C != 256 && C != 320) ||
      (part0 != 0 && part0 != 16) || out_stride < 109 || out_stride > 256)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_parebias: bad arguments");
  PareArgs a{};
  a.pooled = pooled; a.lc_w = lc_w; a.lin_w = lin_w; a.lin_b = lin_b; a.mix_wp = mix_wp; a.mix_b = mix_b;
  a.out = out; a.B = B; a.C = C; a.part0 = part0; a.out_stride = out_stride;
  hipError_t e = launch_parebias(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "parebias: %s", hipGetErrorString(e));
}

int acrmi_cam_trans(const float* joints_dev, const float* pj2d_dev, int n, float focal_length, float img_size,
                    float* trans_dev, void* stream) {
  if (n < 0 || (n > 0 && (!joints_dev || !pj2d_dev || !trans_dev)) || !(focal_length > 0.f) || !(img_size > 0.f))
    return fail(nullptr, ACRMI_EINVAL, "acrmi_cam_trans: bad arguments");
  hipError_t e = launch_cam_trans(joints_dev, pj2d_dev, n, focal_length, img_size, trans_dev, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "cam_trans: %s", hipGetErrorString(e));
}

// ---- mesh overlay (csrc/render.hip) ----
int acrmi_mesh_topology(const int32_t* faces_host, int n_faces, int n_verts, int32_t* blob_host, int n_ints) {
  if (n_faces <= 0 || n_verts <= 0) return fail(nullptr, ACRMI_EINVAL, "acrmi_mesh_topology: bad arguments");
  const long long need = mesh_topology_ints(n_faces, n_verts);
  if (need > 0x7fffffffll) return fail(nullptr, ACRMI_EINVAL, "acrmi_mesh_topology: mesh too large");
  if (!blob_host) return (int)need;      // size query
  if (!faces_host || n_ints < need) return fail(nullptr, ACRMI_EINVAL, "acrmi_mesh_topology: bad arguments (%lld ints needed)", need);
  if (!build_mesh_topology(faces_host, n_faces, n_verts, blob_host))
    return fail(nullptr, ACRMI_EINVAL, "acrmi_mesh_topology: a face names a vertex outside [0, %d)", n_verts);
  return (int)need;
}

size_t acrmi_render_workspace(int n_meshes, int n_faces) {
  return n_meshes > 0 && n_faces > 0 ? render_workspace_bytes(n_meshes, n_faces) : 0;
}

static int rasterize(const char* who, bool per_mesh, const float* verts_dev, const float* trans_dev, int n_meshes, int n_verts,
                     int n_faces, const int32_t* topo_dev, const int32_t* topo2_dev, const int32_t* mesh_topo_dev,
                     const int32_t* mesh_frame_dev, const float* rgb_dev, const float* view_dev, float focal,
                     float visible_weight, const uint8_t* img_in_dev, uint8_t* img_out_dev, int n_frames, int H, int W,
                     int32_t* ids_out_dev, void* ws_dev, void* stream, const float* vcol_dev = nullptr, bool colored = false) {
  if ((per_mesh && !view_dev) || (colored && (!vcol_dev || !vertex_color_sizes_ok(n_meshes, n_verts))) ||
      !verts_dev || !topo_dev || !mesh_frame_dev || !rgb_dev || !img_in_dev || !img_out_dev || !ws_dev || n_meshes <= 0 ||
      n_verts <= 0 || n_verts > RENDER_MAX_VERTS || n_faces <= 0 || n_frames <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384 ||
      (long long)n_meshes * n_faces > 0x7fffffffll || n_frames > 65535 || !(focal > 0.f) ||
      !(visible_weight >= 0.f && visible_weight <= 1.f))
    return fail(nullptr, ACRMI_EINVAL, "%s: bad arguments", who);
  RenderArgs a{};
  a.verts = verts_dev; a.trans = trans_dev; a.topo[0] = topo_dev; a.topo[1] = topo2_dev; a.mesh_topo = mesh_topo_dev;
  a.mesh_frame = mesh_frame_dev; a.rgb = rgb_dev; a.view = per_mesh ? nullptr : view_dev; a.mesh_view = per_mesh ? view_dev : nullptr;
  a.focal = focal; a.visible_weight = visible_weight;
  a.img_in = img_in_dev; a.img_out = img_out_dev; a.ids_out = ids_out_dev; a.ws = (char*)ws_dev;
  a.n_meshes = n_meshes; a.n_verts = n_verts; a.n_faces = n_faces; a.n_frames = n_frames; a.H = H; a.W = W;
  a.vcol = vcol_dev;
  hipError_t e = launch_render(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "rasterize: %s", hipGetErrorString(e));
}

int acrmi_rasterize(const float* verts_dev, const float* trans_dev, int n_meshes, int n_verts, int n_faces,
                    const int32_t* topo_dev, const int32_t* topo2_dev, const int32_t* mesh_topo_dev,
                    const int32_t* mesh_frame_dev, const float* rgb_dev, const float* view_dev, float focal,
                    float visible_weight, const uint8_t* img_in_dev, uint8_t* img_out_dev, int n_frames, int H, int W,
                    int32_t* ids_out_dev, void* ws_dev, void* stream) {
  return rasterize("acrmi_rasterize", false, verts_dev, trans_dev, n_meshes, n_verts, n_faces, topo_dev, topo2_dev, mesh_topo_dev,
                   mesh_frame_dev, rgb_dev, view_dev, focal, visible_weight, img_in_dev, img_out_dev, n_frames, H, W, ids_out_dev,
                   ws_dev, stream);
}

int acrmi_rasterize_views(const float* verts_dev, const float* trans_dev, int n_meshes, int n_verts, int n_faces,
                          const int32_t* topo_dev, const int32_t* topo2_dev, const int32_t* mesh_topo_dev,
                          const int32_t* mesh_frame_dev, const float* rgb_dev, const float* view_dev, float focal,
                          float visible_weight, const uint8_t* img_in_dev, uint8_t* img_out_dev, int n_frames, int H, int W,
                          int32_t* ids_out_dev, void* ws_dev, void* stream) {
  return rasterize("acrmi_rasterize_views", true, verts_dev, trans_dev, n_meshes, n_verts, n_faces, topo_dev, topo2_dev,
                   mesh_topo_dev, mesh_frame_dev, rgb_dev, view_dev, focal, visible_weight, img_in_dev, img_out_dev, n_frames, H, W,
                   ids_out_dev, ws_dev, stream);
}

int acrmi_rasterize_colored(const float* verts_dev, const float* trans_dev, int n_meshes, int n_verts, int n_faces,
                            const int32_t* topo_dev, const int32_t* topo2_dev, const int32_t* mesh_topo_dev,
                            const int32_t* mesh_frame_dev, const float* rgb_dev, const float* vcol_dev, const float* view_dev,
                            int view_per_mesh, float focal, float visible_weight, const uint8_t* img_in_dev, uint8_t* img_out_dev,
                            int n_frames, int H, int W, int32_t* ids_out_dev, void* ws_dev, void* stream) {
  return rasterize("acrmi_rasterize_colored", view_per_mesh != 0, verts_dev, trans_dev, n_meshes, n_verts, n_faces, topo_dev,
                   topo2_dev, mesh_topo_dev, mesh_frame_dev, rgb_dev, view_dev, focal, visible_weight, img_in_dev, img_out_dev,
                   n_frames, H, W, ids_out_dev, ws_dev, stream, vcol_dev, true);
}

// ---- per-vertex colours (csrc/vertex_color.hip; csrc/vertex_color_plan.h) ----
int acrmi_vertex_colors(const float* values_dev, const int32_t* flags_dev, const float* base_rgb_dev, int M, int V, float lo,
                        float hi, int reverse, const float* flag_rgb_host, const uint8_t* lut_host, int bgr, float* vcol_dev,
                        void* stream) {
  const char* who = "acrmi_vertex_colors";
  if (M < 0 || V < 1) return fail(nullptr, ACRMI_EINVAL, "%s: bad sizes (%d meshes of %d vertices)", who, M, V);
  if (!vertex_color_range_ok(lo, hi)) return fail(nullptr, ACRMI_EINVAL, "%s: lo and hi must be finite, hi > lo", who);
  if (!vertex_color_sizes_ok(M, V)) return fail(nullptr, ACRMI_EINVAL, "%s: %d meshes of %d vertices are beyond 2^31 - 1 elements", who, M, V);
  if (M == 0) return ACRMI_OK;
  if (!values_dev || !base_rgb_dev || !flag_rgb_host || !vcol_dev) return fail(nullptr, ACRMI_EINVAL, "%s: a null pointer", who);
  VertexColorArgs a{};
  a.values = values_dev; a.flags = flags_dev; a.base_rgb = base_rgb_dev; a.vcol = vcol_dev; a.lo = lo; a.hi = hi;
  a.flag_rgb[0] = flag_rgb_host[0]; a.flag_rgb[1] = flag_rgb_host[1]; a.flag_rgb[2] = flag_rgb_host[2];
  a.reverse = reverse != 0; a.M = M; a.V = V;
  if (lut_host) std::memcpy(a.lut, lut_host, 768);
  else heatmap_default_lut(bgr != 0, a.lut);
  const hipError_t e = launch_vertex_colors(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "%s: %s", who, hipGetErrorString(e));
}

int acrmi_contact_values(const float* d2_dev, const float* s_dev, const int32_t* cross_dev, int B, int K, int V, float max_depth,
                         float* value_dev, int32_t* flag_dev, void* stream) {
  const char* who = "acrmi_contact_values";
  if (B < 0 || K < 1 || K > ACRMI_MAX_HAND || V < 1)
    return fail(nullptr, ACRMI_EINVAL, "%s: bad sizes (%d rows, %d hands per side in 1..%d, %d vertices)", who, B, K, ACRMI_MAX_HAND, V);
  if (!(max_depth >= 0.f)) return fail(nullptr, ACRMI_EINVAL, "%s: max_depth must be >= 0 (+inf allowed)", who);
  if (!contact_values_sizes_ok(B, K, V)) return fail(nullptr, ACRMI_EINVAL, "%s: %d rows of %d x %d pairs of %d vertices are beyond 2^31 - 1 elements", who, B, K, K, V);
  if ((s_dev != nullptr) == (cross_dev != nullptr))
    return fail(nullptr, ACRMI_EINVAL, "%s: exactly one of s_dev (nearest-vertex measure) and cross_dev (surface measure)", who);
  if (B == 0) return ACRMI_OK;
  if (!d2_dev || !value_dev || !flag_dev) return fail(nullptr, ACRMI_EINVAL, "%s: a null pointer", who);
  const ContactValuesArgs a{d2_dev, s_dev, cross_dev, max_depth, value_dev, flag_dev, B, K, V};
  const hipError_t e = launch_contact_values(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "%s: %s", who, hipGetErrorString(e));
}

// ---- the two contact measures between meshes (csrc/contact.hip; csrc/contact_plan.h, csrc/surface_contact_plan.h) ----
size_t acrmi_contact_workspace(int n_meshes, int n_verts) { return contact_workspace_bytes(n_meshes, n_verts); }
size_t acrmi_surface_contact_workspace(int n_meshes, int n_verts, int n_faces) {
  return surface_workspace_bytes(n_meshes, n_verts, n_faces);
}

// What both stateless entry points check, in this order: the sizes, the limits (max_faces 0: the measure has none on the
// faces), the parameters; then - n_pairs == 0 is a success that touches nothing - the pointers (own: the measure's own
// outputs), the workspace's alignment and the plan's verdict.
static int check_mesh_contact(const char* who, const ContactFrame& f, int max_faces, std::initializer_list<const void*> own,
                              bool plan_ok) {
  if (f.n_meshes <= 0 || f.n_verts <= 0 || f.n_faces <= 0 || f.n_pairs < 0)
    return fail(nullptr, ACRMI_EINVAL, "%s: bad sizes (%d meshes, %d vertices, %d faces, %d pairs)", who, f.n_meshes, f.n_verts,
                f.n_faces, f.n_pairs);
  if (f.n_verts > CONTACT_MAX_VERTS || (max_faces && f.n_faces > max_faces))
    return max_faces ? fail(nullptr, ACRMI_EINVAL, "%s: %d vertices and %d faces, at most %d and %d", who, f.n_verts, f.n_faces,
                            CONTACT_MAX_VERTS, max_faces)
                     : fail(nullptr, ACRMI_EINVAL, "%s: %d vertices, at most %d (the other mesh is held in LDS)", who, f.n_verts,
                            CONTACT_MAX_VERTS);
  if (!contact_params_ok(f.contact_dist, f.max_depth))
    return fail(nullptr, ACRMI_EINVAL, "%s: contact_dist must be finite and >= 0, max_depth >= 0 (+inf allowed)", who);
  if (f.n_pairs == 0) return ACRMI_OK;
  bool all = f.verts && f.topo[0] && f.pairs && f.d2 && f.sum_f && f.sum_i && f.ws;
  for (const void* p : own) all = all && p;
  if (!all) return fail(nullptr, ACRMI_EINVAL, "%s: a null pointer", who);
  if (((uintptr_t)f.ws & 15) != 0) return fail(nullptr, ACRMI_EINVAL, "%s: the workspace is not 16-byte aligned", who);
  if (!plan_ok)
    return max_faces ? fail(nullptr, ACRMI_EINVAL, "%s: %d pairs of %d vertices (or %d meshes of %d faces) are beyond 2^31 - 1 elements",
                            who, f.n_pairs, f.n_verts, f.n_meshes, f.n_faces)
                     : fail(nullptr, ACRMI_EINVAL, "%s: %d pairs of %d vertices (or %d meshes) are beyond 2^31 - 1 elements", who,
                            f.n_pairs, f.n_verts, f.n_meshes);
  return ACRMI_OK;
}

int acrmi_mesh_contact(const float* verts_dev, const float* trans_dev, int n_meshes, int n_verts, int n_faces,
                       const int32_t* topo_dev, const int32_t* topo2_dev, const int32_t* mesh_topo_dev, const int32_t* sign_dev,
                       const int32_t* pairs_dev, int n_pairs, float contact_dist, float max_depth, int32_t* nn_dev, float* d2_dev,
                       float* s_dev, float* sum_f_dev, int32_t* sum_i_dev, void* ws_dev, void* stream) {
  const char* who = "acrmi_mesh_contact";
  const ContactArgs a{{verts_dev, trans_dev, {topo_dev, topo2_dev}, mesh_topo_dev, pairs_dev, contact_dist, max_depth, d2_dev,
                       (float4*)ws_dev, sum_f_dev, sum_i_dev, n_meshes, n_verts, n_faces, n_pairs},
                      sign_dev, nn_dev, s_dev};
  const int r = check_mesh_contact(who, a, 0, {nn_dev, s_dev}, contact_plan(n_meshes, n_verts, n_pairs).ok);
  if (r != ACRMI_OK || n_pairs == 0) return r;
  const hipError_t e = launch_contact(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "%s: %s", who, hipGetErrorString(e));
}

int acrmi_mesh_surface_contact(const float* verts_dev, const float* trans_dev, int n_meshes, int n_verts, int n_faces,
                               const int32_t* topo_dev, const int32_t* topo2_dev, const int32_t* mesh_topo_dev,
                               const int32_t* pairs_dev, int n_pairs, float contact_dist, float max_depth, int32_t* face_dev,
                               float* d2_dev, float* point_dev, int32_t* cross_dev, float* sum_f_dev, int32_t* sum_i_dev,
                               void* ws_dev, void* stream) {
  const char* who = "acrmi_mesh_surface_contact";
  const SurfaceContactArgs a{{verts_dev, trans_dev, {topo_dev, topo2_dev}, mesh_topo_dev, pairs_dev, contact_dist, max_depth, d2_dev,
                              (float4*)ws_dev, sum_f_dev, sum_i_dev, n_meshes, n_verts, n_faces, n_pairs},
                             face_dev, cross_dev, point_dev};
  const int r = check_mesh_contact(who, a, SURFACE_MAX_FACES, {face_dev, point_dev, cross_dev},
                                   surface_plan(n_meshes, n_verts, n_faces, n_pairs).ok);
  if (r != ACRMI_OK || n_pairs == 0) return r;
  const hipError_t e = launch_surface_contact(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "%s: %s", who, hipGetErrorString(e));
}

// ---- scoring against ground truth (csrc/score.hip; csrc/score_plan.h) ----
size_t acrmi_score_board_bytes(int n, int n_groups, int n_bins) { return score_board_bytes(n, n_groups, n_bins); }
size_t acrmi_score_pair_bytes(int n_groups) { return score_pair_bytes(n_groups); }

int acrmi_pose_errors(const float* pred_dev, const float* gt_dev, const uint8_t* valid_dev, int N, int n, int root,
                      const float* origin_pred_dev, const float* origin_gt_dev, const float* trans_dev, const int32_t* group_dev,
                      int n_groups, const float* flags_dev, float* e_ra_dev, float* e_pa_dev, float* row_f_dev, int32_t* row_i_dev,
                      float* xform_dev, float* pair_err_dev, void* stream) {
  const char* who = "acrmi_pose_errors";
  if (N < 0 || n < 1 || n > SCORE_MAX_POINTS)
    return fail(nullptr, ACRMI_EINVAL, "%s: %d rows of %d points (n in 1..%d)", who, N, n, SCORE_MAX_POINTS);
  if (root < -1 || root >= n) return fail(nullptr, ACRMI_EINVAL, "%s: root %d outside -1..%d", who, root, n - 1);
  if (!score_groups_ok(n_groups)) return fail(nullptr, ACRMI_EINVAL, "%s: n_groups %d outside 1..%d", who, n_groups, SCORE_MAX_GROUPS);
  if (!score_sizes_ok(N, n)) return fail(nullptr, ACRMI_EINVAL, "%s: %d rows of %d points are beyond 2^31 - 1 elements", who, N, n);
  if (N == 0) return ACRMI_OK;
  if (!pred_dev || !gt_dev || !e_ra_dev || !e_pa_dev || !row_f_dev || !row_i_dev || (origin_pred_dev == nullptr) != (origin_gt_dev == nullptr))
    return fail(nullptr, ACRMI_EINVAL, "%s: a null pointer", who);
  ScoreArgs a{};
  a.set[0] = ScoreSet{pred_dev, gt_dev, valid_dev, origin_pred_dev, origin_gt_dev, nullptr, trans_dev, e_ra_dev, e_pa_dev,
                      row_f_dev, row_i_dev, xform_dev, pair_err_dev, n, root, 3, 0};
  a.n_sets = 1;
  a.group = group_dev;
  a.flags = flags_dev;
  a.flag_stride = 1;
  a.N = N;
  a.n_groups = n_groups;
  const hipError_t e = launch_pose_errors(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "%s: %s", who, hipGetErrorString(e));
}

int acrmi_score_accumulate(const float* e_ra_dev, const float* e_pa_dev, int N, int n, const int32_t* group_dev, int n_groups,
                           const float* flags_dev, const float* pair_err_dev, int n_bins, double bin_width, void* board_dev,
                           void* pair_board_dev, void* stream) {
  const char* who = "acrmi_score_accumulate";
  if (N < 0 || n < 1 || n > SCORE_MAX_POINTS)
    return fail(nullptr, ACRMI_EINVAL, "%s: %d rows of %d points (n in 1..%d)", who, N, n, SCORE_MAX_POINTS);
  if (!score_groups_ok(n_groups)) return fail(nullptr, ACRMI_EINVAL, "%s: n_groups %d outside 1..%d", who, n_groups, SCORE_MAX_GROUPS);
  if (!score_bins_ok(n_bins, bin_width))
    return fail(nullptr, ACRMI_EINVAL, "%s: n_bins in 1..%d, bin_width finite and > 0", who, SCORE_MAX_BINS);
  if (!score_sizes_ok(N, n)) return fail(nullptr, ACRMI_EINVAL, "%s: %d rows of %d points are beyond 2^31 - 1 elements", who, N, n);
  if (N == 0) return ACRMI_OK;
  if (!e_ra_dev || !e_pa_dev || !board_dev) return fail(nullptr, ACRMI_EINVAL, "%s: a null pointer", who);
  if (((uintptr_t)board_dev & 7) != 0 || ((uintptr_t)pair_board_dev & 7) != 0)
    return fail(nullptr, ACRMI_EINVAL, "%s: the board is not 8-byte aligned", who);
  const ScoreAccArgs a{e_ra_dev, e_pa_dev, group_dev, 0, flags_dev, 1, pair_err_dev, N, n, n_groups, n_bins, bin_width,
                       (int64_t*)board_dev, (int64_t*)pair_board_dev};
  const hipError_t e = launch_score_accumulate(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "%s: %s", who, hipGetErrorString(e));
}

// ---- matching decoded hands to ground truth (csrc/match.hip; csrc/match_plan.h) ----
size_t acrmi_match_board_bytes(void) { return match_board_bytes(); }

int acrmi_match_hands(const float* pred_dev, const float* truth_dev, const uint8_t* valid_dev, const uint8_t* truth_valid_dev,
                      const float* flags_dev, int flag_stride, const float* trans_dev, const int32_t* group_dev, int B, int K, int G,
                      int n, int D, float gate, int min_points, int32_t* match_dev, int32_t* pred_of_dev, float* cost_dev,
                      int32_t* counts_dev, int32_t* group_out_dev, void* stream) {
  const char* who = "acrmi_match_hands";
  if (B < 0 || K < 1 || K > MATCH_MAX || G < 1 || G > MATCH_MAX)
    return fail(nullptr, ACRMI_EINVAL, "%s: %d frames, K = %d, G = %d (K, G in 1..%d)", who, B, K, G, MATCH_MAX);
  if (n < 1 || n > MATCH_MAX_POINTS || (D != 2 && D != 3))
    return fail(nullptr, ACRMI_EINVAL, "%s: %d points of %d coordinates (n in 1..%d, D 2 or 3)", who, n, D, MATCH_MAX_POINTS);
  if (!match_sizes_ok(B, K, G, n, D)) return fail(nullptr, ACRMI_EINVAL, "%s: %d frames are beyond 2^31 - 1 elements", who, B);
  if (!match_gate_ok(gate)) return fail(nullptr, ACRMI_EINVAL, "%s: gate must be finite and >= 0, or +inf", who);
  if (min_points < 1 || min_points > n) return fail(nullptr, ACRMI_EINVAL, "%s: min_points %d outside 1..%d", who, min_points, n);
  if (flags_dev && flag_stride < 1) return fail(nullptr, ACRMI_EINVAL, "%s: flag_stride %d < 1", who, flag_stride);
  if (B == 0) return ACRMI_OK;
  if (!pred_dev || !truth_dev || !match_dev || !pred_of_dev || !cost_dev || !counts_dev || !group_out_dev)
    return fail(nullptr, ACRMI_EINVAL, "%s: a null pointer", who);
  const MatchArgs a{pred_dev, truth_dev, valid_dev, truth_valid_dev, flags_dev, (size_t)flag_stride, trans_dev, group_dev, B, K, G, n, D,
                    gate, min_points, match_dev, pred_of_dev, cost_dev, counts_dev, group_out_dev};
  const hipError_t e = launch_match(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "%s: %s", who, hipGetErrorString(e));
}

int acrmi_match_gather(const float* src_dev, const int32_t* index_dev, int B, int Ks, int Kd, int W, float* dst_dev, void* stream) {
  const char* who = "acrmi_match_gather";
  if (!match_gather_sizes_ok(B, Ks, Kd, W))
    return fail(nullptr, ACRMI_EINVAL, "%s: %d frames, Ks = %d, Kd = %d (1..%d), W = %d (>= 1), at most 2^31 - 1 elements", who, B, Ks,
                Kd, MATCH_MAX, W);
  if (B == 0) return ACRMI_OK;
  if (!src_dev || !index_dev || !dst_dev) return fail(nullptr, ACRMI_EINVAL, "%s: a null pointer", who);
  if (((uintptr_t)src_dev & 3) != 0 || ((uintptr_t)dst_dev & 3) != 0 || ((uintptr_t)index_dev & 3) != 0)
    return fail(nullptr, ACRMI_EINVAL, "%s: a pointer is not 4-byte aligned", who);
  const MatchGatherArgs a{src_dev, index_dev, dst_dev, 2ll * B * Kd, W, Ks, Kd};
  const hipError_t e = launch_match_gather(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "%s: %s", who, hipGetErrorString(e));
}

int acrmi_match_accumulate(const int32_t* counts_dev, const float* cost_dev, int B, int K, void* board_dev, void* stream) {
  const char* who = "acrmi_match_accumulate";
  if (B < 0 || K < 1 || K > MATCH_MAX || 2ll * B * K > 0x7fffffffll)
    return fail(nullptr, ACRMI_EINVAL, "%s: %d frames, K = %d (1..%d)", who, B, K, MATCH_MAX);
  if (B == 0) return ACRMI_OK;
  if (!counts_dev || !cost_dev || !board_dev) return fail(nullptr, ACRMI_EINVAL, "%s: a null pointer", who);
  if (((uintptr_t)board_dev & 7) != 0) return fail(nullptr, ACRMI_EINVAL, "%s: the board is not 8-byte aligned", who);
  const MatchAccArgs a{counts_dev, cost_dev, B, K, (int64_t*)board_dev};
  const hipError_t e = launch_match_accumulate(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "%s: %s", who, hipGetErrorString(e));
}

// ---- key-point skeleton and heat-map views (csrc/overlay.hip) ----
int acrmi_overlay_tables(int bgr, uint8_t* colors_host, uint8_t* lut_host) {
  if (colors_host) skeleton_default_colors(bgr != 0, colors_host);
  if (lut_host) heatmap_default_lut(bgr != 0, lut_host);
  return ACRMI_OK;
}

static bool overlay_image_ok(int n, int H, int W) {
  return n > 0 && n <= OVERLAY_MAX_FRAMES && H > 0 && W > 0 && H <= OVERLAY_MAX_DIM && W <= OVERLAY_MAX_DIM;
}

int acrmi_draw_skeletons(const float* kps_dev, const int32_t* hand_frame_dev, int n_hands, const uint8_t* colors_host, int bgr,
                         int line_width, int circle_rad, const uint8_t* img_in_dev, uint8_t* img_out_dev, int n_frames, int H,
                         int W, void* stream) {
  if (!kps_dev || !hand_frame_dev || !img_in_dev || !img_out_dev || n_hands <= 0 || !overlay_image_ok(n_frames, H, W) ||
      line_width < 1 || line_width > OVERLAY_MAX_WIDTH || circle_rad < 0 || circle_rad > OVERLAY_MAX_RAD)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_draw_skeletons: bad arguments (line_width 1..%d, circle_rad 0..%d, H, W <= %d)",
                OVERLAY_MAX_WIDTH, OVERLAY_MAX_RAD, OVERLAY_MAX_DIM);
  SkeletonArgs a{};
  a.kps = kps_dev; a.hand_frame = hand_frame_dev; a.n_hands = n_hands; a.n_frames = n_frames; a.H = H; a.W = W;
  a.line_width = line_width; a.circle_rad = circle_rad; a.img_in = img_in_dev; a.img_out = img_out_dev;
  if (colors_host) std::memcpy(a.colors, colors_host, 63);
  else skeleton_default_colors(bgr != 0, a.colors);
  hipError_t e = launch_skeleton(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "draw_skeletons: %s", hipGetErrorString(e));
}

// What acrmi_draw_heatmaps and acrmi_draw_region_heatmaps check and fill alike: n fp32 maps (pairs) of h x w drawn over
// n_frames frames; own_ok = the caller's own pointers are there.
static int heatmap_args(const char* who, HeatmapBase& a, bool own_ok, const float* maps_l, const float* maps_r, long long frame_stride,
                        int n, int h, int w, float weight, const uint8_t* lut_host, int bgr, const uint8_t* img_in, uint8_t* out_l,
                        uint8_t* out_r, int n_frames, int H, int W) {
  if (!own_ok || !maps_l || !img_in || !out_l || (maps_r != nullptr) != (out_r != nullptr) || out_l == out_r ||
      (out_r && out_r == img_in) || n <= 0 || !overlay_image_ok(n_frames, H, W) || h <= 0 || w <= 0 || h > OVERLAY_MAX_DIM ||
      w > OVERLAY_MAX_DIM || frame_stride < (long long)h * w || !(weight >= 0.f && weight <= 1.f))
    return fail(nullptr, ACRMI_EINVAL, "%s: bad arguments", who);
  a.maps[0] = maps_l; a.maps[1] = maps_r; a.frame_stride = frame_stride; a.pix_stride = 1; a.dtype = ACRMI_DT_F32;
  a.n = n; a.h = h; a.w = w; a.H = H; a.W = W; a.weight = weight; a.img_in = img_in; a.out[0] = out_l; a.out[1] = out_r;
  if (lut_host) std::memcpy(a.lut, lut_host, 768);
  else heatmap_default_lut(bgr != 0, a.lut);
  return ACRMI_OK;
}

int acrmi_draw_heatmaps(const float* maps_l_dev, const float* maps_r_dev, long long frame_stride, int n, int h, int w,
                        const float* view_dev, float weight, const uint8_t* lut_host, int bgr, const uint8_t* img_in_dev,
                        uint8_t* out_l_dev, uint8_t* out_r_dev, int H, int W, void* stream) {
  HeatmapArgs a{};
  if (int r = heatmap_args("acrmi_draw_heatmaps", a, true, maps_l_dev, maps_r_dev, frame_stride, n, h, w, weight, lut_host, bgr,
                           img_in_dev, out_l_dev, out_r_dev, n, H, W))
    return r;
  a.view = view_dev;
  hipError_t e = launch_heatmap(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "draw_heatmaps: %s", hipGetErrorString(e));
}

int acrmi_draw_region_heatmaps(const float* maps_l_dev, const float* maps_r_dev, long long frame_stride, int n, int h, int w,
                               const float* offsets_dev, const int32_t* region_frame_dev, float weight,
                               const uint8_t* lut_host, int bgr, const uint8_t* img_in_dev, uint8_t* out_l_dev,
                               uint8_t* out_r_dev, int n_frames, int H, int W, void* stream) {
  RegionHeatmapArgs a{};
  if (int r = heatmap_args("acrmi_draw_region_heatmaps", a, offsets_dev && region_frame_dev, maps_l_dev, maps_r_dev, frame_stride,
                           n, h, w, weight, lut_host, bgr, img_in_dev, out_l_dev, out_r_dev, n_frames, H, W))
    return r;
  a.offsets = offsets_dev; a.region_frame = region_frame_dev; a.n_frames = n_frames;
  hipError_t e = launch_region_heatmap(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "draw_region_heatmaps: %s", hipGetErrorString(e));
}

}  // extern "C"

// ---- the part segmentation as an output (csrc/segm.hip; csrc/segm_plan.h) ----
int acrmi_segm_tables(int bgr, int C, uint8_t* colors_host) {
  if (!segm_classes_ok(C) || !colors_host)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_segm_tables: C = %d must be odd and in %d..%d, colors_host not NULL", C, SEGM_MIN_C, SEGM_MAX_C);
  segm_default_colors(bgr != 0, C, colors_host);
  return ACRMI_OK;
}

int segm_labels_call(acrmi_ctx* c, const char* who, const float* logits, long long frame_stride, int pix_stride, int n, int h, int w,
                     int C, const float* view, const float* offsets, float weight, const uint8_t* colors_host, int bgr,
                     const uint8_t* img_in, uint8_t* out, uint8_t* labels, int H, int W, void* stream) {
  if (!segm_classes_ok(C)) return fail(c, ACRMI_EINVAL, "%s: C = %d must be odd and in %d..%d", who, C, SEGM_MIN_C, SEGM_MAX_C);
  if (pix_stride < C) return fail(c, ACRMI_EINVAL, "%s: pix_stride %d is less than the %d classes of a cell", who, pix_stride, C);
  if (!segm_dim_ok(h) || !segm_dim_ok(w) || !segm_dim_ok(H) || !segm_dim_ok(W) || n < 0 || n > SEGM_MAX_FRAMES)
    return fail(c, ACRMI_EINVAL, "%s: bad sizes (%d frames of %d x %d from maps of %d x %d; each in 1..%d, at most %d frames)", who, n,
                H, W, h, w, SEGM_MAX_DIM, SEGM_MAX_FRAMES);
  if (frame_stride < (long long)h * w * pix_stride)
    return fail(c, ACRMI_EINVAL, "%s: frame_stride %lld is less than %d x %d cells of %d floats", who, frame_stride, h, w, pix_stride);
  if (!(weight >= 0.f && weight <= 1.f)) return fail(c, ACRMI_EINVAL, "%s: weight must be in [0, 1]", who);
  if (view && offsets) return fail(c, ACRMI_EINVAL, "%s: view_dev or offsets_dev, not both", who);
  if (!out && !labels) return fail(c, ACRMI_EINVAL, "%s: neither out_dev nor labels_dev: nothing to write", who);
  if (out && !img_in) return fail(c, ACRMI_EINVAL, "%s: out_dev needs img_in_dev", who);
  if (n == 0) return ACRMI_OK;
  if (!logits) return fail(c, ACRMI_EINVAL, "%s: logits_dev is NULL", who);
  SegmArgs a{};
  a.logits = logits; a.frame_stride = frame_stride; a.pix_stride = pix_stride; a.C = C; a.n = n; a.h = h; a.w = w; a.H = H; a.W = W;
  a.view = view; a.offsets = offsets; a.weight = weight; a.img_in = img_in; a.out = out; a.labels = labels;
  if (colors_host) std::memcpy(a.colors, colors_host, 3 * (size_t)C);
  else segm_default_colors(bgr != 0, C, a.colors);
  const hipError_t e = launch_segm(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(c, ACRMI_EHIP, "%s: %s", who, hipGetErrorString(e));
}

int acrmi_segm_labels(const float* logits_dev, long long frame_stride, int pix_stride, int n, int h, int w, int C,
                      const float* view_dev, const float* offsets_dev, float weight, const uint8_t* colors_host, int bgr,
                      const uint8_t* img_in_dev, uint8_t* out_dev, uint8_t* labels_dev, int H, int W, void* stream) {
  return segm_labels_call(nullptr, "acrmi_segm_labels", logits_dev, frame_stride, pix_stride, n, h, w, C, view_dev, offsets_dev, weight,
                          colors_host, bgr, img_in_dev, out_dev, labels_dev, H, W, stream);
}

size_t acrmi_segm_stats_ws_ints(int n, int H, int W) { return segm_stats_ws_ints(n, H, W); }

int acrmi_segm_stats(const uint8_t* labels_dev, const int32_t* ids_dev, int n_faces, int n, int H, int W, int C,
                     int32_t* counts_dev, int32_t* boxes_dev, int32_t* agree_dev, int32_t* ws_dev, void* stream) {
  const char* who = "acrmi_segm_stats";
  if (!segm_classes_ok(C)) return fail(nullptr, ACRMI_EINVAL, "%s: C = %d must be odd and in %d..%d", who, C, SEGM_MIN_C, SEGM_MAX_C);
  if (!segm_dim_ok(H) || !segm_dim_ok(W) || n < 0 || n > SEGM_MAX_FRAMES)
    return fail(nullptr, ACRMI_EINVAL, "%s: bad sizes (%d frames of %d x %d; each in 1..%d, at most %d frames)", who, n, H, W,
                SEGM_MAX_DIM, SEGM_MAX_FRAMES);
  if ((ids_dev != nullptr) != (agree_dev != nullptr)) return fail(nullptr, ACRMI_EINVAL, "%s: agree_dev goes with ids_dev", who);
  if (ids_dev && n_faces <= 0) return fail(nullptr, ACRMI_EINVAL, "%s: ids_dev needs n_faces > 0", who);
  if (n == 0) return ACRMI_OK;
  if (!labels_dev || !counts_dev || !boxes_dev || !ws_dev) return fail(nullptr, ACRMI_EINVAL, "%s: a null pointer", who);
  const SegmStatsArgs a{labels_dev, ids_dev, n_faces, n, H, W, C, counts_dev, boxes_dev, agree_dev, ws_dev};
  const hipError_t e = launch_segm_stats(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "%s: %s", who, hipGetErrorString(e));
}
