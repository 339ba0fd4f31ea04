// libacrmi.so: context life cycle, options and the fused entry points of the C ABI declared in include/acrmi.h
// (program replay: acrmi_program.hip; stand-alone operators: acrmi_ops.hip; RCCL: acrmi_comm.hip).
#include "acrmi_ctx.h"
#include "mano_fit_plan.h"
#include "score_plan.h"
#include "surface_contact_plan.h"      // and contact_plan.h
#include "vertex_color_plan.h"

#include <initializer_list>
#include <type_traits>

std::string g_err;

int fail(acrmi_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_err = buf;
  return code;
}

// the blob is freed by the last context that holds it (contexts are single-threaded per the ABI; sharing contexts of one
// pool are driven by one host thread)
void release_weights(acrmi_ctx* c) {
  // (the use count is atomic: contexts of one pool may be destroyed / re-programmed from different host threads)
  if (c->weights_ref && c->weights_ref->fetch_sub(1) == 1) {
    (void)hipFree(c->weights);
    delete c->weights_ref;
  }
  c->weights = nullptr;
  c->weights_ref = nullptr;
  c->n_weights = 0;
}

// a context call that forwarded to a context-free one: the error it left becomes the context's
static int from_global(acrmi_ctx* c, int r) {
  if (r) c->err = g_err;
  return r;
}

// What the calls that take a device NUMBER do first: there is a HIP device, `device` is one of them and can be selected.  It
// stays selected while the object lives; then the caller's current device is restored.
struct NewOnDevice {
  int rc = ACRMI_OK;
  std::optional<DeviceGuard> guard;
  NewOnDevice(const char* who, int device) {
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) rc = fail(nullptr, ACRMI_EHIP, "%s: no HIP device (%s)", who, hipGetErrorString(e));
    else if (device < 0 || device >= n) rc = fail(nullptr, ACRMI_EINVAL, "%s: device %d of %d", who, device, n);
    else if (guard.emplace(device).err != hipSuccess) rc = fail(nullptr, ACRMI_EHIP, "hipSetDevice: %s", hipGetErrorString(guard->err));
  }
};

// ---- what the two contact entry points share (below: "contact between the hands of a row") ----
// A measure's scratch in the context for n = B * K hand pairs: [pairs n*K*2 | mesh_topo 2n | sign 2n] int32 (sized for K =
// ACRMI_MAX_HAND) and the measure's records of the 2n meshes behind them.
static size_t contact_head_bytes(long long n) {
  return ((size_t)n * (2 * CONTACT_MAX_HAND + 4) * sizeof(int32_t) + 255) / 256 * 256;
}

// What acrmi_contact and acrmi_surface_contact do around their kernels: the checks (own: the measure's own outputs, already in
// `a`), the measure's scratch (allocated at the first call, again when n grows - or the face count changes, which only the
// surface records depend on), its carve-up, the prep kernel, which forms the pairs from the slot flags (sign_host: the two
// orientation signs), the frame of the launch, and the launch on the context's device.
template <class Args>
static int contact_call(acrmi_ctx* c, const char* who, acrmi_ctx::ContactScratch acrmi_ctx::*scratch,
                        hipError_t (*launch)(const Args&, hipStream_t), Args a, std::initializer_list<const void*> own,
                        const float* verts, const float* cam_trans, const float* slots, int B, int K, const int32_t* sign_host,
                        float contact_dist, float max_depth, float* d2, float* sum_f, int32_t* sum_i, void* stream) {
  constexpr bool surface = std::is_same<Args, SurfaceContactArgs>::value;
  bool all = c && verts && cam_trans && slots && d2 && sum_f && sum_i && B > 0;
  for (const void* p : own) all = all && p;
  if (!all) return fail(c, ACRMI_EINVAL, "%s: bad arguments", who);
  if (K < 1 || K > ACRMI_MAX_HAND) return fail(c, ACRMI_EINVAL, "%s: max_hand %d outside 1..%d", who, K, ACRMI_MAX_HAND);
  if (!contact_params_ok(contact_dist, max_depth))
    return fail(c, ACRMI_EINVAL, "%s: contact_dist must be finite and >= 0, max_depth >= 0 (+inf allowed)", who);
  if (!c->faces_topo[0] || !c->faces_topo[1]) return fail(c, ACRMI_ESTATE, "%s: MANO faces not loaded (acrmi_load_faces)", who);
  const int F = c->n_faces[0];
  if (surface && (c->n_faces[1] != F || F > SURFACE_MAX_FACES))
    return fail(c, ACRMI_EINVAL, "%s: the two sides have %d and %d faces (equal counts, at most %d)", who, F, c->n_faces[1],
                SURFACE_MAX_FACES);
  const long long n = (long long)B * K, n_pairs = n * K;
  if (2 * n > 0x7fffffffll || n_pairs > 0x7fffffffll ||
      !(surface ? surface_plan((int)(2 * n), 778, F, (int)n_pairs).ok : contact_plan((int)(2 * n), 778, (int)n_pairs).ok))
    return fail(c, ACRMI_EINVAL, "%s: %d frames of %d x %d pairs are beyond 2^31 - 1 elements", who, B, K, K);
  ON_DEVICE(c);
  acrmi_ctx::ContactScratch& sc = c->*scratch;
  if (n > sc.hands || (surface && F != sc.faces)) {
    if (sc.ws) {
      HIPCHK(c, hipDeviceSynchronize());
      (void)hipFree(sc.ws);
      sc = {};
    }
    HIPCHK(c, hipMalloc(&sc.ws, contact_head_bytes(n) + (surface ? surface_workspace_bytes((int)(2 * n), 778, F)
                                                                 : contact_workspace_bytes((int)(2 * n), 778))));
    sc.hands = n;
    sc.faces = F;
  }
  int32_t* pairs = (int32_t*)sc.ws;
  int32_t* mesh_topo = pairs + 2 * n_pairs;
  int32_t* sign = mesh_topo + 2 * n;
  hipError_t e = launch_contact_prep(slots, B, K, sign_host[0] < 0 ? -1 : 1, sign_host[1] < 0 ? -1 : 1, pairs, mesh_topo, sign,
                                     (hipStream_t)stream);
  if (e != hipSuccess) return fail(c, ACRMI_EHIP, "%s: prep: %s", who, hipGetErrorString(e));
  static_cast<ContactFrame&>(a) =
      ContactFrame{verts, cam_trans, {c->faces_topo[0], c->faces_topo[1]}, mesh_topo, pairs, contact_dist, max_depth, d2,
                   (float4*)(sc.ws + contact_head_bytes(sc.hands)), sum_f, sum_i, (int)(2 * n), 778, F, (int)n_pairs};
  if constexpr (!surface) a.sign = sign;
  e = launch(a, (hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(c, ACRMI_EHIP, "%s: %s", who, hipGetErrorString(e));
}

extern "C" {

int acrmi_version(void) { return ACRMI_VERSION; }

const char* acrmi_last_error(const acrmi_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int acrmi_create(acrmi_ctx** out, int device) {
  if (!out) return fail(nullptr, ACRMI_EINVAL, "acrmi_create: out is NULL");
  const NewOnDevice on("acrmi_create", device);
  if (on.rc) return on.rc;
  acrmi_ctx* c = new acrmi_ctx();
  c->device = device;
  *out = c;
  return ACRMI_OK;
}

void acrmi_destroy(acrmi_ctx* c) {
  if (!c) return;
  DeviceGuard guard_(c->device);
  comm_destroy(c);
  free_program(c);
  for (int l = 0; l < MAX_LANES; ++l) {
    if (c->lanes[l]) (void)hipStreamDestroy(c->lanes[l]);
    if (c->join_ev[l]) (void)hipEventDestroy(c->join_ev[l]);
  }
  if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
  release_weights(c);
  acrmi_streams_destroy(c->own_streams);
  if (c->render_ws) (void)hipFree(c->render_ws);
  if (c->contact_ws.ws) (void)hipFree(c->contact_ws.ws);
  if (c->surface_ws.ws) (void)hipFree(c->surface_ws.ws);
  if (c->region_hand_frame) (void)hipFree(c->region_hand_frame);
  for (int32_t* p : c->faces_topo)
    if (p) (void)hipFree(p);
  for (auto& side : c->mano_allocs)
    for (float* p : side)
      if (p) (void)hipFree(p);
  delete c;
}

int acrmi_load_weights(acrmi_ctx* c, const float* blob, size_t n) {
  if (!c || !blob || n == 0) return fail(c, ACRMI_EINVAL, "acrmi_load_weights: bad arguments");
  ON_DEVICE(c);
  release_weights(c);
  // the context takes the blob only once it is complete on the device: a failed copy leaves it without weights, not with a
  // blob that has no use count
  float* w = nullptr;
  HIPCHK(c, hipMalloc(&w, n * sizeof(float)));
  hipError_t e = hipMemcpy(w, blob, n * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(w);
    return fail(c, ACRMI_EHIP, "acrmi_load_weights: hipMemcpy of %zu floats: %s", n, hipGetErrorString(e));
  }
  c->weights = w;
  c->n_weights = n;
  c->weights_ref = new std::atomic<int>(1);
  return ACRMI_OK;
}

int acrmi_share_weights(acrmi_ctx* c, acrmi_ctx* donor) {
  if (!c || !donor || c == donor) return fail(c, ACRMI_EINVAL, "acrmi_share_weights: bad arguments");
  if (!donor->weights || !donor->weights_ref) return fail(c, ACRMI_ESTATE, "acrmi_share_weights: the donor holds no weights");
  if (c->device != donor->device) return fail(c, ACRMI_EINVAL, "acrmi_share_weights: contexts on different devices (%d, %d)", c->device, donor->device);
  ON_DEVICE(c);
  release_weights(c);
  c->weights = donor->weights;
  c->n_weights = donor->n_weights;
  c->weights_ref = donor->weights_ref;
  c->weights_ref->fetch_add(1);
  return ACRMI_OK;
}

// The orientation of a side's topology (csrc/contact_plan.h) from its template vertices, once both are loaded; +1 before.
static void update_contact_sign(acrmi_ctx* c, int side) {
  c->contact_sign[side] = 1;
  if (c->v_template_host[side].size() == 778 * 3 && !c->faces_host[side].empty())
    c->contact_sign[side] = contact_orientation_sign(c->v_template_host[side].data(), c->faces_host[side].data(),
                                                     (int)(c->faces_host[side].size() / 3));
}

int acrmi_load_mano(acrmi_ctx* c, int side, const float* v_template, const float* shapedirs, const float* posedirs,
                    const float* J_regressor, const float* weights, const float* hands_mean) {
  if (!c || side < 0 || side > 1 || !v_template || !shapedirs || !posedirs || !J_regressor || !weights || !hands_mean)
    return fail(c, ACRMI_EINVAL, "acrmi_load_mano: bad arguments");
  ON_DEVICE(c);
  // a reload replaces the side's tables: nothing of an earlier launch may still be reading the old ones
  HIPCHK(c, hipDeviceSynchronize());
  for (float*& p : c->mano_allocs[side]) {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
  c->have_mano[side] = false;
  constexpr int NV3 = 2334;
  std::vector<float> sd_t((size_t)10 * NV3), pd_t((size_t)135 * NV3);
  for (int i = 0; i < NV3; ++i) {
    for (int k = 0; k < 10; ++k) sd_t[(size_t)k * NV3 + i] = shapedirs[(size_t)i * 10 + k];
    for (int k = 0; k < 135; ++k) pd_t[(size_t)k * NV3 + i] = posedirs[(size_t)i * 135 + k];
  }
  int n_up = 0;
  auto up = [&](const float* h, size_t n, const float** dst) -> int {
    float* d = nullptr;
    HIPCHK(c, hipMalloc(&d, n * sizeof(float)));
    c->mano_allocs[side][n_up++] = d;
    HIPCHK(c, hipMemcpy(d, h, n * sizeof(float), hipMemcpyHostToDevice));
    *dst = d;
    return ACRMI_OK;
  };
  c->v_template_host[side].assign(v_template, v_template + NV3);
  update_contact_sign(c, side);
  ManoTables& t = c->mano[side];
  int r;
  if ((r = up(v_template, NV3, &t.v_template))) return r;
  if ((r = up(sd_t.data(), sd_t.size(), &t.shapedirs_t))) return r;
  if ((r = up(pd_t.data(), pd_t.size(), &t.posedirs_t))) return r;
  if ((r = up(J_regressor, 16 * 778, &t.jreg))) return r;
  if ((r = up(weights, 778 * 16, &t.weights))) return r;
  if ((r = up(hands_mean, 45, &t.hands_mean))) return r;
  // f16 copies of the blend-shape tables and the skinning weights (ACRMI_OPT_MANO_FP16), rounded to nearest even
  auto up16 = [&](const float* h, size_t n, const unsigned short** dst) -> int {
    std::vector<unsigned short> bits(n + (n & 1));
    for (size_t i = 0; i < n; ++i) {
      const _Float16 v = (_Float16)h[i];
      memcpy(&bits[i], &v, 2);
    }
    float* d = nullptr;
    HIPCHK(c, hipMalloc(&d, bits.size() * 2));
    c->mano_allocs[side][n_up++] = d;
    HIPCHK(c, hipMemcpy(d, bits.data(), bits.size() * 2, hipMemcpyHostToDevice));
    *dst = reinterpret_cast<const unsigned short*>(d);
    return ACRMI_OK;
  };
  if ((r = up16(sd_t.data(), sd_t.size(), &t.shapedirs_h))) return r;
  if ((r = up16(pd_t.data(), pd_t.size(), &t.posedirs_h))) return r;
  if ((r = up16(weights, 778 * 16, &t.weights_h))) return r;
  // the residuals of the two small tables (value = hi + lo): what brings the f16 MANO stage from 6.4e-5 m to the 1e-5 class
  auto residual = [](const float* h, size_t n) {
    std::vector<float> lo(n);
    for (size_t i = 0; i < n; ++i) lo[i] = h[i] - (float)(_Float16)h[i];
    return lo;
  };
  {
    const std::vector<float> lo_s = residual(sd_t.data(), sd_t.size()), lo_w = residual(weights, 778 * 16);
    if ((r = up16(lo_s.data(), lo_s.size(), &t.shapedirs_l))) return r;
    if ((r = up16(lo_w.data(), lo_w.size(), &t.weights_l))) return r;
  }
  c->have_mano[side] = true;
  return ACRMI_OK;
}

int acrmi_backbone_heads(acrmi_ctx* c, const uint8_t* img, int B, void* stream) {
  return run_program(c, img, B, stream, /*point=*/false);   // the dense maps are this call's result
}

int acrmi_point_heads(acrmi_ctx* c, int B, void* stream) {
  if (!c) return fail(c, ACRMI_EINVAL, "acrmi_point_heads: ctx is NULL");
  if (!c->have_program) return fail(c, ACRMI_ESTATE, "acrmi_point_heads: no program");
  if (B <= 0 || B > c->max_batch) return fail(c, ACRMI_EINVAL, "batch %d outside 1..%d", B, c->max_batch);
  ON_DEVICE(c);
  int n = 0;
  for (const acrmi_op& op : c->ops)
    if (op.kind == ACRMI_OP_POINTHEADS) {
      int r = run_op(c, op, nullptr, B, (hipStream_t)stream);
      if (r) return r;
      ++n;
    }
  if (!n) return fail(c, ACRMI_EINVAL, "acrmi_point_heads: the program has no point-heads ops");
  return ACRMI_OK;
}

static bool has_point_heads_ops(const acrmi_ctx* c) {
  bool any = false;
  for (const acrmi_op& op : c->ops) any |= op.kind == ACRMI_OP_POINTHEADS;
  return any;
}

int acrmi_point_heads_multi(acrmi_ctx* c, int B, int max_hand, void* stream) {
  if (!c) return fail(c, ACRMI_EINVAL, "acrmi_point_heads_multi: ctx is NULL");
  if (!c->have_program) return fail(c, ACRMI_ESTATE, "acrmi_point_heads_multi: no program");
  if (B <= 0 || B > c->max_batch) return fail(c, ACRMI_EINVAL, "acrmi_point_heads_multi: batch %d outside 1..%d", B, c->max_batch);
  if (max_hand < 1 || max_hand > ACRMI_MAX_HAND)
    return fail(c, ACRMI_EINVAL, "acrmi_point_heads_multi: max_hand %d outside 1..%d", max_hand, ACRMI_MAX_HAND);
  if (!has_point_heads_ops(c)) return fail(c, ACRMI_EINVAL, "acrmi_point_heads_multi: the program has no point-heads ops");
  ON_DEVICE(c);
  for (const acrmi_op& op : c->ops)
    if (op.kind == ACRMI_OP_POINTHEADS) {
      // (run_op's point_hands = 1 is the classic pick with its gate; here max_hand = 1 is the K = 1 case of the plan)
      HIPCHK(c, launch_point_heads_multi(point_args(c, op, B), max_hand, (hipStream_t)stream));
    }
  return ACRMI_OK;
}

int acrmi_set_option(acrmi_ctx* c, int option, int value) {
  if (!c) return fail(c, ACRMI_EINVAL, "acrmi_set_option: ctx is NULL");
  if (option == ACRMI_OPT_POINT_HEADS || option == ACRMI_OPT_POINT_HEADS_MULTI) {
    if (value && c->have_program && !has_point_heads_ops(c))
      return fail(c, ACRMI_EINVAL, "acrmi_set_option: the program has no point-heads ops");
    (option == ACRMI_OPT_POINT_HEADS ? c->point_heads : c->point_heads_multi) = value != 0;
    return ACRMI_OK;
  }
  if (option == ACRMI_OPT_LANES || option == ACRMI_OPT_LANE_PLAN) {      // what the four schedules are built from
    if (option == ACRMI_OPT_LANE_PLAN) c->lane_plan = value != 0;
    else if (value < 0 || value > MAX_LANES) return fail(c, ACRMI_EINVAL, "acrmi_set_option: lanes %d outside 0..%d", value, MAX_LANES);
    else c->want_lanes = value;
    if (c->have_program)
      for (int v = 0; v < 4; ++v) build_schedule(c, v & 1, v & 2);
    return ACRMI_OK;
  }
  if (option == ACRMI_OPT_CENTER_IDX) {
    if (value < -1 || value > 20) return fail(c, ACRMI_EINVAL, "acrmi_set_option: center_idx %d outside -1..20", value);
    c->center_idx = value;
    return ACRMI_OK;
  }
  if (option == ACRMI_OPT_TEMPORAL) {
    c->temporal = value != 0;
    return ACRMI_OK;
  }
  if (option == ACRMI_OPT_MANO_FP16) {
    c->mano_f16 = value != 0;
    return ACRMI_OK;
  }
  if (option == ACRMI_OPT_BATCH_PRIOR) {
    c->batch_prior = value != 0;
    return ACRMI_OK;
  }
  return fail(c, ACRMI_EINVAL, "acrmi_set_option: unknown option %d", option);
}

int acrmi_set_option_f(acrmi_ctx* c, int option, float value) {
  if (!c) return fail(c, ACRMI_EINVAL, "acrmi_set_option_f: ctx is NULL");
  if (option == ACRMI_OPT_CONF_THRESH) {
    if (!(value == value)) return fail(c, ACRMI_EINVAL, "acrmi_set_option_f: threshold is NaN");
    c->conf_thresh = value;
    return ACRMI_OK;
  }
  if (option == ACRMI_OPT_SMOOTH_COEFF) {
    if (!(value > 0.f)) return fail(c, ACRMI_EINVAL, "acrmi_set_option_f: smooth_coeff must be > 0");
    c->smooth_coeff = value;
    return ACRMI_OK;
  }
  return fail(c, ACRMI_EINVAL, "acrmi_set_option_f: unknown option %d", option);
}

// ---- the tables: what acrmi_streams and acrmi_tracks share (StateTable) ---------------------------------------------------
// `t` (new; deleted here on failure) becomes a table of `capacity` streams on `device`: one zeroed allocation of `bytes`, of
// which the first state_bytes are the filter rows and the rest - the init flags first - is what a reset of every stream clears.
// shared: the table carries the event that orders the launches of different contexts and is zeroed before the call returns;
// else (a context's own table) it is zeroed on `stream`, where the context's first smoothing launch follows it.
static int table_create(const char* who, StateTable* t, int device, int capacity, size_t state_bytes, size_t bytes, bool shared,
                        hipStream_t stream) {
  const NewOnDevice on(who, device);
  hipError_t e = hipSuccess;
  if (!on.rc) {
    t->device = device;
    t->capacity = capacity;
    t->last.assign((size_t)capacity, -1);
    t->reset_bytes = bytes - state_bytes;
    e = hipMalloc(&t->state, bytes);
    if (e == hipSuccess && !shared) e = hipMemsetAsync(t->state, 0, bytes, stream);
    if (e == hipSuccess && shared) {
      // zeroed = every stream starts fresh, every slot free; complete before the call returns: the streams that will use the
      // table are not known here and need not be ordered behind the null stream.  Once per table.
      e = hipMemset(t->state, 0, bytes);
      if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&t->order, hipEventDisableTiming);
    }
    if (e == hipSuccess) {
      t->init = reinterpret_cast<int*>(reinterpret_cast<char*>(t->state) + state_bytes);
      return ACRMI_OK;
    }
    if (t->state) (void)hipFree(t->state);
  }
  delete t;
  return on.rc ? on.rc : fail(nullptr, ACRMI_EHIP, "%s: %d streams, %zu bytes: %s", who, capacity, bytes, hipGetErrorString(e));
}

static void table_destroy(StateTable* t) {
  if (!t) return;
  DeviceGuard guard_(t->device);
  if (t->order) (void)hipEventDestroy(t->order);
  (void)hipFree(t->state);      // (waits for the launches that still use the table)
  delete t;
}

// One call's launches on a table: the table's lock is held, `s` waits for the table's ordering event before them and
// done() records it behind them - also behind a call that failed midway, so that the next context still queues behind
// whatever that call launched.
struct TableOrder {
  StateTable* t;
  hipStream_t s;
  std::lock_guard<std::mutex> lock;
  hipError_t err;
  TableOrder(StateTable* table, hipStream_t stream)
      : t(table), s(stream), lock(table->mu), err(table->order ? hipStreamWaitEvent(stream, table->order, 0) : hipSuccess) {}
  hipError_t done(hipError_t e) {
    if (t->order && err == hipSuccess) {
      const hipError_t r = hipEventRecord(t->order, s);
      if (e == hipSuccess) e = r;
    }
    return e;
  }
};

// The listed streams - all of them when ids is null - start afresh: launch() clears what the table keeps for up to
// SMOOTH_FRAMES_PER_LAUNCH of them.  A filter row behind a cleared init flag is overwritten by its next sample.
typedef hipError_t (*ResetLaunch)(StateTable* t, const SmoothIds& ids, int n, hipStream_t s);
static int table_reset(const char* who, StateTable* t, const int32_t* ids, int n, ResetLaunch launch, hipStream_t stream) {
  if (!t || (ids && n < 0)) return fail(nullptr, ACRMI_EINVAL, "%s: bad arguments", who);
  if (ids) {
    const int bad = smooth_bad_id(ids, n, t->capacity, 0);
    if (bad >= 0) return fail(nullptr, ACRMI_EINVAL, "%s: ids[%d] = %d outside 0..%d", who, bad, ids[bad], t->capacity - 1);
  }
  DeviceGuard guard_(t->device);
  if (guard_.err != hipSuccess) return fail(nullptr, ACRMI_EHIP, "hipSetDevice(%d): %s", t->device, hipGetErrorString(guard_.err));
  TableOrder ord(t, stream);
  hipError_t e = ord.err;
  if (e == hipSuccess && !ids) e = hipMemsetAsync(t->init, 0, t->reset_bytes, stream);
  for (int i0 = 0; ids && e == hipSuccess && i0 < n; i0 += SMOOTH_FRAMES_PER_LAUNCH) {
    const int m = n - i0 < SMOOTH_FRAMES_PER_LAUNCH ? n - i0 : SMOOTH_FRAMES_PER_LAUNCH;
    SmoothIds k{};
    memcpy(k.id, ids + i0, (size_t)m * sizeof(int32_t));
    e = launch(t, k, m, stream);
  }
  e = ord.done(e);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "%s: %s", who, hipGetErrorString(e));
}

// what the calls that take a table and the ids of their B frames check before anything is launched (c may be null)
static int check_table(acrmi_ctx* c, const StateTable* t, const int32_t* ids, int B, const char* who) {
  if (c && t->device != c->device) return fail(c, ACRMI_EINVAL, "%s: the table is on device %d, the context on %d", who, t->device, c->device);
  const int bad = smooth_bad_id(ids, B, t->capacity, -1);
  if (bad >= 0) return fail(c, ACRMI_EINVAL, "%s: ids[%d] = %d outside -1..%d", who, bad, ids[bad], t->capacity - 1);
  return ACRMI_OK;
}

// ---- temporal smoothing (acr/main.py:69-83) -------------------------------------------------------------
static int streams_create(acrmi_streams** out, int device, int capacity, bool shared, hipStream_t stream) {
  if (!out) return fail(nullptr, ACRMI_EINVAL, "acrmi_streams_create: out is NULL");
  if (capacity < 1 || capacity > SMOOTH_MAX_STREAMS)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_streams_create: capacity %d outside 1..%d", capacity, SMOOTH_MAX_STREAMS);
  acrmi_streams* t = new acrmi_streams();
  const size_t state_bytes = (size_t)capacity * 2 * 3 * 64 * sizeof(float);
  const int r = table_create("acrmi_streams_create", t, device, capacity, state_bytes, state_bytes + (size_t)capacity * 2 * sizeof(int),
                             shared, stream);
  if (!r) *out = t;
  return r;
}

int acrmi_streams_create(acrmi_streams** out, int device, int capacity) { return streams_create(out, device, capacity, true, nullptr); }

void acrmi_streams_destroy(acrmi_streams* t) { table_destroy(t); }

int acrmi_streams_reset(acrmi_streams* t, const int32_t* ids, int n, void* stream) {
  return table_reset("acrmi_streams_reset", t, ids, n,
                     [](StateTable* t, const SmoothIds& k, int m, hipStream_t s) { return launch_smooth_reset(k, m, t->init, s); },
                     (hipStream_t)stream);
}

// ids (may be null: every frame is stream 0) are valid for t.  Successive launches of SMOOTH_FRAMES_PER_LAUNCH frames on the
// stream, in frame order: a stream's chain continues in the next launch from the row the previous one wrote.
static void smooth_coefficients(SmoothArgs& a, float smooth_coeff) {
  // create_OneEuroFilter (acr/utils.py:1472-1473): poses / global_orient (smooth_coeff, 0.7), betas (0.6, 0.7);
  // dcutoff 1.0, freq 30.  The derivative filter's alpha is a python double rounded once when it meets the tensor.
  a.mincutoff = smooth_coeff; a.mincutoff_betas = 0.6f; a.beta = 0.7f; a.freq = 30.f;
  const double te = 1.0 / 30.0, tau = 1.0 / (2 * M_PI * 1.0), alpha_d = 1.0 / (1.0 + tau / te);
  a.alpha_d = (float)alpha_d; a.one_minus_alpha_d = (float)(1.0 - alpha_d);
  a.two_pi = (float)(2 * M_PI); a.te = (float)te;
}

static int smooth_on(acrmi_ctx* c, acrmi_streams* t, float* slots, int B, const int32_t* ids, hipStream_t stream) {
  SmoothArgs a{};
  a.state = t->state;
  a.init = t->init;
  smooth_coefficients(a, c->smooth_coeff);
  TableOrder ord(t, stream);
  hipError_t e = ord.err;
  for (int f0 = 0; e == hipSuccess && f0 < B; f0 += SMOOTH_FRAMES_PER_LAUNCH) {
    const int m = B - f0 < SMOOTH_FRAMES_PER_LAUNCH ? B - f0 : SMOOTH_FRAMES_PER_LAUNCH;
    const int n_streams = smooth_plan(ids ? ids + f0 : nullptr, m, &a.b, t->last.data());
    if (!n_streams) continue;      // every frame of this launch is left alone
    a.slots = slots + (size_t)f0 * 2 * ACRMI_SLOT;
    e = launch_smooth(a, n_streams, stream);
  }
  e = ord.done(e);
  return e == hipSuccess ? ACRMI_OK : fail(c, ACRMI_EHIP, "smoothing: %s", hipGetErrorString(e));
}

// what acrmi_smooth_streams and acrmi_forward_streams check before anything is launched
static int check_streams(acrmi_ctx* c, const acrmi_streams* t, const int32_t* ids, int B, const char* who) {
  if (!t || !ids || B <= 0) return fail(c, ACRMI_EINVAL, "%s: bad arguments", who);
  return check_table(c, t, ids, B, who);
}

int acrmi_smooth_streams(acrmi_ctx* c, acrmi_streams* t, float* slots, int B, const int32_t* ids, void* stream) {
  if (!c || !slots) return fail(c, ACRMI_EINVAL, "acrmi_smooth_streams: bad arguments");
  const int r = check_streams(c, t, ids, B, "acrmi_smooth_streams");
  if (r) return r;
  ON_DEVICE(c);
  return smooth_on(c, t, slots, B, ids, (hipStream_t)stream);
}

int acrmi_smooth_reset(acrmi_ctx* c, void* stream) {
  if (!c) return fail(c, ACRMI_EINVAL, "acrmi_smooth_reset: ctx is NULL");
  if (!c->own_streams)      // (a new table is zeroed, on `stream`)
    return from_global(c, streams_create(&c->own_streams, c->device, 1, false, (hipStream_t)stream));
  return from_global(c, acrmi_streams_reset(c->own_streams, nullptr, 0, stream));
}

int acrmi_smooth(acrmi_ctx* c, float* slots, int B, void* stream) {
  if (!c || !slots || B <= 0) return fail(c, ACRMI_EINVAL, "acrmi_smooth: bad arguments");
  ON_DEVICE(c);
  if (!c->own_streams) {
    int r = acrmi_smooth_reset(c, stream);
    if (r) return r;
  }
  return smooth_on(c, c->own_streams, slots, B, nullptr, (hipStream_t)stream);
}

// ---- tracks: hand identity across frames with max_hand > 1 (assoc_plan.h) -------------------------
int acrmi_tracks_create(acrmi_tracks** out, int device, int capacity, int max_hand, int gate, int max_miss) {
  if (!out) return fail(nullptr, ACRMI_EINVAL, "acrmi_tracks_create: out is NULL");
  if (!assoc_params_ok(max_hand, gate, max_miss))
    return fail(nullptr, ACRMI_EINVAL, "acrmi_tracks_create: max_hand %d outside 1..%d, gate %d outside 0..%d or max_miss %d < -1",
                max_hand, ASSOC_MAX_HAND, gate, ASSOC_GATE_ANY, max_miss);
  if (capacity < 1 || (long long)capacity * max_hand > ASSOC_MAX_TRACKS)
    return fail(nullptr, ACRMI_EINVAL, "acrmi_tracks_create: capacity %d x max_hand %d outside 1..%d hands per side", capacity,
                max_hand, ASSOC_MAX_TRACKS);
  acrmi_tracks* t = new acrmi_tracks();
  t->max_hand = max_hand; t->gate = gate; t->max_miss = max_miss;
  const size_t hands = (size_t)capacity * max_hand * 2;
  const size_t state_bytes = hands * 3 * 64 * sizeof(float), init_bytes = hands * sizeof(int);
  // (zeroed = every slot free, every id counter at 0)
  const int r = table_create("acrmi_tracks_create", t, device, capacity, state_bytes,
                             state_bytes + init_bytes + (size_t)capacity * 2 * sizeof(AssocSide), true, nullptr);
  if (r) return r;
  t->meta = reinterpret_cast<AssocSide*>(reinterpret_cast<char*>(t->init) + init_bytes);
  *out = t;
  return ACRMI_OK;
}

void acrmi_tracks_destroy(acrmi_tracks* t) { table_destroy(t); }

int acrmi_tracks_reset(acrmi_tracks* t, const int32_t* ids, int n, void* stream) {
  return table_reset("acrmi_tracks_reset", t, ids, n,
                     [](StateTable* st, const SmoothIds& k, int m, hipStream_t s) {
                       acrmi_tracks* t = static_cast<acrmi_tracks*>(st);
                       return launch_assoc_reset(k, m, t->max_hand, t->meta, t->init, s);
                     },
                     (hipStream_t)stream);
}

// what acrmi_associate and acrmi_forward_tracks check before anything is launched
static int check_tracks(acrmi_ctx* c, const acrmi_tracks* t, const int32_t* ids, int B, int max_hand, const char* who) {
  if (!t || !ids || B <= 0) return fail(c, ACRMI_EINVAL, "%s: bad arguments", who);
  if (max_hand < 1 || max_hand > ACRMI_MAX_HAND) return fail(c, ACRMI_EINVAL, "%s: max_hand %d outside 1..%d", who, max_hand, ACRMI_MAX_HAND);
  if (max_hand != t->max_hand) return fail(c, ACRMI_EINVAL, "%s: max_hand %d, the table holds %d slots per side", who, max_hand, t->max_hand);
  return check_table(c, t, ids, B, who);
}

// arguments valid for t.  Successive launches of SMOOTH_FRAMES_PER_LAUNCH frames on the stream, in frame order.
static int associate_on(acrmi_ctx* c, acrmi_tracks* t, float* slots, int B, const int32_t* ids, int smooth, int32_t* track_ids,
                        int32_t* perm, hipStream_t stream) {
  AssocArgs a{};
  a.s.state = t->state;
  a.s.init = t->init;
  smooth_coefficients(a.s, c ? c->smooth_coeff : 4.0f /* a new context's ACRMI_OPT_SMOOTH_COEFF */);
  a.meta = t->meta;
  a.K = t->max_hand; a.gate = t->gate; a.max_miss = t->max_miss; a.smooth = smooth ? 1 : 0;
  const size_t frame_rows = (size_t)2 * t->max_hand;
  TableOrder ord(t, stream);
  hipError_t e = ord.err;
  for (int f0 = 0; e == hipSuccess && f0 < B; f0 += SMOOTH_FRAMES_PER_LAUNCH) {
    const int m = B - f0 < SMOOTH_FRAMES_PER_LAUNCH ? B - f0 : SMOOTH_FRAMES_PER_LAUNCH;
    const int n_streams = smooth_plan(ids + f0, m, &a.s.b, t->last.data());
    bool any_loose = false;
    memset(a.loose, 0, sizeof a.loose);
    for (int i = 0; i < m; ++i)
      if (ids[f0 + i] < 0) { a.loose[i >> 5] |= 1u << (i & 31); any_loose = true; }
    a.m = m;
    a.s.slots = slots + (size_t)f0 * frame_rows * ACRMI_SLOT;
    a.track_ids = track_ids + (size_t)f0 * frame_rows;
    a.perm = perm ? perm + (size_t)f0 * frame_rows : nullptr;
    e = launch_associate(a, n_streams, any_loose, stream);
  }
  e = ord.done(e);
  return e == hipSuccess ? ACRMI_OK : fail(c, ACRMI_EHIP, "association: %s", hipGetErrorString(e));
}

int acrmi_associate(acrmi_ctx* c, acrmi_tracks* t, float* slots, int B, int max_hand, const int32_t* ids, int smooth,
                    int32_t* track_ids, int32_t* perm, void* stream) {
  if (!slots || !track_ids) return fail(c, ACRMI_EINVAL, "acrmi_associate: bad arguments");
  const int r = check_tracks(c, t, ids, B, max_hand, "acrmi_associate");
  if (r) return r;
  DeviceGuard guard_(t->device);
  if (guard_.err != hipSuccess) return fail(c, ACRMI_EHIP, "hipSetDevice(%d): %s", t->device, hipGetErrorString(guard_.err));
  return associate_on(c, t, slots, B, ids, smooth, track_ids, perm, (hipStream_t)stream);
}

int acrmi_program_groups(acrmi_ctx* c, int B) {
  if (!c) return fail(c, ACRMI_EINVAL, "acrmi_program_groups: bad arguments");
  if (!c->have_program) return fail(c, ACRMI_ESTATE, "no program");
  if (B <= 0 || B > c->max_batch) return fail(c, ACRMI_EINVAL, "batch %d outside 1..%d", B, c->max_batch);
  return c->sched[c->point_heads ? 1 : 0][B > AUTO_SMALL_BATCH ? 1 : 0].n_groups;
}

int acrmi_profile_ops(acrmi_ctx* c, const uint8_t* img, int B, float* ms_out, int n_ms, void* stream) {
  if (!c || !img || !ms_out) return fail(c, ACRMI_EINVAL, "acrmi_profile_ops: bad arguments");
  if (!c->have_program) return fail(c, ACRMI_ESTATE, "no program");
  const int n = (int)c->ops.size();
  if (n_ms < n) return fail(c, ACRMI_EINVAL, "ms_out too small (%d < %d)", n_ms, n);
  ON_DEVICE(c);
  hipStream_t s = (hipStream_t)stream;
  const bool point = c->point_heads;
  int r = run_program(c, img, B, stream, point);
  if (r) return r;
  std::vector<hipEvent_t> ev(n + 1, nullptr);
  auto cleanup = [&]() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  };
  hipError_t he = hipSuccess;
  for (auto& e : ev)
    if ((he = hipEventCreate(&e)) != hipSuccess) break;
  if (he == hipSuccess) he = hipEventRecord(ev[0], s);
  for (int i = 0; i < n && he == hipSuccess && r == ACRMI_OK; ++i) {
    if (op_active(c->ops[i], point)) r = run_op(c, c->ops[i], img, B, s);
    if (r == ACRMI_OK) he = hipEventRecord(ev[i + 1], s);
  }
  if (he == hipSuccess && r == ACRMI_OK) he = hipStreamSynchronize(s);
  for (int i = 0; i < n && he == hipSuccess && r == ACRMI_OK; ++i) he = hipEventElapsedTime(&ms_out[i], ev[i], ev[i + 1]);
  cleanup();
  if (r) return r;
  if (he != hipSuccess) return fail(c, ACRMI_EHIP, "acrmi_profile_ops: %s", hipGetErrorString(he));
  if (B <= AUTO_SMALL_BATCH) {      // the small-batch schedules are planned from these times (ACRMI_OPT_LANE_PLAN)
    c->op_ms[point ? 1 : 0].assign(ms_out, ms_out + n);
    build_schedule(c, point, false);
  }
  return n;
}

void* acrmi_buffer_ptr(acrmi_ctx* c, int buf, int* h, int* w, int* cs) {
  if (!c || !c->have_program || buf < 0 || buf >= (int)c->bufs.size()) return nullptr;
  if (h) *h = c->bufs[buf].h;
  if (w) *w = c->bufs[buf].w;
  if (cs) *cs = c->bufs[buf].cs;
  return c->buf_ptr[buf];
}

int acrmi_buffer_dtype(acrmi_ctx* c, int buf) {
  if (!c || !c->have_program || buf < 0 || buf >= (int)c->bufs.size()) return -1;
  return c->bufs[buf].dtype;
}

// The decode of the context's head buffers: the classic one, one hand per side, with the optional gate - or (top_k) the
// max_hand best centres of each side.  Two different paths also at max_hand 1 (acrmi_ops.hip).
static int decode_ctx(acrmi_ctx* c, const char* who, int B, const int32_t* prior_gate, bool top_k, int max_hand, float* slots,
                      void* stream) {
  if (!c || !slots) return fail(c, ACRMI_EINVAL, "%s: bad arguments", who);
  if (top_k && (max_hand < 1 || max_hand > ACRMI_MAX_HAND))
    return fail(c, ACRMI_EINVAL, "%s: max_hand %d outside 1..%d", who, max_hand, ACRMI_MAX_HAND);
  if (!c->have_program) return fail(c, ACRMI_ESTATE, "%s: no program", who);
  if (B <= 0 || B > c->max_batch) return fail(c, ACRMI_EINVAL, "batch %d outside 1..%d", B, c->max_batch);
  ON_DEVICE(c);
  const acrmi_head_layout& h = c->heads;
  return from_global(c, decode_maps_impl(c->buf_ptr[h.center_buf[0]], c->buf_ptr[h.center_buf[1]], c->bufs[h.center_buf[0]].cs,
                                         c->buf_ptr[h.params_buf[0]], c->buf_ptr[h.params_buf[1]], c->bufs[h.params_buf[0]].cs,
                                         c->buf_ptr[h.prior_buf[0]], c->buf_ptr[h.prior_buf[1]], c->bufs[h.prior_buf[0]].cs, B,
                                         c->conf_thresh, prior_gate, c->range_flag, slots, stream, top_k ? max_hand : 0));
}

int acrmi_decode(acrmi_ctx* c, int B, float* slots, void* stream) { return acrmi_decode_gated(c, B, nullptr, slots, stream); }

int acrmi_decode_gated(acrmi_ctx* c, int B, const int32_t* prior_gate, float* slots, void* stream) {
  return decode_ctx(c, "acrmi_decode", B, prior_gate, false, 0, slots, stream);
}

int acrmi_decode_multi(acrmi_ctx* c, int B, int max_hand, float* slots, void* stream) {
  return decode_ctx(c, "acrmi_decode_multi", B, nullptr, true, max_hand, slots, stream);
}

int acrmi_prior_gate(acrmi_ctx* c, const float* slots, int B, int32_t* gate, void* stream) {
  if (!slots || !gate || B <= 0) return fail(c, ACRMI_EINVAL, "acrmi_prior_gate: bad arguments");
  if (c) {
    ON_DEVICE(c);
    return from_global(c, acrmi_prior_gate(nullptr, slots, B, gate, stream));
  }
  HIPCHK(c, launch_prior_gate(slots, B, gate, (hipStream_t)stream));      // stand-alone (like acrmi_decode_maps): current device
  return ACRMI_OK;
}

int acrmi_check_range(acrmi_ctx* c, void* stream) {
  if (!c) return fail(c, ACRMI_EINVAL, "acrmi_check_range: ctx is NULL");
  if (!c->range_flag) return ACRMI_OK;      // no split-f16 convolution in the program: nothing can overflow
  ON_DEVICE(c);
  unsigned v = 0;
  HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));
  HIPCHK(c, hipMemcpy(&v, c->range_flag, sizeof(v), hipMemcpyDeviceToHost));
  if (!v) return ACRMI_OK;
  // cleared ON the caller's stream (the streams of acrmi_stream_create are non-blocking: a null-stream memset is not ordered
  // against work the caller queues next and could wipe a later launch's flag), then waited for
  HIPCHK(c, hipMemsetAsync(c->range_flag, 0, sizeof(v), (hipStream_t)stream));
  HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));
  return fail(c, ACRMI_ERANGE, "an activation of the 'fp16x3' program left the f16 range (|x| > 65504): its split halves are "
                               "inf / -inf and the results since the last check are invalid (slots and meshes were written as "
                               "NaN); use precision 'bf16x3' or 'fp32' for this checkpoint");
}

// MANO of H rows the caller names one by one: what acrmi_mano and acrmi_mano_rotmat share.  m holds the poses and whatever
// only one of the two knows.
static int mano_rows(acrmi_ctx* c, const char* who, ManoArgs& m, const float* betas, int beta_stride, const int32_t* side, int H,
                     int center_idx, float* verts, float* joints, float* center, void* stream) {
  if (!c) return fail(c, ACRMI_EINVAL, "%s: ctx is NULL", who);
  if (H == 0) return ACRMI_OK;    // ManoLayer accepts N == 0 (acr/mano_wrapper.py:43 comment)
  if (H < 0 || !m.poses || !betas || !verts || !joints || center_idx >= 21) return fail(c, ACRMI_EINVAL, "%s: bad arguments", who);
  if (!c->have_mano[0] && !c->have_mano[1]) return fail(c, ACRMI_ESTATE, "%s: MANO tables not loaded", who);
  ON_DEVICE(c);
  // a context may hold one side only (a lone ManoLayer); rows must then all be of that side
  m.t[0] = c->have_mano[0] ? c->mano[0] : c->mano[1];
  m.t[1] = c->have_mano[1] ? c->mano[1] : c->mano[0];
  m.betas = betas; m.beta_stride = beta_stride;
  m.side = side; m.H = H; m.center_idx = center_idx;
  m.verts = verts; m.joints = joints; m.center = center;
  m.off_div = 1;
  m.lbs_f16 = c->mano_f16;
  HIPCHK(c, launch_mano(m, (hipStream_t)stream));
  return ACRMI_OK;
}

int acrmi_mano(acrmi_ctx* c, const float* poses, int pose_stride, const float* betas, int beta_stride,
               const int32_t* side, int H, int center_idx, float* verts, float* joints, float* center,
               const float* cam, int cam_stride, const float* offsets, float* verts_camed, float* pj2d,
               float* pj2d_org, void* stream) {
  ManoArgs m{};
  m.poses = poses; m.pose_stride = pose_stride;
  m.cam = cam; m.cam_stride = cam_stride; m.offsets = offsets;
  m.verts_camed = verts_camed; m.pj2d = pj2d; m.pj2d_org = pj2d_org;
  return mano_rows(c, "acrmi_mano", m, betas, beta_stride, side, H, center_idx, verts, joints, center, stream);
}

int acrmi_mano_rotmat(acrmi_ctx* c, const float* rotmats, const float* betas, int beta_stride, const int32_t* side, int H,
                      int center_idx, float* verts, float* joints, float* center, void* stream) {
  ManoArgs m{};
  m.poses = rotmats; m.pose_stride = 144; m.pose_rotmat = 1;
  return mano_rows(c, "acrmi_mano_rotmat", m, betas, beta_stride, side, H, center_idx, verts, joints, center, stream);
}

int acrmi_mano_backward(acrmi_ctx* c, const float* poses, int pose_stride, const float* betas, int beta_stride,
                        const int32_t* side, int H, int center_idx, const float* g_verts, const float* g_joints,
                        const float* g_center, float* g_poses, float* g_betas, void* stream) {
  if (!c) return fail(c, ACRMI_EINVAL, "acrmi_mano_backward: ctx is NULL");
  if (H < 0 || center_idx < -1 || center_idx > 20 || pose_stride < 48 || beta_stride < 10)
    return fail(c, ACRMI_EINVAL, "acrmi_mano_backward: bad arguments (H >= 0, center_idx -1..20, pose_stride >= 48, beta_stride >= 10)");
  if (H == 0) return ACRMI_OK;
  if (!poses || !betas || !g_poses || !g_betas) return fail(c, ACRMI_EINVAL, "acrmi_mano_backward: NULL poses, betas or outputs");
  if (!c->have_mano[0] && !c->have_mano[1]) return fail(c, ACRMI_ESTATE, "acrmi_mano_backward: MANO tables not loaded");
  ON_DEVICE(c);
  if (!g_verts && !g_joints && !g_center) {      // no cotangent at all: the gradients are zero
    HIPCHK(c, hipMemsetAsync(g_poses, 0, (size_t)H * 48 * sizeof(float), (hipStream_t)stream));
    HIPCHK(c, hipMemsetAsync(g_betas, 0, (size_t)H * 10 * sizeof(float), (hipStream_t)stream));
    return ACRMI_OK;
  }
  ManoGradArgs m{};
  // a context may hold one side only (a lone ManoLayer), as in acrmi_mano
  m.t[0] = c->have_mano[0] ? c->mano[0] : c->mano[1];
  m.t[1] = c->have_mano[1] ? c->mano[1] : c->mano[0];
  m.poses = poses; m.pose_stride = pose_stride;
  m.betas = betas; m.beta_stride = beta_stride;
  m.side = side; m.H = H; m.center_idx = center_idx;
  m.g_verts = g_verts; m.g_joints = g_joints; m.g_center = g_center;
  m.g_poses = g_poses; m.g_betas = g_betas;
  HIPCHK(c, launch_mano_backward(m, (hipStream_t)stream));
  return ACRMI_OK;
}

int acrmi_mano_fit_state_floats(void) { return FIT_STATE; }

int acrmi_mano_fit(acrmi_ctx* c, float* state, const int32_t* side, int H, int center_idx, const float* y3, const float* w3,
                   const float* y2, const float* w2, const float* yv, const float* wv, const float* prior, double lam_pose,
                   double lam_beta, const double* lr5, double b1, double b2, double eps, int steps, int dense, float* poses,
                   float* betas, float* trans, float* cam, float* loss, float* grad, void* stream) {
  if (!c) return fail(c, ACRMI_EINVAL, "acrmi_mano_fit: ctx is NULL");
  if (H < 0 || !fit_steps_ok(steps) || !fit_center_ok(center_idx))
    return fail(c, ACRMI_EINVAL, "acrmi_mano_fit: bad arguments (H >= 0, steps 0..%d, center_idx -1..20)", FIT_MAX_STEPS);
  if (!state || !lr5) return fail(c, ACRMI_EINVAL, "acrmi_mano_fit: NULL state or learning rates");
  if (!(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0 && eps >= 0.0 && lam_pose >= 0.0 && lam_beta >= 0.0))
    return fail(c, ACRMI_EINVAL, "acrmi_mano_fit: b1 and b2 must lie in [0, 1), eps and the regulariser weights must not be negative");
  for (int g = 0; g < FIT_GROUPS; ++g)
    if (!(lr5[g] >= 0.0)) return fail(c, ACRMI_EINVAL, "acrmi_mano_fit: a learning rate is negative or NaN");
  if (H == 0) return ACRMI_OK;
  if (!poses || !betas || !trans || !cam || !loss) return fail(c, ACRMI_EINVAL, "acrmi_mano_fit: NULL outputs");
  if (!c->have_mano[0] && !c->have_mano[1]) return fail(c, ACRMI_ESTATE, "acrmi_mano_fit: MANO tables not loaded");
  ON_DEVICE(c);
  ManoFitArgs m{};
  // a context may hold one side only (a lone ManoLayer), as in acrmi_mano
  m.t[0] = c->have_mano[0] ? c->mano[0] : c->mano[1];
  m.t[1] = c->have_mano[1] ? c->mano[1] : c->mano[0];
  m.state = state; m.side = side; m.H = H; m.center_idx = center_idx;
  m.y3 = y3; m.w3 = w3; m.y2 = y2; m.w2 = w2; m.yv = yv; m.wv = wv; m.prior = prior;
  m.lam_pose = lam_pose; m.lam_beta = lam_beta;
  for (int g = 0; g < FIT_GROUPS; ++g) m.lr[g] = lr5[g];
  m.b1 = b1; m.b2 = b2; m.eps = eps;
  m.steps = steps; m.dense = dense;
  m.poses = poses; m.betas = betas; m.trans = trans; m.cam = cam; m.loss = loss; m.grad = grad;
  HIPCHK(c, launch_mano_fit(m, (hipStream_t)stream));
  return ACRMI_OK;
}

// The last op that writes the backbone map (heads.backbone_buf) and the channels it leaves there: an op whose out_buf is the
// map - or, in large-batch fp32 programs, the ACRMI_CONV_DUAL convolution whose SECOND output (aux_buf: the full-resolution HR
// fuse sum of the last stage, written at channel 0) is the map.  first = the op behind it (-1: none), c0 = channels.
static void backbone_writer(const acrmi_ctx* c, int* first, int* c0) {
  const int bb = c->heads.backbone_buf;
  *first = -1;
  *c0 = 0;
  for (int i = 0; i < (int)c->ops.size(); ++i) {
    const acrmi_op& op = c->ops[i];
    if (op.kind == ACRMI_OP_COORDFILL) continue;
    if (op.out_buf == bb) {
      *first = i + 1;
      *c0 = op.out_coff + op.cout * (op.kind == ACRMI_OP_CONV ? op.groups : 1);
    } else if (op.kind == ACRMI_OP_CONV && (op.flags & ACRMI_CONV_DUAL) && op.aux_buf == bb) {
      *first = i + 1;
      *c0 = op.cout;
    }
  }
}

int acrmi_heads(acrmi_ctx* c, const float* feat_nchw, int B, void* stream) {
  if (!c || !feat_nchw) return fail(c, ACRMI_EINVAL, "acrmi_heads: bad arguments");
  if (!c->have_program) return fail(c, ACRMI_ESTATE, "acrmi_heads: no program");
  if (B <= 0 || B > c->max_batch) return fail(c, ACRMI_EINVAL, "batch %d outside 1..%d", B, c->max_batch);
  const int bb = c->heads.backbone_buf;
  const acrmi_buffer_desc& d = c->bufs[bb];
  if (d.dtype != ACRMI_DT_F32)
    return fail(c, ACRMI_EINVAL, "acrmi_heads: the program stores its backbone output in 16 bits; features are taken by "
                                 "fp32-storage programs (fp32, fp16x3, bf16x3)");
  // the head ops = everything behind the last op that writes the backbone map (acr/model.py:47: head_forward starts there)
  int first = -1, c0 = 0;
  backbone_writer(c, &first, &c0);
  if (first < 0 || c0 <= 0 || c0 > d.cs) return fail(c, ACRMI_ESTATE, "acrmi_heads: the program has no backbone output op");
  ON_DEVICE(c);
  HIPCHK(c, launch_nchw_to_nhwc(feat_nchw, B, c0, d.h, d.w, c->buf_ptr[bb], d.cs, 0, (hipStream_t)stream));
  return run_program(c, nullptr, B, stream, /*point=*/false, first);
}

int acrmi_backbone_channels(acrmi_ctx* c) {
  if (!c || !c->have_program) return fail(c, ACRMI_ESTATE, "acrmi_backbone_channels: no program");
  int first = -1, c0 = 0;
  backbone_writer(c, &first, &c0);
  return c0;
}

// ---- the fused forward calls ------------------------------------------------------------------------------------------------
// MANO of the rows_per_frame * n_frames rows of slots [n_frames,rows_per_frame,ACRMI_SLOT] (side = row & 1), placeholders included
static int mano_from_slots(acrmi_ctx* c, float* slots, int rows_per_frame, int n_frames, const float* offsets, float* verts,
                           float* joints, float* verts_camed, float* pj2d, float* pj2d_org, hipStream_t stream) {
  ManoArgs m{};
  m.t[0] = c->mano[0]; m.t[1] = c->mano[1];
  m.poses = slots + ACRMI_SLOT_POSES; m.pose_stride = ACRMI_SLOT;
  m.betas = slots + ACRMI_SLOT_BETAS; m.beta_stride = ACRMI_SLOT;
  m.side = nullptr; m.H = rows_per_frame * n_frames; m.center_idx = c->center_idx;
  m.verts = verts; m.joints = joints; m.center = nullptr;
  const bool proj = verts_camed || pj2d || pj2d_org;
  m.cam = proj ? slots + ACRMI_SLOT_CAM : nullptr; m.cam_stride = ACRMI_SLOT;
  m.offsets = offsets; m.off_div = rows_per_frame;
  m.verts_camed = verts_camed; m.pj2d = pj2d; m.pj2d_org = pj2d_org;
  m.lbs_f16 = c->mano_f16;
  HIPCHK(c, launch_mano(m, stream));
  return ACRMI_OK;
}

// What distinguishes the four acrmi_forward* calls: the step between decode and MANO (acr/main.py:69-83), and whether the
// caller names a hand count.
struct ForwardKind {
  // OPTION: what ACRMI_OPT_TEMPORAL says - nothing, or the frames as one stream on the context's own table;
  // STREAMS: `streams` + ids; TRACKS: `tracks` + ids, smooth, track_ids (the track table takes the place of the smoothing)
  enum { OPTION, STREAMS, TRACKS } temporal = OPTION;
  bool multi = false;      // acrmi_forward_multi / _tracks: max_hand is the caller's, and ACRMI_OPT_POINT_HEADS_MULTI, not
                           // ACRMI_OPT_POINT_HEADS, says whether the point variant of the program runs
  acrmi_streams* streams = nullptr;
  acrmi_tracks* tracks = nullptr;
  const int32_t* ids = nullptr;
  int smooth = 0;
  int32_t* track_ids = nullptr;
};

// program + decode + temporal step + MANO on one stream.  max_hand: 0 with the calls that have none; up to 1 the classic decode
// with every option of acrmi_forward, above the top-K decode.
static int fused_forward(acrmi_ctx* c, const char* who, const ForwardKind& k, int max_hand, const uint8_t* img, int B,
                         const float* offsets, float* slots, float* verts, float* joints, float* verts_camed, float* pj2d,
                         float* pj2d_org, void* stream) {
  if (!c || !slots || !verts || !joints || (k.temporal == ForwardKind::TRACKS && !k.track_ids))
    return fail(c, ACRMI_EINVAL, "%s: bad arguments", who);
  int r = ACRMI_OK;
  if (k.temporal == ForwardKind::STREAMS) r = check_streams(c, k.streams, k.ids, B, who);
  else if (k.temporal == ForwardKind::TRACKS) r = check_tracks(c, k.tracks, k.ids, B, max_hand, who);
  else if (k.multi && (max_hand < 1 || max_hand > ACRMI_MAX_HAND))
    r = fail(c, ACRMI_EINVAL, "%s: max_hand %d outside 1..%d", who, max_hand, ACRMI_MAX_HAND);
  if (r) return r;
  // the batch-wide prior rules and the smoothing filters know one hand of each side per frame (the reference cannot run
  // either with more: acr/result_parser.py:134, acr/main.py:77)
  if (max_hand > 1 && c->batch_prior) return fail(c, ACRMI_EINVAL, "%s: ACRMI_OPT_BATCH_PRIOR with max_hand %d > 1", who, max_hand);
  if (max_hand > 1 && k.temporal == ForwardKind::OPTION && c->temporal)
    return fail(c, ACRMI_EINVAL, "%s: ACRMI_OPT_TEMPORAL with max_hand %d > 1", who, max_hand);
  if (!c->have_mano[0] || !c->have_mano[1]) return fail(c, ACRMI_ESTATE, "%s: MANO tables not loaded", who);
  ON_DEVICE(c);
  // the calls with a hand count: the dense heads unless ACRMI_OPT_POINT_HEADS_MULTI asks for the towers at the top max_hand centres
  const bool point = k.multi ? c->point_heads_multi : c->point_heads;
  if ((r = run_program(c, img, B, stream, point, 0, k.multi ? max_hand : 1))) return r;
  hipStream_t s = (hipStream_t)stream;
  if (max_hand > 1) {
    if ((r = acrmi_decode_multi(c, B, max_hand, slots, stream))) return r;
  } else {
    if ((r = acrmi_decode(c, B, slots, stream))) return r;
    if (c->batch_prior && B > 1) {
      // the reference's batch-wide prior rules (acr/result_parser.py:42-47, 102-145), all on the device: the first decode's flags
      // and centers -> one decision per frame -> a second decode that applies it (the decode is ~40 us per 64 frames)
      HIPCHK(c, launch_prior_gate(slots, B, c->gate_buf, s));
      if ((r = acrmi_decode_gated(c, B, c->gate_buf, slots, stream))) return r;
    }
  }
  if (k.temporal == ForwardKind::TRACKS) r = associate_on(c, k.tracks, slots, B, k.ids, k.smooth, k.track_ids, nullptr, s);
  else if (k.temporal == ForwardKind::STREAMS) r = smooth_on(c, k.streams, slots, B, k.ids, s);
  else if (c->temporal) r = acrmi_smooth(c, slots, B, stream);
  if (r) return r;
  return mano_from_slots(c, slots, max_hand > 1 ? 2 * max_hand : 2, B, offsets, verts, joints, verts_camed, pj2d, pj2d_org, s);
}

int acrmi_forward(acrmi_ctx* c, const uint8_t* img, int B, const float* offsets, float* slots, float* verts,
                  float* joints, float* verts_camed, float* pj2d, float* pj2d_org, void* stream) {
  return fused_forward(c, "acrmi_forward", ForwardKind{}, 0, img, B, offsets, slots, verts, joints, verts_camed, pj2d, pj2d_org,
                       stream);
}

int acrmi_forward_multi(acrmi_ctx* c, const uint8_t* img, int B, int max_hand, const float* offsets, float* slots, float* verts,
                        float* joints, float* verts_camed, float* pj2d, float* pj2d_org, void* stream) {
  ForwardKind k;
  k.multi = true;
  return fused_forward(c, "acrmi_forward_multi", k, max_hand, img, B, offsets, slots, verts, joints, verts_camed, pj2d, pj2d_org,
                       stream);
}

int acrmi_forward_tracks(acrmi_ctx* c, acrmi_tracks* t, const int32_t* ids, int smooth, const uint8_t* img, int B, int max_hand,
                         const float* offsets, float* slots, float* verts, float* joints, float* verts_camed, float* pj2d,
                         float* pj2d_org, int32_t* track_ids, void* stream) {
  ForwardKind k;
  k.temporal = ForwardKind::TRACKS; k.multi = true;
  k.tracks = t; k.ids = ids; k.smooth = smooth; k.track_ids = track_ids;
  return fused_forward(c, "acrmi_forward_tracks", k, max_hand, img, B, offsets, slots, verts, joints, verts_camed, pj2d, pj2d_org,
                       stream);
}

int acrmi_forward_streams(acrmi_ctx* c, acrmi_streams* t, const int32_t* ids, const uint8_t* img, int B, const float* offsets,
                          float* slots, float* verts, float* joints, float* verts_camed, float* pj2d, float* pj2d_org, void* stream) {
  ForwardKind k;
  k.temporal = ForwardKind::STREAMS;
  k.streams = t; k.ids = ids;
  return fused_forward(c, "acrmi_forward_streams", k, 0, img, B, offsets, slots, verts, joints, verts_camed, pj2d, pj2d_org,
                       stream);
}

// ---- mesh overlay (csrc/render.hip) --------------------------------------------------------------------------------
int acrmi_load_faces(acrmi_ctx* c, int side, const int32_t* faces_host, int n_faces) {
  if (!c || side < 0 || side > 1 || !faces_host || n_faces <= 0) return fail(c, ACRMI_EINVAL, "acrmi_load_faces: bad arguments");
  if (c->faces_topo[1 - side] && c->n_faces[1 - side] != n_faces)
    return fail(c, ACRMI_EINVAL, "acrmi_load_faces: %d faces, the other side has %d (one face count for both hands)", n_faces,
                c->n_faces[1 - side]);
  std::vector<int32_t> blob((size_t)mesh_topology_ints(n_faces, 778));
  if (!build_mesh_topology(faces_host, n_faces, 778, blob.data()))
    return fail(c, ACRMI_EINVAL, "acrmi_load_faces: a face names a vertex outside [0, 778)");
  ON_DEVICE(c);
  HIPCHK(c, hipDeviceSynchronize());      // a reload: nothing of an earlier launch may still read the old table
  if (c->faces_topo[side]) (void)hipFree(c->faces_topo[side]);
  c->faces_topo[side] = nullptr;
  c->n_faces[side] = 0;
  int32_t* d = nullptr;
  HIPCHK(c, hipMalloc(&d, blob.size() * sizeof(int32_t)));
  const hipError_t e = hipMemcpy(d, blob.data(), blob.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return fail(c, ACRMI_EHIP, "acrmi_load_faces: hipMemcpy: %s", hipGetErrorString(e));
  }
  c->faces_topo[side] = d;
  c->n_faces[side] = n_faces;
  c->faces_host[side].assign(faces_host, faces_host + 3 * (size_t)n_faces);      // (validated by build_mesh_topology above)
  update_contact_sign(c, side);
  return ACRMI_OK;
}

// The context's render scratch for B frames (or regions) of two hands: [mesh_frame | mesh_topo | rgb | view rows] and the
// rasteriser's workspace behind them.  The head is sized for one view row per MESH, the larger of the two layouts.
struct RenderScratch {
  int32_t *mesh_frame, *mesh_topo;      // [2B] each
  float *rgb, *view;                    // [2B,3]; [B,4] per frame or [2B,4] per mesh
  char* ws;
};
static size_t render_head_bytes(int B) {
  const size_t M = 2 * (size_t)B;
  return (M * 4 * 2 + M * 3 * 4 + M * 4 * 4 + 255) / 256 * 256;
}

// Allocates at the first call and when B grows: the one place the render calls allocate.
static int render_scratch(acrmi_ctx* c, int B, RenderScratch* sc) {
  if (B > c->render_ws_frames) {
    if (c->render_ws) {
      HIPCHK(c, hipDeviceSynchronize());
      (void)hipFree(c->render_ws);
      c->render_ws = nullptr;
      c->render_ws_frames = 0;
    }
    HIPCHK(c, hipMalloc(&c->render_ws, render_head_bytes(B) + render_workspace_bytes(2 * B, c->n_faces[0])));
    c->render_ws_frames = B;
  }
  sc->mesh_frame = (int32_t*)c->render_ws;
  sc->mesh_topo = sc->mesh_frame + 2 * B;
  sc->rgb = (float*)(sc->mesh_topo + 2 * B);
  sc->view = sc->rgb + 3 * 2 * B;
  sc->ws = c->render_ws + render_head_bytes(B);
  return ACRMI_OK;
}

// the reference's colours by hand type (acr/visualization.py:76), as RGB
static const float kHandColors[6] = {0.46f, 0.59f, 0.64f, 0.94f, 0.71f, 0.53f};

// the n_meshes hands the prep kernel described in sc, drawn into n_frames frames; one of view / mesh_view (or neither)
static hipError_t render_launch(const acrmi_ctx* c, const RenderScratch& sc, const float* verts, const float* cam_trans,
                                const float* view, const float* mesh_view, float focal, float visible_weight, const uint8_t* img_in,
                                uint8_t* img_out, int32_t* ids_out, int n_meshes, int n_frames, int H, int W, hipStream_t stream,
                                const float* vcol = nullptr) {
  RenderArgs a{};
  a.verts = verts; a.trans = cam_trans; a.topo[0] = c->faces_topo[0]; a.topo[1] = c->faces_topo[1];
  a.mesh_topo = sc.mesh_topo; a.mesh_frame = sc.mesh_frame; a.rgb = sc.rgb; a.view = view; a.mesh_view = mesh_view;
  a.focal = focal; a.visible_weight = visible_weight; a.img_in = img_in; a.img_out = img_out; a.ids_out = ids_out;
  a.ws = sc.ws; a.vcol = vcol;
  a.n_meshes = n_meshes; a.n_verts = 778; a.n_faces = c->n_faces[0]; a.n_frames = n_frames; a.H = H; a.W = W;
  return launch_render(a, stream);
}

// acrmi_render / acrmi_render_colored (colored: vcol must be there; B * 2 * 778 * 3 colours within 2^31 - 1)
static int render_call(acrmi_ctx* c, const char* who, bool colored, const float* vcol, const float* verts, const float* cam_trans,
                       const float* slots, int B, const float* offsets, const float* colors_host, float focal, float visible_weight,
                       const uint8_t* img_in, uint8_t* img_out, int H, int W, int32_t* ids_out, void* stream) {
  if (!c || !verts || !cam_trans || !slots || !img_in || !img_out || B <= 0 || H <= 0 || W <= 0 || !(focal > 0.f) ||
      !(visible_weight >= 0.f && visible_weight <= 1.f) || (colored && (!vcol || !vertex_color_sizes_ok(2ll * B, 778))))
    return fail(c, ACRMI_EINVAL, "%s: bad arguments", who);
  if (!c->faces_topo[0] || !c->faces_topo[1]) return fail(c, ACRMI_ESTATE, "%s: MANO faces not loaded (acrmi_load_faces)", who);
  ON_DEVICE(c);
  RenderScratch sc;
  if (int r = render_scratch(c, B, &sc)) return r;
  hipError_t e = launch_render_prep(slots, offsets, B, ACRMI_SLOT, ACRMI_SLOT_FLAG, colors_host ? colors_host : kHandColors,
                                    sc.mesh_frame, sc.mesh_topo, sc.rgb, sc.view, (hipStream_t)stream);
  if (e != hipSuccess) return fail(c, ACRMI_EHIP, "render prep: %s", hipGetErrorString(e));
  e = render_launch(c, sc, verts, cam_trans, offsets ? sc.view : nullptr, nullptr, focal, visible_weight, img_in, img_out, ids_out,
                    2 * B, B, H, W, (hipStream_t)stream, vcol);
  return e == hipSuccess ? ACRMI_OK : fail(c, ACRMI_EHIP, "render: %s", hipGetErrorString(e));
}

int acrmi_render(acrmi_ctx* c, const float* verts, const float* cam_trans, const float* slots, int B, const float* offsets,
                 const float* colors_host, float focal, float visible_weight, const uint8_t* img_in, uint8_t* img_out, int H,
                 int W, int32_t* ids_out, void* stream) {
  return render_call(c, "acrmi_render", false, nullptr, verts, cam_trans, slots, B, offsets, colors_host, focal, visible_weight,
                     img_in, img_out, H, W, ids_out, stream);
}

int acrmi_render_colored(acrmi_ctx* c, const float* verts, const float* cam_trans, const float* slots, int B, const float* offsets,
                         const float* colors_host, const float* vcol, float focal, float visible_weight, const uint8_t* img_in,
                         uint8_t* img_out, int H, int W, int32_t* ids_out, void* stream) {
  return render_call(c, "acrmi_render_colored", true, vcol, verts, cam_trans, slots, B, offsets, colors_host, focal,
                     visible_weight, img_in, img_out, H, W, ids_out, stream);
}

// ---- contact between the hands of a row (csrc/contact.hip) ---------------------------------------------------------------
int acrmi_contact(acrmi_ctx* c, const float* verts, const float* cam_trans, const float* slots, int B, int K, const int32_t* sign_host,
                  float contact_dist, float max_depth, int32_t* nn, float* d2, float* s_out, float* sum_f, int32_t* sum_i,
                  void* stream) {
  ContactArgs a{};
  a.nn = nn; a.side = s_out;
  return contact_call(c, "acrmi_contact", &acrmi_ctx::contact_ws, launch_contact, a, {nn, s_out}, verts, cam_trans, slots, B, K,
                      sign_host || !c ? sign_host : c->contact_sign, contact_dist, max_depth, d2, sum_f, sum_i, stream);
}

// The surface measure of the same pairs.  It has no orientation sign: the prep kernel's sign array is written and not read.
int acrmi_surface_contact(acrmi_ctx* c, const float* verts, const float* cam_trans, const float* slots, int B, int K,
                          float contact_dist, float max_depth, int32_t* face, float* d2, float* point, int32_t* cross, float* sum_f,
                          int32_t* sum_i, void* stream) {
  static const int32_t kNoSign[2] = {1, 1};
  SurfaceContactArgs a{};
  a.face = face; a.cross = cross; a.point = point;
  return contact_call(c, "acrmi_surface_contact", &acrmi_ctx::surface_ws, launch_surface_contact, a, {face, point, cross}, verts,
                      cam_trans, slots, B, K, kNoSign, contact_dist, max_depth, d2, sum_f, sum_i, stream);
}

// ---- the hands of a forward call against ground truth (csrc/score.hip; csrc/score_plan.h) --------------------------------
int acrmi_score_hands(acrmi_ctx* c, const float* joints, const float* verts, const float* slots, const float* cam_trans,
                      const float* gt_joints, const float* gt_verts, const uint8_t* joint_valid, const int32_t* group, int B, int K,
                      int n_groups, int n_bins, double bin_width, void* board, float* j_e_ra, float* j_e_pa, float* j_row_f,
                      int32_t* j_row_i, float* v_e_ra, float* v_e_pa, float* v_row_f, int32_t* v_row_i, float* pair_err,
                      void* stream) {
  const char* who = "acrmi_score_hands";
  if (!c) return fail(c, ACRMI_EINVAL, "%s: ctx is NULL", who);
  if (B <= 0 || K < 1 || K > ACRMI_MAX_HAND) return fail(c, ACRMI_EINVAL, "%s: %d frames, max_hand %d outside 1..%d", who, B, K, ACRMI_MAX_HAND);
  if (!score_groups_ok(n_groups)) return fail(c, ACRMI_EINVAL, "%s: n_groups %d outside 1..%d", who, n_groups, SCORE_MAX_GROUPS);
  if (board && !score_bins_ok(n_bins, bin_width))
    return fail(c, ACRMI_EINVAL, "%s: n_bins in 1..%d, bin_width finite and > 0", who, SCORE_MAX_BINS);
  const long long N = 2ll * B * K;
  if (N > 0x7fffffffll || !score_sizes_ok(N, 778)) return fail(c, ACRMI_EINVAL, "%s: %d frames of %d pairs are beyond 2^31 - 1 elements", who, B, K);
  if (!joints || !slots || !gt_joints || !j_e_ra || !j_e_pa || !j_row_f || !j_row_i || !pair_err ||
      (gt_verts && (!verts || !v_e_ra || !v_e_pa || !v_row_f || !v_row_i)))
    return fail(c, ACRMI_EINVAL, "%s: a null pointer", who);
  if (((uintptr_t)board & 7) != 0) return fail(c, ACRMI_EINVAL, "%s: the board is not 8-byte aligned", who);
  ON_DEVICE(c);
  const int root = c->center_idx;
  ScoreArgs a{};
  a.set[0] = ScoreSet{joints, gt_joints, joint_valid, nullptr, nullptr, nullptr, cam_trans, j_e_ra, j_e_pa, j_row_f, j_row_i, nullptr,
                      pair_err, 21, root, 3, 0};
  // the vertices on the joints' origins: the root joint's rows, 63 floats apart, good where that joint is valid (root < 0: no
  // origins, like the joints)
  a.set[1] = ScoreSet{verts, gt_verts, nullptr, root >= 0 ? joints + 3 * root : nullptr, root >= 0 ? gt_joints + 3 * root : nullptr,
                      root >= 0 && joint_valid ? joint_valid + root : nullptr, cam_trans, v_e_ra, v_e_pa, v_row_f, v_row_i, nullptr,
                      nullptr, 778, -1, 63, 21};
  a.n_sets = gt_verts ? 2 : 1;
  a.group = group;
  a.group_side = 1;
  a.flags = slots + ACRMI_SLOT_FLAG;
  a.flag_stride = ACRMI_SLOT;
  a.N = (int)N;
  a.n_groups = n_groups;
  hipError_t e = launch_pose_errors(a, (hipStream_t)stream);
  if (e != hipSuccess) return fail(c, ACRMI_EHIP, "%s: %s", who, hipGetErrorString(e));
  if (!board) return ACRMI_OK;
  int64_t* b = (int64_t*)board;
  int64_t* pair_board = b + (score_board_bytes(21, n_groups, n_bins) + score_board_bytes(778, n_groups, n_bins)) / 8;
  for (int k = 0; k < a.n_sets; ++k) {
    const ScoreSet& st = a.set[k];
    const ScoreAccArgs acc{st.e_ra, st.e_pa, group, 1, a.flags, a.flag_stride, st.pair_err, a.N, st.n, n_groups, n_bins, bin_width,
                           b + (k ? score_board_bytes(21, n_groups, n_bins) / 8 : 0), k ? nullptr : pair_board};
    if ((e = launch_score_accumulate(acc, (hipStream_t)stream)) != hipSuccess)
      return fail(c, ACRMI_EHIP, "%s: accumulate: %s", who, hipGetErrorString(e));
  }
  return ACRMI_OK;
}

// ---- key-point skeleton / centre heat maps over the frames (csrc/overlay.hip) ------------------------------------------
// what acrmi_overlay (n = n_frames = its batch) and acrmi_overlay_regions check first
static int check_overlay(acrmi_ctx* c, const char* who, int what, const float* slots, const float* kps, int n, const uint8_t* img_in,
                         const uint8_t* out, const uint8_t* out2, int n_frames, int H, int W) {
  if (!c || !img_in || !out || n <= 0 || n_frames <= 0 || n_frames > OVERLAY_MAX_FRAMES || H <= 0 || W <= 0 || H > OVERLAY_MAX_DIM ||
      W > OVERLAY_MAX_DIM || (what != ACRMI_OVERLAY_SKELETON && what != ACRMI_OVERLAY_CENTERMAP))
    return fail(c, ACRMI_EINVAL, "%s: bad arguments", who);
  if (what == ACRMI_OVERLAY_SKELETON ? (!slots || !kps) : (!out2 || out2 == out || out2 == img_in))
    return fail(c, ACRMI_EINVAL, "%s: bad arguments", who);
  if (!c->have_program || c->last_batch <= 0) return fail(c, ACRMI_ESTATE, "%s: no program has run", who);
  return ACRMI_OK;
}

// the skeletons of n_hands hands, each drawn where its slot's flag says (hand h in frame h / 2) or into hand_frame[h]
static hipError_t skeleton_launch(const float* kps, const float* slots, const int32_t* hand_frame, int normalized, int n_hands,
                                  int n_frames, int H, int W, int bgr, const uint8_t* img_in, uint8_t* out, hipStream_t stream) {
  SkeletonArgs a{};
  a.kps = kps; a.hand_frame = hand_frame; a.normalized = normalized;
  if (slots) { a.slots = slots; a.slot_stride = ACRMI_SLOT; a.flag_at = ACRMI_SLOT_FLAG; }
  a.n_hands = n_hands; a.n_frames = n_frames; a.H = H; a.W = W; a.line_width = 3; a.circle_rad = 3;
  a.img_in = img_in; a.img_out = out;
  skeleton_default_colors(bgr != 0, a.colors);
  return launch_skeleton(a, stream);
}

// What HeatmapArgs and RegionHeatmapArgs share: the maps are the head buffers the last program run left for n frames (NHWC,
// channel 0, the buffer's channel stride between two cells); a 16-bit storage program's are converted to fp32 as the kernels
// stage them in LDS.
static int heatmap_fill(acrmi_ctx* c, const char* who, HeatmapBase& a, int n, const float* offsets, int bgr, const uint8_t* img_in,
                        uint8_t* out, uint8_t* out2, int H, int W) {
  if (n != c->last_batch)
    return fail(c, ACRMI_ESTATE, "%s: the resident centre maps are those of a batch of %d, not %d", who, c->last_batch, n);
  const acrmi_head_layout& hl = c->heads;
  const acrmi_buffer_desc& d = c->bufs[hl.center_buf[0]];
  a.maps[0] = c->buf_ptr[hl.center_buf[0]]; a.maps[1] = c->buf_ptr[hl.center_buf[1]];
  a.pix_stride = d.cs; a.frame_stride = (long long)d.h * d.w * d.cs; a.dtype = d.dtype;
  a.n = n; a.h = d.h; a.w = d.w; a.H = H; a.W = W; a.offsets = offsets; a.weight = 0.7f;
  a.img_in = img_in; a.out[0] = out; a.out[1] = out2;
  heatmap_default_lut(bgr != 0, a.lut);
  return ACRMI_OK;
}

int acrmi_overlay(acrmi_ctx* c, int what, const float* slots, const float* pj2d, int B, const float* offsets, int bgr,
                  const uint8_t* img_in, uint8_t* out, uint8_t* out2, int H, int W, void* stream) {
  if (int r = check_overlay(c, "acrmi_overlay", what, slots, pj2d, B, img_in, out, out2, B, H, W)) return r;
  ON_DEVICE(c);
  hipError_t e;
  if (what == ACRMI_OVERLAY_SKELETON) {
    e = skeleton_launch(pj2d, slots, nullptr, offsets ? 0 : 1, 2 * B, B, H, W, bgr, img_in, out, (hipStream_t)stream);
  } else {
    HeatmapArgs a{};
    if (int r = heatmap_fill(c, "acrmi_overlay", a, B, offsets, bgr, img_in, out, out2, H, W)) return r;
    e = launch_heatmap(a, (hipStream_t)stream);
  }
  return e == hipSuccess ? ACRMI_OK : fail(c, ACRMI_EHIP, "overlay: %s", hipGetErrorString(e));
}

// ---- the part segmentation of the last program run (csrc/segm.hip) -----------------------------------
int acrmi_segment(acrmi_ctx* c, int B, const float* offsets, float weight, const uint8_t* colors_host, int bgr,
                  const uint8_t* img_in, uint8_t* out, uint8_t* labels, int H, int W, void* stream) {
  const char* who = "acrmi_segment";
  if (!c) return fail(c, ACRMI_EINVAL, "%s: ctx is NULL", who);
  if (B <= 0) return fail(c, ACRMI_EINVAL, "%s: B = %d", who, B);
  if (!c->have_program || c->last_batch <= 0) return fail(c, ACRMI_ESTATE, "%s: no program has run", who);
  if (B != c->last_batch)
    return fail(c, ACRMI_ESTATE, "%s: the resident segmentation is that of a batch of %d, not %d", who, c->last_batch, B);
  const int id = c->heads.segm_buf;
  const acrmi_buffer_desc& d = c->bufs[id];
  if (d.dtype != ACRMI_DT_F32) return fail(c, ACRMI_ESTATE, "%s: the segmentation buffer is not fp32", who);
  ON_DEVICE(c);
  // 33 classes (background + 16 parts of each hand: what attpool reads from this buffer) at the buffer's own geometry and stride
  return segm_labels_call(c, who, (const float*)c->buf_ptr[id], (long long)d.h * d.w * d.cs, d.cs, B, d.h, d.w, 33, nullptr, offsets,
                          weight, colors_host, bgr, img_in, out, labels, H, W, stream);
}

// ---- views over regions (DESIGN.md "Views over regions") ------------------------------------------------------------------
static int render_regions_call(acrmi_ctx* c, const char* who, bool colored, const float* vcol, const float* verts,
                               const float* cam_trans, const float* slots, int n, const float* offsets, const int32_t* region_frame,
                               const float* colors_host, float focal, float visible_weight, const uint8_t* img_in, uint8_t* img_out,
                               int n_frames, int H, int W, int32_t* ids_out, void* stream) {
  if ((colored && (!vcol || n <= 0 || !vertex_color_sizes_ok(2ll * n, 778))) || !c || !verts || !cam_trans || !slots || !offsets || !region_frame || !img_in || !img_out || n <= 0 || n_frames <= 0 ||
      n_frames > OVERLAY_MAX_FRAMES || H <= 0 || W <= 0 || H > OVERLAY_MAX_DIM || W > OVERLAY_MAX_DIM || !(focal > 0.f) ||
      !(visible_weight >= 0.f && visible_weight <= 1.f) || n > 0x3fffffff || (c->n_faces[0] > 0 && 2ll * n * c->n_faces[0] > 0x7fffffffll))
    return fail(c, ACRMI_EINVAL, "%s: bad arguments", who);
  if (!c->faces_topo[0] || !c->faces_topo[1]) return fail(c, ACRMI_ESTATE, "%s: MANO faces not loaded (acrmi_load_faces)", who);
  ON_DEVICE(c);
  RenderScratch sc;
  if (int r = render_scratch(c, n, &sc)) return r;
  hipError_t e = launch_render_region_prep(slots, offsets, region_frame, n, n_frames, H, W, ACRMI_SLOT, ACRMI_SLOT_FLAG,
                                           colors_host ? colors_host : kHandColors, sc.mesh_frame, sc.mesh_topo, sc.rgb, sc.view,
                                           (hipStream_t)stream);
  if (e != hipSuccess) return fail(c, ACRMI_EHIP, "render region prep: %s", hipGetErrorString(e));
  e = render_launch(c, sc, verts, cam_trans, nullptr, sc.view, focal, visible_weight, img_in, img_out, ids_out, 2 * n, n_frames, H, W,
                    (hipStream_t)stream, vcol);
  return e == hipSuccess ? ACRMI_OK : fail(c, ACRMI_EHIP, "render regions: %s", hipGetErrorString(e));
}

int acrmi_render_regions(acrmi_ctx* c, const float* verts, const float* cam_trans, const float* slots, int n, const float* offsets,
                         const int32_t* region_frame, const float* colors_host, float focal, float visible_weight,
                         const uint8_t* img_in, uint8_t* img_out, int n_frames, int H, int W, int32_t* ids_out, void* stream) {
  return render_regions_call(c, "acrmi_render_regions", false, nullptr, verts, cam_trans, slots, n, offsets, region_frame, colors_host,
                             focal, visible_weight, img_in, img_out, n_frames, H, W, ids_out, stream);
}

int acrmi_render_regions_colored(acrmi_ctx* c, const float* verts, const float* cam_trans, const float* slots, int n,
                                 const float* offsets, const int32_t* region_frame, const float* colors_host, const float* vcol,
                                 float focal, float visible_weight, const uint8_t* img_in, uint8_t* img_out, int n_frames, int H,
                                 int W, int32_t* ids_out, void* stream) {
  return render_regions_call(c, "acrmi_render_regions_colored", true, vcol, verts, cam_trans, slots, n, offsets, region_frame,
                             colors_host, focal, visible_weight, img_in, img_out, n_frames, H, W, ids_out, stream);
}

int acrmi_overlay_regions(acrmi_ctx* c, int what, const float* slots, const float* pj2d_org, int n, const float* offsets,
                          const int32_t* region_frame, int bgr, const uint8_t* img_in, uint8_t* out, uint8_t* out2, int n_frames,
                          int H, int W, void* stream) {
  if (!offsets || !region_frame || n > 0x3fffffff) return fail(c, ACRMI_EINVAL, "acrmi_overlay_regions: bad arguments");
  if (int r = check_overlay(c, "acrmi_overlay_regions", what, slots, pj2d_org, n, img_in, out, out2, n_frames, H, W)) return r;
  ON_DEVICE(c);
  hipError_t e;
  if (what == ACRMI_OVERLAY_SKELETON) {
    if (n > c->region_hand_cap) {      // (first call / more regions: the one place this call allocates)
      if (c->region_hand_frame) {
        HIPCHK(c, hipDeviceSynchronize());
        (void)hipFree(c->region_hand_frame);
        c->region_hand_frame = nullptr;
        c->region_hand_cap = 0;
      }
      HIPCHK(c, hipMalloc(&c->region_hand_frame, sizeof(int32_t) * 2 * (size_t)n));
      c->region_hand_cap = n;
    }
    e = launch_render_region_prep(slots, offsets, region_frame, n, n_frames, H, W, ACRMI_SLOT, ACRMI_SLOT_FLAG, nullptr,
                                  c->region_hand_frame, nullptr, nullptr, nullptr, (hipStream_t)stream);
    if (e != hipSuccess) return fail(c, ACRMI_EHIP, "overlay region prep: %s", hipGetErrorString(e));
    e = skeleton_launch(pj2d_org, nullptr, c->region_hand_frame, 0, 2 * n, n_frames, H, W, bgr, img_in, out, (hipStream_t)stream);
  } else {
    RegionHeatmapArgs a{};
    if (int r = heatmap_fill(c, "acrmi_overlay_regions", a, n, offsets, bgr, img_in, out, out2, H, W)) return r;
    a.n_frames = n_frames; a.region_frame = region_frame;
    e = launch_region_heatmap(a, (hipStream_t)stream);
  }
  return e == hipSuccess ? ACRMI_OK : fail(c, ACRMI_EHIP, "overlay regions: %s", hipGetErrorString(e));
}

// Plain HIP streams for hosts that have no stream API of their own at hand (Python: torch.cuda.Stream() instantiates
// torch's whole pool of 32 streams per priority, and with that many streams alive the few in use share hardware
// queues); engine.EnginePool runs its contexts on these.
int acrmi_stream_create(int device, void** stream) {
  if (!stream) return fail(nullptr, ACRMI_EINVAL, "acrmi_stream_create: null argument");
  int prev = 0;
  if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess)
    return fail(nullptr, ACRMI_EHIP, "acrmi_stream_create: cannot select device %d", device);
  hipStream_t st = nullptr;
  const hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  (void)hipSetDevice(prev);
  if (e != hipSuccess) return fail(nullptr, ACRMI_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
  *stream = st;
  return ACRMI_OK;
}

int acrmi_stream_destroy(void* stream) {
  if (!stream) return ACRMI_OK;
  const hipError_t e = hipStreamDestroy((hipStream_t)stream);
  return e == hipSuccess ? ACRMI_OK : fail(nullptr, ACRMI_EHIP, "hipStreamDestroy: %s", hipGetErrorString(e));
}

int acrmi_tune(int key, int value) {
  if (key == 0) { conv_force_cfg(value); return ACRMI_OK; }
  if (key == 3) { conv_set_phase_delay(value); return ACRMI_OK; }
  if (key == 4) { conv_set_xcd_swizzle(value); return ACRMI_OK; }   // XCD-banded item order on/off (default on)
  if (key == 5) { program_set_grouping(value != 0); return ACRMI_OK; }   // grouped launches in the programs set from now on
  static long long* dbg = nullptr;
  if (key == 1) {   // enable (value != 0) / disable the conv kernel's cycle stamps (workgroup 0, wave 0)
    if (value && !dbg) { if (hipMalloc(&dbg, 128 * sizeof(long long)) != hipSuccess) return ACRMI_EHIP; }
    if (dbg) (void)hipMemset(dbg, 0, 128 * sizeof(long long));
    conv_set_debug(value ? dbg : nullptr);
    return ACRMI_OK;
  }
  if (key == 2) {   // print the stamps of the last conv launch as deltas (device is synchronised first)
    if (!dbg) return ACRMI_OK;
    long long h[128];
    if (hipDeviceSynchronize() != hipSuccess) return ACRMI_EHIP;
    if (hipMemcpy(h, dbg, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return ACRMI_EHIP;
    const int n = (int)h[63];
    printf("conv stamps (%d):", n);
    for (int i = 1; i < n && i < 60; ++i) printf(" %lld", h[i] - h[i - 1]);
    printf("\n");
    const int nl = (int)h[127];   // loader wave 0 (conv_wino2_kernel only)
    if (nl > 0) {
      printf("loader stamps (%d):", nl);
      for (int i = 1; i < nl && i < 60; ++i) printf(" %lld", h[64 + i] - h[64 + i - 1]);
      printf("\n");
    }
    return ACRMI_OK;
  }
  return fail(nullptr, ACRMI_EINVAL, "acrmi_tune: unknown key %d", key);
}

}  // extern "C"
