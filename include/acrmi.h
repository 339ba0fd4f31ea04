/*
 * acrmi.h - C ABI of libacrmi.so: the MI355X (gfx950) ACR inference hot path.
 *
 * uint8 frame batch -> HRNet-W32 backbone -> ACR heads -> center decode -> MANO (L+R)
 * -> 778x3 vertices + 21x3 joints per hand.  Plain pointers and sizes only: no torch,
 * no C++ types.  All pointers marked "dev" are device (HBM) pointers owned by the caller
 * unless stated otherwise; every call is asynchronous on the given hipStream_t (passed as
 * void*; NULL = the null stream) and performs no hidden synchronisation.  Return value:
 * 0 on success, a negative ACRMI_E* code otherwise (acrmi_last_error() has the text).
 * One context per device, not thread-safe (the reference is single-threaded:
 * /root/reference/acr/main.py:126-141).
 *
 * The reference has no FFI layer; each entry point names the reference Python
 * interface it replaces (paths relative to the reference tree).
 */
#ifndef ACRMI_H
#define ACRMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACRMI_VERSION 303

#define ACRMI_OK 0
#define ACRMI_EINVAL (-1)  /* bad argument / unsupported shape  (reference: ValueError / assert) */
#define ACRMI_EHIP (-2)    /* HIP runtime error                                              */
#define ACRMI_ESTATE (-3)  /* call order violated (weights/program/MANO tables not loaded)   */
#define ACRMI_ENOMEM (-4)
#define ACRMI_ERANGE (-5)  /* an 'fp16x3' program met an activation outside the f16 range (acrmi_check_range) */

typedef struct acrmi_ctx acrmi_ctx;

/* ---------------------------------------------------------------------------------------
 * Program description.  The Python host (packer.py) folds BatchNorm into the conv weights,
 * packs them in the MFMA fragment order, and lowers the network topology
 * (acr/model.py:785-865 backbone, :47-166 heads) into a flat op list over numbered
 * activation buffers (NHWC, channel stride = cs elements; fp32, or f16 / bf16 between the layers of
 * a 16-bit program).  The library owns the buffers and replays the list; it knows nothing about HRNet.
 * ------------------------------------------------------------------------------------- */
/* Storage type of an activation buffer.  An fp32 program (the reference's configs/demo.yml, model_precision fp32) uses
 * ACRMI_DT_F32 everywhere.  A 16-bit program (the reference's autocast branch, acr/model.py:33-37, --model_precision
 * fp16; bf16 is the same program with the other 16-bit type) stores the activations BETWEEN layers as f16 / bf16, keeps
 * fp32 accumulation and fp32 bias / residual / ReLU arithmetic inside every kernel, and keeps the head outputs (center,
 * params, prior, segm maps), the pooled part features and everything behind them in fp32 (acr/model.py:56-62 .float()). */
enum { ACRMI_DT_F32 = 0, ACRMI_DT_F16 = 1, ACRMI_DT_BF16 = 2 };

typedef struct {
  int32_t h, w, cs;      /* per-frame height, width, channel stride in ELEMENTS (a multiple of 16 bytes) */
  int32_t persistent;    /* 1: never aliased with another buffer (holds init-time constants) */
  int32_t dtype;         /* ACRMI_DT_*; all 16-bit buffers of a program share one type */
} acrmi_buffer_desc;

enum {
  ACRMI_OP_U8NORM = 1,   /* uint8 NHWC image -> fp32 (x/255*2-1), pad channel zeroed (acr/model.py:832) */
  ACRMI_OP_CONV = 2,     /* KxK conv (K in {1,3}, stride in {1,2}) + bias [+ residual] [+ ReLU] */
  ACRMI_OP_FUSESUM = 3,  /* out = [relu](sum_t nearest_up(term_t, 2^shift_t))  (acr/model.py:677-684) */
  ACRMI_OP_BILINEAR2X = 4, /* bilinear x2, align_corners=True (acr/model.py:432)              */
  ACRMI_OP_POW11 = 5,    /* ch0 := 1.1 ** ch0 (acr/model.py:95-96)                            */
  ACRMI_OP_ATTPOOL = 6,  /* softmax-over-pixels weighted feature pooling (acr/model.py:103-113) */
  ACRMI_OP_PAREBIAS = 7, /* LocallyConnected2d + Linear + mix-conv pare bias (acr/model.py:145-164) */
  ACRMI_OP_COORDFILL = 8, /* init-time: write coord maps into 2 channels (acr/model.py:340-369) */
  ACRMI_OP_POINTHEADS = 9, /* params/cam/prior head towers + 109x109 mix at the decoded centers only (one op per
                             side = flags; in = backbone+coord buffer, res = pre-mix 109-ch map, out = params
                             map, aux = per-frame bias; w_off = 3 packed towers, w_off2 = mix weights);
                             acr/model.py:71-99,160-164 restricted to the pixels acr/result_parser.py:49-57,
                             141-145 samples */
  ACRMI_OP_PAIR1X1 = 12,  /* two chained 1x1 convolutions of layer1 (acr/model.py:519-539) in one kernel: out = relu(W3 in +
                             b3 + res) (64 -> 256 channels; in_buf, res_buf, out_buf) and aux = relu(W1 out + b1) (256 -> 64;
                             aux_buf = the next block's conv1 output); w_off = packer.pack_pair1x1 (both matrices + biases in
                             the kernel's LDS order, 33088 floats); fp32 programs */
  ACRMI_OP_MAXPOOL = 11,  /* max pooling 3x3 stride 2 pad 1 of cin channels (ResNet stem; in -> out [B,(H-1)/2+1,(W-1)/2+1]) */
  ACRMI_OP_STEM = 10      /* uint8 image -> relu(conv3x3 stride 2 (x/255*2-1) + b), 3 -> 64 channels: U8NORM + the
                             first CONV in one kernel (acr/model.py:832,589-603; in = the image, out = [B,H/2,W/2,>=64]);
                             w_off = packer.pack_stem fragments [14][2][64], b_off = 64 biases.  ksize = 7: the ResNet stem
                             (7x7 stride 2 pad 3; BASELINE.json configs[1]'s backbone), w_off = packer.pack_stem7
                             fragments [74][2][64] */
};

/* acrmi_op.flags of a CONV, bit 3: a position-bias map - [Ho][Wo][round4(groups*Cout)] fp32 at blob offset w_off2 -
 * is added to EVERY frame's output before the ReLU, in the place of a residual (res_buf must be -1; fp32 programs; not
 * algo 3).  It stands for input channels that are a fixed function of the pixel position: the two coordinate channels
 * of the reference's head convs (acr/model.py:52,340-369) leave the contraction (34 -> 32 input channels) and come back
 * as conv(coord maps, their filter columns), computed once at lowering time (packer.coord_bias_map). */
#define ACRMI_CONV_BIAS_MAP 8
/* acrmi_op.flags of a CONV, bit 4: split-K (algo 2, fp32, small-batch programs).  `groups` K-slices of ONE convolution:
 * slice s reads input channels [in_coff + s*cin, in_coff + (s+1)*cin) with its own packed filters (w_off: `groups`
 * consecutive pack_conv(winograd2d_weights(w[:, s*cin:(s+1)*cin])), b_off: `groups` bias rows of which the first is
 * used), all slices produce the same cout channels.  The slices are separate work items on separate CUs; their partial
 * tiles meet in a workspace of the context and are summed in slice order by whichever item arrives last (bit-reproducible
 * results).  cin % 32 == 0, cin >= 64, 2 <= groups <= 8.  What it is for: a 256 -> 256 layer on a 16x16 map is 16 work
 * items of 8 chunks for 256 CUs at batch 1 - 64 items of 2 chunks with 4 slices. */
#define ACRMI_CONV_SPLITK 16
/* acrmi_op.flags of a CONV, bit 5: second output (algo 3 only: 3x3 stride 1, Cin <= 32, Cout = 32).  out_buf receives the
 * convolution as usual (bias, residual, ReLU); the op's nterms extra maps are NOT added to it but to a second map:
 * aux_buf = relu(((out + up(term 0)) + up(term 1)) + up(term 2)), each term read at (y >> shift, x >> shift).  This is the
 * HR-module fuse sum of the FULL resolution (acr/model.py:672-686, i = 0): its first term, the output of branch 0's last
 * conv2, is also the input of the downsampling chains, so both maps are needed.  Bit-equal to the ACRMI_OP_FUSESUM launch. */
#define ACRMI_CONV_DUAL 32

/* acrmi_op.mode: which variant of the head program an op belongs to. */
enum {
  ACRMI_MODE_BOTH = 0,
  ACRMI_MODE_DENSE = 1,  /* only when the full head maps are computed (default)            */
  ACRMI_MODE_POINT = 2   /* only with ACRMI_OPT_POINT_HEADS (acrmi_forward)                */
};

typedef struct {
  int32_t kind;
  int32_t in_buf, out_buf, res_buf;       /* buffer ids, -1 = none (U8NORM: in = the image)  */
  int32_t in_coff, out_coff, res_coff;    /* channel offsets inside the buffers              */
  int32_t cin, cout;                      /* logical channels (per group)                    */
  int32_t ksize, stride, relu, groups;
  int64_t w_off, b_off;                   /* float offsets into the weight blob              */
  int32_t bias_per_frame;                 /* 1: bias comes from aux buffer, row per frame    */
  int32_t aux_buf;                        /* PAREBIAS/ATTPOOL output or per-frame bias input */
  int32_t nterms;                         /* FUSESUM: 1..4 terms.  CONV (fp32 3x3 stride 2, Cout % 32 = 0): 0..3 EXTRA residual terms */
  int32_t term_buf[4], term_coff[4], term_shift[4];   /* added behind res_buf and before the ReLU, in this order, term t read
                                             at pixel (y >> shift, x >> shift) of a map 1 / 2^shift the output's size (nearest
                                             upsampling): the HR-module fuse sum (acr/model.py:672-686) in the epilogue of the
                                             x0 downsampling chain's last convolution */
  int64_t w_off2, b_off2, w_off3;         /* PAREBIAS: linear weights/bias, mix-conv pare columns */
  int32_t flags;                          /* CONV: algo 0..7 (bits 0-2) | ACRMI_CONV_BIAS_MAP; PAREBIAS: part slice start
                                             (0 right / 16 left); POINTHEADS: side (0 left / 1 right) */
  int32_t mode;                           /* ACRMI_MODE_*                                    */
} acrmi_op;

/* Where the head outputs live (buffer ids of the program), needed by acrmi_decode. */
typedef struct {
  int32_t center_buf[2];   /* [left,right] center maps  [B,64,64,cs], channel 0   */
  int32_t params_buf[2];   /* final 109-ch params maps  (acr/model.py:163-164)    */
  int32_t prior_buf[2];    /* 106-ch prior maps                                   */
  int32_t segm_buf;        /* 33-ch part-segmentation logits [B,256,256,cs]       */
  int32_t backbone_buf;    /* 32(+2 coord)-ch backbone output [B,128,128,cs]      */
} acrmi_head_layout;

/* Fixed per-(frame,hand) result slot written by acrmi_decode: ACRMI_SLOT floats.
 * hand 0 = left, 1 = right (acr/result_parser.py:166-168 ordering is rebuilt on the host). */
#define ACRMI_SLOT 176
#define ACRMI_SLOT_FLAG 0      /* 1.0 if center score > ACRMI_OPT_CONF_THRESH (strict)      */
#define ACRMI_SLOT_FLATIND 1   /* y*64+x of the center (0 when not detected)               */
#define ACRMI_SLOT_SCORE 2
#define ACRMI_SLOT_CAM 3       /* 3  */
#define ACRMI_SLOT_POSES 6     /* 48: global orient (3) + 15 joints axis-angle              */
#define ACRMI_SLOT_BETAS 54    /* 10 */
#define ACRMI_SLOT_PARAMS 64   /* 109: sampled params (+ cross-hand prior)                  */

int acrmi_version(void);
const char* acrmi_last_error(const acrmi_ctx* ctx); /* ctx may be NULL: last error of acrmi_create */

/* acr/main.py:57-63 (_build_model_): one context per device. */
int acrmi_create(acrmi_ctx** out, int device);
void acrmi_destroy(acrmi_ctx* ctx);

/* acr/utils.py:1153-1168 (load_model/copy_state_dict): host blob of packed fp32 weights
 * (BN folded, MFMA fragment order) copied once into HBM; static residency replaces
 * nn.DataParallel's per-call replicate (acr/main.py:61). */
int acrmi_load_weights(acrmi_ctx* ctx, const float* blob_host, size_t n_floats);
/* The same blob for several contexts of one device (a pool of contexts that take batches in turn): `ctx` uses
 * the device copy `donor` holds instead of uploading its own - 330 MB per extra context at HRNet-W32 fp32.  The copy is freed
 * when the last context holding it is destroyed or loads other weights.  Both contexts need the same program.  Thread safety:
 * contexts sharing a blob may be destroyed from different threads; this call itself must not run concurrently with a destroy or
 * a weight reload of `donor` (serialize them in the host). */
int acrmi_share_weights(acrmi_ctx* ctx, acrmi_ctx* donor);

/* Lowered topology of acr/model.py:785-865 + :47-166; allocates activation buffers for
 * up to max_batch frames (aliasing non-overlapping lifetimes) and runs the init-time ops. */
int acrmi_set_program(acrmi_ctx* ctx, const acrmi_buffer_desc* bufs, int n_bufs, const acrmi_op* ops,
                      int n_ops, const acrmi_head_layout* heads, int max_batch);

/* mano/manolayer.py:13-102 (ManoLayer.__init__ buffers) for side 0 = left, 1 = right.
 * Host pointers, row-major as the reference registers them: v_template[778*3],
 * shapedirs[778*3*10], posedirs[778*3*135], J_regressor[16*778], weights[778*16],
 * hands_mean[45].  The left-hand shapedirs x-flip (acr/mano_wrapper.py:35) is the caller's job. */
int acrmi_load_mano(acrmi_ctx* ctx, int side, const float* v_template, const float* shapedirs,
                    const float* posedirs, const float* J_regressor, const float* weights,
                    const float* hands_mean);

/* acr/model.py:32-44 minus the parser: backbone + head_forward on B frames.
 * img_dev: uint8 [B,512,512,3] RGB NHWC (meta_data['image']).  Results stay in the
 * program's head buffers (see acrmi_buffer_ptr). */
int acrmi_backbone_heads(acrmi_ctx* ctx, const uint8_t* img_dev, int B, void* stream);
/* acr/model.py:47-65 (ACR.head_forward(x)): the heads alone on backbone features the caller holds - feat_nchw_dev is fp32
 * [B, C0, 128, 128] (C0 = acrmi_backbone_channels: 32 for HRNet-W32), e.g. what acr.model.ACR.backbone returned.  The
 * features are copied into the program's backbone map (coordinate channels are already there) and the ops behind the backbone
 * run in program order on `stream`; results as after acrmi_backbone_heads (acrmi_buffer_ptr / acrmi_decode).  fp32-storage
 * programs only (ACRMI_EINVAL for the 16-bit storage programs). */
int acrmi_heads(acrmi_ctx* ctx, const float* feat_nchw_dev, int B, void* stream);
int acrmi_backbone_channels(acrmi_ctx* ctx); /* channels of the backbone output (without the 2 coordinate maps); < 0: error */

/* Device pointer / geometry of program buffer `buf` (valid until the next set_program); cs counts elements of
 * acrmi_buffer_dtype(ctx, buf) (ACRMI_DT_*, -1 for an unknown buffer). */
void* acrmi_buffer_ptr(acrmi_ctx* ctx, int buf, int* h, int* w, int* cs);
int acrmi_buffer_dtype(acrmi_ctx* ctx, int buf);

/* acr/result_parser.py:21-40,85-190 (ResultParser.parse/parse_maps) + acr/utils.py:334-382
 * (6D -> axis-angle), per-frame semantics: slots_dev [B,2,ACRMI_SLOT]. */
int acrmi_decode(acrmi_ctx* ctx, int B, float* slots_dev, void* stream);
/* The same with the cross-hand prior decided by the CALLER per frame: prior_gate_dev [B] int32 on the device (NULL = as
 * acrmi_decode): < 0 = this frame by the per-frame rule, 0 = no prior, 1 = prior when the frame has both hands.  This is how
 * the host reproduces the reference's batch > 1 behaviour (acr/result_parser.py:131: the prior only when EVERY flag of the
 * batch is set; :42-47: determine_coeff reads row 0 of each side's list) - acr/result_parser.py ResultParser(batch_semantics=
 * 'reference') decodes once, applies those batch-wide rules to the flags / centers, and decodes again with the gate. */
int acrmi_decode_gated(acrmi_ctx* ctx, int B, const int32_t* prior_gate_dev, float* slots_dev, void* stream);
/* acr/result_parser.py:42-47 (determine_coeff) + :102-145 (parse_maps at batch > 1), the rules that look ACROSS frames, on the
 * device: slots_dev [B,2,ACRMI_SLOT] of a first decode -> gate_dev [B] int32 for acrmi_decode_gated: 1 in the frames that have
 * both hands, provided the batch holds a left and a right detection at all (:131) and the left center of the first
 * left-detected frame is <= 32 map pixels from the right center of the first right-detected frame (:42-47, row 0 of each
 * list); else 0.  acrmi_forward does decode -> this -> gated decode by itself when ACRMI_OPT_BATCH_PRIOR is set.  ctx may be
 * NULL (stand-alone use next to acrmi_decode_maps_gated: the current device). */
int acrmi_prior_gate(acrmi_ctx* ctx, const float* slots_dev, int B, int32_t* gate_dev, void* stream);
/* 'fp16x3' programs (fp32 tensors, operands split into two f16 numbers - conv algo 6): an activation with |x| > 65504 cannot
 * be split (hi = inf).  The split kernels track it per launch at one v_max3 per two values; while the flag is set acrmi_decode /
 * acrmi_forward write every slot as NaN (so the meshes are NaN too: nothing plausible-looking leaves the library).  This call
 * waits for `stream`, returns ACRMI_ERANGE if the flag was set since the last check and clears it; ACRMI_OK otherwise and for
 * programs without split-f16 convolutions (fp32, bf16x3: fp32's exponent range). */
int acrmi_check_range(acrmi_ctx* ctx, void* stream);

/* Several hands of each side per frame: the max_hand (1..ACRMI_MAX_HAND) best candidates of each NMS'd
 * center map - value descending, lower flat index first on an exact tie, CenterMap.parse_centermap_heatmap_adaptive_scale_batch
 * with K = max_hand (acr/result_parser.py:218-243) - each flagged when its score > ACRMI_OPT_CONF_THRESH (strict), else a
 * placeholder that samples pixel 0.  slots_dev [B,max_hand,2,ACRMI_SLOT]: pair k holds (left rank k, right rank k) - a storage
 * convention, the two hands of a pair have nothing to do with each other - and every slot field is as acrmi_decode writes
 * it, so the result is B * max_hand rows of the [n,2,...] shape every call behind the decode takes.  The cross-hand prior
 * (acr/result_parser.py:42-47,131-145) is decided per HAND: its own prior map at the center of its partner = the nearest
 * flagged hand of the other side in the frame (lower rank on a tie), added unless they are more than 32 map pixels apart.
 * max_hand = 1 writes exactly what acrmi_decode writes. */
#define ACRMI_MAX_HAND 8
int acrmi_decode_multi(acrmi_ctx* ctx, int B, int max_hand, float* slots_dev, void* stream);

/* Same decode on caller-supplied NHWC maps (unit tests / callers with their own maps):
 * center [B,64,64,center_cs] (ch 0), params [B,64,64,params_cs] (109 ch), prior (106 ch). */
int acrmi_decode_maps(const float* l_center, const float* r_center, int center_cs,
                      const float* l_params, const float* r_params, int params_cs,
                      const float* l_prior, const float* r_prior, int prior_cs, int B,
                      float conf_thresh /* CenterMap.conf_thresh = args().centermap_conf_thresh, 0.35 */,
                      float* slots_dev, void* stream);
int acrmi_decode_maps_gated(const float* l_center, const float* r_center, int center_cs,
                            const float* l_params, const float* r_params, int params_cs,
                            const float* l_prior, const float* r_prior, int prior_cs, int B, float conf_thresh,
                            const int32_t* prior_gate_dev /* see acrmi_decode_gated */, float* slots_dev, void* stream);
/* acrmi_decode_multi on caller-supplied maps: slots_dev [B,max_hand,2,ACRMI_SLOT]. */
int acrmi_decode_maps_multi(const float* l_center, const float* r_center, int center_cs,
                            const float* l_params, const float* r_params, int params_cs,
                            const float* l_prior, const float* r_prior, int prior_cs, int B, int max_hand,
                            float conf_thresh, float* slots_dev, void* stream);

/* mano/manolayer.py:104-276 (ManoLayer.forward, use_pca=False, flat_hand_mean=False,
 * center_idx as given; <0 = no root alignment) fused with acr/utils.py:384-412
 * (batch_orth_proj / convert_kp2d_from_input_to_orgimg).
 * Row r reads poses[r*pose_stride..+48], betas[r*beta_stride..+10]; side[r] (0 left / 1 right)
 * or, when side == NULL, side = r & 1 (slot order).  cam/offsets/verts_camed/pj2d/pj2d_org may
 * be NULL (projection skipped).  cam row stride = cam_stride, offsets [H,10] row per hand. */
int acrmi_mano(acrmi_ctx* ctx, const float* poses, int pose_stride, const float* betas, int beta_stride,
               const int32_t* side, int H, int center_idx, float* verts, float* joints, float* center,
               const float* cam, int cam_stride, const float* offsets, float* verts_camed, float* pj2d,
               float* pj2d_org, void* stream);

/* mano/manolayer.py:151-162 (joint_rot_mode='rotmat', use_pca=False): the pose of row r is rotmats[r*144..+144] = 16 row-major
 * 3x3 rotation matrices, root first, ALREADY orthonormal (the reference projects them with a CPU SVD in batch_rotprojs,
 * :436-453; the Python ManoLayer of this package does the same on the host).  No Rodrigues, th_hands_mean is not applied.
 * Everything behind the rotations - blend shapes, joint regression, chain, skinning, tips, root alignment - is acrmi_mano's. */
int acrmi_mano_rotmat(acrmi_ctx* ctx, const float* rotmats, const float* betas, int beta_stride, const int32_t* side,
                      int H, int center_idx, float* verts, float* joints, float* center, void* stream);

/* The backward of acrmi_mano's axis-angle mode: the gradient of (verts, joints, center) with respect to the poses and betas
 * of every row, from the cotangents g_verts [H,778,3], g_joints [H,21,3], g_center [H,3] (device pointers; each may be NULL =
 * zeros; all three NULL: zero gradients are written).  poses / betas / side / center_idx as in acrmi_mano (pose_stride >= 48,
 * beta_stride >= 10, center_idx -1..20; with center_idx < 0 center is constant and g_center is not read).  Writes all of
 * g_poses [H,48] and g_betas [H,10].  One workgroup per hand, fixed summation orders, no atomics: a row's result does not
 * depend on the batch it is in.  Always differentiates the fp32 tables, also under ACRMI_OPT_MANO_FP16.  The rotation-matrix
 * mode and the projection outputs have no backward.  ACRMI_ESTATE before a side's tables are loaded; H == 0 is a success. */
int acrmi_mano_backward(acrmi_ctx* ctx, const float* poses, int pose_stride, const float* betas, int beta_stride,
                        const int32_t* side, int H, int center_idx, const float* g_verts, const float* g_joints,
                        const float* g_center, float* g_poses, float* g_betas, void* stream);

/* The fused fitter: `steps` (0..1024) iterations of Adam per hand in ONE launch, on the 64 parameters of a
 * hand - pose [48] (root rotation, articulation), betas [10], trans [3], cam [3] = (s, tx, ty) - against any mix of
 *   y3 [H,21,3] with w3 [H,21]: J3 = joints + trans;   y2 [H,21,2] with w2 [H,21]: P2 = joints[:, :2] * s + (tx, ty), acrmi_mano's
 *   pj2d;   yv [H,778,3] with wv [H]: V3 = verts + trans,
 * (verts, joints) being acrmi_mano's axis-angle outputs at center_idx (-1..20), plus lam_pose |pose[3:48] - prior[3:48]|^2 +
 * lam_beta |betas - prior[48:58]|^2 (prior [H,58], NULL = zeros).  A NULL target removes its term (its weights are then not
 * read), NULL weights are ones, a weight that is exactly 0 removes its point (its target is not read into the arithmetic).
 * state [H, acrmi_mano_fit_state_floats()] is the caller's: parameters [64] | m [64] | v [64] | t | loss of the last evaluated
 * step | loss of the first | 0; a fresh fit starts from the caller's parameters with everything behind them zero, a later call
 * continues it bit for bit.  lr5 (HOST, 5 doubles): the learning rates of root rotation, articulation, betas, trans, cam; 0
 * freezes a group (parameters, m and v keep their bytes).  b1, b2, eps: torch.optim.Adam's (0.9, 0.999, 1e-8); no weight
 * decay, no amsgrad.  yv != NULL or dense != 0 runs the dense vertex level (all 778 vertices, as acrmi_mano_backward),
 * otherwise only the five fingertips are skinned and the pose blend table is never read.  Writes poses [H,48], betas [H,10],
 * trans [H,3], cam [H,3], loss [H,2] (first and last evaluated step of the fit) and, when not NULL, grad [H,64]: the gradient
 * of the last evaluated step (untouched when steps == 0, which only copies the state's parameters and losses out).  One
 * workgroup per hand, fixed summation orders, no atomics; always the fp32 tables.  ACRMI_EINVAL for a NULL state, steps or
 * center_idx out of range - before a device is touched; ACRMI_ESTATE without MANO tables; H == 0 is a success. */
int acrmi_mano_fit(acrmi_ctx* ctx, float* state, const int32_t* side, int H, int center_idx, const float* y3, const float* w3,
                   const float* y2, const float* w2, const float* yv, const float* wv, const float* prior, double lam_pose,
                   double lam_beta, const double* lr5, double b1, double b2, double eps, int steps, int dense, float* poses,
                   float* betas, float* trans, float* cam, float* loss, float* grad, void* stream);
int acrmi_mano_fit_state_floats(void);

/* acr/utils.py:430-472 + :474-519 (estimate_translation_np / estimate_translation, the reference's closed-form
 * least-squares branch, unit joint confidences): joints [n,21,3] and pj2d [n,21,2] (in [-1,1]; the 2-D targets are
 * (pj2d+1)*img_size/2) on the device -> cam_trans [n,3].  Solved in fp64 like the reference. */
int acrmi_cam_trans(const float* joints_dev, const float* pj2d_dev, int n, float focal_length, float img_size,
                    float* trans_dev, void* stream);

/* acr/main.py:126-141 + :85 in one call: frames -> slots [B,2,ACRMI_SLOT], verts [B,2,778,3],
 * joints [B,2,21,3] (root-aligned on joint ACRMI_OPT_CENTER_IDX = 9, metres; threshold ACRMI_OPT_CONF_THRESH;
 * smoothed when ACRMI_OPT_TEMPORAL).  offsets_dev [B,10] may be NULL. */
int acrmi_forward(acrmi_ctx* ctx, const uint8_t* img_dev, int B, const float* offsets_dev, float* slots_dev,
                  float* verts_dev, float* joints_dev, float* verts_camed_dev, float* pj2d_dev,
                  float* pj2d_org_dev, void* stream);

/* acrmi_forward for up to max_hand (1..ACRMI_MAX_HAND) hands of each side per frame: the program with its DENSE heads
 * (whatever ACRMI_OPT_POINT_HEADS says) or, with ACRMI_OPT_POINT_HEADS_MULTI, with the head towers at the top max_hand
 * centers of each side only, acrmi_decode_multi, one MANO launch over
 * the 2 * max_hand * B rows (placeholders included) -> slots [B,max_hand,2,ACRMI_SLOT], verts [B,max_hand,2,778,3], joints
 * [B,max_hand,2,21,3], the projections alike; offsets_dev [B,10] = one row per FRAME.  max_hand = 1 is acrmi_forward with
 * dense heads.  ACRMI_EINVAL, before anything is launched, for max_hand outside 1..ACRMI_MAX_HAND and for max_hand > 1 with
 * ACRMI_OPT_BATCH_PRIOR or ACRMI_OPT_TEMPORAL set (neither rule knows two hands of one side). */
int acrmi_forward_multi(acrmi_ctx* ctx, const uint8_t* img_dev, int B, int max_hand, const float* offsets_dev,
                        float* slots_dev, float* verts_dev, float* joints_dev, float* verts_camed_dev, float* pj2d_dev,
                        float* pj2d_org_dev, void* stream);

/* Stand-alone operators (same kernels the program uses; for parity tests and embedding).
 * w_packed/bias come from the Python packer (pack_conv).  algo: 0 = direct convolution;
 * 1 = Winograd F(2,3) along x (3x3 stride 1 only; w_packed = pack_conv(winograd_weights(w)));
 * 2 = Winograd F(2x2,3x3) (3x3 stride 1 only; w_packed = pack_conv(winograd2d_weights(w)));
 * 3 = Winograd F(2x2,3x3) with the layer's taps resident in LDS (groups 1, Cin <= 32, Cout = 32, H % 8 == 0,
 *     W % 16 == 0; w_packed = pack_wino3(w), 64 KiB);
 * 4 = Winograd F(2x4,3x3): F(2,3) along y, F(4,3) along x (3x3 stride 1, Cin > 32; w_packed =
 *     pack_conv(winograd24_weights(w)), 4x6 taps);
 * 5 = 3x3 STRIDE 2 in polyphase form with F(2,2) on the two-tap phases (Cin % 16 == 0, Cout % 32 == 0, H % 16 == 0,
 *     W % 32 == 0; w_packed = pack_conv(polyphase2_weights(w)), 4 waves x 7 taps; csrc/conv_pp2.inc);
 * 6 = 3x3 stride 1 (or 1x1 stride 1 with H W % 256 == 0: csrc/conv_x3p.inc) with SPLIT operands on the 16-bit matrix pipe: fp32 tensors, every operand split into f16 hi + lo
 *     in registers, three products per MAC on v_mfma_f32_32x32x16_f16, fp32 accumulation (Cin % 32 == 0, Cout % 32 == 0,
 *     H % 8 == 0, W % 32 == 0, |x| < 65504; w_packed = pack_conv_x3([(w, b)]): split f16 fragments of the filters scaled by
 *     a power of two + one trailing float holding the inverse scale; csrc/conv_x3.inc).  The 'fp16x3' programs;
 * 7 = the same with bf16 halves (v_mfma_f32_32x32x16_bf16; 16-bit operands, fp32's exponent range: no |x| limit;
 *     w_packed = pack_conv_x3([(w, b)], DT_BF16)).  The 'bf16x3' programs.
 * algo | ACRMI_CONV_BIAS_MAP (not with 3): res is ONE map [Ho][Wo][res_cs] added to every frame (see acrmi_op.flags). */
int acrmi_conv2d(const float* in, int B, int H, int W, int in_cs, int in_coff, int cin, const float* w_packed,
                 const float* bias, int bias_frame_stride, const float* res, int res_cs, int res_coff,
                 float* out, int out_cs, int out_coff, int cout, int ksize, int stride, int relu, int groups,
                 int algo, void* stream);
/* Up to two INDEPENDENT fp32 convolutions as ONE launch: problem 1's work items follow problem 0's inside the persistent
 * workgroups, so the second start-up and one launch boundary are not paid.  The fields are acrmi_conv2d's arguments.  n = 1 is
 * acrmi_conv2d; n = 2 needs two problems that the library routes to one kernel instantiation with a group form (today: algo 4,
 * 3x3 stride 1, Cin >= 64 and % 32 == 0, Cout % 64 == 0, maps of whole 8x32-pixel tiles), else ACRMI_EINVAL - never two quiet
 * launches.  No output may be read or written by the other problem.  Each output is bit-identical to acrmi_conv2d's. */
typedef struct acrmi_conv_problem {
  const float* in;
  const float* w_packed;
  const float* bias;
  const float* res;
  float* out;
  int32_t B, H, W, in_cs, in_coff, cin, bias_frame_stride, res_cs, res_coff, out_cs, out_coff, cout, ksize, stride, relu,
      groups, algo, reserved;
} acrmi_conv_problem;
int acrmi_conv2d_group(const acrmi_conv_problem* problems, int n, void* stream);
/* The convolution of a 16-bit program (acr/model.py:33-37, the autocast branch): in / res / out point at f16 (dtype =
 * ACRMI_DT_F16) or bf16 (ACRMI_DT_BF16) NHWC tensors, strides / offsets / channel counts in elements (strides multiples
 * of 8), w_packed = packer.pack_conv_h16(w, b, dtype) (BN-folded filters rounded once to the storage type, A fragments
 * of v_mfma_f32_32x32x16_{f16,bf16}), bias fp32.  fp32 accumulation; bias, residual and ReLU in fp32; ONE rounding of
 * the result.  out_f32 != 0: out AND res are fp32 tensors (strides multiples of 4; stride-1 shapes only) - the head
 * exits, whose maps the reference converts with .float() (acr/model.py:56-62). */
/* Split-K form of acrmi_conv2d with algo 2 (see ACRMI_CONV_SPLITK): cin_slice channels per slice, `splits` slices,
 * w_packed / bias = the slices' pack_conv outputs one after the other.  workspace: acrmi_conv2d_splitk_workspace() bytes
 * of device memory, 16-byte aligned, ZEROED ONCE by the caller (every launch leaves its counters zero again) and not
 * shared by launches that may overlap. */
size_t acrmi_conv2d_splitk_workspace(int B, int H, int W, int cout, int splits);
int acrmi_conv2d_splitk(const float* in, int B, int H, int W, int in_cs, int in_coff, int cin_slice, int splits,
                        const float* w_packed, const float* bias, const float* res, int res_cs, int res_coff, float* out,
                        int out_cs, int out_coff, int cout, int relu, void* workspace, size_t workspace_bytes, void* stream);

int acrmi_conv2d_h16(const void* in, int B, int H, int W, int in_cs, int in_coff, int cin, const void* w_packed,
                     const float* bias, int bias_frame_stride, const void* res, int res_cs, int res_coff, void* out,
                     int out_cs, int out_coff, int cout, int ksize, int stride, int relu, int groups, int dtype,
                     int out_f32, void* stream);
/* acr/utils.py:1276-1337 (img_preprocess / image_pad_white_bg / cv2.resize INTER_CUBIC): n BGR uint8 frames
 * [n,H,W,3] on the device -> RGB uint8 [n,512,512,3]: white pad to square (imgaug 0.4.0
 * compute_paddings_to_reach_aspect_ratio + Pad), then OpenCV's uint8 INTER_CUBIC restated bit for bit (a = -0.75,
 * 11-bit fixed-point coefficients, clamped border, (v + 2^21) >> 22; see oracle/preprocess.py).  offsets_host
 * [n,10] (may be NULL) receives the reference's `offsets` rows (padded h, padded w, crop trbl = 0, pad trbl). */
int acrmi_preprocess(const uint8_t* bgr_dev, int n, int H, int W, uint8_t* out_rgb_dev, float* offsets_host,
                     void* stream);
/* The same for frames of DIFFERENT sizes in one call (img_preprocess is per image, acr/utils.py:1315-1337; folder mode,
 * acr/main.py:144-205, mixes sizes): frames_host [n] = where each BGR uint8 frame [H,W,3] lives on the device and its size -
 * frames need not share an allocation.  Same arithmetic, bit for bit; out_rgb_dev [n,512,512,3]; offsets_host [n,10] (may be
 * NULL) = each image's own `offsets` row.  The geometry travels in the kernel arguments (64 frames per launch): nothing is
 * allocated or uploaded, the host array may be freed when the call returns. */
typedef struct acrmi_frame {
  const uint8_t* bgr_dev;
  int32_t H, W;
} acrmi_frame;
int acrmi_preprocess_frames(const acrmi_frame* frames_host, int n, uint8_t* out_rgb_dev, float* offsets_host, void* stream);
/* NV12 video surfaces as the input (DESIGN.md "NV12 input"): what hardware and software decoders hand out - a luma plane and a
 * half-height plane of interleaved chroma, pitched rows, 1.5 bytes per pixel - instead of the packed BGR frame cv2 makes of it
 * (acr/main.py:126-141 reads frames with cv2).  The colour rule is integer, chroma is nearest (each 2x2 block of luma shares one
 * U, V pair); it is OpenCV's published cvtColor(COLOR_YUV2BGR_NV12) arithmetic with the coefficient row as a parameter.  For
 * bytes Y, U, V and a row (cy, cub, cug, cvg, cvr, y_off):
 *   y = max(0, Y - y_off) * cy;  u = U - 128;  v = V - 128;  r = 1 << 19
 *   R = clamp((y + cvr v + r) >> 20);  G = clamp((y + cug u + cvg v + r) >> 20);  B = clamp((y + cub u + r) >> 20)
 * (arithmetic shift, clamp to 0..255).  A row is refused (ACRMI_EINVAL) when y_off is outside 0..255 or when
 * 255 |cy| + 128 max(|cub|, |cvr|, |cug| + |cvg|) + 2^19 >= 2^31: the int32 sums cannot overflow. */
typedef struct acrmi_nv12_frame {      /* 32 bytes */
  const uint8_t* y_dev;                /* [H, y_pitch]  */
  const uint8_t* uv_dev;               /* [H/2, uv_pitch], U at even bytes, V at odd */
  int32_t H, W;                        /* both even, >= 2 */
  int32_t y_pitch, uv_pitch;           /* bytes per row, >= W; nothing beyond W bytes of a row is read */
} acrmi_nv12_frame;
/* The named coefficient rows.  CV601: OpenCV's literal integers (NV12 -> the BGR frame cv2 gives the reference); the others:
 * round(x * 2^20) of the textbook Kr / Kb forms, limited range (y_off 16) or full range (y_off 0). */
#define ACRMI_NV12_CV601 0
#define ACRMI_NV12_BT601 1
#define ACRMI_NV12_BT601_FULL 2
#define ACRMI_NV12_BT709 3
#define ACRMI_NV12_BT709_FULL 4
int acrmi_nv12_matrix(int which, int32_t coef6[6]);   /* host only */
/* acrmi_preprocess_frames on NV12 frames: each of the 16 cubic taps is converted to 8-bit R, G, B by the rule above before it
 * enters the sums, so out_rgb_dev [n,512,512,3] is byte for byte what converting the whole frame and calling
 * acrmi_preprocess_frames gives, without a full-resolution RGB frame; pad taps are white.  coef6_host: six integers, NULL =
 * CV601.  offsets_host [n,10] (may be NULL): the rows acrmi_preprocess_frames writes for the same H, W.  Everything is checked
 * before anything is queued (the message names the frame); geometry travels in the kernel arguments, 64 frames per launch,
 * further frames in further launches; frames_host may be freed when the call returns. */
int acrmi_preprocess_nv12(const acrmi_nv12_frame* frames_host, int n, const int32_t* coef6_host, uint8_t* out_rgb_dev,
                          float* offsets_host, void* stream);
/* The plain conversion at full resolution (frames to draw over, or to look at): dst_dev_host [n] device pointers to tight
 * [H,W,3] uint8 images, RGB, or BGR when bgr != 0. */
int acrmi_nv12_to_rgb(const acrmi_nv12_frame* frames_host, int n, const int32_t* coef6_host, int bgr,
                      uint8_t* const* dst_dev_host, void* stream);
/* NV12 surfaces as the OUTPUT (DESIGN.md "NV12 output"): drawn frames handed to a video encoder.  All arithmetic is int32, the
 * shift is arithmetic, results clamp to 0..255.  For a row (cry, cgy, cby, cru, cgu, cbu, crv, cgv, cbv, y_off):
 *   per pixel:      Y = clamp((cry R + cgy G + cby B + (y_off << 20) + (1 << 19)) >> 20)
 *   per 2x2 block:  R4, G4, B4 = the sums of the four pixels' R, G, B   (0..1020)
 *                   U = clamp((cru R4 + cgu G4 + cbu B4 + (128 << 22) + (1 << 21)) >> 22)
 *                   V = clamp((crv R4 + cgv G4 + cbv B4 + (128 << 22) + (1 << 21)) >> 22)
 * Chroma is the mean of the block folded into the shift: for four equal pixels it is the per-pixel value, the counterpart of the
 * input rule's nearest chroma.  The named rows go by ACRMI_NV12_*, so a name selects the input and the output row: the four BT
 * rows are round(x * 2^20) of the textbook forms; CV601 holds the constants of OpenCV's RGB -> YUV 4:2:0 code as remembered,
 * NOT verified against its source.  No row is claimed to equal cv2: it writes no NV12, and its I420 path takes chroma from one
 * pixel of the block.  A row is refused (ACRMI_EINVAL) when y_off is outside 0..255, when
 * 255 (|cry| + |cgy| + |cby|) + (y_off << 20) + 2^19 >= 2^31, or when
 * 1020 max(|cru| + |cgu| + |cbu|, |crv| + |cgv| + |cbv|) + (128 << 22) + 2^21 >= 2^31: the int32 sums cannot overflow. */
int acrmi_nv12_out_matrix(int which, int32_t coef10[10]);   /* host only */
typedef struct acrmi_nv12_surface {    /* 32 bytes: acrmi_nv12_frame with writable planes */
  uint8_t* y_dev;                      /* [H, y_pitch]  */
  uint8_t* uv_dev;                     /* [H/2, uv_pitch], U at even bytes, V at odd */
  int32_t H, W;                        /* both even, >= 2 */
  int32_t y_pitch, uv_pitch;           /* bytes per row, >= W; nothing beyond W bytes of a row is written */
} acrmi_nv12_surface;
/* The plain conversion: src_dev_host [n] device pointers to tight [H,W,3] uint8 frames (RGB, or BGR when bgr != 0) of the sizes
 * surfaces_host [n] name -> those surfaces.  coef10_host: ten integers, NULL = CV601.  Everything is checked before anything is
 * queued (even sizes >= 2, pitches >= W, null pointers, the row); geometry travels in the kernel arguments, 64 frames per launch,
 * further frames in further launches on the same stream; the host arrays may be freed when the call returns.  A surface must
 * not overlap its source or another surface: that is the caller's duty. */
int acrmi_rgb_to_nv12(const uint8_t* const* src_dev_host, const acrmi_nv12_surface* surfaces_host, int n,
                      const int32_t* coef10_host, int bgr, void* stream);
/* Compose: the drawn frame drawn_dev_host[i] (tight [H,W,3], RGB or BGR) over the source surface it was drawn from.  A pixel is
 * CHANGED when its drawn triple differs from what the input rule (coef6_host, NULL = CV601) makes of the source's Y, U, V.
 *   out Y    = Y(drawn triple) for a changed pixel, else the source byte
 *   out U, V = U, V(sums of the block's four drawn triples) when any pixel of the block is changed, else the source bytes
 * so composing the frame acrmi_nv12_to_rgb made of a surface gives that surface back byte for byte, whatever its bytes, and one
 * drawn pixel changes one Y byte and one U, V pair.  The output surface must have the source's size (ACRMI_EINVAL otherwise).  It
 * may BE the source surface - the same plane pointers and pitches: a thread reads and writes only its own blocks.  Otherwise the
 * output planes must overlap neither the source planes, nor the drawn frame, nor each other; guaranteeing that is the caller's
 * duty, nothing checks it.  58 frames per launch (what fits the 4 KB argument block); otherwise as acrmi_rgb_to_nv12. */
int acrmi_nv12_compose(const acrmi_nv12_frame* src_frames_host, const uint8_t* const* drawn_dev_host,
                       const acrmi_nv12_surface* out_surfaces_host, int n, const int32_t* coef6_host, const int32_t* coef10_host,
                       int bgr, void* stream);
/* Regions of interest (DESIGN.md "Regions of interest"): the box of a person or hand detector instead of the whole frame, the
 * reference's image_crop_pad with a bbox (acr/utils.py:1287-1301).  A region names a frame of the call and a box in that frame's
 * pixels, r and b exclusive.  The box is clamped to the H x W frame as crop amounts
 *   crop_trbl = (max(0, t), max(0, W - r), max(0, H - b), max(0, l)),   window = frame[ct : H - cb, cl : W - cr]
 * and the window is pre-processed exactly as a frame of its own size: white pad to a square, cubic resize to 512 x 512, RGB -
 * byte for byte what acrmi_preprocess_frames gives for a copy of the window.  Filter taps beyond the window are its clamped
 * border or the white pad, never the neighbouring pixels of the frame.  A window without pixels is ACRMI_EINVAL.
 * The `offsets` row is [padded h, padded w, ct, cr, cb, cl, pt, pr, pb, pl]: pj2d_org lands in the pixels of the original frame. */
typedef struct acrmi_roi {             /* 20 bytes */
  int32_t frame;                       /* index into the call's frames */
  int32_t l, t, r, b;                  /* columns [l, r), rows [t, b); may overhang the frame */
} acrmi_roi;
/* Host only: the clamped window (l, t, r, b) and the `offsets` row of one box in an H x W frame; either output may be NULL. */
int acrmi_roi_offsets(int H, int W, const acrmi_roi* roi, int32_t window_ltrb[4], float offsets10[10]);
/* n regions of n_frames BGR frames -> out_rgb_dev [n,512,512,3] and offsets_host [n,10] (may be NULL), in region order.  Several
 * regions may name one frame, in any order; a frame no region names is not read.  Everything is checked before anything is
 * queued (the message names the region); geometry travels in the kernel arguments, 64 regions per launch, further regions in
 * further launches; both host arrays may be freed when the call returns. */
int acrmi_preprocess_rois(const acrmi_frame* frames_host, int n_frames, const acrmi_roi* rois_host, int n,
                          uint8_t* out_rgb_dev, float* offsets_host, void* stream);
/* The same on NV12 surfaces (the frame checks and coef6_host of acrmi_preprocess_nv12): byte for byte acrmi_preprocess_frames on
 * the window of the frame acrmi_nv12_to_rgb makes.  Chroma is addressed in frame coordinates, so odd l and t are fine. */
int acrmi_preprocess_rois_nv12(const acrmi_nv12_frame* frames_host, int n_frames, const acrmi_roi* rois_host, int n,
                               const int32_t* coef6_host, uint8_t* out_rgb_dev, float* offsets_host, void* stream);
/* Tracking on the device (DESIGN.md "Tracking on the device"): frame k -> boxes -> frame k+1 as launches on one stream.
 * The box rule is acr.utils.boxes_from_keypoints for fp32 points, in double, integer for integer: the points whose two
 * coordinates are finite; centre and extent of their bounding box; side = max(longer extent * scale, min_size); the square
 * floor / ceil'ed outwards, moved back inside the H x W frame and cut to it; no such point: the whole frame (0, 0, W, H).  One
 * clause more: a result without pixels (r <= l or b <= t: the side was lost against a huge centre) is the whole frame too.
 * scale finite and > 0, min_size >= 1, else ACRMI_EINVAL. */
/* host only: the rule on n_pts fp32 points [n_pts,2] (n_pts may be 0) */
int acrmi_track_box(const float* pts_host, int n_pts, int H, int W, double scale, int min_size, int32_t box_ltrb[4]);
/* pj2d_org_dev [n,2,21,2], slots_dev [n,2,ACRMI_SLOT], frame_hw_dev int32 [n,2] = (H, W) -> boxes_dev int32 [n,4].  The 21 points
 * of a hand take part when its ACRMI_SLOT_FLAG > 0.5; the coordinates of another hand are not looked at.  A frame size that
 * is not positive gives the box (0, 0, 0, 0), which acrmi_preprocess_rois_dev turns into its frame's whole window.  One launch. */
int acrmi_track_boxes(const float* pj2d_org_dev, const float* slots_dev, const int32_t* frame_hw_dev, int n, double scale,
                      int min_size, int32_t* boxes_dev, void* stream);
/* acrmi_preprocess_rois with the boxes in device memory: region i = box boxes_dev[i] of frame roi_frame_host[i] (NULL: frame i,
 * needs n == n_frames); offsets_dev float [n,10] and status_dev int32 [n] (0 = the box as given, 1 = it left no pixel and the
 * whole frame was taken) are written on the device; either may be NULL.  The kernel clamps the box to its frame itself, so no
 * box, whatever it holds, makes it read outside the frame.  The same launches as acrmi_preprocess_rois for the same n; no
 * copy, no synchronise, no allocation. */
int acrmi_preprocess_rois_dev(const acrmi_frame* frames_host, int n_frames, const int32_t* roi_frame_host, const int32_t* boxes_dev,
                              int n, uint8_t* out_rgb_dev, float* offsets_dev, int32_t* status_dev, void* stream);
int acrmi_preprocess_rois_nv12_dev(const acrmi_nv12_frame* frames_host, int n_frames, const int32_t* roi_frame_host,
                                   const int32_t* boxes_dev, int n, const int32_t* coef6_host, uint8_t* out_rgb_dev,
                                   float* offsets_dev, int32_t* status_dev, void* stream);
int acrmi_u8norm(const uint8_t* img, int n_pixels, float* out, void* stream);
/* ACRMI_OP_STEM stand-alone: img uint8 RGB [B,H,W,3] (H % 16 == 0, W % 128 == 0) -> [relu](conv3x3 stride 2 pad 1 of
 * (x/255*2-1) + bias) into channels out_coff..out_coff+63 of out [B,H/2,W/2,out_cs]; w_packed = packer.pack_stem(w
 * [64,3,3,3]) (acr/model.py:832,589-603). */
int acrmi_stem_conv(const uint8_t* img, int B, int H, int W, const float* w_packed, const float* bias, float* out,
                    int out_cs, int out_coff, int relu, void* stream);
int acrmi_bilinear2x(const float* in, int B, int H, int W, int in_cs, int C, float* out, int out_cs, void* stream);
int acrmi_fuse_sum(int nterms, const float* const* terms, const int* term_cs, const int* term_shift, int B, int H,
                   int W, int C, float* out, int out_cs, int relu, void* stream);
/* acr/model.py:103-113,126-136: pooled[b][part][c] = sum over the 128x128 pixels of softmax_pix(segm logit of the
 * part at the even pixels of the 256x256 map) * feat[b][pix][c].  ws: device workspace of at least
 * acrmi_attpool_ws_floats(B, C) floats. */
size_t acrmi_attpool_ws_floats(int B, int C);
int acrmi_attpool(const float* segm, int segm_cs, const float* feat, int feat_cs, int C, int B, float* ws,
                  float* pooled, void* stream);
/* acr/model.py:141-164 per frame and hand: LocallyConnected2d (:559-569) on the 16 pooled part features of this side
 * (parts part0..part0+15 of pooled [B,32,C]; C = 320: 256 contact + 64 shape channels as the reference pools them),
 * the shape Linear, and the mix conv's pare columns: out[b][co] = mix_b[co] + sum_k mix_wp[co][k] * pare[k],
 * pare = [offsets 96 | shape 10].  lc_w [6][256][16], lin_w [10][(C==320 ? 64 : 256)*16], mix_wp [109][106]. */
int acrmi_parebias(const float* pooled_dev, int C, int part0, const float* lc_w_dev, const float* lin_w_dev,
                   const float* lin_b_dev, const float* mix_wp_dev, const float* mix_b_dev, int B, float* out_dev,
                   int out_stride, void* stream);

/* Options.  ACRMI_OPT_POINT_HEADS (0/1, default 0): acrmi_forward evaluates the params/cam/prior head towers and
 * the mix conv only at the pixels the decode samples (same slots/vertices within fp32 round-off; the dense
 * l/r_params_maps and l/r_prior_maps are then NOT produced - acrmi_backbone_heads always computes them). */
#define ACRMI_OPT_POINT_HEADS 1
/* ACRMI_OPT_LANES (0..8, default 0): the program's independent chains (HRNet branches, head towers, segm and part
 * heads; found from the ops' buffer reads/writes) run on that many HIP streams: lane 0 is the caller's stream, the
 * others fork from it at the start of a call and join it before the call's decode, so the caller still sees one
 * stream-ordered operation.  0 = chosen by batch size (4 lanes up to 32 frames, 2 above), 1 = single stream.
 * Same kernels, bit-identical results. */
#define ACRMI_OPT_LANES 2
/* ACRMI_OPT_CENTER_IDX (-1..20, default 9): the joint acrmi_forward's MANO stage aligns the mesh root on
 * (args().align_idx when args().mano_mesh_root_align, acr/mano_wrapper.py:19-33); -1 = no alignment. */
#define ACRMI_OPT_CENTER_IDX 3
/* ACRMI_OPT_TEMPORAL (0/1, default 0): acrmi_forward smooths the decoded poses/betas (acrmi_smooth) before MANO -
 * the reference's -t / temporal_optimization (acr/main.py:69-83).  The frames of a call are then ONE video stream
 * in order. */
#define ACRMI_OPT_TEMPORAL 4
/* ACRMI_OPT_MANO_FP16 (0/1, default 0; BASELINE.json configs[4] "fp16 MANO LBS"): the MANO stage (acrmi_mano and
 * acrmi_forward) reads its blend-shape tables (shapedirs, posedirs) and skinning weights from f16 copies made at
 * acrmi_load_mano - half the table traffic per hand; all products and sums stay fp32, v_template / J_regressor / the
 * kinematic chain are untouched.  Measured deviation from the fp32 tables: see tests/test_gpu_h16.py. */
#define ACRMI_OPT_MANO_FP16 7
/* ACRMI_OPT_LANE_PLAN (0/1, default 0 - planning is explicit): once acrmi_profile_ops has run at a small batch (<= 32 frames;
 * it stores the op times of the head mode that was active, dense or point, measured on one stream), the lanes of the
 * small-batch schedules are assigned by list scheduling over the MEASURED per-op times (every op goes to the lane where
 * it can start first; a cross-stream dependency is charged what it costs on MI355X, ~16 us over an in-stream one)
 * instead of by the structure of the graph alone.  Results do not depend on the assignment.  0 = structural only. */
#define ACRMI_OPT_LANE_PLAN 8
/* ACRMI_OPT_BATCH_PRIOR (0/1, default 0): 0 = every frame decides its cross-hand prior for itself - how the reference treats a
 * batch of ONE frame, the only way acr/main.py:126-141 ever calls it; 1 = acrmi_forward applies the reference's BATCH-WIDE
 * rules at B > 1 (acr/result_parser.py:42-47, 102-145: see acrmi_prior_gate) - decode, acrmi_prior_gate, gated decode, all on
 * the stream, no host round trip.  What ResultParser(batch_semantics='reference') / forward_batch(batch_semantics=...) set. */
#define ACRMI_OPT_BATCH_PRIOR 9
/* ACRMI_OPT_POINT_HEADS_MULTI (0/1, default 0): acrmi_forward_multi and acrmi_forward_tracks run the point variant of the
 * program, with the params/cam/prior towers and the mix conv at the pixels acrmi_decode_multi reads for max_hand - the distinct
 * top-max_hand centers of each side and the distinct partners (csrc/point_plan.h): at most 3 * max_hand tower points per side
 * and frame, found on the device, no host read.  Same slots / vertices within fp32 round-off (centers, flags and scores exactly);
 * the dense params / prior maps are then not produced.  0 = the dense heads, whatever ACRMI_OPT_POINT_HEADS says.  acrmi_forward
 * and acrmi_forward_streams do not look at it.  Setting it on a program without point-heads ops is ACRMI_EINVAL, as for
 * ACRMI_OPT_POINT_HEADS.  Measured on one MI355X (every rank with a detection, the most points there can
 * be): at batch 64 the call is 1.9 / 1.7 / 1.0 ms of 33 faster than with the dense heads at max_hand 2 / 4 / 8 - no crossover up
 * to ACRMI_MAX_HAND; at batch 1 it is 0.14 - 0.22 ms of 2.7 SLOWER at every max_hand, as ACRMI_OPT_POINT_HEADS is there: an
 * option for large batches. */
#define ACRMI_OPT_POINT_HEADS_MULTI 10
int acrmi_set_option(acrmi_ctx* ctx, int option, int value);
/* ACRMI_OPT_CONF_THRESH (default 0.35): center score threshold, strict > (args().centermap_conf_thresh,
 * acr/result_parser.py:198-205,241).  ACRMI_OPT_SMOOTH_COEFF (default 4.0): One-Euro mincutoff of the pose filters
 * (args().smooth_coeff, acr/main.py:45-47). */
#define ACRMI_OPT_CONF_THRESH 5
#define ACRMI_OPT_SMOOTH_COEFF 6
int acrmi_set_option_f(acrmi_ctx* ctx, int option, float value);

/* acr/main.py:69-83 + acr/utils.py:1466-1527 (smooth_results / OneEuroFilter / LowPassFilter): One-Euro smoothing
 * of slots_dev [B,2,ACRMI_SLOT] in place - poses[3:48] and betas directly, the global orientation as a rotation
 * matrix (acr/utils.py:1466-1470) - for the hands whose flag is set, frames in order, one filter set per hand type.
 * The filter state of ONE video stream lives in the context; acrmi_smooth_reset starts a new stream. */
int acrmi_smooth(acrmi_ctx* ctx, float* slots_dev, int B, void* stream);
int acrmi_smooth_reset(acrmi_ctx* ctx, void* stream);

/* The same smoothing for MANY video streams in one batch (N cameras, one frame of each per call): a stream table holds the
 * filter state the reference keeps per video in its filter_dict (acr/main.py:50-53, create_OneEuroFilter acr/utils.py:1472-1473)
 * for `capacity` streams (1..65536, else ACRMI_EINVAL) - per stream 2 hand types x (x_raw | x_filt | dx_filt)[64] floats
 * (element 0..44 finger pose, 45..54 betas, 55..63 rotation matrix) + an init flag per (stream, hand).  The table belongs to
 * no context: the contexts of a pool share one, and it outlives a context that a checkpoint reload replaces.  Created
 * zeroed: every stream starts fresh (its first sample passes through, acr/utils.py:1489-1496). */
typedef struct acrmi_streams acrmi_streams;
int acrmi_streams_create(acrmi_streams** out, int device, int capacity);
void acrmi_streams_destroy(acrmi_streams* t);
/* ids_host == NULL: every stream; else the n listed streams (each in [0, capacity)) start a new sequence - what a new video
 * does to the reference's filters (acr/main.py:50-53).  Queued on `stream`, ordered with the smoothing calls like them. */
int acrmi_streams_reset(acrmi_streams* t, const int32_t* ids_host, int n, void* stream);
/* acr/main.py:69-83 per stream: slots_dev [B,2,ACRMI_SLOT] smoothed in place with the coefficients of acrmi_smooth
 * (ACRMI_OPT_SMOOTH_COEFF of ctx; betas 0.6, beta 0.7, dcutoff 1, 30 Hz); ids_host [B] = the stream of each frame, -1 = leave
 * this frame alone.  Frames that carry the same id are ONE sequence, applied in batch order, wherever they stand in the batch;
 * different streams never see each other; a hand whose flag is not set (NaN included) leaves its filter untouched
 * (acr/main.py:78-80); nothing but poses and betas is written.  An id < -1 or >= capacity is ACRMI_EINVAL and nothing is
 * launched.  The ids travel in the kernel arguments (256 frames per launch, longer batches as successive launches in frame
 * order): nothing is allocated or uploaded, ids_host may be freed when the call returns.
 * Ordering between contexts: the table carries one HIP event; every call makes `stream` wait for it before its launches and
 * records it behind them, so calls of several contexts on several streams update a shared table in the order they were
 * made (host threads may call concurrently; the order is then the one in which they got the table's lock). */
int acrmi_smooth_streams(acrmi_ctx* ctx, acrmi_streams* t, float* slots_dev, int B, const int32_t* ids_host, void* stream);
/* acrmi_forward with acrmi_smooth_streams between decode and MANO (acr/main.py:69-83 sits there), whatever
 * ACRMI_OPT_TEMPORAL says.  The ids are checked before anything is launched. */
int acrmi_forward_streams(acrmi_ctx* ctx, acrmi_streams* t, const int32_t* ids_host, const uint8_t* img_dev, int B,
                          const float* offsets_dev, float* slots_dev, float* verts_dev, float* joints_dev,
                          float* verts_camed_dev, float* pj2d_dev, float* pj2d_org_dev, void* stream);

/* Tracks: with max_hand > 1 a hand's row is its rank by centre score, and ranks swap between frames.
 * A track table keeps, per video stream and side, max_hand track slots (live, frames missed, id, last centre, a One-Euro state
 * row in the layout of acrmi_streams) and says which hand of a frame continues which track: greedy nearest centre within
 * `gate` map pixels (0..128, 128 = any distance), a track unseen for more than `max_miss` frames (-1 = never, else >= 0) ends,
 * an unmatched hand starts a new track with the stream-and-side's next id (0, 1, ...) in the lowest free slot (evicting the
 * longest-unseen track when none is free).  The rule in full: csrc/assoc_plan.h.  gate = 8 and max_miss = 5 are the package's
 * defaults of these PARAMETERS, not measurements.  capacity >= 1 and capacity * max_hand <= 65536 (a hand's state is about
 * 0.8 KB), max_hand 1..ACRMI_MAX_HAND, else ACRMI_EINVAL.  Created zeroed: every slot free.  Ordering between contexts: the
 * table's event and host mutex, exactly as acrmi_streams. */
typedef struct acrmi_tracks acrmi_tracks;
int acrmi_tracks_create(acrmi_tracks** out, int device, int capacity, int max_hand, int gate, int max_miss);
void acrmi_tracks_destroy(acrmi_tracks* t);
/* ids_host == NULL: every stream; else the n listed streams (each in [0, capacity)): every slot free, the ids restart at 0. */
int acrmi_tracks_reset(acrmi_tracks* t, const int32_t* ids_host, int n, void* stream);
/* slots_dev [B,max_hand,2,ACRMI_SLOT] in place: per frame and side the rows are PERMUTED (whole rows; the two sides never look
 * at each other) so that row k holds the hand of track slot k - the slots without a hand in this frame receive the remaining
 * ranks in ascending order - and, with smooth != 0, every row that continues or starts a track is smoothed with that slot's own
 * One-Euro state (the arithmetic and coefficients of acrmi_smooth_streams; ctx NULL: the default ACRMI_OPT_SMOOTH_COEFF, 4.0, on the table's device).
 * ids_host [B]: the stream of each frame; frames that share an id are one sequence in batch order; -1 = the frame is left as
 * it is (track_ids -1, perm the identity).  track_ids_dev int32 [B,max_hand,2]: the id of the slot's track, -1 where the slot
 * has no hand in this frame; perm_dev int32 [B,max_hand,2] or NULL: the rank that moved there.  ACRMI_EINVAL before anything is
 * launched for an id < -1 or >= capacity and for a max_hand that is not the table's. */
int acrmi_associate(acrmi_ctx* ctx, acrmi_tracks* t, float* slots_dev, int B, int max_hand, const int32_t* ids_host, int smooth,
                    int32_t* track_ids_dev, int32_t* perm_dev, void* stream);
/* acrmi_forward_multi with acrmi_associate between decode and MANO: the meshes come out in track order.  ACRMI_OPT_TEMPORAL is
 * not looked at (`smooth` says whether the tracks are smoothed); ACRMI_OPT_BATCH_PRIOR with max_hand > 1 is ACRMI_EINVAL. */
int acrmi_forward_tracks(acrmi_ctx* ctx, acrmi_tracks* t, const int32_t* ids_host, int smooth, const uint8_t* img_dev, int B,
                         int max_hand, const float* offsets_dev, float* slots_dev, float* verts_dev, float* joints_dev,
                         float* verts_camed_dev, float* pj2d_dev, float* pj2d_org_dev, int32_t* track_ids_dev, void* stream);
/* Host only, no device: the rule for one frame of one (stream, side).  rows_host: the max_hand rows of that side in rank order,
 * row j at rows_host + j * row_stride floats (a frame's slots: rows_host = frame + side * ACRMI_SLOT, row_stride = 2 *
 * ACRMI_SLOT); state int32 [ACRMI_ASSOC_STATE] in and out: next_id, then live, miss, id, cy, cx of 8 slots each (all zero =
 * every slot free); track_ids, perm int32 [max_hand]; born int32 [max_hand] or NULL: 1 where the slot's track starts here. */
#define ACRMI_ASSOC_STATE 41
int acrmi_assoc_step(int max_hand, int gate, int max_miss, const float* rows_host, int row_stride, int32_t* state,
                     int32_t* track_ids, int32_t* perm, int32_t* born);

/* ---------------------------------------------------------------------------------------
 * Mesh overlay: acr/visualization.py:100-218 (Visualizer.visulize_result_live, show_items=['mesh'], settings ['put_org'])
 * + acr/renderer/renderer_pyrd.py / renderer_pt3d.py - the frame with the hand meshes drawn over it.  Nothing of those
 * renderers is used; the conventions are (DESIGN.md "Rendering"): camera-space point P = v + trans, +Z away from the
 * camera; on the 512 canvas x = 256 + focal X / Z, y = 256 + focal Y / Z; the frame's viewport x' = x * view[0] + view[2],
 * y' = y * view[1] + view[3] (the pj2d -> pj2d_org map of acrmi_mano); positions snapped to 1/256 pixel, exact integer
 * coverage with the top-left rule, pixel centres at +0.5; 1/Z depth test, the lower global face id wins a tie; smooth
 * shading 0.3 + 0.7 |n_z| interpolated perspective-correctly; covered pixel = floor(w 255 rgb shade + (1 - w) img), every
 * other pixel = img.  Triangles of zero area, with a vertex at Z <= 0.05 or with a snapped coordinate beyond +-2^22 are
 * dropped whole.  No atomics: results are deterministic.
 * ------------------------------------------------------------------------------------- */
/* Pure host (works without a GPU): faces [n_faces,3] of a mesh with n_verts vertices -> one int32 blob
 * [n_faces, n_verts | faces 3F | row V+1 | col 3F], (row, col) = the vertex -> faces table in CSR form, one entry per corner,
 * by face and then by corner: the order in which acrmi_rasterize sums a vertex's face normals.  Returns the number of ints
 * of the blob (also when blob_host == NULL: size query); n_ints = capacity of blob_host. */
int acrmi_mesh_topology(const int32_t* faces_host, int n_faces, int n_verts, int32_t* blob_host, int n_ints);
/* Bytes of device workspace acrmi_rasterize needs for n_meshes meshes of n_faces faces (0 for non-positive sizes). */
size_t acrmi_render_workspace(int n_meshes, int n_faces);
/* verts_dev [n_meshes,n_verts,3] fp32, trans_dev [n_meshes,3] or NULL; topo_dev = an acrmi_mesh_topology blob on the device,
 * topo2_dev (may be NULL) a second one with the SAME vertex and face counts (left / right MANO), mesh_topo_dev [n_meshes]
 * int32 0 / 1 = which of the two (NULL: all the first); mesh_frame_dev [n_meshes] int32 = the frame a mesh is drawn into,
 * < 0 = not drawn; rgb_dev [n_meshes,3] base colour in the image's channel order; view_dev [n_frames,4] (scale x, scale y,
 * shift x, shift y) or NULL = identity; img_in_dev / img_out_dev uint8 [n_frames,H,W,3] (may be the same buffer: drawn in
 * place); ids_out_dev int32 [n_frames,H,W] or NULL: mesh * n_faces + face of the visible triangle, -1 where none;
 * ws_dev: acrmi_render_workspace() bytes, 256-byte aligned, not shared by launches that may overlap.  All meshes of a frame
 * go through ONE depth-tested pass.  n_verts <= 4000. */
int acrmi_rasterize(const float* verts_dev, const float* trans_dev, int n_meshes, int n_verts, int n_faces,
                    const int32_t* topo_dev, const int32_t* topo2_dev, const int32_t* mesh_topo_dev,
                    const int32_t* mesh_frame_dev, const float* rgb_dev, const float* view_dev, float focal,
                    float visible_weight, const uint8_t* img_in_dev, uint8_t* img_out_dev, int n_frames, int H, int W,
                    int32_t* ids_out_dev, void* ws_dev, void* stream);
/* mano/manolayer.py:68,115 (th_faces) for side 0 = left, 1 = right: faces_host int32 [n_faces,3] over the 778 MANO vertices
 * (both sides the same face count). */
int acrmi_load_faces(acrmi_ctx* ctx, int side, const int32_t* faces_host, int n_faces);
/* The outputs of acrmi_forward in, frames out: verts_dev [B,2,778,3], cam_trans_dev [B,2,3] (acrmi_cam_trans), slots_dev
 * [B,2,ACRMI_SLOT] (a hand is drawn when its ACRMI_SLOT_FLAG > 0.5; hand type = slot index), offsets_dev [B,10] or NULL
 * (NULL: the 512 x 512 network input, identity viewport; else the frames the `offsets` rows describe), colors_host [2][3]
 * left / right in the image's channel order (NULL: the reference's, as RGB), img_in / img_out uint8 [B,H,W,3] on the device
 * (may alias), ids_out int32 [B,H,W] or NULL ((2 b + hand) * n_faces + face).  The context's scratch is allocated at the
 * first call (and when B grows); otherwise asynchronous on `stream`.  ACRMI_ESTATE before both sides' faces are loaded. */
int acrmi_render(acrmi_ctx* ctx, const float* verts_dev, const float* cam_trans_dev, const float* slots_dev, int B,
                 const float* offsets_dev, const float* colors_host, float focal, float visible_weight,
                 const uint8_t* img_in_dev, uint8_t* img_out_dev, int H, int W, int32_t* ids_out_dev, void* stream);

/* ---------------------------------------------------------------------------------------
 * Contact and interpenetration between two meshes (csrc/contact_plan.h, csrc/contact.hip): are the
 * two hands touching, where, and do the reconstructions run through each other.  The reference has no such measure.  It is
 * the usual nearest-VERTEX half-space heuristic - not a point-to-triangle distance and not a true inside test - and is
 * meaningful for closed meshes.  All fp32, every operation rounded on its own:
 *  position  P_m[i] = verts[m,i] + trans[m] per component; without trans the vertex as given.
 *  normal    N_m[i] = sign[m] * the sum, over the faces incident to vertex i in the order of the vertex -> faces table of
 *            acrmi_mesh_topology (by face, then by corner), of (v1 - v0) x (v2 - v0) taken on verts as given (before trans),
 *            each component (a*b) - (c*d), accumulated from 0.  NOT normalised: only its sign is used, there is no square
 *            root and no division.  sign[m] = +1 / -1 makes the rule hold for a topology wound inwards.  A vertex no face
 *            references has N = 0.
 *  nearest   for the ordered pair (a, b) and every vertex i of a: d = P_a[i] - P_b[j], d2(i,j) = (dx*dx + dy*dy) + dz*dz;
 *            nn[i] = the j with the smallest d2, the lowest j on a tie.  A NaN d2 never wins, nor does +inf (an overflowed
 *            square); if no j qualifies nn = -1, d2 = +inf, s = 0.
 *  side      s[i] = (dx*Nx + dy*Ny) + dz*Nz with the d and N_b of j = nn[i].  Vertex i is IN CONTACT when d2[i] <= r*r (r =
 *            contact_dist, the product in fp32) and INSIDE when s[i] < 0 and d2[i] <= m*m (m = max_depth, +inf allowed).
 *  both directions of a pair are computed: direction 0 = the vertices of a against b, direction 1 = those of b against a.
 *  summary   sum_f = (the smallest d2 of direction 0, the largest d2 among the inside vertices of direction 0, of direction 1
 *            - 0 when there are none; its square root is the penetration depth estimate -, 0);  sum_i = (i, j of that
 *            smallest d2 - the lowest i on a tie, (-1, -1) when there is none -, contact vertices of direction 0, 1, inside
 *            vertices of direction 0, 1).
 *  skipped   a pair with a mesh index < 0 (or >= n_meshes) is skipped: nn = -1, d2 = +inf, s = 0, zero counts, (-1, -1).
 * The defaults of the Python layer, contact_dist = 0.005 m and max_depth = 0.02 m, are parameters, not measurements.  The
 * relative placement of two hands is only as good as their two independent cam_trans fits.  No atomics on global memory:
 * deterministic; a pair computed alone equals the same pair computed in a batch.
 * ------------------------------------------------------------------------------------- */
/* Bytes of device workspace acrmi_mesh_contact needs for n_meshes meshes of n_verts vertices (0 for non-positive sizes). */
size_t acrmi_contact_workspace(int n_meshes, int n_verts);
/* verts_dev [n_meshes,n_verts,3] fp32, trans_dev [n_meshes,3] or NULL; topo_dev / topo2_dev / mesh_topo_dev as acrmi_rasterize
 * takes them; sign_dev [n_meshes] int32 (< 0: -1, else +1) or NULL = all +1; pairs_dev [n_pairs,2] int32 mesh indices (a
 * mesh may sit in several pairs, or be paired with itself); outputs nn_dev int32, d2_dev, s_dev fp32, each
 * [n_pairs,2,n_verts], sum_f_dev [n_pairs,4], sum_i_dev [n_pairs,6]; ws_dev: acrmi_contact_workspace() bytes, 16-byte aligned,
 * not shared by launches that may overlap.  n_verts <= 4000; contact_dist finite and >= 0, max_depth >= 0; n_pairs * 2 *
 * n_verts and n_meshes * n_verts at most 2^31 - 1.  NULL pointers and sizes are checked before any GPU call (ACRMI_EINVAL);
 * n_pairs == 0 is success and touches nothing.  The topology blobs are trusted (acrmi_mesh_topology validates them); the
 * pair indices are read on the device and need not be valid. */
int acrmi_mesh_contact(const float* verts_dev, const float* trans_dev, int n_meshes, int n_verts, int n_faces,
                       const int32_t* topo_dev, const int32_t* topo2_dev, const int32_t* mesh_topo_dev, const int32_t* sign_dev,
                       const int32_t* pairs_dev, int n_pairs, float contact_dist, float max_depth, int32_t* nn_dev, float* d2_dev,
                       float* s_dev, float* sum_f_dev, int32_t* sum_i_dev, void* ws_dev, void* stream);
/* The outputs of the forward calls in: verts_dev [B,K,2,778,3], cam_trans_dev [B,K,2,3], slots_dev [B,K,2,ACRMI_SLOT] (the row
 * layout of acrmi_forward_multi; K = 1: what acrmi_forward writes), K = 1..ACRMI_MAX_HAND.  The pairs of row b are (left rank
 * i, right rank j) with pair index (b*K + i)*K + j, direction 0 = the left hand's vertices; a pair with either ACRMI_SLOT_FLAG
 * not > 0.5 is skipped - the flags are read on the device, there is no host visit.  Pairs are formed inside a row only.
 * sign_host [2] (left, right) or NULL = the signs the context derived when the faces were loaded: the orientation of the
 * side's faces on its template vertices (sign of sum v0 . (v1 x v2) in double, +1 when 0 or before acrmi_load_mano).
 * Outputs as acrmi_mesh_contact with n_pairs = B*K*K, n_verts = 778.  The context's scratch is allocated at the first call
 * (and when B*K grows); otherwise asynchronous on `stream`.  ACRMI_ESTATE before both sides' faces are loaded. */
int acrmi_contact(acrmi_ctx* ctx, const float* verts_dev, const float* cam_trans_dev, const float* slots_dev, int B, int K,
                  const int32_t* sign_host, float contact_dist, float max_depth, int32_t* nn_dev, float* d2_dev, float* s_dev,
                  float* sum_f_dev, int32_t* sum_i_dev, void* stream);

/* ---------------------------------------------------------------------------------------
 * The SURFACE contact measure between two meshes (csrc/surface_contact_plan.h,
 * csrc/contact.hip): the distance from every vertex to the other mesh's surface with the point on it, and
 * containment by counting ray crossings in a way that is exact on a closed mesh.  The measure above stays the default; this
 * one costs every vertex against every face.  All fp32, every operation rounded on its own, `/` correctly rounded:
 *  dot(a,b) = (ax*bx + ay*by) + az*bz; a cross component is (a*b) - (c*d); P_m[i] = verts[m,i] + trans[m] as above.
 *  For the ordered pair (a, b), vertex p = P_a[i] and face f of b with corners A, B, C = P_b[f0], P_b[f1], P_b[f2]:
 *  closest   point of the triangle (Ericson, Real-Time Collision Detection 5.1.5); every comparison is false on NaN, the first
 *            true branch wins.  ab = B-A, ac = C-A, ap = p-A, d1 = dot(ab,ap), d2 = dot(ac,ap); bp = p-B, d3 = dot(ab,bp),
 *            d4 = dot(ac,bp); cp = p-C, d5 = dot(ab,cp), d6 = dot(ac,cp); vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6,
 *            va = d3*d6 - d5*d4; e43 = d4-d3, e56 = d5-d6.
 *            1. d1<=0 && d2<=0: q = A.   2. d3>=0 && d4<=d3: q = B.   3. vc<=0 && d1>=0 && d3<=0: q = A + (d1/(d1-d3))*ab.
 *            4. d6>=0 && d5<=d6: q = C.   5. vb<=0 && d2>=0 && d6<=0: q = A + (d2/(d2-d6))*ac.
 *            6. va<=0 && e43>=0 && e56>=0: q = B + (e43/(e43+e56))*(C-B).
 *            7. otherwise: den = 1/((va+vb)+vc), q = (A + ab*(vb*den)) + ac*(vc*den).
 *            e = p-q, D2(i,f) = dot(e,e).  face[i] = the f with the smallest D2 below +inf, the lowest f on a tie; NaN and
 *            +inf never win, degenerate faces need no special case; d2[i] is that value and point[i] that face's q.  When no
 *            face qualifies: face = -1, d2 = +inf, point = 0.
 *  crossings of the ray from p towards +Z.  For each face edge u -> v (mesh vertex indices; f0->f1, f1->f2, f2->f0): lo, hi =
 *            the positions of min(u,v), max(u,v); E = (hi.x-lo.x)*(p.y-lo.y) - (hi.y-lo.y)*(p.x-lo.x); sc = (E >= 0) ? +1 : -1;
 *            the edge's sign is sc when u < v, -sc when u > v, 0 when u == v.  The face covers p when its three signs are
 *            equal and not zero.  The ray meets the face's plane in front of p when o = dot(ap, n), n = ab x ac, and n.z have
 *            strictly opposite signs (neither zero, NaN fails).  cross[i] = the number of faces that do both; vertex i is
 *            inside when cross[i] is odd.  The two faces that share an edge compute its value identically: exact on a closed
 *            mesh, meaningless on an open one.
 *  flags     per direction (surface distance is not symmetric).  IN CONTACT: face >= 0 and d2 <= r*r.  INSIDE: face >= 0,
 *            cross odd and d2 <= m*m.
 *  summary   sum_f = (min d2 of direction 0, of direction 1, depth2 of direction 0, of direction 1: the largest d2 among the
 *            inside vertices, 0 when there are none); sum_i = (closest (i, face) of direction 0, of direction 1 - the lowest
 *            i on a tie, (-1, -1) when there is none -, contact vertices of direction 0, 1, inside vertices of direction 0, 1).
 *  skipped   a pair with a mesh index < 0 (or >= n_meshes): face = -1, d2 = +inf, point = 0, cross = 0, zero counts, (-1, -1).
 * No cull, no atomics on global memory: deterministic; a pair computed alone equals the same pair computed in a batch.
 * ------------------------------------------------------------------------------------- */
/* Bytes of device workspace acrmi_mesh_surface_contact needs (0 for non-positive sizes). */
size_t acrmi_surface_contact_workspace(int n_meshes, int n_verts, int n_faces);
/* Arguments as acrmi_mesh_contact takes them (there is no sign: the crossing rule does not depend on the winding).  Outputs
 * face_dev, cross_dev int32 and d2_dev fp32 [n_pairs,2,n_verts], point_dev fp32 [n_pairs,2,n_verts,3], sum_f_dev [n_pairs,4],
 * sum_i_dev [n_pairs,8]; ws_dev: acrmi_surface_contact_workspace() bytes, 16-byte aligned, not shared by launches that may
 * overlap.  n_verts <= 4000, n_faces <= 8000; contact_dist finite and >= 0, max_depth >= 0; n_pairs * 6 * n_verts, n_meshes *
 * n_verts and n_meshes * n_faces * 3 at most 2^31 - 1: beyond any of these ACRMI_EINVAL, nothing is clamped.  NULL pointers
 * and sizes are checked before any GPU call; n_pairs == 0 is success and touches nothing.  The topology blobs are trusted;
 * the pair indices are read on the device and need not be valid. */
int acrmi_mesh_surface_contact(const float* verts_dev, const float* trans_dev, int n_meshes, int n_verts, int n_faces,
                               const int32_t* topo_dev, const int32_t* topo2_dev, const int32_t* mesh_topo_dev,
                               const int32_t* pairs_dev, int n_pairs, float contact_dist, float max_depth, int32_t* face_dev,
                               float* d2_dev, float* point_dev, int32_t* cross_dev, float* sum_f_dev, int32_t* sum_i_dev,
                               void* ws_dev, void* stream);
/* The surface measure of the pairs acrmi_contact forms (same inputs, same pair order, the context's face tables, which must
 * have equally many faces on both sides); outputs as acrmi_mesh_surface_contact with n_pairs = B*K*K, n_verts = 778.  Its
 * scratch is the context's own, allocated at the first call (and when B*K grows); otherwise asynchronous on `stream`. */
int acrmi_surface_contact(acrmi_ctx* ctx, const float* verts_dev, const float* cam_trans_dev, const float* slots_dev, int B,
                          int K, float contact_dist, float max_depth, int32_t* face_dev, float* d2_dev, float* point_dev,
                          int32_t* cross_dev, float* sum_f_dev, int32_t* sum_i_dev, void* stream);

/* ---------------------------------------------------------------------------------------
 * Scoring against ground truth (csrc/score_plan.h, csrc/score.hip): MPJPE / MPVPE root-aligned and
 * Procrustes-aligned, per point and per row, and a device-resident BOARD of running sums (per-joint tables, a histogram for
 * the PCK curve, MRRPE) that the host visits once, at the end.  The reference ships no evaluation code.
 * Inputs fp32, arithmetic fp64 with every operation rounded on its own; outputs are the fp64 value rounded to fp32.  A row is
 * one hand, a point set n <= 4000 points.
 *  counted   point i counts when valid[i] != 0 (or there is no valid array) and the six coordinates of P[i] (prediction) and
 *            G[i] (truth) are finite.  A row is SCORED when group[row] is in [0, n_groups) and its flag is > 0.5 (no flags:
 *            every row is flagged; no groups: group 0); a MISS when the group is in range and the flag is not set - counted
 *            per group, enters no error; a group out of range (negative, >= n_groups, INT_MIN): the row is not looked at.  A
 *            row that is not scored has -1 in its per-point outputs and in row_f, and zero counts.
 *  origins   oP, oG = P[root], G[root] when root >= 0, else the rows of the two origin arrays, else zero; GOOD when the root
 *            point is counted / the six values are finite.
 *  e_ra      |(P[i] - oP) - (G[i] - oG)| of a counted point of a row with good origins; |d| = sqrt((dx*dx + dy*dy) + dz*dz).
 *  sums      over the points: thread t of T (64 when n <= 64, else 256) adds its points t, t + T, ... in ascending order (a
 *            point that does not count adds +0), then the fixed tree for (s = T/2; s >= 1; s /= 2) v[t] += v[t + s], t < s.
 *  e_pa      over the c counted points: means muP, muG; Pc = P - muP, Gc = G - muG; S[a][b] = sum Pc_a Gc_b; vP = sum
 *            (Pcx*Pcx + Pcy*Pcy) + Pcz*Pcz; Horn's (1987) symmetric 4 x 4 matrix N of S; cyclic Jacobi on N, pairs (0,1) (0,2)
 *            (0,3) (1,2) (1,3) (2,3), exactly 6 sweeps, no convergence test: a zero a_pq is skipped, else theta = (a_qq - a_pp)
 *            / (2 a_pq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)) with sign(0) = +1 (an overflowing theta^2 gives t =
 *            0), c = 1 / sqrt(t^2 + 1), s = t c, a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0, a_rp' = c a_rp - s a_rq, a_rq' = s a_rp
 *            + c a_rq, the eigenvector columns alike.  The quaternion (w, x, y, z) is the eigenvector of the largest diagonal
 *            element, the lowest index on a tie; R is built from it; scale = lambda / vP;
 *            e_pa[i] = |(scale * (R Pc[i]) + muG) - G[i]|.  Only with c >= 3 and vP > 0.
 *  row_f     [N,4]: mean e_ra, mean e_pa (the sum of the fp64 errors over their count; -1 without one), scale (-1 without
 *            e_pa), |(oP + trans) - oG| (-1 without a finite trans or good origins).   row_i [N,2]: the two counts.
 *  xform     [N,8], optional: quaternion, scale, translation muG - scale * (R muP) (zeros with scale -1 without e_pa).
 *  pair_err  [N/2], optional: rows 2p, 2p + 1 are the left and right hand of pair p; |((oP_R + t_R) - (oP_L + t_L)) - (oG_R -
 *            oG_L)| when both are scored, have good origins and a finite trans, else -1 (the MRRPE term).
 *  board     of one point set, 8-byte words, per group: sum_ra[n], sum_pa[n] fp64, cnt_ra[n], cnt_pa[n] int64, hist[n_bins + 1]
 *            int64 of the set's e_ra (bin min(n_bins, (int64)((double)e / bin_width)); -1 and NaN are never binned), rows
 *            scored, rows missed.  The pair board: per (left group, right group) the pair_err sum fp64 and count int64.  A
 *            call continues from the board's values and adds the fp32 outputs >= 0, converted to double, in ascending row
 *            order: 2B rows in one call equal two calls of B rows bit for bit.  No floating-point atomics, no atomics on
 *            global memory, one writer per element.  The defaults of the Python layer, 100 bins of 0.5 mm, are parameters.
 * ------------------------------------------------------------------------------------- */
/* Bytes of the board of a set of n points (0 for sizes outside n 1..4000, n_groups 1..16, n_bins 1..4096), of the pair board. */
size_t acrmi_score_board_bytes(int n, int n_groups, int n_bins);
size_t acrmi_score_pair_bytes(int n_groups);
/* pred_dev, gt_dev [N,n,3] fp32; valid_dev [N,n] bytes or NULL; root in -1..n-1; origin_pred_dev / origin_gt_dev [N,3] (both or
 * neither; read when root < 0); trans_dev [N,3] or NULL; group_dev [N] int32 or NULL; flags_dev [N] fp32 or NULL.  Outputs
 * e_ra_dev, e_pa_dev [N,n], row_f_dev [N,4], row_i_dev [N,2], optional xform_dev [N,8] and pair_err_dev [N/2].  N * n * 3 at
 * most 2^31 - 1.  Pointers and sizes are checked before any GPU call (ACRMI_EINVAL); N == 0 is success and touches nothing. */
int acrmi_pose_errors(const float* pred_dev, const float* gt_dev, const uint8_t* valid_dev, int N, int n, int root,
                      const float* origin_pred_dev, const float* origin_gt_dev, const float* trans_dev, const int32_t* group_dev,
                      int n_groups, const float* flags_dev, float* e_ra_dev, float* e_pa_dev, float* row_f_dev, int32_t* row_i_dev,
                      float* xform_dev, float* pair_err_dev, void* stream);
/* Adds the rows of one acrmi_pose_errors call to a board: e_ra_dev, e_pa_dev, pair_err_dev (or NULL) as it wrote them, group_dev
 * and flags_dev as it took them; board_dev acrmi_score_board_bytes(), pair_board_dev acrmi_score_pair_bytes() or NULL, both 8-byte
 * aligned, zeroed by the caller before the first call.  n_bins 1..4096, bin_width finite and > 0. */
int acrmi_score_accumulate(const float* e_ra_dev, const float* e_pa_dev, int N, int n, const int32_t* group_dev, int n_groups,
                           const float* flags_dev, const float* pair_err_dev, int n_bins, double bin_width, void* board_dev,
                           void* pair_board_dev, void* stream);
/* The outputs of the forward calls against truth: joints_dev [B,K,2,21,3], verts_dev [B,K,2,778,3], slots_dev
 * [B,K,2,ACRMI_SLOT], cam_trans_dev [B,K,2,3] or NULL (then no root error and no MRRPE); gt_joints_dev like joints_dev,
 * gt_verts_dev like verts_dev or NULL, joint_valid_dev [B,K,2,21] bytes or NULL, group_dev [B,K,2] int32 or NULL = the side.
 * Row = hand, flag = ACRMI_SLOT_FLAG.  Both point sets in one call: the joints with root = the context's centre index (< 0: no
 * alignment), the vertices on the joints' origins; pairs are (left rank k, right rank k).  Outputs j_* as acrmi_pose_errors
 * over n = 21, v_* over n = 778 (ignored without gt_verts_dev), pair_err_dev [B*K].  board_dev NULL, or the board of n = 21, then
 * the board of n = 778, then the pair board, to which the call is added. */
int acrmi_score_hands(acrmi_ctx* ctx, const float* joints_dev, const float* verts_dev, const float* slots_dev,
                      const float* cam_trans_dev, const float* gt_joints_dev, const float* gt_verts_dev,
                      const uint8_t* joint_valid_dev, const int32_t* group_dev, int B, int K, int n_groups, int n_bins,
                      double bin_width, void* board_dev, float* j_e_ra_dev, float* j_e_pa_dev, float* j_row_f_dev,
                      int32_t* j_row_i_dev, float* v_e_ra_dev, float* v_e_pa_dev, float* v_row_f_dev, int32_t* v_row_i_dev,
                      float* pair_err_dev, void* stream);

/* ---------------------------------------------------------------------------------------
 * Matching decoded hands to ground truth (csrc/match_plan.h, csrc/match.hip): with max_hand = K a frame
 * holds up to K hands of each side in the order of their centre confidence, which says nothing about the order of the
 * annotations.  These calls find, per (frame b, side s), the exact assignment of predictions to truths on the device, gather
 * rows into truth order - what acrmi_score_hands then takes unchanged - and count true positives, false positives and misses.
 * A PROBLEM is one (b, s): predictions i = 0..K-1, truths g = 0..G-1, 1 <= K, G <= 8, independent of each other; point sets of
 * n points (1 <= n <= 256) of D coordinates, D = 2 (pixels) or 3 (metres).  Inputs fp32, arithmetic fp64 with every operation
 * rounded on its own.
 *  cost      of the pair (i, g): point j counts when valid[b,g,s,j] != 0 (or there is no valid array) and all 2D coordinates
 *            are finite.  P is the prediction plus trans[b,i,s] when trans is given, added in fp64.  d_j = sqrt(dx*dx + dy*dy)
 *            for D = 2, sqrt((dx*dx + dy*dy) + dz*dz) for D = 3.  cost = (sum of d_j in ascending j, a point that does not
 *            count adds +0) / count.
 *  allowed   a pair is allowed when the prediction's flag is > 0.5 (read with a stride, so ACRMI_SLOT_FLAG of the slots goes in
 *            as it is; NaN is not flagged; flags NULL: every prediction is flagged), truth_valid[b,g,s] != 0 (or NULL), count >=
 *            min_points, and the cost is finite and <= (double)gate.  gate is finite and >= 0, or +inf; min_points in 1..n.
 *  objective among one-to-one matchings of allowed pairs the most pairs, among those the smallest cost sum.
 *  rule      the subset recurrence: state m = bitmask of used truths, value (cnt, sum); dp[0] = (0, +0.0), every other state
 *            unreachable.  For i = 0..K-1 in order and every m: start from dp[m] (prediction i stays unmatched); then for g
 *            ascending with bit g set in m, (i, g) allowed and dp[m ^ (1 << g)] reachable, the candidate (cnt + 1, sum +
 *            cost[i][g]) replaces the current best only on a strict improvement: a larger cnt, or an equal cnt and a smaller
 *            sum.  The choice (-1 or g) is recorded per (i, m).  The final state is the best over m ascending, strict
 *            improvement again; backtrack from i = K-1 down.
 *  outputs   match int32 [B,K,2]: the truth of each prediction or -1; pred_of int32 [B,G,2]: the inverse; cost fp32 [B,K,2]: the
 *            matched pair's cost rounded to fp32, -1 when unmatched; counts int32 [B,2,3]: TP = matched pairs, FP = flagged
 *            predictions left unmatched, FN = valid truths left unmatched; group int32 [B,G,2]: the caller's group (default
 *            the side) where the truth is valid, else -1.
 *  gather    dst[b,q,s,:] = src[b, index[b,q,s], s, :] for fp32 rows of any width W; an index outside [0, Ks) gives a row of
 *            +0 bytes.  Every index is range-checked before it becomes an address.
 *  board     8 words of 8 bytes, per side [TP, FP, FN int64 | matched-cost sum fp64].  A call continues from the board's values
 *            and adds the counts and the fp32 costs >= 0, converted to double, in ascending frame order, one writer per element,
 *            no atomics: 2B frames in one call equal two calls of B frames bit for bit.
 * Anything outside the limits is refused with ACRMI_EINVAL before any GPU call and never clamped; B == 0 is success and
 * touches nothing.
 * ------------------------------------------------------------------------------------- */
size_t acrmi_match_board_bytes(void);
/* pred_dev [B,K,2,n,D], truth_dev [B,G,2,n,D] fp32; valid_dev [B,G,2,n] bytes or NULL; truth_valid_dev [B,G,2] bytes or NULL;
 * flags_dev: the flag of prediction (b,i,s) at flags_dev[((b*K + i)*2 + s) * flag_stride], or NULL; trans_dev [B,K,2,D] or NULL;
 * group_dev [B,G,2] int32 or NULL = the side.  B * max(K,G) * 2 * n * D at most 2^31 - 1. */
int acrmi_match_hands(const float* pred_dev, const float* truth_dev, const uint8_t* valid_dev, const uint8_t* truth_valid_dev,
                      const float* flags_dev, int flag_stride, const float* trans_dev, const int32_t* group_dev, int B, int K, int G,
                      int n, int D, float gate, int min_points, int32_t* match_dev, int32_t* pred_of_dev, float* cost_dev,
                      int32_t* counts_dev, int32_t* group_out_dev, void* stream);
/* src_dev [B,Ks,2,W] fp32, index_dev [B,Kd,2] int32, dst_dev [B,Kd,2,W]; Ks, Kd in 1..8, W >= 1, pointers 4-byte aligned.
 * 16-byte accesses when W % 4 == 0 and src_dev and dst_dev are 16-byte aligned, 4-byte accesses otherwise. */
int acrmi_match_gather(const float* src_dev, const int32_t* index_dev, int B, int Ks, int Kd, int W, float* dst_dev, void* stream);
/* Adds counts_dev [B,2,3] and cost_dev [B,K,2] of one acrmi_match_hands call to board_dev (acrmi_match_board_bytes(), 8-byte
 * aligned, zeroed by the caller before the first call).  K only indexes cost_dev. */
int acrmi_match_accumulate(const int32_t* counts_dev, const float* cost_dev, int B, int K, void* board_dev, void* stream);

/* ---------------------------------------------------------------------------------------
 * Key-point skeleton and centre heat-map views: acr/visualization.py:228-300 (Visualizer.visulize_result_live with
 * show_items 'pj2d' / 'centermap', vis_keypoints, make_heatmaps), drawn on the device.  Nothing of PIL or cv2 is used; the
 * rules are (DESIGN.md "Key-point and heat-map views"):
 *  Skeleton - integer throughout.  The 21 key points of a hand are re-ordered by mano2interhand_mapper
 *   {4,3,2,1, 8,7,6,5, 12,11,10,9, 16,15,14,13, 20,19,18,17, 0}; the tree is mano/skeleton.txt: joint i has parent i + 1,
 *   the base of each finger (i % 4 == 3) has parent 20, the wrist, which has none.  A key point is truncated toward zero to
 *   the pixel k; a hand with a non-finite key point is not drawn; a primitive with an end point at |k| >= 16384 is dropped.
 *   Disc of radius r at k: (x-kx)^2 + (y-ky)^2 <= r^2 + r.  Bone a -> b of width w, d = b - a, L2 = |d|^2 > 0, u = p - a:
 *   0 <= u.d <= L2, |u x d| < 2^18 and 4 (u x d)^2 <= w^2 L2.  Painter's order: per hand (in hand order), per joint i = 0..20
 *   with parent p: bone(i, p) in colour[p], disc(i) in colour[i], disc(p) in colour[p] (the wrist: its disc only); the last
 *   primitive that covers a pixel wins and its colour is written opaque, every other pixel is the input byte for byte.
 *  Heat map - fp32, every operation rounded on its own, in this order.  Canvas coordinate of pixel (x, y):
 *   cx = (x + 0.5 - ox) / sx with the image's view row (sx, sy, ox, oy) (the one acrmi_rasterize takes), cx = (x + 0.5) *
 *   (512 / W) without one; a pixel with cx or cy outside [0, 512) - and every pixel of a view with sx or sy not > 0 - keeps
 *   the input.  s = max(cx * (w / 512) - 0.5, 0), i0 = min(int(s), w - 1), i1 = min(i0 + 1, w - 1), l1 = s - i0, l0 = 1 - l1,
 *   the same in y; v = ly0 (lx0 a + lx1 b) + ly1 (lx0 c + lx1 d); idx = int(min(max(v * 255, 0), 255)) (truncated; NaN -> 0);
 *   out = floor(weight * LUT[idx] + (1 - weight) * img).  Default LUT [256][3], RGB, t = i / 255: red clamp(1.5 - |4t - 3|),
 *   green clamp(1.5 - |4t - 2|), blue clamp(1.5 - |4t - 1|), clamped to [0, 1], byte = floor(255 v + 0.5) - which is the
 *   integer clamp(383 - |4 i - 255 k|, 0, 255), k = 3, 2, 1.  A piece-wise linear "jet", NOT cv2.COLORMAP_JET byte for byte.
 * No atomics on global memory: deterministic; a frame drawn alone equals the frame drawn in a batch; in place = out of place.
 * ------------------------------------------------------------------------------------- */
#define ACRMI_OVERLAY_SKELETON 0
#define ACRMI_OVERLAY_CENTERMAP 1
/* Pure host: the default tables in RGB order, or flipped (bgr != 0): colors_host [21][3] by skeleton joint (the values
 * get_keypoint_rgb yields for mano/skeleton.txt), lut_host [256][3].  Either may be NULL. */
int acrmi_overlay_tables(int bgr, uint8_t* colors_host, uint8_t* lut_host);
/* kps_dev fp32 [n_hands,21,2] in pixels of the image drawn into, MANO joint order; hand_frame_dev int32 [n_hands] = the frame
 * a hand is drawn into, < 0 (or >= n_frames) = not drawn; colors_host [21][3] bytes by skeleton joint in the image's channel
 * order, NULL = the default table (flipped when bgr != 0); line_width 1..11, circle_rad 0..255; img_in_dev / img_out_dev
 * uint8 [n_frames,H,W,3], may be the same buffer; H, W <= 16384, n_frames <= 65535. */
int acrmi_draw_skeletons(const float* kps_dev, const int32_t* hand_frame_dev, int n_hands, const uint8_t* colors_host, int bgr,
                         int line_width, int circle_rad, const uint8_t* img_in_dev, uint8_t* img_out_dev, int n_frames, int H,
                         int W, void* stream);
/* maps_l_dev / maps_r_dev fp32: the [h,w] map of image i starts at element i * frame_stride (>= h * w); maps_r_dev and
 * out_r_dev are both NULL for one view; view_dev [n,4] or NULL; weight in [0,1] (the reference: 0.7); lut_host [256][3] bytes
 * in the image's channel order, NULL = the default (flipped when bgr != 0); img_in_dev, out_l_dev, out_r_dev uint8
 * [n,H,W,3] - ONE launch reads the image once and writes both views; out_l_dev may be img_in_dev. */
int acrmi_draw_heatmaps(const float* maps_l_dev, const float* maps_r_dev, long long frame_stride, int n, int h, int w,
                        const float* view_dev, float weight, const uint8_t* lut_host, int bgr, const uint8_t* img_in_dev,
                        uint8_t* out_l_dev, uint8_t* out_r_dev, int H, int W, void* stream);
/* The outputs of acrmi_forward in, frames out, like acrmi_render.  what = ACRMI_OVERLAY_SKELETON: slots_dev [B,2,ACRMI_SLOT]
 * (a hand is drawn when its ACRMI_SLOT_FLAG > 0.5) and pj2d_dev [B,2,21,2] - with offsets_dev NULL the projected key points
 * `pj2d` in [-1,1], drawn at (pj2d + 1) / 2 * 512 on the 512 x 512 network input (acr/visualization.py:241); with
 * offsets_dev [B,10] `pj2d_org`, pixels of the original frames; default colours, line_width = circle_rad = 3; out2_dev
 * unused.  what = ACRMI_OVERLAY_CENTERMAP: the left / right centre maps the context's head buffers hold since the last
 * program run, which must have been at batch B (a 16-bit storage program's maps are converted to fp32 inside the kernel),
 * over the frames at weight 0.7 -> out_dev (left), out2_dev (right); the view of frame b comes from its offsets row as in
 * acrmi_render (NULL: the network input); slots_dev / pj2d_dev unused.  bgr != 0: the default tables flipped.
 * ACRMI_ESTATE before a program has run (acrmi_forward / acrmi_backbone_heads / acrmi_heads). */
int acrmi_overlay(acrmi_ctx* ctx, int what, const float* slots_dev, const float* pj2d_dev, int B, const float* offsets_dev,
                  int bgr, const uint8_t* img_in_dev, uint8_t* out_dev, uint8_t* out2_dev, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------
 * Views over REGIONS of interest (DESIGN.md "Views over regions"; the rule once in csrc/region_view_plan.h): n regions of
 * n_frames equal-sized frames, region i described by its `offsets` row (acrmi_roi_offsets, acrmi_preprocess_rois*) and
 * region_frame_dev[i] int32, both in device memory - what acrmi_preprocess_rois_dev wrote goes in as it is.  fp32, every
 * operation rounded on its own:
 *  view   (sx, sy, ox, oy) = (o[0] / 512, o[1] / 512, o[5] - o[9], o[2] - o[6]), as acrmi_render / acrmi_overlay
 *  window l = o[5], t = o[2], r = W - o[3], b = H - o[4], clamped into the frame (NaN -> 0); a pixel belongs to it when its
 *         centre does.  A region whose window has no pixel, whose sx or sy is not > 0, or whose frame index is outside
 *         [0, n_frames) draws nothing; no row, whatever it holds, makes a kernel touch memory outside the frames.
 *  meshes hand h of region i is projected on the 512 canvas and mapped by ITS region's view; it is not clipped to the window.
 *         All meshes of all regions of a frame go through one depth-tested pass; the depth value of a vertex is sx / Z (one
 *         virtual camera per frame: two regions of a frame have cameras of different scale).  ids: (2 i + h) * n_faces + face.
 *  heat   region i covers pixel (x, y) of frame f when region_frame[i] == f, the pixel is in i's window and its canvas
 *  maps   coordinate under i's view is in [0, 512); idx_i as acrmi_draw_heatmaps; the pixel's index is the MAXIMUM of idx_i over
 *         the covering regions; out = floor(weight * LUT[idx] + (1 - weight) * img); a pixel no region covers keeps the input.
 * ------------------------------------------------------------------------------------- */
/* acrmi_rasterize with one view row per MESH: view_dev [n_meshes,4] (not NULL), and the depth value view[0] / Z. */
int acrmi_rasterize_views(const float* verts_dev, const float* trans_dev, int n_meshes, int n_verts, int n_faces,
                          const int32_t* topo_dev, const int32_t* topo2_dev, const int32_t* mesh_topo_dev,
                          const int32_t* mesh_frame_dev, const float* rgb_dev, const float* view_dev, float focal,
                          float visible_weight, const uint8_t* img_in_dev, uint8_t* img_out_dev, int n_frames, int H, int W,
                          int32_t* ids_out_dev, void* ws_dev, void* stream);
/* acrmi_draw_heatmaps for regions: the [h,w] map of REGION i starts at element i * frame_stride; offsets_dev [n,10],
 * region_frame_dev [n]; img_in_dev, out_l_dev, out_r_dev uint8 [n_frames,H,W,3]; the rest as acrmi_draw_heatmaps. */
int acrmi_draw_region_heatmaps(const float* maps_l_dev, const float* maps_r_dev, long long frame_stride, int n, int h, int w,
                               const float* offsets_dev, const int32_t* region_frame_dev, float weight,
                               const uint8_t* lut_host, int bgr, const uint8_t* img_in_dev, uint8_t* out_l_dev,
                               uint8_t* out_r_dev, int n_frames, int H, int W, void* stream);
/* acrmi_render for the outputs of a forward on n regions: verts_dev [n,2,778,3], cam_trans_dev [n,2,3], slots_dev
 * [n,2,ACRMI_SLOT]; img_in / img_out uint8 [n_frames,H,W,3] (may alias), ids_out int32 [n_frames,H,W] or NULL. */
int acrmi_render_regions(acrmi_ctx* ctx, const float* verts_dev, const float* cam_trans_dev, const float* slots_dev, int n,
                         const float* offsets_dev, const int32_t* region_frame_dev, const float* colors_host, float focal,
                         float visible_weight, const uint8_t* img_in_dev, uint8_t* img_out_dev, int n_frames, int H, int W,
                         int32_t* ids_out_dev, void* stream);
/* acrmi_overlay for n regions.  ACRMI_OVERLAY_SKELETON: pj2d_org_dev [n,2,21,2] (pixels of the frames); hand h of region i is
 * drawn into frame region_frame[i] when its flag is set and the region draws.  ACRMI_OVERLAY_CENTERMAP: the centre maps of the
 * last program run, which must have been at batch n -> out_dev (left), out2_dev (right), [n_frames,H,W,3] each. */
int acrmi_overlay_regions(acrmi_ctx* ctx, int what, const float* slots_dev, const float* pj2d_org_dev, int n,
                          const float* offsets_dev, const int32_t* region_frame_dev, int bgr, const uint8_t* img_in_dev,
                          uint8_t* out_dev, uint8_t* out2_dev, int n_frames, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------
 * Per-vertex colours: the contact and error views (csrc/vertex_color_plan.h, csrc/vertex_color.hip,
 * csrc/render.hip).  The reference has no such view.  All fp32, every operation rounded on its own, `/` and sqrt correctly
 * rounded.
 *  raster   with vcol [n_meshes,n_verts,3] (base colours in [0,1], the image's channel order) the base colour of a covered pixel
 *           replaces rgb[mesh] for every mesh of the call.  v0, v1, v2 = the vertices of the pixel's visible triangle after
 *           its re-orientation to positive area, b_k their barycentrics from the integer edge values, iz_k their depth values:
 *             w_k = b_k * iz_k;  d = (w_0 + w_1) + w_2 (the depth value);
 *             base_c = ((w_0 * vcol[v0][c] + w_1 * vcol[v1][c]) + w_2 * vcol[v2][c]) / d;
 *             out_c = uint8(clamp(floor(((w * 255) * base_c) * shade + (1 - w) * img_c), 0, 255)).
 *           Shade, coverage, depth test, tie rule and ids are those of acrmi_rasterize; a NaN colour gives 0; no colour value
 *           moves a store, and vcol is read only at vertex indices of the (validated) topology blobs.
 *  colours  per vertex: flag != 0 -> the flag colour; else a NaN value -> base_rgb[mesh]; else t = (v - lo) / (hi - lo) clamped
 *           to [0,1] (infinities clamp), i = (int)(t * 255), with `reverse` 255 - i, colour_c = (float)lut[i][c] / 255.
 *  values   what acrmi_contact / acrmi_surface_contact wrote for B rows at K hands per side -> per hand (b, k, side) and vertex:
 *           the partners in ascending rank are, for left rank k, the pairs (b*K + k)*K + j in direction 0, for right rank k the
 *           pairs (b*K + i)*K + k in direction 1; m2 = the smallest d2 over them (strict < from +inf: NaN and +inf never win),
 *           value = sqrt(m2), NaN when m2 stayed +inf (no computed pair); flag = 1 when in any partner pair d2 <= m*m (m =
 *           max_depth) and s < 0, respectively cross odd - the INSIDE rules above.
 * No atomics, no host visit: deterministic; a row alone equals the row in a batch.
 * ------------------------------------------------------------------------------------- */
/* values_dev [M,V] fp32, flags_dev [M,V] int32 or NULL (no vertex flagged), base_rgb_dev [M,3], flag_rgb_host [3], lut_host
 * [256][3] bytes in the image's channel order or NULL = the default table of acrmi_overlay_tables (flipped when bgr != 0), the
 * way acrmi_draw_heatmaps takes its table; vcol_dev [M,V,3] out.  lo, hi finite, hi > lo; M * V * 3 at most 2^31 - 1; checked
 * with the pointers before any GPU call (ACRMI_EINVAL).  M == 0 is success and touches nothing. */
int acrmi_vertex_colors(const float* values_dev, const int32_t* flags_dev, const float* base_rgb_dev, int M, int V, float lo,
                        float hi, int reverse, const float* flag_rgb_host, const uint8_t* lut_host, int bgr, float* vcol_dev,
                        void* stream);
/* d2_dev [B*K*K,2,V] and exactly one of s_dev fp32 (acrmi_contact) and cross_dev int32 (acrmi_surface_contact), shaped alike;
 * K in 1..ACRMI_MAX_HAND; max_depth >= 0 (+inf allowed); outputs value_dev fp32 and flag_dev int32 [B,K,2,V].  B * K * K * 2 * V at
 * most 2^31 - 1.  Checked before any GPU call; B == 0 is success and touches nothing. */
int acrmi_contact_values(const float* d2_dev, const float* s_dev, const int32_t* cross_dev, int B, int K, int V, float max_depth,
                         float* value_dev, int32_t* flag_dev, void* stream);
/* acrmi_rasterize with vcol_dev [n_meshes,n_verts,3] (not NULL; rgb_dev is still required and not read for a colour);
 * view_per_mesh == 0: view_dev [n_frames,4] or NULL as acrmi_rasterize; != 0: view_dev [n_meshes,4] as acrmi_rasterize_views. */
int acrmi_rasterize_colored(const float* verts_dev, const float* trans_dev, int n_meshes, int n_verts, int n_faces,
                            const int32_t* topo_dev, const int32_t* topo2_dev, const int32_t* mesh_topo_dev,
                            const int32_t* mesh_frame_dev, const float* rgb_dev, const float* vcol_dev, const float* view_dev,
                            int view_per_mesh, float focal, float visible_weight, const uint8_t* img_in_dev, uint8_t* img_out_dev,
                            int n_frames, int H, int W, int32_t* ids_out_dev, void* ws_dev, void* stream);
/* acrmi_render with vcol_dev [B,2,778,3] (not NULL). */
int acrmi_render_colored(acrmi_ctx* ctx, const float* verts_dev, const float* cam_trans_dev, const float* slots_dev, int B,
                         const float* offsets_dev, const float* colors_host, const float* vcol_dev, float focal,
                         float visible_weight, const uint8_t* img_in_dev, uint8_t* img_out_dev, int H, int W, int32_t* ids_out_dev,
                         void* stream);
/* acrmi_render_regions with vcol_dev [n,2,778,3] (not NULL). */
int acrmi_render_regions_colored(acrmi_ctx* ctx, const float* verts_dev, const float* cam_trans_dev, const float* slots_dev, int n,
                                 const float* offsets_dev, const int32_t* region_frame_dev, const float* colors_host,
                                 const float* vcol_dev, float focal, float visible_weight, const uint8_t* img_in_dev,
                                 uint8_t* img_out_dev, int n_frames, int H, int W, int32_t* ids_out_dev, void* stream);

/* ---------------------------------------------------------------------------------------
 * The hand-part segmentation as an output (the rule once in csrc/segm_plan.h, on the map sampling
 * of csrc/map_view_plan.h that the heat-map views share; csrc/segm.hip).  The
 * network computes C = 33 part logits per cell of a 256 x 256 map (backbone.hand_segm, the reference's `segms`); the reference
 * turns them into labels with map2labels (acr/model.py:397-401) and draws nothing.  All fp32, every operation rounded on its
 * own:
 *  canvas  of pixel (x, y): cx = (x + 0.5 - ox) / sx with the frame's view row (sx, sy, ox, oy) - given, or taken from its
 *          `offsets` row as acrmi_render does - and cx = (x + 0.5) * (512 / W) without one.  A pixel with cx or cy outside
 *          [0, 512), and every pixel of a frame with sx or sy not > 0, is NOT COVERED.
 *  taps    s = max(cx * (w / 512) - 0.5, 0), i0 = min(int(s), w - 1), i1 = min(i0 + 1, w - 1), l1 = s - i0, l0 = 1 - l1, the
 *          same in y with h: acrmi_draw_heatmaps' rule with the map's own h, w
 *  value   v_c = ly0 (lx0 a_c + lx1 b_c) + ly1 (lx0 c_c + lx1 d_c) for every class c: bilinear logits, not nearest labels
 *  label   best = v_0, label = 0; for c = 1 .. C - 1 in order, c is taken when v_c > best (strict: the lowest class wins a
 *          tie, a NaN never wins).  A pixel that is not covered gets ACRMI_SEGM_NONE.  C is odd, 3 <= C <= 63; class 0 is
 *          background, classes 1 .. (C-1)/2 are the RIGHT hand's parts, the rest the LEFT hand's (acr/model.py:141-144).
 *          Which part is which bone is not known: the reference ships no list.
 *  view    for 1 <= label < C: out = floor(weight * colour[label] + (1 - weight) * img); every other pixel keeps the input
 *          byte for byte.  Default colours: right part p = label - 1 takes the heat maps' LUT[128 + 8 p], left part p =
 *          label - 1 - (C-1)/2 takes LUT[127 - 8 p] (index clamped into the table), flipped for BGR.
 *  stats   counts[c] = pixels of label c (ACRMI_SEGM_NONE is not counted); box of side s (0 left, 1 right) = the smallest
 *          (l, t, r, b) around its pixels, r and b exclusive as acrmi_roi's, zeros when it has none; agree of side s =
 *          (pixels in both, mask pixels, silhouette pixels) with the silhouette = pixels whose rasteriser id is >= 0 and
 *          ((id / n_faces) & 1) == s.  Integers only: IoU = inter / (mask + sil - inter) is the caller's division.
 * No atomics on global memory; a frame alone equals the frame in a batch; in place = out of place; nothing is zeroed by the
 * caller.  Arguments are checked before any device call (ACRMI_EINVAL); n == 0 is a success that touches nothing.
 * ------------------------------------------------------------------------------------- */
#define ACRMI_SEGM_NONE 255
/* Pure host: the default colours of C classes, colors_host [C][3] in RGB order or flipped (bgr != 0); row 0 is zero. */
int acrmi_segm_tables(int bgr, int C, uint8_t* colors_host);
/* logits_dev fp32: cell (y, x) of frame i starts at element i * frame_stride + (y * w + x) * pix_stride and holds C classes;
 * pix_stride >= C, frame_stride >= h * w * pix_stride (when pix_stride is a multiple of 4 whole cells of pix_stride floats
 * are read).  At most one of view_dev [n,4] and offsets_dev [n,10].  out_dev uint8 [n,H,W,3] or NULL: the view over
 * img_in_dev (needed with out_dev only; they may be the same buffer); labels_dev uint8 [n,H,W] or NULL; one of the two at
 * least.  weight in [0,1]; colors_host [C][3] in the image's channel order, NULL = the default (flipped when bgr != 0).
 * h, w, H, W <= 16384, n <= 65535.  ONE launch reads the logits once. */
int acrmi_segm_labels(const float* logits_dev, long long frame_stride, int pix_stride, int n, int h, int w, int C,
                      const float* view_dev, const float* offsets_dev, float weight, const uint8_t* colors_host, int bgr,
                      const uint8_t* img_in_dev, uint8_t* out_dev, uint8_t* labels_dev, int H, int W, void* stream);
/* int32 words of acrmi_segm_stats' workspace (0 for sizes it would refuse). */
size_t acrmi_segm_stats_ws_ints(int n, int H, int W);
/* labels_dev uint8 [n,H,W]; ids_dev int32 [n,H,W] (what acrmi_render / acrmi_rasterize wrote for the same frames, with its
 * n_faces > 0) or NULL; counts_dev int32 [n,C], boxes_dev int32 [n,2,4], agree_dev int32 [n,2,3] - with ids_dev, else NULL;
 * ws_dev: acrmi_segm_stats_ws_ints(n, H, W) int32, nothing in it needs to be set. */
int acrmi_segm_stats(const uint8_t* labels_dev, const int32_t* ids_dev, int n_faces, int n, int H, int W, int C,
                     int32_t* counts_dev, int32_t* boxes_dev, int32_t* agree_dev, int32_t* ws_dev, void* stream);
/* acrmi_segm_labels on the context's own segmentation buffer as the last program run left it, which must have been at batch
 * B (geometry and channel stride as acrmi_buffer_ptr reports them; the buffer is fp32 in every storage type); offsets_dev
 * [B,10] or NULL (the 512 x 512 network input, or any frame the canvas fills).  ACRMI_ESTATE before a program has run or
 * after one at another batch size, as acrmi_overlay(ACRMI_OVERLAY_CENTERMAP). */
int acrmi_segment(acrmi_ctx* ctx, int B, const float* offsets_dev, float weight, const uint8_t* colors_host, int bgr,
                  const uint8_t* img_in_dev, uint8_t* out_dev, uint8_t* labels_dev, int H, int W, void* stream);

/* Multi-GPU (replaces nn.DataParallel's scatter/gather, acr/main.py:61): frames are sharded by the caller, one
 * process per GPU; the only collective is ONE all-gather per batch of each rank's flat result buffer
 * [slots | verts | joints] over RCCL/xGMI.  recv_dev holds n_ranks * n_floats floats, rank-major.
 * acrmi_comm_unique_id: 128-byte ncclUniqueId, created on rank 0 and handed to every rank by the host's own means;
 * acrmi_comm_init: ncclCommInitRank on the context's device (collective: every rank calls it);
 * acrmi_allgather: ncclAllGather on `stream`; nccl_comm = NULL uses the context's communicator, otherwise a
 * caller-owned ncclComm_t.  RCCL is resolved at run time (dlopen); without it these calls return ACRMI_ESTATE.
 * ONE RCCL communicator per process: a process that also holds another one (e.g. torch.distributed's NCCL backend) pays ~11 ms
 * per batch for a side-stream all-gather next to a running batch (measured at world size 1: 46.8 vs 35.4 ms; +0.2 ms with this
 * library's communicator alone).  The library cannot see other libraries' communicators; the Python host refuses the
 * combination (Engine.comm_init / parallel.ShardedRunner(transport='c') next to a torch NCCL group raise unless overridden) -
 * another host either passes ITS communicator as nccl_comm, or runs its control plane over something else (bench.py: gloo). */
int acrmi_comm_unique_id(void* id128_out);
int acrmi_comm_init(acrmi_ctx* ctx, int n_ranks, int rank, const void* id128);
int acrmi_comm_destroy(acrmi_ctx* ctx);
int acrmi_allgather(acrmi_ctx* ctx, void* nccl_comm, const float* send_dev, float* recv_dev, size_t n_floats,
                    void* stream);

/* Runs only the point-heads ops on the resident buffers of the last acrmi_backbone_heads / acrmi_forward call:
 * params/cam/prior towers + mix (acr/model.py:71-99,160-164) at the centers of the CURRENT center maps, written
 * into the pixels of the params/prior maps acrmi_decode samples. */
int acrmi_point_heads(acrmi_ctx* ctx, int B, void* stream);
/* acrmi_point_heads for the max_hand (1..ACRMI_MAX_HAND) best centers of each side: the towers and the mix at the pixels
 * acrmi_decode_multi(ctx, B, max_hand, ...) reads (csrc/point_plan.h), nothing else is written.  max_hand = 1 writes the bits
 * acrmi_point_heads writes without ACRMI_OPT_BATCH_PRIOR (which this call does not look at).  ACRMI_EINVAL / ACRMI_ESTATE before any device call: NULL ctx, no program, B or max_hand out of
 * range, a program without point-heads ops. */
int acrmi_point_heads_multi(acrmi_ctx* ctx, int B, int max_hand, void* stream);

/* Profiling aid for bench.py: time every op of the program with hipEvents on `stream`
 * (one untimed warm-up pass first; ops outside the active head mode report 0).  ms_out[n_ops]; returns n_ops or <0.
 * At a small batch (<= 32 frames) the times are also kept in the context (per head mode) as the input of
 * ACRMI_OPT_LANE_PLAN; they change how later calls are scheduled only after that option has been switched on. */
int acrmi_profile_ops(acrmi_ctx* ctx, const uint8_t* img_dev, int B, float* ms_out, int n_ms, void* stream);
/* Diagnostic: the grouped launches (acrmi_conv2d_group's launch, formed by the executor between independent convolutions of one
 * kernel instantiation; csrc/group_plan.h) in the schedule a call at batch B replays; < 0 on error.  Programs of contexts with
 * max_batch >= 16 only, and none with ACRMI_GROUP=0 in the environment / after acrmi_tune(5, 0). */
int acrmi_program_groups(acrmi_ctx* ctx, int B);

/* A non-blocking HIP stream on `device` / its release - for hosts without a stream API of their own (the Python
 * package runs the contexts of an EnginePool on these instead of torch's pooled streams). */
int acrmi_stream_create(int device, void** stream);
int acrmi_stream_destroy(void* stream);

/* Tuning hook for kernel experiments (tools/conv_bench.py, tools/ab_cfg.py); process-wide, not part of the
 * reference-facing surface.  key 0: force a conv kernel variant (-1 = automatic selection; 8xx ids are listed next to
 * the launchers in csrc/conv_mfma.hip, conv_wino2.inc, conv_wino3.inc, conv_ws2.inc - e.g. 806 large-batch item shapes
 * at any batch, 837 the 16x32 wave tile of conv_wino3b_kernel, 839 no store waves); key 1: cycle stamps of
 * workgroup 0 on/off; key 2: print them; key 3: loader-wave switches (8 idle loader - wrong results, 9 priority 0);
 * key 4: XCD-banded item order on/off; key 5: grouped launches on/off in the programs set from now on (default on; the
 * environment variable ACRMI_GROUP=0, read when the library loads, starts with off). */
int acrmi_tune(int key, int value);

#ifdef __cplusplus
}
#endif
#endif /* ACRMI_H */
