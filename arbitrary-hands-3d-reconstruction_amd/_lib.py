"""ctypes binding of libacrmi.so (include/acrmi.h).  No CPU fallback: if the HIP library is
missing or fails to load, every entry point raises."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('ACRMI_LIB') or os.path.join(HERE, 'libacrmi.so')   # ACRMI_LIB: kernel experiments

OP_U8NORM, OP_CONV, OP_FUSESUM, OP_BILINEAR2X, OP_POW11, OP_ATTPOOL, OP_PAREBIAS, OP_COORDFILL, OP_POINTHEADS, OP_STEM = range(1, 11)
OP_MAXPOOL, OP_PAIR1X1 = 11, 12
MODE_BOTH, MODE_DENSE, MODE_POINT = 0, 1, 2
CONV_BIAS_MAP = 8      # acrmi_op.flags of a CONV / acrmi_conv2d's algo: ACRMI_CONV_BIAS_MAP
CONV_SPLITK = 16       # acrmi_op.flags of a CONV: ACRMI_CONV_SPLITK
CONV_DUAL = 32         # acrmi_op.flags of a CONV: ACRMI_CONV_DUAL (second output = the full-resolution HR fuse sum)
OPT_POINT_HEADS, OPT_LANES, OPT_CENTER_IDX, OPT_TEMPORAL, OPT_CONF_THRESH, OPT_SMOOTH_COEFF, OPT_MANO_FP16 = 1, 2, 3, 4, 5, 6, 7
OPT_LANE_PLAN = 8
OPT_BATCH_PRIOR = 9
OPT_POINT_HEADS_MULTI = 10
VERSION = 303
DT_F32, DT_F16, DT_BF16 = 0, 1, 2
SLOT = 176
MAX_HAND = 8      # ACRMI_MAX_HAND
ASSOC_STATE = 41  # ACRMI_ASSOC_STATE
SLOT_FLAG, SLOT_FLATIND, SLOT_SCORE, SLOT_CAM, SLOT_POSES, SLOT_BETAS, SLOT_PARAMS = 0, 1, 2, 3, 6, 54, 64
E_INVAL, E_HIP, E_STATE, E_NOMEM, E_RANGE = -1, -2, -3, -4, -5
# acrmi_mano_fit (csrc/mano_fit_plan.h): floats of a state row (acrmi_mano_fit_state_floats) and the steps of one launch
FIT_STATE, FIT_MAX_STEPS = 196, 1024
OVERLAY_SKELETON, OVERLAY_CENTERMAP = 0, 1      # acrmi_overlay `what`
SEGM_NONE = 255      # ACRMI_SEGM_NONE: the label of a pixel the canvas does not cover


class BufferDesc(C.Structure):
    _fields_ = [('h', C.c_int32), ('w', C.c_int32), ('cs', C.c_int32), ('persistent', C.c_int32), ('dtype', C.c_int32)]


class Op(C.Structure):
    _fields_ = [('kind', C.c_int32),
                ('in_buf', C.c_int32), ('out_buf', C.c_int32), ('res_buf', C.c_int32),
                ('in_coff', C.c_int32), ('out_coff', C.c_int32), ('res_coff', C.c_int32),
                ('cin', C.c_int32), ('cout', C.c_int32),
                ('ksize', C.c_int32), ('stride', C.c_int32), ('relu', C.c_int32), ('groups', C.c_int32),
                ('w_off', C.c_int64), ('b_off', C.c_int64),
                ('bias_per_frame', C.c_int32), ('aux_buf', C.c_int32), ('nterms', C.c_int32),
                ('term_buf', C.c_int32 * 4), ('term_coff', C.c_int32 * 4), ('term_shift', C.c_int32 * 4),
                ('w_off2', C.c_int64), ('b_off2', C.c_int64), ('w_off3', C.c_int64),
                ('flags', C.c_int32), ('mode', C.c_int32)]


class Frame(C.Structure):      # acrmi_frame
    _fields_ = [('bgr_dev', C.c_void_p), ('H', C.c_int32), ('W', C.c_int32)]


class NV12Frame(C.Structure):      # acrmi_nv12_frame
    _fields_ = [('y_dev', C.c_void_p), ('uv_dev', C.c_void_p), ('H', C.c_int32), ('W', C.c_int32),
                ('y_pitch', C.c_int32), ('uv_pitch', C.c_int32)]


class NV12Surface(C.Structure):      # acrmi_nv12_surface: the same layout, writable planes
    _fields_ = NV12Frame._fields_


class Roi(C.Structure):      # acrmi_roi
    _fields_ = [('frame', C.c_int32), ('l', C.c_int32), ('t', C.c_int32), ('r', C.c_int32), ('b', C.c_int32)]


# acrmi_nv12_matrix `which` (ACRMI_NV12_*) by the name the Python layer takes
NV12_MATRICES = {'cv601': 0, 'bt601': 1, 'bt601-full': 2, 'bt709': 3, 'bt709-full': 4}


class HeadLayout(C.Structure):
    _fields_ = [('center_buf', C.c_int32 * 2), ('params_buf', C.c_int32 * 2), ('prior_buf', C.c_int32 * 2),
                ('segm_buf', C.c_int32), ('backbone_buf', C.c_int32)]


class ConvProblem(C.Structure):      # acrmi_conv_problem
    _fields_ = [('in_', C.c_void_p), ('w_packed', C.c_void_p), ('bias', C.c_void_p), ('res', C.c_void_p), ('out', C.c_void_p)] + \
               [(k, C.c_int32) for k in ('B', 'H', 'W', 'in_cs', 'in_coff', 'cin', 'bias_frame_stride', 'res_cs', 'res_coff', 'out_cs',
                                         'out_coff', 'cout', 'ksize', 'stride', 'relu', 'groups', 'algo', 'reserved')]


EXPORTS = ['acrmi_version', 'acrmi_last_error', 'acrmi_create', 'acrmi_destroy', 'acrmi_load_weights',
           'acrmi_set_program', 'acrmi_load_mano', 'acrmi_backbone_heads', 'acrmi_buffer_ptr', 'acrmi_decode',
           'acrmi_decode_maps', 'acrmi_mano', 'acrmi_forward', 'acrmi_conv2d', 'acrmi_u8norm', 'acrmi_bilinear2x',
           'acrmi_fuse_sum', 'acrmi_attpool', 'acrmi_attpool_ws_floats', 'acrmi_stem_conv', 'acrmi_stream_create', 'acrmi_stream_destroy', 'acrmi_profile_ops', 'acrmi_tune', 'acrmi_preprocess', 'acrmi_cam_trans',
           'acrmi_set_option', 'acrmi_point_heads', 'acrmi_set_option_f', 'acrmi_smooth', 'acrmi_smooth_reset',
           'acrmi_comm_unique_id', 'acrmi_comm_init', 'acrmi_comm_destroy', 'acrmi_allgather', 'acrmi_parebias',
           'acrmi_buffer_dtype', 'acrmi_conv2d_h16', 'acrmi_conv2d_splitk', 'acrmi_conv2d_splitk_workspace',
           'acrmi_decode_gated', 'acrmi_decode_maps_gated', 'acrmi_share_weights', 'acrmi_mano_rotmat', 'acrmi_heads',
           'acrmi_backbone_channels', 'acrmi_check_range', 'acrmi_prior_gate', 'acrmi_preprocess_frames',
           'acrmi_mesh_topology', 'acrmi_render_workspace', 'acrmi_rasterize', 'acrmi_load_faces', 'acrmi_render',
           'acrmi_overlay_tables', 'acrmi_draw_skeletons', 'acrmi_draw_heatmaps', 'acrmi_overlay',
           'acrmi_streams_create', 'acrmi_streams_destroy', 'acrmi_streams_reset', 'acrmi_smooth_streams',
           'acrmi_forward_streams', 'acrmi_nv12_matrix', 'acrmi_preprocess_nv12', 'acrmi_nv12_to_rgb',
           'acrmi_roi_offsets', 'acrmi_preprocess_rois', 'acrmi_preprocess_rois_nv12', 'acrmi_track_box', 'acrmi_track_boxes',
           'acrmi_preprocess_rois_dev', 'acrmi_preprocess_rois_nv12_dev', 'acrmi_nv12_out_matrix', 'acrmi_rgb_to_nv12',
           'acrmi_nv12_compose', 'acrmi_rasterize_views', 'acrmi_draw_region_heatmaps', 'acrmi_render_regions',
           'acrmi_overlay_regions', 'acrmi_decode_multi', 'acrmi_decode_maps_multi', 'acrmi_forward_multi',
           'acrmi_tracks_create', 'acrmi_tracks_destroy', 'acrmi_tracks_reset', 'acrmi_associate', 'acrmi_forward_tracks',
           'acrmi_assoc_step', 'acrmi_point_heads_multi', 'acrmi_contact_workspace', 'acrmi_mesh_contact', 'acrmi_contact',
           'acrmi_conv2d_group', 'acrmi_program_groups', 'acrmi_surface_contact_workspace', 'acrmi_mesh_surface_contact',
           'acrmi_surface_contact', 'acrmi_score_board_bytes', 'acrmi_score_pair_bytes', 'acrmi_pose_errors',
           'acrmi_score_accumulate', 'acrmi_score_hands', 'acrmi_vertex_colors', 'acrmi_contact_values',
           'acrmi_rasterize_colored', 'acrmi_render_colored', 'acrmi_render_regions_colored', 'acrmi_segm_tables',
           'acrmi_segm_labels', 'acrmi_segm_stats_ws_ints', 'acrmi_segm_stats', 'acrmi_segment', 'acrmi_match_board_bytes',
           'acrmi_match_hands', 'acrmi_match_gather', 'acrmi_match_accumulate', 'acrmi_mano_backward',
           'acrmi_mano_fit', 'acrmi_mano_fit_state_floats']

_lib = None


class AcrmiError(RuntimeError):
    pass


class AcrmiRangeError(AcrmiError, OverflowError):
    """ACRMI_ERANGE: an 'fp16x3' program met an activation outside the f16 range (acrmi_check_range); the results since the
    last check are invalid (and were written as NaN)."""


def lib():
    """Loads libacrmi.so (built in-tree by build.py).  Raises if it is absent: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AcrmiError('libacrmi.so not built: run `python __graft_entry__.py build` (needs hipcc). '
                         'The ACR path has no CPU fallback.')
    L = C.CDLL(LIB_PATH)
    vp, i32, f32p, u8p = C.c_void_p, C.c_int, C.c_void_p, C.c_void_p
    L.acrmi_version.restype = C.c_int
    if L.acrmi_version() != VERSION:
        # the argument lists below are those of VERSION: a stale build (or an ACRMI_LIB override from another round)
        # would be called with shifted arguments
        raise AcrmiError('%s is ABI version %d, this package binds version %d: rebuild it (`python __graft_entry__.py build`)'
                         % (LIB_PATH, L.acrmi_version(), VERSION))
    L.acrmi_last_error.restype = C.c_char_p
    L.acrmi_last_error.argtypes = [vp]
    L.acrmi_create.argtypes = [C.POINTER(vp), i32]
    L.acrmi_destroy.argtypes = [vp]
    L.acrmi_destroy.restype = None
    L.acrmi_load_weights.argtypes = [vp, vp, C.c_size_t]
    L.acrmi_set_program.argtypes = [vp, C.POINTER(BufferDesc), i32, C.POINTER(Op), i32, C.POINTER(HeadLayout), i32]
    L.acrmi_load_mano.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.acrmi_backbone_heads.argtypes = [vp, u8p, i32, vp]
    L.acrmi_buffer_ptr.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.acrmi_buffer_ptr.restype = vp
    L.acrmi_decode.argtypes = [vp, i32, f32p, vp]
    L.acrmi_decode_maps.argtypes = [f32p, f32p, i32, f32p, f32p, i32, f32p, f32p, i32, i32, C.c_float, f32p, vp]
    L.acrmi_decode_gated.argtypes = [vp, i32, vp, f32p, vp]
    L.acrmi_share_weights.argtypes = [vp, vp]
    L.acrmi_decode_maps_gated.argtypes = [f32p, f32p, i32, f32p, f32p, i32, f32p, f32p, i32, i32, C.c_float, vp, f32p, vp]
    L.acrmi_mano.argtypes = [vp, f32p, i32, f32p, i32, vp, i32, i32, f32p, f32p, f32p, f32p, i32, f32p, f32p, f32p,
                             f32p, vp]
    L.acrmi_mano_rotmat.argtypes = [vp, f32p, f32p, i32, vp, i32, i32, f32p, f32p, f32p, vp]
    L.acrmi_mano_backward.argtypes = [vp, f32p, i32, f32p, i32, vp, i32, i32, f32p, f32p, f32p, f32p, f32p, vp]
    L.acrmi_mano_fit.argtypes = [vp, f32p, vp, i32, i32, f32p, f32p, f32p, f32p, f32p, f32p, f32p, C.c_double, C.c_double,
                                 C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double, i32, i32, f32p, f32p, f32p, f32p,
                                 f32p, f32p, vp]
    L.acrmi_mano_fit_state_floats.argtypes = []
    L.acrmi_heads.argtypes = [vp, f32p, i32, vp]
    L.acrmi_backbone_channels.argtypes = [vp]
    L.acrmi_check_range.argtypes = [vp, vp]
    L.acrmi_prior_gate.argtypes = [vp, f32p, i32, vp, vp]
    L.acrmi_preprocess_frames.argtypes = [C.POINTER(Frame), i32, vp, vp, vp]
    L.acrmi_nv12_matrix.argtypes = [i32, vp]
    L.acrmi_preprocess_nv12.argtypes = [C.POINTER(NV12Frame), i32, vp, vp, vp, vp]
    L.acrmi_nv12_to_rgb.argtypes = [C.POINTER(NV12Frame), i32, vp, i32, C.POINTER(vp), vp]
    L.acrmi_nv12_out_matrix.argtypes = [i32, vp]
    L.acrmi_rgb_to_nv12.argtypes = [C.POINTER(vp), C.POINTER(NV12Surface), i32, vp, i32, vp]
    L.acrmi_nv12_compose.argtypes = [C.POINTER(NV12Frame), C.POINTER(vp), C.POINTER(NV12Surface), i32, vp, vp, i32, vp]
    L.acrmi_roi_offsets.argtypes = [i32, i32, C.POINTER(Roi), vp, vp]
    L.acrmi_preprocess_rois.argtypes = [C.POINTER(Frame), i32, C.POINTER(Roi), i32, vp, vp, vp]
    L.acrmi_preprocess_rois_nv12.argtypes = [C.POINTER(NV12Frame), i32, C.POINTER(Roi), i32, vp, vp, vp, vp]
    L.acrmi_track_box.argtypes = [f32p, i32, i32, i32, C.c_double, i32, vp]
    L.acrmi_track_boxes.argtypes = [f32p, f32p, vp, i32, C.c_double, i32, vp, vp]
    L.acrmi_preprocess_rois_dev.argtypes = [C.POINTER(Frame), i32, vp, vp, i32, vp, vp, vp, vp]
    L.acrmi_preprocess_rois_nv12_dev.argtypes = [C.POINTER(NV12Frame), i32, vp, vp, i32, vp, vp, vp, vp, vp]
    L.acrmi_forward.argtypes = [vp, u8p, i32, f32p, f32p, f32p, f32p, f32p, f32p, f32p, vp]
    L.acrmi_conv2d.argtypes = [f32p, i32, i32, i32, i32, i32, i32, f32p, f32p, i32, f32p, i32, i32, f32p, i32, i32,
                               i32, i32, i32, i32, i32, i32, vp]
    L.acrmi_conv2d_h16.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, f32p, i32, vp, i32, i32, vp, i32, i32,
                                   i32, i32, i32, i32, i32, i32, i32, vp]
    L.acrmi_conv2d_splitk.argtypes = [f32p, i32, i32, i32, i32, i32, i32, i32, f32p, f32p, f32p, i32, i32, f32p, i32, i32,
                                      i32, i32, vp, C.c_size_t, vp]
    L.acrmi_conv2d_splitk_workspace.argtypes = [i32, i32, i32, i32, i32]
    L.acrmi_conv2d_splitk_workspace.restype = C.c_size_t
    L.acrmi_buffer_dtype.argtypes = [vp, i32]
    L.acrmi_u8norm.argtypes = [u8p, i32, f32p, vp]
    L.acrmi_bilinear2x.argtypes = [f32p, i32, i32, i32, i32, i32, f32p, i32, vp]
    L.acrmi_fuse_sum.argtypes = [i32, C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), i32, i32, i32, i32, f32p, i32,
                                 i32, vp]
    L.acrmi_attpool.argtypes = [f32p, i32, f32p, i32, i32, i32, f32p, f32p, vp]
    L.acrmi_attpool_ws_floats.argtypes = [i32, i32]
    L.acrmi_stream_create.argtypes = [i32, C.POINTER(C.c_void_p)]
    L.acrmi_stream_destroy.argtypes = [vp]
    L.acrmi_stem_conv.argtypes = [vp, i32, i32, i32, f32p, f32p, f32p, i32, i32, i32, vp]
    L.acrmi_attpool_ws_floats.restype = C.c_size_t
    L.acrmi_profile_ops.argtypes = [vp, u8p, i32, vp, i32, vp]
    L.acrmi_tune.argtypes = [i32, i32]
    L.acrmi_conv2d_group.argtypes = [C.POINTER(ConvProblem), i32, vp]
    L.acrmi_program_groups.argtypes = [vp, i32]
    L.acrmi_preprocess.argtypes = [u8p, i32, i32, i32, u8p, vp, vp]
    L.acrmi_cam_trans.argtypes = [f32p, f32p, i32, C.c_float, C.c_float, f32p, vp]
    L.acrmi_set_option.argtypes = [vp, i32, i32]
    L.acrmi_point_heads.argtypes = [vp, i32, vp]
    L.acrmi_point_heads_multi.argtypes = [vp, i32, i32, vp]
    L.acrmi_set_option_f.argtypes = [vp, i32, C.c_float]
    L.acrmi_smooth.argtypes = [vp, f32p, i32, vp]
    L.acrmi_smooth_reset.argtypes = [vp, vp]
    L.acrmi_streams_create.argtypes = [C.POINTER(vp), i32, i32]
    L.acrmi_streams_destroy.argtypes = [vp]
    L.acrmi_streams_destroy.restype = None
    L.acrmi_streams_reset.argtypes = [vp, vp, i32, vp]
    L.acrmi_smooth_streams.argtypes = [vp, vp, f32p, i32, vp, vp]
    L.acrmi_forward_streams.argtypes = [vp, vp, vp, u8p, i32, f32p, f32p, f32p, f32p, f32p, f32p, f32p, vp]
    L.acrmi_comm_unique_id.argtypes = [vp]
    L.acrmi_comm_init.argtypes = [vp, i32, i32, vp]
    L.acrmi_comm_destroy.argtypes = [vp]
    L.acrmi_allgather.argtypes = [vp, vp, f32p, f32p, C.c_size_t, vp]
    L.acrmi_parebias.argtypes = [f32p, i32, i32, f32p, f32p, f32p, f32p, f32p, i32, f32p, i32, vp]
    L.acrmi_mesh_topology.argtypes = [vp, i32, i32, vp, i32]
    L.acrmi_render_workspace.argtypes = [i32, i32]
    L.acrmi_render_workspace.restype = C.c_size_t
    L.acrmi_rasterize.argtypes = [f32p, f32p, i32, i32, i32, vp, vp, vp, vp, f32p, f32p, C.c_float, C.c_float, u8p, u8p, i32,
                                  i32, i32, vp, vp, vp]
    L.acrmi_load_faces.argtypes = [vp, i32, vp, i32]
    L.acrmi_render.argtypes = [vp, f32p, f32p, f32p, i32, f32p, vp, C.c_float, C.c_float, u8p, u8p, i32, i32, vp, vp]
    L.acrmi_overlay_tables.argtypes = [i32, u8p, u8p]
    L.acrmi_draw_skeletons.argtypes = [f32p, vp, i32, u8p, i32, i32, i32, u8p, u8p, i32, i32, i32, vp]
    L.acrmi_draw_heatmaps.argtypes = [f32p, f32p, C.c_longlong, i32, i32, i32, f32p, C.c_float, u8p, i32, u8p, u8p, u8p, i32,
                                      i32, vp]
    L.acrmi_overlay.argtypes = [vp, i32, f32p, f32p, i32, f32p, i32, u8p, u8p, u8p, i32, i32, vp]
    L.acrmi_rasterize_views.argtypes = list(L.acrmi_rasterize.argtypes)
    L.acrmi_draw_region_heatmaps.argtypes = [f32p, f32p, C.c_longlong, i32, i32, i32, f32p, vp, C.c_float, u8p, i32, u8p, u8p,
                                             u8p, i32, i32, i32, vp]
    L.acrmi_render_regions.argtypes = [vp, f32p, f32p, f32p, i32, f32p, vp, vp, C.c_float, C.c_float, u8p, u8p, i32, i32, i32,
                                       vp, vp]
    L.acrmi_overlay_regions.argtypes = [vp, i32, f32p, f32p, i32, f32p, vp, i32, u8p, u8p, u8p, i32, i32, i32, vp]
    L.acrmi_decode_multi.argtypes = [vp, i32, i32, f32p, vp]
    L.acrmi_decode_maps_multi.argtypes = [f32p, f32p, i32, f32p, f32p, i32, f32p, f32p, i32, i32, i32, C.c_float, f32p, vp]
    L.acrmi_forward_multi.argtypes = [vp, u8p, i32, i32, f32p, f32p, f32p, f32p, f32p, f32p, f32p, vp]
    L.acrmi_tracks_create.argtypes = [C.POINTER(vp), i32, i32, i32, i32, i32]
    L.acrmi_tracks_destroy.argtypes = [vp]
    L.acrmi_tracks_destroy.restype = None
    L.acrmi_tracks_reset.argtypes = [vp, vp, i32, vp]
    L.acrmi_associate.argtypes = [vp, vp, f32p, i32, i32, vp, i32, vp, vp, vp]
    L.acrmi_forward_tracks.argtypes = [vp, vp, vp, i32, u8p, i32, i32, f32p, f32p, f32p, f32p, f32p, f32p, f32p, vp, vp]
    L.acrmi_assoc_step.argtypes = [i32, i32, i32, vp, i32, vp, vp, vp, vp]
    L.acrmi_contact_workspace.argtypes = [i32, i32]
    L.acrmi_contact_workspace.restype = C.c_size_t
    L.acrmi_mesh_contact.argtypes = [f32p, f32p, i32, i32, i32, vp, vp, vp, vp, vp, i32, C.c_float, C.c_float, vp, f32p, f32p,
                                     f32p, vp, vp, vp]
    L.acrmi_contact.argtypes = [vp, f32p, f32p, f32p, i32, i32, vp, C.c_float, C.c_float, vp, f32p, f32p, f32p, vp, vp]
    L.acrmi_surface_contact_workspace.argtypes = [i32, i32, i32]
    L.acrmi_surface_contact_workspace.restype = C.c_size_t
    L.acrmi_mesh_surface_contact.argtypes = [f32p, f32p, i32, i32, i32, vp, vp, vp, vp, i32, C.c_float, C.c_float, vp, f32p, f32p,
                                             vp, f32p, vp, vp, vp]
    L.acrmi_surface_contact.argtypes = [vp, f32p, f32p, f32p, i32, i32, C.c_float, C.c_float, vp, f32p, f32p, vp, f32p, vp, vp]
    L.acrmi_score_board_bytes.argtypes = [i32, i32, i32]
    L.acrmi_score_board_bytes.restype = C.c_size_t
    L.acrmi_score_pair_bytes.argtypes = [i32]
    L.acrmi_score_pair_bytes.restype = C.c_size_t
    L.acrmi_pose_errors.argtypes = [f32p, f32p, u8p, i32, i32, i32, f32p, f32p, f32p, vp, i32, f32p, f32p, f32p, f32p, vp, f32p, f32p, vp]
    L.acrmi_score_accumulate.argtypes = [f32p, f32p, i32, i32, vp, i32, f32p, f32p, i32, C.c_double, vp, vp, vp]
    L.acrmi_score_hands.argtypes = [vp, f32p, f32p, f32p, f32p, f32p, f32p, u8p, vp, i32, i32, i32, i32, C.c_double, vp,
                                    f32p, f32p, f32p, vp, f32p, f32p, f32p, vp, f32p, vp]
    L.acrmi_vertex_colors.argtypes = [f32p, vp, f32p, i32, i32, C.c_float, C.c_float, i32, f32p, u8p, i32, f32p, vp]
    L.acrmi_contact_values.argtypes = [f32p, f32p, vp, i32, i32, i32, C.c_float, f32p, vp, vp]
    L.acrmi_rasterize_colored.argtypes = [f32p, f32p, i32, i32, i32, vp, vp, vp, vp, f32p, f32p, f32p, i32, C.c_float, C.c_float,
                                          u8p, u8p, i32, i32, i32, vp, vp, vp]
    L.acrmi_render_colored.argtypes = [vp, f32p, f32p, f32p, i32, f32p, vp, f32p, C.c_float, C.c_float, u8p, u8p, i32, i32, vp, vp]
    L.acrmi_render_regions_colored.argtypes = [vp, f32p, f32p, f32p, i32, f32p, vp, vp, f32p, C.c_float, C.c_float, u8p, u8p, i32,
                                               i32, i32, vp, vp]
    L.acrmi_segm_tables.argtypes = [i32, i32, u8p]
    L.acrmi_segm_labels.argtypes = [f32p, C.c_longlong, i32, i32, i32, i32, i32, f32p, f32p, C.c_float, u8p, i32, u8p, u8p, u8p,
                                    i32, i32, vp]
    L.acrmi_segm_stats_ws_ints.argtypes = [i32, i32, i32]
    L.acrmi_segm_stats_ws_ints.restype = C.c_size_t
    L.acrmi_segm_stats.argtypes = [u8p, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.acrmi_segment.argtypes = [vp, i32, f32p, C.c_float, u8p, i32, u8p, u8p, u8p, i32, i32, vp]
    L.acrmi_match_board_bytes.argtypes = []
    L.acrmi_match_board_bytes.restype = C.c_size_t
    L.acrmi_match_hands.argtypes = [f32p, f32p, u8p, u8p, f32p, i32, f32p, vp, i32, i32, i32, i32, i32, C.c_float, i32, vp, vp, f32p,
                                    vp, vp, vp]
    L.acrmi_match_gather.argtypes = [f32p, vp, i32, i32, i32, i32, f32p, vp]
    L.acrmi_match_accumulate.argtypes = [vp, f32p, i32, i32, vp, vp]
    for name in EXPORTS:
        fn = getattr(L, name)
        if name not in ('acrmi_last_error', 'acrmi_destroy', 'acrmi_buffer_ptr', 'acrmi_attpool_ws_floats',
                        'acrmi_render_workspace', 'acrmi_streams_destroy', 'acrmi_tracks_destroy', 'acrmi_contact_workspace',
                        'acrmi_surface_contact_workspace', 'acrmi_score_board_bytes', 'acrmi_score_pair_bytes',
                        'acrmi_segm_stats_ws_ints', 'acrmi_match_board_bytes'):
            fn.restype = C.c_int
    _lib = L
    return L


def check(rc, ctx=None):
    """Maps the C error codes onto the exceptions the reference raises (ValueError for bad
    configuration/arguments, RuntimeError otherwise)."""
    if rc >= 0:
        return rc
    msg = lib().acrmi_last_error(ctx)
    msg = msg.decode() if msg else 'acrmi error %d' % rc
    if rc == E_INVAL:
        raise ValueError(msg)
    if rc == E_RANGE:
        raise AcrmiRangeError(msg)
    raise AcrmiError(msg)
