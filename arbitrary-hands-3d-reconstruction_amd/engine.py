"""Engine: one libacrmi context on one GPU.  torch tensors are used only as HBM containers
(allocation, stream handle, host<->device copies); all arithmetic runs in libacrmi.so."""
import ctypes as C

import numpy as np
import torch

from . import _lib, match as match_mod, ops as ops_mod, packer, score as score_mod
from .ops import HAND_COLORS_RGB


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def torch_nccl_group_active():
    """True when torch.distributed is initialised with the NCCL (= RCCL on ROCm) backend in this process."""
    try:
        import torch.distributed as dist
        return bool(dist.is_available() and dist.is_initialized() and str(dist.get_backend()).lower() == 'nccl')
    except Exception:      # noqa: BLE001 - no torch.distributed in this build
        return False


def stream_ids(ids, B):
    """The stream id of each of B frames (any int sequence or int tensor of length B; -1 = leave the frame alone) as the
    contiguous host int32 array the library reads.  A host sequence or CPU tensor is converted without touching the
    device; a device tensor is copied to the host (that copy waits for the work that produces it)."""
    if isinstance(ids, torch.Tensor):
        if ids.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
            raise ValueError('streams must hold integers, got %s' % ids.dtype)
        a = ids.detach().cpu().numpy()
    else:
        a = np.asarray(ids)
        if a.dtype.kind not in 'iu':
            raise ValueError('streams must hold integers, got %s' % a.dtype)
    if a.ndim != 1 or a.shape[0] != B:
        raise ValueError('streams must name one stream per frame: shape %s for %d frames' % (tuple(a.shape), B))
    if a.size and (int(a.min()) < -2 ** 31 or int(a.max()) >= 2 ** 31):
        raise ValueError('streams: an id does not fit 32 bits')
    return np.ascontiguousarray(a, dtype=np.int32)


def check_max_hand(max_hand):
    """max_hand of decode / forward: an int in 1.._lib.MAX_HAND, else ValueError."""
    k = int(max_hand)
    if k != max_hand or not 1 <= k <= _lib.MAX_HAND:
        raise ValueError('max_hand %r: an integer in 1..%d' % (max_hand, _lib.MAX_HAND))
    return k


def stream_args(streams, table, B):
    """`streams=` / `table=` of Engine.smooth and Engine.forward: both or neither.  -> host int32 ids [B], or None."""
    if streams is None and table is None:
        return None
    if streams is None or table is None:
        raise ValueError('streams= and table= go together: the ids of the frames and the StreamTable that holds their state')
    if getattr(table, 'handle', None) is None:
        raise ValueError('table must be an open StreamTable')
    return stream_ids(streams, B)


class _Table(object):
    """What StreamTable and TrackTable share: a table of the library on one GPU that belongs to no Engine.  A subclass names
    the library's three calls (`_calls`: create, reset, destroy) and what it is called (`_name`)."""
    _calls = _name = None

    def _open(self, device, capacity, *params):
        self.L = _lib.lib()
        self.device = torch.device('cuda', device if isinstance(device, int) else torch.device(device).index or 0)
        self.capacity = int(capacity)
        self.handle = None
        h = C.c_void_p()
        _lib.check(getattr(self.L, self._calls[0])(C.byref(h), self.device.index, self.capacity, *params))
        self.handle = h

    def reset(self, ids=None):
        """The listed streams - every stream when ids is None - start afresh.  A StreamTable: they start a new sequence, their
        next sample passes through.  A TrackTable: they lose their tracks, every slot free, ids from 0 again.  Queued on the
        current stream, ordered with the smoothing / association calls of every context."""
        if self.handle is None:
            raise ValueError('the %s is closed' % self._name)
        arr, n = None, 0
        if ids is not None:
            a = np.atleast_1d(np.asarray(ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else ids))
            if a.size == 0:
                return
            a = stream_ids(a, a.shape[0])
            arr, n = a.ctypes.data_as(C.c_void_p), a.shape[0]
        _lib.check(getattr(self.L, self._calls[1])(self.handle, arr, n, _stream(self.device)))

    def close(self):
        h, self.handle = self.handle, None
        if h:
            getattr(self.L, self._calls[2])(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StreamTable(_Table):
    """One-Euro filter state of `capacity` video streams on one GPU (acrmi_streams; acr/main.py:50-53 keeps one filter set
    per video): what `Engine.smooth(..., streams=, table=)` / `Engine.forward(..., streams=, table=)` update.  It belongs to
    no Engine: the contexts of an EnginePool share one (the library orders their updates by the order of the calls), and
    it outlives an Engine that a checkpoint reload replaces.  Every stream starts fresh."""
    _calls, _name = ('acrmi_streams_create', 'acrmi_streams_reset', 'acrmi_streams_destroy'), 'StreamTable'

    def __init__(self, device=0, capacity=64):
        self._open(device, capacity)


class TrackTable(_Table):
    """The tracks of `capacity` video streams with max_hand slots per side on one GPU (acrmi_tracks):
    what `Engine.associate(..., tracks=, table=)` / `Engine.forward(..., max_hand=K, tracks=, track_table=)` update.  gate: the
    largest centre distance in map pixels at which a hand continues a track (0..128, 128 = any); max_miss: how many frames a
    track may go unseen and still be continued (-1 = for ever).  8 and 5 are defaults of parameters, not measurements.  Like a
    StreamTable it belongs to no Engine, and the library orders the updates of several contexts by the order of the calls."""
    _calls, _name = ('acrmi_tracks_create', 'acrmi_tracks_reset', 'acrmi_tracks_destroy'), 'TrackTable'

    def __init__(self, device=0, capacity=64, max_hand=2, gate=8, max_miss=5):
        self.max_hand, self.gate, self.max_miss = check_max_hand(max_hand), int(gate), int(max_miss)
        self._open(device, capacity, self.max_hand, self.gate, self.max_miss)


def track_args(tracks, track_table, streams, table, K, B):
    """`tracks=` / `track_table=` of Engine.forward: both or neither, and not next to streams= / table=.  -> host int32 ids [B]
    or None."""
    if tracks is None and track_table is None:
        return None
    if tracks is None or track_table is None:
        raise ValueError('tracks= and track_table= go together: the stream of each frame and the TrackTable that holds the tracks')
    if streams is not None or table is not None:
        raise ValueError('tracks= smooths every track with its own filter: not together with streams= / table=')
    ops_mod.check_track_table(track_table, K)
    return ops_mod.track_stream_ids(tracks, track_table, B)


def score_truth(gt, lead, device):
    """The ground truth of Engine.score as the library reads it: {'joints' fp32 lead + [21,3], 'verts' fp32 lead + [778,3] or
    None, 'joint_valid' uint8 lead + [21] or None, 'group' int32 lead or None}, contiguous on `device`.  Tensors that already
    are what is asked for are passed through untouched (no kernel is queued for them)."""
    if not isinstance(gt, dict) or gt.get('joints') is None:
        raise ValueError("gt must be a dict with 'joints'")
    res = {}
    for key, dtype, tail in (('joints', torch.float32, (21, 3)), ('verts', torch.float32, (778, 3)),
                             ('joint_valid', torch.uint8, (21,)), ('group', torch.int32, ())):
        t = gt.get(key)
        if t is not None:
            t = torch.as_tensor(t)
            if tuple(t.shape) != tuple(lead) + tail:
                raise ValueError("gt['%s'] must be %s, got %s" % (key, list(tuple(lead) + tail), list(t.shape)))
            t = ops_mod._score_arg(t, device, dtype, t.shape, key, as_bool=key == 'joint_valid')
        res[key] = t
    return res


class ScoreBoard(object):
    """A device-resident running score: per point set and group the per-point error sums and counts, a
    histogram of the root-aligned errors, the rows scored and missed, and per pair of groups the MRRPE sums.  The caller owns
    it; Engine.score / EnginePool.score / ACR.forward_batch(board=) add batches to it without visiting the host, and
    `summary()` is the one host visit.  sets / names: the point sets, by default the 21 joints and the 778 vertices of a hand;
    n_groups: by default 2, the side; n_bins bins of bin_width metres (defaults 100 x 0.5 mm: parameters, not measurements) for
    the PCK curve.  Boards of several devices or ranks are summed by the caller (`words`)."""

    def __init__(self, device=0, sets=(21, 778), names=('joints', 'verts'), n_groups=2, n_bins=score_mod.N_BINS,
                 bin_width=score_mod.BIN_WIDTH):
        self.sets, self.n_groups, self.n_bins, self.bin_width = score_mod.check_board_params(sets, n_groups, n_bins, bin_width)
        if len(names) != len(self.sets):
            raise ValueError('one name per point set')
        self.names = tuple(names)
        self.device = torch.device('cuda', device) if isinstance(device, int) else torch.device(device)
        self._offsets, self._pair_at, total = score_mod.board_layout(self.sets, self.n_groups, self.n_bins)
        L = _lib.lib()
        assert total * 8 == sum(L.acrmi_score_board_bytes(n, self.n_groups, self.n_bins) for n in self.sets) + \
            L.acrmi_score_pair_bytes(self.n_groups)
        self.words = torch.zeros(total, dtype=torch.int64, device=self.device)
        self._event = None      # recorded behind the last call that touched the board, on whichever stream it ran

    def set_words(self, k):
        """The board of point set k (a view)."""
        return self.words[self._offsets[k]:self._offsets[k] + score_mod.group_words(self.sets[k], self.n_bins) * self.n_groups]

    def pair_words(self):
        return self.words[self._pair_at:]

    def order_on(self, stream):
        """Makes `stream` (a torch stream) wait for the last call that touched the board: calls from several streams update
        it in the order they were made."""
        if self._event is not None:
            stream.wait_event(self._event)

    def touched_on(self, stream):
        self._event = torch.cuda.Event()
        self._event.record(stream)

    def add(self, k, res, group=None, flags=None):
        """Adds an ops.pose_errors result over point set k (with its pair_err, if it has one) on the current stream."""
        st = torch.cuda.current_stream(self.device)
        self.order_on(st)
        ops_mod.score_accumulate(self.set_words(k), self.pair_words() if res.get('pair_err') is not None else None, res,
                                 self.n_groups, self.n_bins, self.bin_width, group=group, flags=flags)
        self.touched_on(st)

    def reset(self):
        st = torch.cuda.current_stream(self.device)
        self.order_on(st)
        self.words.zero_()
        self.touched_on(st)

    def arrays(self):
        """The board on the host (score.board_arrays): the host waits for the calls queued so far."""
        self.order_on(torch.cuda.current_stream(self.device))
        return score_mod.board_arrays(self.words.cpu().numpy(), self.sets, self.n_groups, self.n_bins)

    def summary(self):
        """The one host visit: MPJPE, PA-MPJPE, MPVPE, PA-MPVPE and MRRPE in metres, per-joint tables, the PCK curve and its
        AUC, rows scored and missed - per group and over all (score.summarize says what is where)."""
        sets, pairs = self.arrays()
        return score_mod.summarize(sets, pairs, self.names, self.bin_width)


MATCH_GATHERED = ('slots', 'joints', 'verts', 'cam_trans', 'pj2d', 'pj2d_org')      # what Engine.match brings into truth order


def match_truth(gt, on, B, device):
    """The ground truth of Engine.match as the library reads it -> (G, {'points' fp32 [B,G,2,21,D], 'joint_valid' uint8
    [B,G,2,21] or None, 'valid' uint8 [B,G,2] or None, 'group' int32 [B,G,2] or None}), contiguous on `device`.  The points are
    gt['kp2d'] for on = 'pj2d_org' / 'pj2d' and gt['joints'] for on = 'joints'."""
    if on not in match_mod.ON_KEYS:
        raise ValueError('on must be one of %s, not %r' % (', '.join(match_mod.ON_KEYS), on))
    key, D = ('joints', 3) if on == 'joints' else ('kp2d', 2)
    if not isinstance(gt, dict) or gt.get(key) is None:
        raise ValueError("on=%r compares with gt['%s']: gt must be a dict that holds it" % (on, key))
    pts = torch.as_tensor(gt[key])
    if pts.dim() != 5 or pts.shape[0] != B or tuple(pts.shape[2:]) != (2, 21, D) or not 1 <= pts.shape[1] <= match_mod.MAX_HANDS:
        raise ValueError("gt['%s'] must be [%d,G,2,21,%d] with G in 1..%d, got %s" % (key, B, D, match_mod.MAX_HANDS, list(pts.shape)))
    G = pts.shape[1]
    lead = (B, G, 2)
    res = {'points': ops_mod._score_arg(pts, device, torch.float32, pts.shape, key)}
    for name, dtype, tail in (('joint_valid', torch.uint8, (21,)), ('valid', torch.uint8, ()), ('group', torch.int32, ())):
        t = gt.get(name)
        res[name] = None if t is None else ops_mod._score_arg(t, device, dtype, lead + tail, "gt['%s']" % name, as_bool=name != 'group')
    return G, res


class MatchBoard(object):
    """A device-resident running detection count: per side the matched pairs (TP), the flagged
    predictions left unmatched (FP), the valid truths left unmatched (FN) and the sum of the matched costs.  The caller owns it;
    Engine.match / EnginePool.match / ACR.forward_batch(match_board=) add batches to it without visiting the host, and
    `summary()` is the one host visit.  Boards of several devices or ranks are summed by the caller (`words`)."""

    def __init__(self, device=0):
        self.device = torch.device('cuda', device) if isinstance(device, int) else torch.device(device)
        assert _lib.lib().acrmi_match_board_bytes() == match_mod.BOARD_WORDS * 8
        self.words = torch.zeros(match_mod.BOARD_WORDS, dtype=torch.int64, device=self.device)
        self._event = None      # recorded behind the last call that touched the board, on whichever stream it ran

    order_on = ScoreBoard.order_on
    touched_on = ScoreBoard.touched_on
    reset = ScoreBoard.reset

    def add(self, res, stream=None):
        """Adds an ops.match_hands result ('counts' and 'cost') on the current stream (or on the raw stream given)."""
        st = torch.cuda.current_stream(self.device) if stream is None else torch.cuda.ExternalStream(stream, device=self.device)
        self.order_on(st)
        ops_mod.match_accumulate(self.words, res['counts'], res['cost'], stream=stream)
        self.touched_on(st)

    def arrays(self):
        """The board on the host (match.board_arrays): the host waits for the calls queued so far."""
        self.order_on(torch.cuda.current_stream(self.device))
        return match_mod.board_arrays(self.words.cpu().numpy())

    def summary(self):
        """The one host visit: TP, FP, FN, precision, recall, F1 and the mean match cost, per side and over all
        (match.summarize says what is where)."""
        return match_mod.summarize(self.arrays())


class ManoFunction(torch.autograd.Function):
    """Engine.mano (axis-angle mode, no projection) with Engine.mano_backward as its backward: apply(engine, poses [H,48],
    betas [H,10], side, center_idx) -> (verts, joints, center).  Once differentiable: a double backward raises torch's error."""

    @staticmethod
    def forward(ctx, engine, poses, betas, side, center_idx):
        verts, joints, center, _ = engine.mano(poses.detach(), betas.detach(), side, center_idx=center_idx)
        ctx.engine, ctx.center_idx = engine, center_idx
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(poses, betas, side)
        if center_idx is None:
            ctx.mark_non_differentiable(center)
        return verts, joints, center

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_verts, g_joints, g_center):
        poses, betas, side = ctx.saved_tensors
        g_poses, g_betas = ctx.engine.mano_backward(poses, betas, side, ctx.center_idx, g_verts, g_joints, g_center)
        return (None, g_poses.to(poses.dtype) if ctx.needs_input_grad[1] else None,
                g_betas.to(betas.dtype) if ctx.needs_input_grad[2] else None, None, None)


class Engine(object):
    def __init__(self, device=0):
        if not torch.cuda.is_available():
            raise _lib.AcrmiError('no GPU visible: the ACR path runs only on the HIP kernels (no CPU fallback)')
        self.L = _lib.lib()
        self.device = torch.device('cuda', device if isinstance(device, int) else torch.device(device).index or 0)
        self.ctx = C.c_void_p()
        _lib.check(self.L.acrmi_create(C.byref(self.ctx), self.device.index))
        self.max_batch = 0
        self.program = None
        self.have_mano = False
        self.point_heads = False
        self.point_heads_multi = False
        self.lanes = 0
        self.lane_plan = False
        self.conf_thresh = 0.35
        self.center_idx = 9
        self.temporal = False
        self.mano_fp16 = False
        self.batch_semantics = 'frame'
        self.smooth_coeff = None          # None = the library default (4.0)
        self.comm_ranks = 0
        self._mano_tables = {}
        self.have_faces = False
        self._faces = {}
        self._contact_sign = [1, 1]            # derived at load_faces / load_mano time (the context derives the same)
        self._contact_sign_set = None          # set_contact_sign's override

    def close(self):
        # (the handle is dropped first and without touching module globals: during interpreter shutdown `C` may already
        # be None, and an exception between the destroy and the reset would let a second __del__ destroy it again)
        ctx, self.ctx = self.ctx, None
        if ctx:
            self.L.acrmi_destroy(ctx)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- setup ---------------------------------------------------------------------------------
    def load_state_dict(self, sd, max_batch=1, keep_taps=False, precision='fp32', keep_weights=False, keep_all=False,
                        wino24='auto', splitk='auto'):
        """acr/utils.py:1153-1168 (load_model): reference-format checkpoint -> resident packed weights.
        keep_taps: see packer.lower (backbone taps stay readable through `buffer(program['taps'][name], B)`).
        precision: 'fp32' | 'fp16' | 'bf16' (args().model_precision, acr/config.py:96; packer.lower) | 'fp16x3' / 'bf16x3' (fp32
        storage, operands split into two f16 / bf16 numbers on the 16-bit matrix pipe for the 3x3 (stride 1, stride 2 outside the HR
        fuse hosts) and 1x1 stride-1 layers: csrc/conv_x3.inc, conv_x3p.inc, conv_x3s2.inc).  'fp16x3' has the f16 RANGE: every activation must stay within |x| <= 65504 - a checkpoint that
        exceeds it makes the affected calls return NaN slots / meshes and `check_range()` raise AcrmiRangeError (the
        host-facing API calls it); 'bf16x3' has fp32's range at 16-bit operand precision (8e-6 m instead of 1e-6 m on the
        bench frames)
        wino24: 'auto' (F(2x4,3x3) for contexts of max_batch >= 16), True / False to force (packer.lower).
        splitk: 'auto' (split-K lowering of the low-resolution 3x3 layers for contexts of max_batch < 16), True / False."""
        # F(2x4,3x3) is a large-batch choice: its items (8x32 pixels x one n-tile) are half as many as conv_wino2's
        # small-batch items, which costs latency when a launch cannot fill the CUs anyway (batch 1: 3.7 vs 3.5 ms)
        small = max_batch < 16        # single-frame / small-batch context: latency lowering (packer.lower)
        if wino24 == 'auto':
            wino24 = None if not small else False
        self.load_program(packer.lower(sd, keep_taps=keep_taps, precision=precision, keep_weights=keep_weights,
                                       keep_all=keep_all, wino24=wino24, splitk=small if splitk == 'auto' else splitk),
                          max_batch)

    def load_program(self, prog, max_batch=1, share_with=None):
        """A program lowered elsewhere (packer.lower, or another Engine's `program`): the same packed weights and op
        list in this context - an EnginePool lowers the checkpoint once.
        share_with: an Engine of the same device that already holds THIS program: its device copy of the weight blob is
        used instead of a second upload (acrmi_share_weights; 330 MB per context at HRNet-W32 fp32)."""
        if share_with is not None and share_with is not self and share_with.program is prog and \
                share_with.device == self.device:
            _lib.check(self.L.acrmi_share_weights(self.ctx, share_with.ctx), self.ctx)
        else:
            blob = prog['blob']
            _lib.check(self.L.acrmi_load_weights(self.ctx, blob.ctypes.data_as(C.c_void_p), blob.size), self.ctx)
        self.program = prog
        self._set_program(max_batch)

    def _set_program(self, max_batch):
        prog = self.program
        bufs = (_lib.BufferDesc * len(prog['bufs']))(*[_lib.BufferDesc(*b) for b in prog['bufs']])
        ops = (_lib.Op * len(prog['ops']))(*prog['ops'])
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()
            _lib.check(self.L.acrmi_set_program(self.ctx, bufs, len(bufs), ops, len(ops), C.byref(prog['heads']),
                                                max_batch), self.ctx)
        self.max_batch = max_batch

    @property
    def has_point_heads(self):
        """True when the loaded program carries the point-heads variant (packer.lower emits it for fp32 HRNet-W32
        programs only: 16-bit programs, HRNet-W48 and the ResNet-50 backbone run the dense heads)."""
        prog = getattr(self, 'program', None)
        return bool(prog) and any(o.kind == _lib.OP_POINTHEADS for o in prog['ops'])

    def set_point_heads(self, on):
        """ACRMI_OPT_POINT_HEADS: `forward` evaluates the params/cam/prior head towers and the mix conv only at the
        pixels ResultParser samples (acr/result_parser.py:49-57,141-145).  Same slots / vertices up to fp32
        round-off; `head_maps` params/prior maps are then only valid after `backbone_heads` (always dense).
        Returns what is in effect: a program without the point-heads ops stays on its dense heads (same results)."""
        on = bool(on) and self.has_point_heads
        _lib.check(self.L.acrmi_set_option(self.ctx, _lib.OPT_POINT_HEADS, int(on)), self.ctx)
        self.point_heads = on
        return on

    def set_point_heads_multi(self, on):
        """ACRMI_OPT_POINT_HEADS_MULTI: `forward(max_hand=K)`, with or without `tracks=`, evaluates the params/cam/prior head
        towers and the mix conv only at the pixels the top-K decode reads - the distinct K best centres of each side and the
        distinct partners (csrc/point_plan.h), at most 3 K tower points per side and frame - instead of running the dense heads.
        Same flags, centres and scores, the rest up to fp32 round-off; `forward` without max_hand does not look at it, and
        set_point_heads is not looked at with max_hand.
        Measured on one MI355X (every rank with a detection): at batch 64 `forward` is 1.9 / 1.7 / 1.0 ms
        of 33 faster than with the dense heads at K = 2 / 4 / 8 - no crossover up to K = 8; at batch 1 it is 0.14 - 0.22 ms of
        2.7 slower at every K, as set_point_heads is there: an option for large batches.
        Returns what is in effect: a program without the point-heads ops stays on its dense heads (same results)."""
        on = bool(on) and self.has_point_heads
        _lib.check(self.L.acrmi_set_option(self.ctx, _lib.OPT_POINT_HEADS_MULTI, int(on)), self.ctx)
        self.point_heads_multi = on
        return on

    def set_lanes(self, n):
        """ACRMI_OPT_LANES: independent chains of the program on n parallel HIP streams (1 = single stream,
        0 = by batch size: the library default)."""
        _lib.check(self.L.acrmi_set_option(self.ctx, _lib.OPT_LANES, int(n)), self.ctx)
        self.lanes = int(n)

    def set_lane_plan(self, on):
        """ACRMI_OPT_LANE_PLAN: small-batch schedules assign lanes from the op times the last `profile_ops` measured
        (list scheduling) instead of from the structure of the graph alone."""
        _lib.check(self.L.acrmi_set_option(self.ctx, _lib.OPT_LANE_PLAN, int(bool(on))), self.ctx)
        self.lane_plan = bool(on)

    def tune_lanes(self, batch=1, candidates=(1, 2, 4, 6), calls=5):
        """Picks ACRMI_OPT_LANES / ACRMI_OPT_LANE_PLAN by measurement IN THIS PROCESS: the ops are profiled once (the
        library keeps the times and plans the lanes from them), then every candidate lane count is timed with the
        structural and with the planned assignment - `calls` network passes (acrmi_backbone_heads on zero frames,
        after 2 warm-ups) each - and the fastest is set.  Why: what parallel lanes gain depends on state the library
        cannot see - ROCm maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4, which this package
        leaves alone since round 6: more queues make five or more busy streams collapse), and lane streams created next to other live streams (torch's
        pools, RCCL, another context) may share a queue with them: measured 7.5-9.9 ms per batch-1 call with four lanes
        in that state against 3.4 ms with their own queues and 5.0 ms on one stream.  Results do not depend on the
        assignment (same kernels, same order per buffer).  When the winner is what the library picks by itself for this
        batch (4 lanes up to 32 frames, 2 above) the lane option goes back to 0 = by batch size, so other batch
        sizes keep their own default; a measurement taken at a batch of the OTHER class than the one the context was built
        for (max_batch <= 32 / > 32) only sets the plan flag and leaves the lane count "by batch size".
        Returns ((lanes, planned), {(lanes, planned): ms}) - `lanes` is what was measured fastest, `self.lanes` what is set."""
        import time
        if self.program is None:
            raise _lib.AcrmiError('no checkpoint loaded')
        x = torch.zeros(batch, 512, 512, 3, dtype=torch.uint8, device=self.device)
        self.set_lanes(1)
        self.profile_ops(x)
        self.profile_ops(x)           # (warm) these times are what the planned schedules use
        ms = {}
        for n in candidates:
            for planned in ((False,) if n == 1 else (False, True)):
                self.set_lane_plan(planned)
                self.set_lanes(n)
                for _ in range(2):
                    self.backbone_heads(x)
                torch.cuda.synchronize(self.device)
                t0 = time.perf_counter()
                for _ in range(calls):
                    self.backbone_heads(x)
                torch.cuda.synchronize(self.device)
                ms[(int(n), planned)] = (time.perf_counter() - t0) / calls * 1e3
        best = min(ms, key=ms.get)
        self.set_lane_plan(best[1])
        # The measurement was taken at `batch`; it only overrides the library's choice for contexts that serve such batches
        # (the library's schedules: 4 lanes up to 32 frames, 2 above).  A context built for large batches keeps "by batch
        # size" after a batch-1 measurement: a batch-1 winner of 1 or 6 lanes must not replace the 2 lanes of its 64-frame
        # calls
        # ... and the other way round: tune_lanes(batch=64) on a max_batch=64 context IS a measurement of the class that context
        # serves, and is applied.  Classes as in the library: up to 32 frames / above (AUTO_SMALL_BATCH).
        same_class = (batch > 32) == (self.max_batch > 32)
        default = 4 if batch <= 32 else 2
        self.set_lanes(best[0] if same_class and best[0] != default else 0)
        return best, ms

    def set_conf_thresh(self, thresh):
        """ACRMI_OPT_CONF_THRESH = args().centermap_conf_thresh (acr/result_parser.py:198-205,241; strict >)."""
        _lib.check(self.L.acrmi_set_option_f(self.ctx, _lib.OPT_CONF_THRESH, float(thresh)), self.ctx)
        self.conf_thresh = float(thresh)

    def set_center_idx(self, idx):
        """ACRMI_OPT_CENTER_IDX: root-alignment joint of the fused path (args().align_idx; None = no alignment,
        acr/mano_wrapper.py:19-33)."""
        _lib.check(self.L.acrmi_set_option(self.ctx, _lib.OPT_CENTER_IDX, -1 if idx is None else int(idx)), self.ctx)
        self.center_idx = idx

    def set_temporal(self, on, smooth_coeff=None):
        """ACRMI_OPT_TEMPORAL: `forward` smooths the decoded poses/betas on the device before MANO
        (acr/main.py:69-83); the frames of a call are then one video stream in order."""
        if smooth_coeff is not None:
            _lib.check(self.L.acrmi_set_option_f(self.ctx, _lib.OPT_SMOOTH_COEFF, float(smooth_coeff)), self.ctx)
            self.smooth_coeff = float(smooth_coeff)
        _lib.check(self.L.acrmi_set_option(self.ctx, _lib.OPT_TEMPORAL, int(bool(on))), self.ctx)
        self.temporal = bool(on)

    def set_mano_fp16(self, on):
        """ACRMI_OPT_MANO_FP16: the MANO stage reads f16 copies of its blend-shape tables and skinning weights
        (BASELINE.json configs[4]); fp32 arithmetic."""
        _lib.check(self.L.acrmi_set_option(self.ctx, _lib.OPT_MANO_FP16, int(bool(on))), self.ctx)
        self.mano_fp16 = bool(on)

    def set_batch_semantics(self, mode):
        """ACRMI_OPT_BATCH_PRIOR: 'frame' (default: every frame decides its cross-hand prior like a batch of one) or
        'reference' (`forward` applies the reference's batch-wide rules at B > 1, acr/result_parser.py:42-47,102-145:
        decode -> acrmi_prior_gate -> gated decode on the device, one call)."""
        if mode not in ('frame', 'reference'):
            raise ValueError("batch_semantics %r: 'frame' or 'reference'" % (mode,))
        _lib.check(self.L.acrmi_set_option(self.ctx, _lib.OPT_BATCH_PRIOR, int(mode == 'reference')), self.ctx)
        self.batch_semantics = mode

    def prior_gate(self, slots):
        """acrmi_prior_gate: slots [B,2,176] of a first decode -> int32 [B] for decode(prior_gate=...), on the device (no
        host round trip): the reference's batch-wide prior decision (acr/result_parser.py:42-47,102-145)."""
        if not slots.is_cuda or slots.dtype != torch.float32 or not slots.is_contiguous():
            raise ValueError('slots must be a contiguous float32 device tensor')
        gate = torch.empty(slots.shape[0], dtype=torch.int32, device=slots.device)
        _lib.check(self.L.acrmi_prior_gate(self.ctx, _ptr(slots), slots.shape[0], _ptr(gate), _stream(self.device)), self.ctx)
        return gate

    def smooth(self, slots, streams=None, table=None):
        """One-Euro smoothing of slots [B,2,176] in place (acr/utils.py:1466-1527), state resident in the context: the
        frames are one video stream in order.  streams= (one id per frame, -1 = leave the frame alone) with table= (a
        StreamTable): every frame is filtered with the state of ITS stream instead (acrmi_smooth_streams) - frames that
        share an id are one sequence in batch order, streams never meet."""
        if not slots.is_cuda or slots.dtype != torch.float32 or not slots.is_contiguous():
            raise ValueError('slots must be a contiguous float32 device tensor')
        ids = stream_args(streams, table, slots.shape[0])
        if ids is None:
            _lib.check(self.L.acrmi_smooth(self.ctx, _ptr(slots), slots.shape[0], _stream(self.device)), self.ctx)
        else:
            _lib.check(self.L.acrmi_smooth_streams(self.ctx, table.handle, _ptr(slots), slots.shape[0],
                                                   ids.ctypes.data_as(C.c_void_p), _stream(self.device)), self.ctx)
        return slots

    def smooth_reset(self):
        _lib.check(self.L.acrmi_smooth_reset(self.ctx, _stream(self.device)), self.ctx)

    def associate(self, slots, tracks, table, smooth=True):
        """ops.associate_hands with this context's smoothing coefficient: slots [B,K,2,176] reordered in place into the
        track order of `table` (a TrackTable of K slots), tracks = the stream of each frame -> (track_ids, perm) int32 [B,K,2]."""
        return ops_mod.associate_hands(slots, tracks, table, smooth=smooth, ctx=self.ctx)

    # ---- multi-GPU ----------------------------------------------------------------
    def comm_init(self, n_ranks, rank, unique_id, allow_second_communicator=False):
        """acrmi_comm_init: RCCL communicator on this context's device (collective).
        Refused when this process already runs a torch.distributed NCCL (= RCCL) process group: a process that holds TWO RCCL
        communicators pays +11 ms per batch for a side-stream all-gather next to a running batch (46.8 vs 35.4 ms at world size
        1, tools/allgather_probe.py) - a host uses ONE of the two transports (the C transport's control
        plane runs over gloo).  allow_second_communicator=True overrides (correctness is unaffected; tests use it)."""
        if not allow_second_communicator and torch_nccl_group_active():
            raise _lib.AcrmiError(
                'acrmi_comm_init: this process already runs a torch.distributed NCCL (RCCL) process group; a second RCCL '
                'communicator next to it costs ~11 ms per batch (DESIGN.md section 6).  Use ONE transport: '
                "ShardedRunner(transport='torch') on the NCCL group, or initialise torch.distributed with backend 'gloo' for the "
                "control plane of transport='c'.  (allow_second_communicator=True overrides.)")
        uid = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        _lib.check(self.L.acrmi_comm_init(self.ctx, int(n_ranks), int(rank), uid), self.ctx)
        self.comm_ranks = int(n_ranks)

    def allgather(self, send, recv, stream=None):
        """acrmi_allgather of a flat float32 device tensor into recv [n_ranks * send.numel()]."""
        if recv.numel() != self.comm_ranks * send.numel():
            raise ValueError('recv must hold n_ranks * send.numel() floats')
        st = _stream(self.device) if stream is None else C.c_void_p(stream.cuda_stream)
        _lib.check(self.L.acrmi_allgather(self.ctx, None, _ptr(send), _ptr(recv), send.numel(), st), self.ctx)
        return recv

    def run_point_heads(self, B, max_hand=1):
        """Re-evaluates the point heads on the resident buffers for the current center maps (acrmi_point_heads); max_hand > 1:
        at the pixels `decode(B, max_hand=max_hand)` reads (acrmi_point_heads_multi)."""
        max_hand = check_max_hand(max_hand)
        if max_hand > 1:
            _lib.check(self.L.acrmi_point_heads_multi(self.ctx, B, max_hand, _stream(self.device)), self.ctx)
        else:
            _lib.check(self.L.acrmi_point_heads(self.ctx, B, _stream(self.device)), self.ctx)

    def ensure_batch(self, B):
        if self.program is None:
            raise _lib.AcrmiError('no checkpoint loaded')
        if B > self.max_batch:
            self._set_program(B)

    def load_mano(self, tables):
        """tables: {'left': {...}, 'right': {...}} numpy arrays as registered by mano/manolayer.py:61-102.
        The left-hand shapedirs x-flip (acr/mano_wrapper.py:35) must already be applied by the caller."""
        for name in ('left', 'right'):
            self.load_mano_side(name, tables[name])

    def adopt(self, other):
        """Takes over the MANO tables and options of an engine this one replaces (a checkpoint reload builds a new
        context; MANOWrapper / callers keep working against the model's current engine)."""
        for name, t in other._mano_tables.items():
            self.load_mano_side(name, t)
        self.set_conf_thresh(other.conf_thresh)
        self.set_center_idx(other.center_idx)
        if other.lanes:
            self.set_lanes(other.lanes)
        self.set_temporal(other.temporal, smooth_coeff=other.smooth_coeff)
        self.set_mano_fp16(other.mano_fp16)
        self.set_batch_semantics(getattr(other, 'batch_semantics', 'frame'))
        self._contact_sign_set = getattr(other, '_contact_sign_set', None)

    def load_mano_side(self, name, t):
        """One side's tables (mano/manolayer.py:61-102 buffers) -> HBM, blend-shape tables transposed."""
        side = {'left': 0, 'right': 1}[name]
        arrs = [np.ascontiguousarray(np.asarray(t[k], np.float32)) for k in
                ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'weights', 'hands_mean')]
        shapes = [(778, 3), (778, 3, 10), (778, 3, 135), (16, 778), (778, 16), (45,)]
        for a, s in zip(arrs, shapes):
            if a.shape != s and a.reshape(-1).shape != (int(np.prod(s)),):
                raise ValueError('MANO table has shape %s, expected %s' % (a.shape, s))
        with torch.cuda.device(self.device):
            torch.cuda.synchronize()      # tables may be replaced while earlier launches still read them
            _lib.check(self.L.acrmi_load_mano(self.ctx, side, *[a.ctypes.data_as(C.c_void_p) for a in arrs]), self.ctx)
        self._mano_tables[name] = {k: a for k, a in zip(('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'weights',
                                                          'hands_mean'), arrs)}
        self.have_mano = len(self._mano_tables) == 2
        self._derive_contact_sign(name)
        if t.get('faces') is not None:      # tables without faces load as before; `render` then raises the ACRMI_ESTATE error
            self.load_faces(name, t['faces'])

    def load_faces(self, name, faces):
        """One side's triangles (mano/manolayer.py:68 `faces`, [F,3] over the 778 vertices) for `render` (acrmi_load_faces)."""
        side = {'left': 0, 'right': 1}[name]
        f = faces.detach().cpu().numpy() if hasattr(faces, 'detach') else np.asarray(faces)
        if f.ndim != 2 or f.shape[1] != 3:
            raise ValueError('faces must be [F,3]')
        f = np.ascontiguousarray(f.astype(np.int32))
        _lib.check(self.L.acrmi_load_faces(self.ctx, side, f.ctypes.data_as(C.c_void_p), f.shape[0]), self.ctx)
        if name in self._mano_tables:
            self._mano_tables[name]['faces'] = f
        self._faces[name] = f
        self.have_faces = len(self._faces) == 2
        self._derive_contact_sign(name)

    def _derive_contact_sign(self, name):
        """The orientation of a side's faces on its template vertices (ops.mesh_orientation), +1 while either is missing -
        what acrmi_load_faces / acrmi_load_mano derive for the context."""
        t, f = self._mano_tables.get(name), self._faces.get(name)
        side = {'left': 0, 'right': 1}[name]
        self._contact_sign[side] = 1
        if t is not None and f is not None:
            self._contact_sign[side] = ops_mod.mesh_orientation(np.asarray(t['v_template'], np.float32).reshape(778, 3), f)

    @property
    def contact_sign(self):
        """(left, right): the sign `contact` multiplies each side's vertex normals with."""
        return tuple(self._contact_sign_set or self._contact_sign)

    def set_contact_sign(self, left, right):
        """Overrides the per-side orientation signs of `contact` (+1: the faces are wound outwards); None, None: back to the
        derived ones."""
        if left is None and right is None:
            self._contact_sign_set = None
            return
        if left not in (1, -1) or right not in (1, -1):
            raise ValueError('contact signs are +1 or -1')
        self._contact_sign_set = [int(left), int(right)]

    # ---- hot path ------------------------------------------------------------------------------
    def _check_img(self, img):
        if img.dtype != torch.uint8 or img.dim() != 4 or tuple(img.shape[1:]) != (512, 512, 3):
            raise ValueError('image must be uint8 [B,512,512,3] RGB, got %s %s' % (img.dtype, tuple(img.shape)))
        if img.device != self.device:
            img = img.to(self.device)
        return img.contiguous()

    def backbone_heads(self, img):
        img = self._check_img(img)
        B = img.shape[0]
        self.ensure_batch(B)
        _lib.check(self.L.acrmi_backbone_heads(self.ctx, _ptr(img), B, _stream(self.device)), self.ctx)
        return B

    def check_range(self):
        """'fp16x3' programs: waits for the current stream and raises _lib.AcrmiRangeError if an activation left the f16
        range (|x| > 65504) since the last check - the split halves are then inf / -inf and the library has written the
        affected calls' slots and meshes as NaN (acrmi_check_range).  A no-op for every other precision.  Engine.forward
        stays asynchronous and does NOT call this; the host-facing API (acr.model.ACR.forward, acr.main.ACR) does."""
        _lib.check(self.L.acrmi_check_range(self.ctx, _stream(self.device)), self.ctx)

    def heads(self, features):
        """acr/model.py:47-65 on backbone features the caller holds: float [B, C0, 128, 128] (NCHW, what the reference's
        head_forward takes; C0 = 32 for HRNet-W32) -> the heads run on them, results as after backbone_heads (head_maps /
        decode).  fp32-storage programs (acrmi_heads)."""
        if self.program is None:
            raise _lib.AcrmiError('no checkpoint loaded')
        c0 = self.L.acrmi_backbone_channels(self.ctx)
        _lib.check(c0, self.ctx)
        if features.dim() != 4 or tuple(features.shape[1:]) != (c0, 128, 128) or not features.is_floating_point():
            raise ValueError('features must be float [B,%d,128,128] (NCHW), got %s %s' % (c0, features.dtype, tuple(features.shape)))
        B = features.shape[0]
        self.ensure_batch(B)
        f = features.to(self.device, torch.float32).contiguous()
        _lib.check(self.L.acrmi_heads(self.ctx, _ptr(f), B, _stream(self.device)), self.ctx)
        return B

    def buffer(self, buf_id, B, channels=None):
        """Zero-copy torch view [B,h,w,cs] of a program buffer (NHWC) in its storage type (float32 / float16 /
        bfloat16: 16-bit programs keep the activations between layers in 16 bits)."""
        h, w, cs = C.c_int(), C.c_int(), C.c_int()
        p = self.L.acrmi_buffer_ptr(self.ctx, buf_id, C.byref(h), C.byref(w), C.byref(cs))
        if not p:
            raise ValueError('no such buffer %d' % buf_id)
        dt = self.L.acrmi_buffer_dtype(self.ctx, buf_id)
        n = B * h.value * w.value * cs.value
        arr = _DevArray(p, n, self.device, '<f4' if dt == _lib.DT_F32 else '<i2')
        t = torch.as_tensor(arr, device=self.device)
        if dt != _lib.DT_F32:
            t = t.view(torch.float16 if dt == _lib.DT_F16 else torch.bfloat16)
        t = t.view(B, h.value, w.value, cs.value)
        return t if channels is None else t[..., :channels]

    def head_maps(self, B, nchw=True):
        """The reference's H11 output dict (acr/model.py:56-63) from the resident head buffers."""
        hl = self.program['heads']
        out = {}
        for si, side in enumerate('lr'):
            out[side + '_params_maps'] = self.buffer(hl.params_buf[si], B, 109)
            out[side + '_center_map'] = self.buffer(hl.center_buf[si], B, 1)
            out[side + '_prior_maps'] = self.buffer(hl.prior_buf[si], B, 106)
        out['segms'] = self.buffer(hl.segm_buf, B, 33)
        if nchw:
            out = {k: v.permute(0, 3, 1, 2).contiguous() for k, v in out.items()}
        return out

    def center_maps(self, B):
        """The left / right centre maps of the last program run as one fp32 tensor [B,2,h,w] (what `overlay(...,
        'centermap')` draws straight from the head buffers; a 16-bit storage program's maps convert exactly)."""
        hl = self.program['heads']
        return torch.stack([self.buffer(hl.center_buf[si], B, 1)[..., 0] for si in (0, 1)], 1).float().contiguous()

    def decode(self, B, prior_gate=None, max_hand=1):
        """prior_gate: int32 device tensor [B] (acrmi_decode_gated: < 0 per-frame rule, 0 no prior, 1 prior when the frame
        has both hands) - how acr.result_parser applies the reference's batch-wide prior rules; None = per frame.
        max_hand > 1 (up to _lib.MAX_HAND): the max_hand best centres of each side per frame -> slots [B,max_hand,2,176]
        (acrmi_decode_multi); the batch-wide gate knows one hand per side: a ValueError with it."""
        max_hand = check_max_hand(max_hand)
        if max_hand > 1:
            if prior_gate is not None:
                raise ValueError('prior_gate is the batch-wide rule of one hand per side: not with max_hand=%d' % max_hand)
            slots = torch.empty(B, max_hand, 2, _lib.SLOT, dtype=torch.float32, device=self.device)
            _lib.check(self.L.acrmi_decode_multi(self.ctx, B, max_hand, _ptr(slots), _stream(self.device)), self.ctx)
            return slots
        slots = torch.empty(B, 2, _lib.SLOT, dtype=torch.float32, device=self.device)
        if prior_gate is None:
            _lib.check(self.L.acrmi_decode(self.ctx, B, _ptr(slots), _stream(self.device)), self.ctx)
        else:
            g = prior_gate.to(device=self.device, dtype=torch.int32).contiguous()
            if g.numel() != B:
                raise ValueError('prior_gate must hold one int per frame')
            _lib.check(self.L.acrmi_decode_gated(self.ctx, B, _ptr(g), _ptr(slots), _stream(self.device)), self.ctx)
        return slots

    def mano(self, poses, betas, side, center_idx=9, cam=None, offsets=None, rotmat=False):
        """poses [H,48], betas [H,10] float32 on device; side: int tensor [H] (0 left, 1 right).
        rotmat: poses are [H,16,3,3] orthonormal rotation matrices (acrmi_mano_rotmat; no projection outputs)."""
        H = poses.shape[0]
        dev = self.device
        poses = poses.to(dev, torch.float32).contiguous()
        if rotmat:
            if tuple(poses.shape[1:]) != (16, 3, 3) or cam is not None:
                raise ValueError('rotmat poses are [H,16,3,3]; the projection is not part of this mode')
            betas = betas.to(dev, torch.float32).contiguous()
            verts = torch.empty(H, 778, 3, dtype=torch.float32, device=dev)
            joints = torch.empty(H, 21, 3, dtype=torch.float32, device=dev)
            center = torch.empty(H, 1, 3, dtype=torch.float32, device=dev)
            if H:
                side = side.to(dev, torch.int32).contiguous()
                _lib.check(self.L.acrmi_mano_rotmat(self.ctx, _ptr(poses), _ptr(betas), 10, _ptr(side), H,
                                                    -1 if center_idx is None else int(center_idx), _ptr(verts), _ptr(joints),
                                                    _ptr(center), _stream(dev)), self.ctx)
            return verts, joints, center, {}
        betas = betas.to(dev, torch.float32).contiguous()
        verts = torch.empty(H, 778, 3, dtype=torch.float32, device=dev)
        joints = torch.empty(H, 21, 3, dtype=torch.float32, device=dev)
        center = torch.empty(H, 1, 3, dtype=torch.float32, device=dev)
        extra = {}
        if H == 0:
            return verts, joints, center, extra
        side = side.to(dev, torch.int32).contiguous()
        vc = pj = org = None
        if cam is not None:
            cam = cam.to(dev, torch.float32).contiguous()
            vc = torch.empty(H, 778, 3, dtype=torch.float32, device=dev)
            pj = torch.empty(H, 21, 2, dtype=torch.float32, device=dev)
            extra = {'verts_camed': vc, 'pj2d': pj}
            if offsets is not None:
                offsets = offsets.to(dev, torch.float32).contiguous()
                org = torch.empty(H, 21, 2, dtype=torch.float32, device=dev)
                extra['pj2d_org'] = org
        _lib.check(self.L.acrmi_mano(self.ctx, _ptr(poses), 48, _ptr(betas), 10, _ptr(side), H,
                                     -1 if center_idx is None else int(center_idx), _ptr(verts), _ptr(joints),
                                     _ptr(center), _ptr(cam), 3, _ptr(offsets), _ptr(vc), _ptr(pj), _ptr(org),
                                     _stream(dev)), self.ctx)
        return verts, joints, center, extra

    @staticmethod
    def check_mano_backward(poses, betas, side, center_idx, g_verts, g_joints, g_center):
        """The argument rules of `mano_backward`, checked on shapes alone (no device needed); ValueError when one is broken."""
        if poses.dim() != 2 or poses.shape[1] < 48:
            raise ValueError('poses must be [H,48] axis-angle rows (or rows of at least 48 values, read in place), got %s'
                             % (tuple(poses.shape),))
        H = poses.shape[0]
        if betas.dim() != 2 or betas.shape[0] != H or betas.shape[1] < 10:
            raise ValueError('betas must be [H,10] with one row per pose, got %s' % (tuple(betas.shape),))
        if side.numel() != H:
            raise ValueError('side must hold one value (0 left, 1 right) per hand')
        if center_idx is not None and not 0 <= int(center_idx) <= 20:
            raise ValueError('center_idx must be None or one of the 21 joints, got %r' % (center_idx,))
        for name, g, shape in (('g_verts', g_verts, (H, 778, 3)), ('g_joints', g_joints, (H, 21, 3))):
            if g is not None and tuple(g.shape) != shape:
                raise ValueError('%s must be %s, got %s' % (name, shape, tuple(g.shape)))
        if g_center is not None and g_center.numel() != 3 * H:
            raise ValueError('g_center must be [H,1,3] or [H,3], got %s' % (tuple(g_center.shape),))

    def mano_backward(self, poses, betas, side, center_idx=9, g_verts=None, g_joints=None, g_center=None):
        """The backward of `mano` in its axis-angle mode (acrmi_mano_backward): cotangents of verts [H,778,3], joints
        [H,21,3] and center [H,1,3] (each may be None = zeros) -> (g_poses [H,48], g_betas [H,10]).  Device tensors,
        queued on the current stream, no host visit.  float32 rows whose values are contiguous - `slots[:, 6:54]` of
        [H,176] slot rows - are read in place; always the fp32 tables, also with set_mano_fp16."""
        self.check_mano_backward(poses, betas, side, center_idx, g_verts, g_joints, g_center)
        dev = self.device
        H = poses.shape[0]

        def rows(t, n):      # [H, >= n] -> a float32 device tensor whose rows can be read in place, and its row stride
            t = t.to(dev, torch.float32)
            if t.stride(1) != 1 or t.stride(0) < n:
                t = t[:, :n].contiguous()
            return t, max(t.stride(0), n)
        poses, pose_stride = rows(poses, 48)
        betas, beta_stride = rows(betas, 10)
        g_poses = torch.empty(H, 48, dtype=torch.float32, device=dev)
        g_betas = torch.empty(H, 10, dtype=torch.float32, device=dev)
        if H == 0:
            return g_poses, g_betas
        side = side.to(dev, torch.int32).contiguous()
        g = [None if t is None else t.to(dev, torch.float32).contiguous() for t in (g_verts, g_joints, g_center)]
        _lib.check(self.L.acrmi_mano_backward(self.ctx, _ptr(poses), pose_stride, _ptr(betas), beta_stride, _ptr(side), H,
                                              -1 if center_idx is None else int(center_idx), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]),
                                              _ptr(g_poses), _ptr(g_betas), _stream(dev)), self.ctx)
        return g_poses, g_betas

    FIT_GROUPS = ('root', 'pose', 'betas', 'trans', 'cam')      # the learning-rate groups of mano_fit, in lr5's order

    @staticmethod
    def check_mano_fit(side, joints=None, kp2d=None, verts=None, w_joints=None, w_kp2d=None, w_verts=None, init=None,
                       state=None, prior=None, lam_pose=0., lam_beta=0., lr=0.02, steps=100, center_idx=9,
                       free=('root', 'pose', 'betas'), dense=False):
        """The argument rules of `mano_fit`, checked on shapes alone (no device needed); ValueError when one is broken.
        -> H, the number of hands."""
        if side.dim() != 1:
            raise ValueError('side must be [H] (0 left, 1 right), got %s' % (tuple(side.shape),))
        H = side.shape[0]
        for name, t, shape in (('joints', joints, (H, 21, 3)), ('kp2d', kp2d, (H, 21, 2)), ('verts', verts, (H, 778, 3)),
                               ('w_joints', w_joints, (H, 21)), ('w_kp2d', w_kp2d, (H, 21)), ('w_verts', w_verts, (H,)),
                               ('prior', prior, (H, 58)), ('state', state, (H, _lib.FIT_STATE))):
            if t is not None and tuple(t.shape) != shape:
                raise ValueError('%s must be %s, got %s' % (name, shape, tuple(t.shape)))
        for w, t, name in ((w_joints, joints, 'joints'), (w_kp2d, kp2d, 'kp2d'), (w_verts, verts, 'verts')):
            if w is not None and t is None:
                raise ValueError('w_%s without %s' % (name, name))
        if init is not None and state is not None:
            raise ValueError('init starts a fresh fit, state continues one: not both')
        if init is not None:
            shapes = {'poses': (H, 48), 'betas': (H, 10), 'trans': (H, 3), 'cam': (H, 3)}
            for k, t in init.items():
                if k not in shapes:
                    raise ValueError('init holds poses / betas / trans / cam, not %r' % (k,))
                if tuple(t.shape) != shapes[k]:
                    raise ValueError('init[%r] must be %s, got %s' % (k, shapes[k], tuple(t.shape)))
        if not isinstance(steps, int) or not 0 <= steps <= _lib.FIT_MAX_STEPS:
            raise ValueError('steps must be 0..%d per call (chain longer fits through state), got %r' % (_lib.FIT_MAX_STEPS, steps))
        if center_idx is not None and not 0 <= int(center_idx) <= 20:
            raise ValueError('center_idx must be None or one of the 21 joints, got %r' % (center_idx,))
        for g in free:
            if g not in Engine.FIT_GROUPS:
                raise ValueError('free names groups of %s, got %r' % (Engine.FIT_GROUPS, g))
        if isinstance(lr, dict):
            for g, v in lr.items():
                if g not in Engine.FIT_GROUPS or not float(v) >= 0:
                    raise ValueError('lr is a float or a dict over %s of values >= 0, got %r: %r' % (Engine.FIT_GROUPS, g, v))
            for g in free:
                if g not in lr:
                    raise ValueError('lr names no rate for the free group %r' % (g,))
        elif not float(lr) >= 0:
            raise ValueError('lr must be >= 0, got %r' % (lr,))
        if not float(lam_pose) >= 0 or not float(lam_beta) >= 0:
            raise ValueError('lam_pose and lam_beta must be >= 0')
        return H

    def mano_fit_state(self, H, init=None):
        """A fresh state [H, FIT_STATE] for `mano_fit`: parameters from init (poses / betas / trans / cam; zeros and
        cam = (1, 0, 0) where absent), m = v = 0, t = 0."""
        dev = self.device
        state = torch.zeros(H, _lib.FIT_STATE, dtype=torch.float32, device=dev)
        state[:, 61] = 1.0
        for k, at, n in (('poses', 0, 48), ('betas', 48, 10), ('trans', 58, 3), ('cam', 61, 3)):
            if init is not None and k in init:
                state[:, at:at + n] = init[k].to(dev, torch.float32)
        return state

    def mano_fit(self, side, joints=None, kp2d=None, verts=None, w_joints=None, w_kp2d=None, w_verts=None, init=None,
                 state=None, prior=None, lam_pose=0., lam_beta=0., lr=0.02, steps=100, center_idx=9,
                 free=('root', 'pose', 'betas'), dense=False, grad=False, betas_adam=(0.9, 0.999), eps=1e-8):
        """Fits MANO pose, shape, translation and camera of H hands with `steps` Adam iterations in ONE launch
        (acrmi_mano_fit) to any mix of joints [H,21,3] (against joints + trans), kp2d [H,21,2] (against
        `mano`'s pj2d: root-aligned joints * s + (tx, ty)) and verts [H,778,3] (against verts + trans), plus
        lam_pose |pose[3:48] - prior|^2 + lam_beta |betas - prior|^2 (prior [H,58] = pose | betas, None = zeros).
        Weights w_joints / w_kp2d [H,21], w_verts [H]; missing ones are 1/21 per joint and 1/778: mean squared distances.
        init (a dict of poses / betas / trans / cam) starts a fresh fit, state (a previous call's 'state') continues one -
        chained calls equal one long call bit for bit.  free names the groups that move ('root', 'pose', 'betas', 'trans',
        'cam'); lr is a float or a dict per group.  dense=True runs the dense vertex level also without verts.
        -> {'poses' [H,48], 'betas' [H,10], 'trans' [H,3], 'cam' [H,3], 'loss' [H,2] (first and last evaluated step),
        'state' [H,FIT_STATE][, 'grad' [H,64] with grad=True: the gradient of the last evaluated step]}.
        Device tensors, queued on the current stream, no host visit."""
        H = self.check_mano_fit(side, joints, kp2d, verts, w_joints, w_kp2d, w_verts, init, state, prior, lam_pose, lam_beta, lr,
                                steps, center_idx, free, dense)
        dev = self.device
        f32 = lambda t: None if t is None else t.to(dev, torch.float32).contiguous()
        state = self.mano_fit_state(H, init) if state is None else state.to(dev, torch.float32).clone(memory_format=torch.contiguous_format)
        out = {'poses': torch.empty(H, 48, dtype=torch.float32, device=dev), 'betas': torch.empty(H, 10, dtype=torch.float32, device=dev),
               'trans': torch.empty(H, 3, dtype=torch.float32, device=dev), 'cam': torch.empty(H, 3, dtype=torch.float32, device=dev),
               'loss': torch.zeros(H, 2, dtype=torch.float32, device=dev), 'state': state}
        if grad:
            out['grad'] = torch.zeros(H, 64, dtype=torch.float32, device=dev)
        if H == 0:
            return out
        joints, kp2d, verts, prior = f32(joints), f32(kp2d), f32(verts), f32(prior)
        if joints is not None:
            w_joints = torch.full((H, 21), 1.0 / 21, dtype=torch.float32, device=dev) if w_joints is None else f32(w_joints)
        if kp2d is not None:
            w_kp2d = torch.full((H, 21), 1.0 / 21, dtype=torch.float32, device=dev) if w_kp2d is None else f32(w_kp2d)
        if verts is not None:
            w_verts = torch.full((H,), 1.0 / 778, dtype=torch.float32, device=dev) if w_verts is None else f32(w_verts)
        rate = lambda g: (float(lr.get(g, 0.0)) if isinstance(lr, dict) else float(lr)) if g in free else 0.0
        lr5 = (C.c_double * 5)(*[rate(g) for g in self.FIT_GROUPS])
        side = side.to(dev, torch.int32).contiguous()
        _lib.check(self.L.acrmi_mano_fit(self.ctx, _ptr(state), _ptr(side), H, -1 if center_idx is None else int(center_idx),
                                         _ptr(joints), _ptr(w_joints), _ptr(kp2d), _ptr(w_kp2d), _ptr(verts), _ptr(w_verts),
                                         _ptr(prior), float(lam_pose), float(lam_beta), lr5, float(betas_adam[0]),
                                         float(betas_adam[1]), float(eps), int(steps), 1 if dense else 0, _ptr(out['poses']),
                                         _ptr(out['betas']), _ptr(out['trans']), _ptr(out['cam']), _ptr(out['loss']),
                                         _ptr(out.get('grad')), _stream(dev)), self.ctx)
        return out

    def refine(self, out, kp2d=None, joints=None, weights=None, steps=50, lam_pose=1e-3, lam_beta=1e-3, max_hand=1, lr=0.02,
               free=('root', 'pose', 'betas', 'cam'), offsets=None, dense=False):
        """Test-time refinement of a forward's hands: every flagged hand of `out` (what `forward(...,
        project=True[, max_hand=K])` returned) is fitted with `mano_fit` - `steps` Adam iterations in one launch - to kp2d
        [B,(K,)2,21,2] in the units of out['pj2d'] (the canvas, -1..1) and / or joints [B,(K,)2,21,3] (root-aligned, metres),
        starting from the slots' pose, betas and cam (SLOT_POSES, SLOT_BETAS, SLOT_CAM) with that same prediction as the
        prior of lam_pose / lam_beta.  weights [B,(K,)2,21] (None: 1/21) apply to both targets; hands whose flag is off get
        all-zero weights and keep their slot bytes.  The fitted values are written into a COPY of the slots and `mano` runs on
        them with the projection (offsets [B,10]: also pj2d_org).  -> an `out` dict of the usual keys plus 'fit_loss'
        [B,(K,)2,2] (first and last evaluated step; 0 for unflagged hands): render, overlay, contact and score take it.  Device
        tensors, the current stream, no host visit."""
        slots = out['slots']
        K = check_max_hand(max_hand)
        lead = tuple(slots.shape[:-1])
        if slots.shape[-1] != _lib.SLOT or lead[-1] != 2 or not ((len(lead) == 2 and K == 1) or (len(lead) == 3 and lead[1] == K)):
            raise ValueError('out does not hold slots [B,%s2,%d] of max_hand=%d' % ('K,' if K > 1 else '', _lib.SLOT, K))
        if kp2d is None and joints is None:
            raise ValueError('refine needs kp2d or joints')
        for name, t, tail in (('kp2d', kp2d, (21, 2)), ('joints', joints, (21, 3)), ('weights', weights, (21,))):
            if t is not None and tuple(t.shape) != lead + tail:
                raise ValueError('%s must be %s, got %s' % (name, lead + tail, tuple(t.shape)))
        dev = self.device
        H = slots.numel() // _lib.SLOT
        rows = slots.reshape(H, _lib.SLOT)
        flat = lambda t, *tail: None if t is None else t.to(dev, torch.float32).reshape((H,) + tail)
        side = (torch.arange(H, device=dev, dtype=torch.int32) & 1)      # slot order: left, right
        on = rows[:, _lib.SLOT_FLAG] > 0.5
        w = flat(weights, 21) if weights is not None else torch.full((H, 21), 1.0 / 21, dtype=torch.float32, device=dev)
        w = w * on.unsqueeze(1).to(torch.float32)
        init = {'poses': rows[:, _lib.SLOT_POSES:_lib.SLOT_POSES + 48], 'betas': rows[:, _lib.SLOT_BETAS:_lib.SLOT_BETAS + 10],
                'cam': rows[:, _lib.SLOT_CAM:_lib.SLOT_CAM + 3]}
        fit = self.mano_fit(side, joints=flat(joints, 21, 3), kp2d=flat(kp2d, 21, 2), w_joints=None if joints is None else w,
                            w_kp2d=None if kp2d is None else w, init=init, prior=torch.cat([init['poses'], init['betas']], 1),
                            lam_pose=lam_pose, lam_beta=lam_beta, lr=lr, steps=steps, center_idx=self.center_idx, free=free,
                            dense=dense)
        new = rows.clone()
        keep = on.unsqueeze(1)
        for key, at, n in (('poses', _lib.SLOT_POSES, 48), ('betas', _lib.SLOT_BETAS, 10), ('cam', _lib.SLOT_CAM, 3)):
            new[:, at:at + n] = torch.where(keep, fit[key], rows[:, at:at + n])
        off = None
        if offsets is not None:
            off = self._frame_offsets(offsets, lead[0]).repeat_interleave(H // lead[0], 0)
        verts, jts, _, extra = self.mano(new[:, _lib.SLOT_POSES:_lib.SLOT_POSES + 48], new[:, _lib.SLOT_BETAS:_lib.SLOT_BETAS + 10],
                                         side, center_idx=self.center_idx, cam=new[:, _lib.SLOT_CAM:_lib.SLOT_CAM + 3], offsets=off)
        res = {k: v for k, v in out.items() if k not in ('cam_trans', 'pj2d_org')}
        res['slots'] = new.reshape(slots.shape)
        got = dict(extra, verts=verts, joints=jts)
        for k, v in got.items():      # an unflagged hand keeps what the forward gave it
            old = out.get(k)
            v = v.reshape(lead + tuple(v.shape[1:]))
            res[k] = v if old is None else torch.where(on.reshape(lead + (1, 1)), v, old.to(dev, torch.float32))
        res['fit_loss'] = torch.where(keep, fit['loss'], torch.zeros((), dtype=torch.float32, device=dev)).reshape(lead + (2,))
        return res

    def mano_autograd(self, poses, betas, side, center_idx=9):
        """`mano` as a node of torch's autograd graph: (verts, joints, center) that carry gradients back to poses [H,48] and
        betas [H,10] through `mano_backward`.  Once differentiable; side and center_idx are not differentiated."""
        if poses.dim() != 2 or poses.shape[1] != 48 or betas.dim() != 2 or tuple(betas.shape) != (poses.shape[0], 10):
            raise ValueError('poses must be [H,48] and betas [H,10], got %s and %s' % (tuple(poses.shape), tuple(betas.shape)))
        return ManoFunction.apply(self, poses.to(self.device, torch.float32), betas.to(self.device, torch.float32),
                                  side.to(self.device, torch.int32), center_idx)

    def forward(self, img, offsets=None, project=False, out=None, stream=None, streams=None, table=None, max_hand=1,
                tracks=None, track_table=None, smooth=True):
        """frames -> (slots [B,2,176], verts [B,2,778,3], joints [B,2,21,3][, verts_camed, pj2d, pj2d_org]).
        stream: raw hipStream_t (int) to queue the call on instead of torch's current stream; tensors this call
        allocates still come from the current stream's pool.
        streams= / table=: as `smooth` - the decoded poses / betas of every frame are smoothed with the state of its video
        stream before MANO (acrmi_forward_streams), whatever set_temporal says.
        max_hand = K > 1 (up to _lib.MAX_HAND): up to K hands of each side per frame (acrmi_forward_multi; DESIGN.md
        section 17) - every output gains a dimension, slots [B,K,2,176], verts [B,K,2,778,3], ...: pair k = (left rank k,
        right rank k), `.flatten(0, 1)` is B * K rows of the usual shape.  The dense heads run whatever set_point_heads
        says, unless set_point_heads_multi(True) asked for the towers at the K best centres of each side; streams=, set_temporal and batch_semantics 'reference' are a ValueError (no identity across frames, and the
        batch-wide rule knows one hand per side).
        tracks= / track_table= (any max_hand): the stream of each frame and a TrackTable of max_hand
        slots - the decoded hands are put into track order and (smooth) each track is smoothed with its own filter before MANO
        (acrmi_forward_tracks); the output gains 'track_ids' int32 [B,K,2] and has the [B,K,...] shapes also for K = 1.  Not
        together with streams= / table=."""
        K = check_max_hand(max_hand)
        multi = K > 1 or tracks is not None or track_table is not None      # the [B,K,...] shapes
        if K > 1 and tracks is None and track_table is None and (streams is not None or table is not None):
            raise ValueError('streams= follows one hand of each side through a video: not with max_hand=%d' % K)
        img = self._check_img(img)
        B = img.shape[0]
        ids = track_args(tracks, track_table, streams, table, K, B) if multi else stream_args(streams, table, B)
        self.ensure_batch(B)
        dev = self.device
        out = self._outputs(out, (B, K, 2) if multi else (B, 2), project, offsets is not None)
        if offsets is not None:
            offsets = offsets.to(dev, torch.float32).contiguous()
            if multi and tuple(offsets.shape) != (B, 10):
                raise ValueError('offsets must be [B,10]: one row per frame')
        tail = (_ptr(offsets), _ptr(out['slots']), _ptr(out['verts']), _ptr(out['joints']), _ptr(out.get('verts_camed')),
                _ptr(out.get('pj2d')), _ptr(out.get('pj2d_org')))
        raw = _stream(dev) if stream is None else C.c_void_p(stream)
        if not multi and ids is None:
            _lib.check(self.L.acrmi_forward(self.ctx, _ptr(img), B, *tail, raw), self.ctx)
        elif not multi:
            _lib.check(self.L.acrmi_forward_streams(self.ctx, table.handle, ids.ctypes.data_as(C.c_void_p), _ptr(img), B, *tail, raw),
                       self.ctx)
        elif ids is None:
            _lib.check(self.L.acrmi_forward_multi(self.ctx, _ptr(img), B, K, *tail, raw), self.ctx)
        else:
            if out.get('track_ids') is None:
                out['track_ids'] = torch.empty(B, K, 2, dtype=torch.int32, device=dev)
            elif tuple(out['track_ids'].shape) != (B, K, 2) or out['track_ids'].dtype != torch.int32 or not out['track_ids'].is_contiguous():
                raise ValueError("out['track_ids'] must be a contiguous int32 tensor [B,K,2]")
            _lib.check(self.L.acrmi_forward_tracks(self.ctx, track_table.handle, ids.ctypes.data_as(C.c_void_p), int(bool(smooth)),
                                                   _ptr(img), B, K, *tail, _ptr(out['track_ids']), raw), self.ctx)
        return out

    def _outputs(self, out, lead, project, org):
        """The result tensors of `forward` for the leading shape `lead` = (B, 2) or (B, K, 2): new ones (project: with
        verts_camed and pj2d; org: and pj2d_org), or the caller's `out`, which must have that shape."""
        if out is not None:
            if tuple(out['slots'].shape) != lead + (_lib.SLOT,) or tuple(out['verts'].shape) != lead + (778, 3):
                raise ValueError('out does not hold %d frames of %d hand pairs' % (lead[0], lead[1] if len(lead) == 3 else 1))
            return out
        new = lambda *tail: torch.empty(lead + tail, dtype=torch.float32, device=self.device)
        out = {'slots': new(_lib.SLOT), 'verts': new(778, 3), 'joints': new(21, 3)}
        if project:
            out['verts_camed'], out['pj2d'] = new(778, 3), new(21, 2)
            if org:
                out['pj2d_org'] = new(21, 2)
        return out

    def track_step(self, frames, boxes, box_frame=None, frame_hw=None, streams=None, table=None, pixel_format='bgr',
                   matrix='cv601', scale=1.5, min_size=64):
        """One step of a video loop on regions that never visits the host (DESIGN.md "Tracking on the device"): the regions
        `boxes` (a contiguous int32 device tensor [n,4]) of `frames` -> (out, next_boxes, status).  Three calls queued in
        order on the current stream: ops.preprocess_rois_device, forward(project=True, offsets=<its device rows>) and
        ops.track_boxes on out['pj2d_org'] and the flags.  next_boxes (int32 device [n,4]) are the regions of the next
        frames; status int32 device [n] is 1 where a box left no pixel and the whole frame was taken; out also carries
        the network input ('image') and the device `offsets` rows ('offsets': what render / overlay take).  frames, box_frame,
        pixel_format, matrix: as ops.preprocess_rois_device; frame_hw: as ops.track_boxes, default the sizes of the
        regions' frames; streams / table: as forward; scale, min_size: as acr.utils.boxes_from_keypoints."""
        from . import ops
        scale, min_size = ops.check_track_args(scale, min_size)
        rgb, offsets, status = ops.preprocess_rois_device(frames, boxes, box_frame, pixel_format=pixel_format, matrix=matrix)
        if frame_hw is None:
            frame_hw = ops.region_frame_sizes(frames, box_frame, pixel_format)
        out = self.forward(rgb, offsets=offsets, project=True, streams=streams, table=table)
        out['image'], out['offsets'] = rgb, offsets      # what the network saw, and the rows render / overlay take
        return out, ops.track_boxes(out['pj2d_org'], out['slots'], frame_hw, scale=scale, min_size=min_size), status

    # ---- views: what render / overlay and their region forms share -----------------------------------------------------------
    @staticmethod
    def _check_frames(images, name, lead):
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3 or not images.is_cuda:
            raise ValueError('%s must be uint8 [%s,H,W,3] on the device' % (name, lead))
        return images.contiguous()

    def _cam_trans(self, out, cam_trans, n, focal_length, st):
        """cam_trans [n,2,3] of render: the caller's, out['cam_trans'], or computed from out['joints'] / out['pj2d']."""
        if cam_trans is None:
            cam_trans = out.get('cam_trans')
        if cam_trans is None:
            if out.get('pj2d') is None:
                raise ValueError('cam_trans is needed (or out from forward(..., project=True))')
            cam_trans = torch.empty(n, 2, 3, dtype=torch.float32, device=self.device)
            _lib.check(self.L.acrmi_cam_trans(_ptr(out['joints']), _ptr(out['pj2d']), 2 * n, float(focal_length), 512.0,
                                              _ptr(cam_trans), st))
        return cam_trans.to(self.device, torch.float32).contiguous()

    @staticmethod
    def _colors(colors, bgr):
        """colors [2,3] of render as a host array, None = the library's (the reference's, RGB)."""
        if colors is None and not bgr:
            return None
        c = np.asarray(colors if colors is not None else [list(reversed(x)) for x in HAND_COLORS_RGB], np.float32)
        if c.shape != (2, 3):
            raise ValueError('colors must be [2,3] (left, right)')
        return np.ascontiguousarray(c)

    @staticmethod
    def _dst(dst, src, shape, name):
        if dst is None:
            return torch.empty(shape, dtype=torch.uint8, device=src.device)
        if dst.dtype != torch.uint8 or tuple(dst.shape) != shape or not dst.is_contiguous() or dst.device != src.device:
            raise ValueError('dst must be a contiguous uint8 tensor %s on the device of the %s' % (shape, name))
        return dst

    def _frame_offsets(self, offsets, B):
        if offsets is not None:
            offsets = offsets.to(self.device, torch.float32).contiguous()
            if tuple(offsets.shape) != (B, 10):
                raise ValueError('offsets must be [B,10]')
        return offsets

    def _render(self, out, src, n, name, offsets, region_frame, cam_trans, focal_length, visible_weight, colors, bgr, dst,
                return_ids, stream, vertex_colors=None):
        """acrmi_render (region_frame None) / acrmi_render_regions of the n frames / regions of `out` over src; with
        vertex_colors [n,2,778,3] their _colored forms."""
        vcol = None
        if vertex_colors is not None:
            if not vertex_colors.is_cuda or tuple(vertex_colors.shape) != (n, 2, 778, 3):
                raise ValueError('vertex_colors must be [%d,2,778,3] on the device' % n)
            vcol = vertex_colors.to(self.device, torch.float32).contiguous()
        N, H, W, _ = src.shape
        st = _stream(self.device) if stream is None else C.c_void_p(stream)
        cam_trans = self._cam_trans(out, cam_trans, n, focal_length, st)
        col = self._colors(colors, bgr)
        dst = self._dst(dst, src, (N, H, W, 3), name)
        ids = torch.empty(N, H, W, dtype=torch.int32, device=self.device) if return_ids else None
        verts, slots = out['verts'].contiguous(), out['slots'].contiguous()
        head = (self.ctx, _ptr(verts), _ptr(cam_trans), _ptr(slots), n, _ptr(offsets))
        tail = ((None if col is None else col.ctypes.data_as(C.c_void_p),) + (() if vcol is None else (_ptr(vcol),)) +
                (float(focal_length), float(visible_weight), _ptr(src), _ptr(dst)))
        if region_frame is None:
            call = self.L.acrmi_render if vcol is None else self.L.acrmi_render_colored
            _lib.check(call(*head, *tail, H, W, _ptr(ids), st), self.ctx)
        else:
            call = self.L.acrmi_render_regions if vcol is None else self.L.acrmi_render_regions_colored
            _lib.check(call(*head, _ptr(region_frame), *tail, N, H, W, _ptr(ids), st), self.ctx)
        self._render_keep = (verts, slots, cam_trans, offsets, region_frame, src, vcol)      # referenced until the next call has been queued
        return (dst, ids) if return_ids else dst

    def _overlay(self, out, src, n, name, what, kps_key, offsets, region_frame, bgr, dst, stream):
        """acrmi_overlay (region_frame None) / acrmi_overlay_regions of the n frames / regions of `out` over src."""
        if what not in ('pj2d', 'centermap'):
            raise ValueError("what: 'pj2d' or 'centermap'")
        N, H, W, _ = src.shape
        st = _stream(self.device) if stream is None else C.c_void_p(stream)
        dst = self._dst(dst, src, (N, H, W, 3) if what == 'pj2d' else (2, N, H, W, 3), name)
        slots = kps = None
        if what == 'pj2d':
            kps = out.get(kps_key)
            if kps is None:
                raise ValueError('out holds no %s (forward(..., project=True%s))' %
                                 (kps_key, ', offsets=offsets' if kps_key == 'pj2d_org' else ''))
            if tuple(kps.shape) != (n, 2, 21, 2) or tuple(out['slots'].shape) != (n, 2, _lib.SLOT):
                raise ValueError('out does not hold the results of %d %s' % (n, 'frames' if region_frame is None else 'regions'))
            kps, slots = kps.contiguous(), out['slots'].contiguous()
            mode, outs = _lib.OVERLAY_SKELETON, (_ptr(dst), None)
        else:
            mode, outs = _lib.OVERLAY_CENTERMAP, (_ptr(dst[0]), _ptr(dst[1]))
        if region_frame is None:
            _lib.check(self.L.acrmi_overlay(self.ctx, mode, _ptr(slots), _ptr(kps), n, _ptr(offsets), int(bool(bgr)), _ptr(src), *outs,
                                            H, W, st), self.ctx)
        else:
            _lib.check(self.L.acrmi_overlay_regions(self.ctx, mode, _ptr(slots), _ptr(kps), n, _ptr(offsets), _ptr(region_frame),
                                                    int(bool(bgr)), _ptr(src), *outs, N, H, W, st), self.ctx)
        self._overlay_keep = (slots, kps, offsets, region_frame, src)      # referenced until the next call has been queued
        return dst

    def render(self, out, images, offsets=None, cam_trans=None, focal_length=1265., visible_weight=0.9, colors=None,
               bgr=False, dst=None, return_ids=False, stream=None, vertex_colors=None):
        """The hands of `out` (what `forward(..., project=True)` returned: slots, verts, joints, pj2d) drawn over `images`
        (acrmi_render; the reference's Visualizer 'mesh' view, acr/visualization.py:100-218, conventions in DESIGN.md
        "Rendering").  images uint8 [B,H,W,3] on the device: the 512 x 512 network input when offsets is None, else the
        original frames the `offsets` rows [B,10] describe (the mesh lands on pj2d / pj2d_org).  A hand is drawn when its
        slot's flag is set.  cam_trans [B,2,3]: computed from out['joints'] / out['pj2d'] (acrmi_cam_trans) when None.
        colors [2,3] left / right in the images' channel order (default: the reference's, RGB or - bgr=True - BGR).
        dst: uint8 tensor like images to draw into (may be `images` itself: in place).  Returns the frames, or (frames,
        ids int32 [B,H,W] = (2 * frame + hand) * F + face, -1 where no hand is) with return_ids.  stream: as `forward`.
        vertex_colors [B,2,778,3] device fp32 (contact_colors / error_colors / ops.vertex_colors): a base colour per vertex in
        the images' channel order instead of `colors` (acrmi_render_colored)."""
        src = self._check_frames(images, 'images', 'B')
        B = src.shape[0]
        if tuple(out['verts'].shape) != (B, 2, 778, 3) or tuple(out['slots'].shape) != (B, 2, _lib.SLOT):
            raise ValueError('out does not hold the results of %d frames' % B)
        return self._render(out, src, B, 'images', self._frame_offsets(offsets, B), None, cam_trans, focal_length, visible_weight,
                            colors, bgr, dst, return_ids, stream, vertex_colors)

    def overlay(self, out, images, what, offsets=None, bgr=False, dst=None, stream=None):
        """The reference's other two views of a result over `images` (acrmi_overlay; acr/visualization.py:228-300, rules in
        DESIGN.md "Key-point and heat-map views").  `out`: what `forward(..., project=True)` returned; images uint8 [B,H,W,3]
        on the device - the 512 x 512 network input when offsets is None, else the original frames the `offsets` rows
        [B,10] describe.  what = 'pj2d': the 21 projected key points of every flagged hand as a coloured skeleton, at
        (pj2d + 1) / 2 * 512, respectively at pj2d_org -> uint8 [B,H,W,3].  what = 'centermap': the left and right centre
        maps of the LAST program run of this context (it must be the forward that produced `out`) in false colour at
        weight 0.7 -> uint8 [2,B,H,W,3] (left, right).  bgr: the images' channel order.  dst: tensor to draw into, shaped
        like the result ('pj2d': may be `images` itself).  stream: as `forward`."""
        src = self._check_frames(images, 'images', 'B')
        B = src.shape[0]
        return self._overlay(out, src, B, 'images', what, 'pj2d' if offsets is None else 'pj2d_org', self._frame_offsets(offsets, B),
                             None, bgr, dst, stream)

    def contact(self, out, max_hand=1, cam_trans=None, contact_dist=None, max_depth=None, focal_length=1265., stream=None,
                mode='vertex'):
        """Contact and interpenetration between the left and the right hands of every row of `out` (what `forward(...,
        project=True[, max_hand=K])` returned) on the GPU (acrmi_contact): the nearest-vertex half-space
        heuristic - not a point-to-triangle distance, not a true inside test - on the two meshes placed by their cam_trans,
        so it is only as good as those two independent fits.  Pairs are formed inside a row only: with regions (boxes=) every
        region has its own camera, and hands of different regions are never paired.
        max_hand = K: the K the forward ran with; pair (b*K + i)*K + j is (left rank i, right rank j) of row b, skipped when
        either hand's flag is not set (read on the device: nothing here waits for it).  cam_trans [B,(K,)2,3]: as `render`
        obtains it - the caller's, out['cam_trans'], or computed from out['joints'] / out['pj2d'].  contact_dist / max_depth:
        metres, defaults ops.CONTACT_DIST / ops.CONTACT_MAX_DEPTH (parameters, not measurements).  The orientation signs:
        `contact_sign` / set_contact_sign.  Returns what ops.mesh_contact returns, for the B*K*K pairs; direction 0 = the left
        hand's vertices.  stream: as `forward`.
        mode='surface' (acrmi_surface_contact): the same pairs by the surface measure - the distance
        from every vertex to the other hand's surface, the point on it, and containment by ray crossings - and what
        ops.mesh_surface_contact returns.  It has no orientation sign.  Any other mode is a ValueError."""
        if mode not in ('vertex', 'surface'):
            raise ValueError("mode must be 'vertex' or 'surface', not %r" % (mode,))
        K = check_max_hand(max_hand)
        slots = out['slots']
        B = slots.shape[0]
        lead = tuple(slots.shape[:-1])
        if lead not in ((B, K, 2),) + (((B, 2),) if K == 1 else ()) or tuple(out['verts'].shape) != lead + (778, 3):
            raise ValueError('out does not hold %d rows of %d hand pairs' % (B, K))
        contact_dist, max_depth = ops_mod.check_contact_params(ops_mod.CONTACT_DIST if contact_dist is None else contact_dist,
                                                               ops_mod.CONTACT_MAX_DEPTH if max_depth is None else max_depth)
        st = _stream(self.device) if stream is None else C.c_void_p(stream)
        flat = out if len(lead) == 2 else {k: out[k].flatten(0, 1) for k in ('joints', 'pj2d', 'cam_trans') if out.get(k) is not None}
        if cam_trans is not None:
            cam_trans = cam_trans.reshape(B * K, 2, 3)
        cam_trans = self._cam_trans(flat, cam_trans, B * K, focal_length, st)
        verts, slots = out['verts'].contiguous(), slots.contiguous()
        m = ops_mod.CONTACT_MEASURES[mode]
        raw = ops_mod.measure_outputs(m, B * K * K, 778, self.device)
        sign = None if self._contact_sign_set is None else (C.c_int32 * 2)(*self._contact_sign_set)
        _lib.check(getattr(self.L, m['ctx'])(self.ctx, _ptr(verts), _ptr(cam_trans), _ptr(slots), B, K, *((sign,) if m['sign'] else ()),
                                             contact_dist, max_depth, *[_ptr(x) for x in raw.values()], st), self.ctx)
        self._contact_keep = (verts, slots, cam_trans)      # referenced until the next call has been queued
        return ops_mod.measure_result(m, raw)

    def score(self, out, gt, board=None, max_hand=1, cam_trans=None, focal_length=1265., n_groups=None, stream=None):
        """Scores the hands of `out` (what `forward(..., project=True[, max_hand=K])` returned) against ground truth on the GPU
        (acrmi_score_hands).  gt: {'joints': [B,(K,)2,21,3], 'verts': [B,(K,)2,778,3] (optional),
        'joint_valid': [B,(K,)2,21] (optional), 'group': int32 [B,(K,)2] (optional, default the side: 0 left, 1 right)}, device
        tensors in metres, in the frame of out['joints'].  A row is a hand: scored where its slot's flag is set (read on the
        device), a miss where it is not, not looked at where its group is outside [0, n_groups).  The joints are aligned on the
        context's centre joint (set_center_idx), the vertices on the same joint; Procrustes alignment is per point set.
        cam_trans [B,(K,)2,3]: as `contact` obtains it; the absolute root error and the MRRPE terms of the pairs (left rank k,
        right rank k) need it.  board: a ScoreBoard of the default point sets to add the batch to (n_groups is then the
        board's).  Nothing waits for the host.  Returns {'joints': what ops.pose_errors returns over the B*K*2 rows, 'verts':
        the same or None, 'pair_err': [B*K]}.  stream: as `forward`."""
        K = check_max_hand(max_hand)
        slots = out['slots']
        B = slots.shape[0]
        lead = tuple(slots.shape[:-1])
        if lead not in ((B, K, 2),) + (((B, 2),) if K == 1 else ()) or tuple(out['joints'].shape) != lead + (21, 3):
            raise ValueError('out does not hold %d rows of %d hand pairs' % (B, K))
        if board is not None:
            if board.sets != (21, 778) or board.device != self.device:
                raise ValueError('board must be a ScoreBoard of sets (21, 778) on %s' % (self.device,))
            if n_groups is not None and int(n_groups) != board.n_groups:
                raise ValueError('the board has %d groups (n_groups=%d)' % (board.n_groups, n_groups))
        G = board.n_groups if board is not None else (2 if n_groups is None else int(n_groups))
        N, dev = B * K * 2, self.device
        truth = score_truth(gt, lead, dev)
        gj, gv, jv, gr = (truth[k] for k in ('joints', 'verts', 'joint_valid', 'group'))
        st = _stream(dev) if stream is None else C.c_void_p(stream)
        tst = torch.cuda.current_stream(dev) if stream is None else torch.cuda.ExternalStream(stream, device=dev)
        flat = out if len(lead) == 2 else {k: out[k].flatten(0, 1) for k in ('joints', 'pj2d', 'cam_trans') if out.get(k) is not None}
        if cam_trans is not None:
            cam_trans = cam_trans.reshape(B * K, 2, 3)
        if cam_trans is not None or out.get('cam_trans') is not None or out.get('pj2d') is not None:
            cam_trans = self._cam_trans(flat, cam_trans, B * K, focal_length, st)
        joints, slots = out['joints'].contiguous(), slots.contiguous()
        verts = out['verts'].contiguous() if gv is not None else None
        rj = ops_mod.score_outputs(N, 21, dev, pairs=True)
        rv = ops_mod.score_outputs(N, 778, dev) if gv is not None else None
        if board is not None:
            board.order_on(tst)
        _lib.check(self.L.acrmi_score_hands(
            self.ctx, _ptr(joints), _ptr(verts), _ptr(slots), _ptr(cam_trans), _ptr(gj), _ptr(gv), _ptr(jv), _ptr(gr), B, K, G,
            board.n_bins if board is not None else 1, board.bin_width if board is not None else 1.0,
            _ptr(board.words) if board is not None else None, *[_ptr(rj[k]) for k in ('e_ra', 'e_pa', 'row_f', 'row_i')],
            *[_ptr(rv[k]) if rv is not None else None for k in ('e_ra', 'e_pa', 'row_f', 'row_i')], _ptr(rj['pair_err']), st), self.ctx)
        if board is not None:
            board.touched_on(tst)
        self._score_keep = (joints, verts, slots, cam_trans, gj, gv, jv, gr)      # referenced until the next call has been queued
        return {'joints': ops_mod.score_result(rj), 'verts': None if rv is None else ops_mod.score_result(rv),
                'pair_err': rj['pair_err']}

    def match(self, out, gt, on='pj2d_org', gate=float('inf'), min_points=1, max_hand=1, cam_trans=None, board=None,
              focal_length=1265., stream=None):
        """Matches the hands of `out` (what `forward(..., project=True[, max_hand=K])` returned) to ground truth on the GPU and
        brings them into truth order (acrmi_match_hands, acrmi_match_gather).  gt: what `score` takes,
        with leading [B,G,2] for any G in 1..8, and two more optional keys: 'kp2d' [B,G,2,21,2] in the units of out[on] (on =
        'pj2d_org' / 'pj2d'), 'valid' [B,G,2] (non-zero = the annotated hand exists).  on='joints' compares out['joints'] +
        cam_trans (as `score` obtains it) with gt['joints'], the frame `score`'s absolute root error assumes.  A prediction is
        looked at where its slot's flag is set (read on the device); gt['joint_valid'] says which points count.  gate: the
        largest mean distance of an allowed pair (pixels, normalized units or metres), min_points: the fewest counted points of
        one - parameters, not measurements.  board: a MatchBoard to add the batch to.  Nothing waits for the host.  Returns
        {'match' int32 [B,K,2], 'pred_of' int32 [B,G,2], 'cost' [B,K,2], 'counts' int32 [B,2,3], 'group' int32 [B,G,2], 'out':
        the slots, joints, verts, cam_trans and pj2d* of `out` as [B,G,2,...] rows in truth order (zeros where a truth has no
        prediction), 'gt': gt with 'group' replaced - ready for score(res['out'], res['gt'], max_hand=G)}.  stream: as
        `forward`."""
        K = check_max_hand(max_hand)
        if on not in match_mod.ON_KEYS:
            raise ValueError('on must be one of %s, not %r' % (', '.join(match_mod.ON_KEYS), on))
        slots = out['slots']
        B = slots.shape[0]
        lead = tuple(slots.shape[:-1])
        if lead not in ((B, K, 2),) + (((B, 2),) if K == 1 else ()) or out.get(on) is None:
            raise ValueError('out does not hold %d rows of %d hand pairs with %r' % (B, K, on))
        dev = self.device
        G, truth = match_truth(gt, on, B, dev)
        D = 3 if on == 'joints' else 2
        gate, min_points = ops_mod.check_match_params(gate, min_points, 21)
        if board is not None and (not isinstance(board, MatchBoard) or board.device != dev):
            raise ValueError('board must be a MatchBoard on %s' % (dev,))
        st = _stream(dev) if stream is None else C.c_void_p(stream)
        tst = torch.cuda.current_stream(dev) if stream is None else torch.cuda.ExternalStream(stream, device=dev)
        trans = None
        if on == 'joints' or cam_trans is not None:
            flat = out if len(lead) == 2 else {k: out[k].flatten(0, 1) for k in ('joints', 'pj2d', 'cam_trans') if out.get(k) is not None}
            if cam_trans is not None:
                cam_trans = cam_trans.reshape(B * K, 2, 3)
            if cam_trans is not None or out.get('cam_trans') is not None or out.get('pj2d') is not None:
                cam_trans = self._cam_trans(flat, cam_trans, B * K, focal_length, st).view(B, K, 2, 3)
            trans = cam_trans if on == 'joints' else None
        slots = slots.contiguous().view(B, K, 2, _lib.SLOT)
        pred = out[on].contiguous()
        if tuple(pred.shape) != lead + (21, D) or pred.dtype != torch.float32:
            raise ValueError("out['%s'] must be fp32 %s" % (on, list(lead + (21, D))))
        raw = ops_mod.match_outputs(B, K, G, dev)
        if board is not None:
            board.order_on(tst)
        _lib.check(self.L.acrmi_match_hands(
            _ptr(pred), _ptr(truth['points']), _ptr(truth['joint_valid']), _ptr(truth['valid']),
            C.c_void_p(slots.data_ptr() + 4 * _lib.SLOT_FLAG), _lib.SLOT, _ptr(trans), _ptr(truth['group']), B, K, G, 21, D, gate,
            min_points, *[_ptr(raw[k]) for k in ('match', 'pred_of', 'cost', 'counts', 'group')], st))
        if board is not None:
            _lib.check(self.L.acrmi_match_accumulate(_ptr(raw['counts']), _ptr(raw['cost']), B, K, _ptr(board.words), st))
            board.touched_on(tst)
        rows, kept = {}, [slots, pred, trans, truth]
        for key in MATCH_GATHERED:
            src = cam_trans if key == 'cam_trans' and cam_trans is not None else out.get(key)
            if src is None:
                continue
            src = src.to(dev, torch.float32).contiguous().view((B, K, 2) + tuple(src.shape[len(lead):]))
            dst = torch.empty((B, G, 2) + tuple(src.shape[3:]), dtype=torch.float32, device=dev)
            _lib.check(self.L.acrmi_match_gather(_ptr(src), _ptr(raw['pred_of']), B, K, G, int(np.prod(src.shape[3:], dtype=np.int64)),
                                                 _ptr(dst), st))
            rows[key] = dst
            kept.append(src)
        self._match_keep = tuple(kept)      # referenced until the next call has been queued
        res = dict(raw)
        res['out'] = rows
        res['gt'] = dict(gt, group=raw['group'])
        return res

    def _regions(self, images, offsets, region_frame, n):
        """images, offsets [n,10], region_frame [n] of the calls over regions, checked without reading device memory ->
        (src, offsets, region_frame) on the device."""
        src = self._check_frames(images, 'frames', 'N')
        _, o, rf = ops_mod.check_regions(offsets, region_frame, n)
        return src, o.to(self.device, torch.float32).contiguous(), rf.to(self.device, torch.int32).contiguous()

    def render_regions(self, out, frames, offsets, region_frame, cam_trans=None, focal_length=1265., visible_weight=0.9,
                       colors=None, bgr=False, dst=None, return_ids=False, stream=None, vertex_colors=None):
        """`render` for the results of a forward on n REGIONS of interest (acrmi_render_regions; DESIGN.md "Views over
        regions"): the hands of region i are drawn into frame region_frame[i] of `frames` (uint8 [N,H,W,3] on the device),
        mapped by the view of ITS `offsets` row; all hands of all regions of a frame go through one depth-tested pass.
        offsets [n,10] and region_frame [n] may be device tensors (out['offsets'] of track_step is one): the kernels read
        them, nothing here waits for the device.  A region whose window has no pixel, whose scale is not > 0 or whose
        frame index is outside [0, N) draws nothing.  The other arguments as `render` (vertex_colors [n,2,778,3]:
        acrmi_render_regions_colored); ids = (2 * region + hand) * F + face."""
        n = out['slots'].shape[0]
        if tuple(out['verts'].shape) != (n, 2, 778, 3) or tuple(out['slots'].shape) != (n, 2, _lib.SLOT):
            raise ValueError('out does not hold the results of %d regions' % n)
        src, offsets, region_frame = self._regions(frames, offsets, region_frame, n)
        return self._render(out, src, n, 'frames', offsets, region_frame, cam_trans, focal_length, visible_weight, colors, bgr, dst,
                            return_ids, stream, vertex_colors)

    # ---- per-vertex colours: the contact and error views -----------------------------------------------
    def _hand_base(self, lead, colors, bgr, tst):
        """The flat colours `render` would give the hands of `lead` = (B,(K,)2) -> [hands,3] on the device, on torch stream tst."""
        col = self._colors(colors, bgr)
        col = np.asarray(HAND_COLORS_RGB, np.float32) if col is None else col
        cache = self.__dict__.setdefault('_hand_base_cache', {})
        pair = cache.get(col.tobytes())
        if pair is None:      # six scalar fills, once per pair of colours: no copy from the host, so nothing waits for it
            if len(cache) >= 16:
                cache.clear()
            with torch.cuda.stream(tst):
                pair = torch.empty(2, 3, dtype=torch.float32, device=self.device)
                for h in range(2):
                    for c in range(3):
                        pair[h, c] = float(col[h, c])
            cache[col.tobytes()] = pair
        with torch.cuda.stream(tst):
            return pair.repeat(int(np.prod(lead[:-1])), 1)

    def _lead(self, out, K):
        slots = out['slots']
        B = slots.shape[0]
        lead = tuple(slots.shape[:-1])
        if lead not in ((B, K, 2),) + (((B, 2),) if K == 1 else ()):
            raise ValueError('out does not hold %d rows of %d hand pairs' % (B, K))
        return B, lead

    def contact_colors(self, con, out, max_hand=1, far=0.02, max_depth=None, colors=None, bgr=False, flag_color=ops_mod.FLAG_COLOR,
                       lut=None, stream=None):
        """What `contact(out, max_hand=K[, mode=])` returned -> a colour per vertex for `render(..., vertex_colors=)`, on the GPU
        (acrmi_contact_values + acrmi_vertex_colors): every vertex by its distance to the nearest hand of
        the OTHER side in its row, near is hot (the default jet reversed: 0 m red, `far` and beyond blue); a vertex inside the
        other hand (the measure's own rule, within max_depth - default ops.CONTACT_MAX_DEPTH) takes flag_color; a hand without
        a computed pair keeps the flat colour `render` gives it (colors / bgr as there).  far = 0.02 m is a PARAMETER of the
        picture, not a measurement.  Returns fp32 [B,(K,)2,778,3] shaped like out['slots']; nothing waits for the host."""
        K = check_max_hand(max_hand)
        B, lead = self._lead(out, K)
        lo, hi = ops_mod.check_color_range(0.0, far)
        tst = torch.cuda.current_stream(self.device) if stream is None else torch.cuda.ExternalStream(stream, device=self.device)
        st = tst.cuda_stream
        cv = ops_mod.contact_values(con, B, K, max_depth=max_depth, stream=st)
        V = cv['value'].shape[-1]
        vcol = ops_mod.vertex_colors(cv['value'].view(-1, V), lo, hi, flags=cv['flag'].view(-1, V), base=self._hand_base(lead, colors, bgr, tst),
                                     flag_color=flag_color, lut=lut, reverse=True, bgr=bgr, stream=st)
        return vcol.view(*lead, V, 3)

    def error_colors(self, sc, out, max_hand=1, kind='ra', hi=0.02, colors=None, bgr=False, lut=None, stream=None):
        """What `score(out, gt, max_hand=K)` returned (gt with 'verts') -> a colour per vertex for `render(..., vertex_colors=)`
        (acrmi_vertex_colors): every vertex by its error against truth, kind='ra' root-aligned, 'pa'
        Procrustes-aligned - 0 m blue, `hi` and beyond red (the default jet).  A hand that scoring did not count, and a
        vertex without an error, keeps the flat colour `render` gives it (colors / bgr as there): its -1 becomes NaN by a torch
        operation on the device.  hi = 0.02 m is a PARAMETER of the picture, not a measurement.  Returns fp32
        [B,(K,)2,778,3] shaped like out['slots']; nothing waits for the host."""
        if kind not in ('ra', 'pa'):
            raise ValueError("kind must be 'ra' or 'pa', not %r" % (kind,))
        K = check_max_hand(max_hand)
        B, lead = self._lead(out, K)
        if not isinstance(sc, dict) or sc.get('verts') is None:
            raise ValueError("sc holds no per-vertex errors: score(out, gt) with gt['verts']")
        e = sc['verts']['e_' + kind]
        if tuple(e.shape) != (B * K * 2, 778) or not e.is_cuda:
            raise ValueError('sc does not hold the scores of %d rows of %d hand pairs' % (B, K))
        lo, hi = ops_mod.check_color_range(0.0, hi)
        tst = torch.cuda.current_stream(self.device) if stream is None else torch.cuda.ExternalStream(stream, device=self.device)
        with torch.cuda.stream(tst):
            values = e.masked_fill(e < 0, float('nan'))
        vcol = ops_mod.vertex_colors(values, lo, hi, base=self._hand_base(lead, colors, bgr, tst), lut=lut, bgr=bgr, stream=tst.cuda_stream)
        return vcol.view(*lead, 778, 3)

    def overlay_regions(self, out, frames, what, offsets, region_frame, bgr=False, dst=None, stream=None):
        """`overlay` for the results of a forward on n REGIONS (acrmi_overlay_regions; DESIGN.md "Views over regions").
        what = 'pj2d': the skeletons of every flagged hand at out['pj2d_org'], hand h of region i into frame region_frame[i]
        -> uint8 [N,H,W,3].  what = 'centermap': the centre maps of the LAST program run of this context (the forward on
        these n regions), region i tinting the pixels of its window; where windows overlap the larger colour index wins ->
        uint8 [2,N,H,W,3].  offsets, region_frame: as `render_regions`; the other arguments as `overlay`."""
        n = out['slots'].shape[0]
        src, offsets, region_frame = self._regions(frames, offsets, region_frame, n)
        return self._overlay(out, src, n, 'frames', what, 'pj2d_org', offsets, region_frame, bgr, dst, stream)

    # ---- the part segmentation as an output -------------------------------------------------------------
    def segment(self, out_or_B, images=None, offsets=None, bgr=False, dst=None, labels=True, stats=False, ids=None, stream=None,
                weight=0.7, colors=None, draw=True):
        """The hand-part segmentation of the LAST program run of this context (it must be the forward that produced `out`) as
        labels, as a view, and as mask statistics (acrmi_segment + acrmi_segm_stats).  out_or_B: what
        `forward` returned, or its batch size.  images uint8 [B,H,W,3] on the device: the frames the labels are made for and the
        view is drawn over - the 512 x 512 network input when offsets is None, else the original frames the `offsets` rows
        [B,10] describe; without images the labels are 512 x 512 under the identity view.  Returns a dict of device tensors:
        'labels' uint8 [B,H,W] (labels=True, or with stats) - 0 background, 1..16 the right hand's parts, 17..32 the left
        hand's, 255 where the canvas does not cover the frame; 'view' uint8 [B,H,W,3] (with images; dst: tensor to draw
        into, may be `images`; bgr, weight, colors [33,3]: as ops.draw_segm); with stats=True 'counts' int32 [B,33] and 'boxes'
        int32 [B,2,4] (ops.segm_stats), and with ids - int32 [B,H,W] of `render(..., return_ids=True)` over the same frames -
        'agree' int32 [B,2,3] = (intersection, mask, silhouette) per side.  draw=False: `images` only say which frames the labels
        are made for, no view is drawn.  The map has no instances: with max_hand > 1 the hands of a side share its mask.
        stream: as `forward`.  Nothing waits for the host."""
        B = int(out_or_B['slots'].shape[0]) if isinstance(out_or_B, dict) else int(out_or_B)
        if ids is not None and not stats:
            raise ValueError('ids= is compared with the masks by stats=True')
        src = None
        H = W = 512
        if images is not None:
            src = self._check_frames(images, 'images', 'B')
            if src.shape[0] != B:
                raise ValueError('images must hold the %d frames of the batch' % B)
            H, W = src.shape[1:3]
        if dst is not None and (images is None or not draw):
            raise ValueError('dst is the view drawn over images=')
        if not (labels or stats or (images is not None and draw)):
            raise ValueError('nothing to make: labels=False and stats=False without a view to draw')
        offsets = self._frame_offsets(offsets, B)
        if ids is not None and (ids.dtype != torch.int32 or tuple(ids.shape) != (B, H, W) or not ids.is_cuda):
            raise ValueError('ids must be int32 [%d,%d,%d] on the device' % (B, H, W))
        tab = None
        if colors is not None:
            tab = np.ascontiguousarray(np.asarray(colors.cpu() if hasattr(colors, 'cpu') else colors))
            if tab.shape != (33, 3) or tab.dtype != np.uint8:
                raise ValueError('colors must be uint8 [33,3]')
        tst = torch.cuda.current_stream(self.device) if stream is None else torch.cuda.ExternalStream(stream, device=self.device)
        res = {}
        with torch.cuda.stream(tst):
            if src is not None and draw:
                res['view'] = self._dst(dst, src, (B, H, W, 3), 'images')
            if labels or stats:
                res['labels'] = torch.empty(B, H, W, dtype=torch.uint8, device=self.device)
        _lib.check(self.L.acrmi_segment(self.ctx, B, _ptr(offsets), float(weight), None if tab is None else tab.ctypes.data_as(C.c_void_p),
                                        int(bool(bgr)), _ptr(src) if draw else None, _ptr(res.get('view')), _ptr(res.get('labels')), H, W,
                                        C.c_void_p(tst.cuda_stream)), self.ctx)
        if stats:
            n_faces = None
            if ids is not None:
                if self._faces.get('left') is None:
                    raise _lib.AcrmiError('ids= needs the MANO faces the ids were rendered with (load_faces)')
                n_faces = self._faces['left'].shape[0]
            with torch.cuda.stream(tst):
                res.update(ops_mod.segm_stats(res['labels'], 33, ids=ids, n_faces=n_faces, stream=tst.cuda_stream))
        self._segment_keep = (offsets, src, ids, dict(res))      # referenced until the next call has been queued
        if not labels:
            res.pop('labels', None)
        return res


    def profile_ops(self, img):
        img = self._check_img(img)
        B = img.shape[0]
        self.ensure_batch(B)
        n = len(self.program['ops'])
        ms = (C.c_float * n)()
        _lib.check(self.L.acrmi_profile_ops(self.ctx, _ptr(img), B, ms, n, _stream(self.device)), self.ctx)
        ops = self.program['ops']
        return [dict(info, ms=float(ms[i]), idx=i, ksize=int(ops[i].ksize), stride=int(ops[i].stride))
                for i, info in enumerate(self.program['op_info'])]


class EnginePool(object):
    """n contexts on ONE GPU that take batches in turn, each on its own HIP stream (serving throughput).

    A batch ends in a tail of kernels with few work items (attention pooling, the per-frame pare bias, decode, MANO: ~1
    ms at batch 64) and the next one starts with pipeline fill; on one stream the 256 CUs idle through both.  With two
    independent program instances in flight the hardware scheduler fills those gaps with the other batch's kernels:
    39.8 -> 39.0 ms per batch of 64 (1607 -> 1642 frames/s), and the parallel lanes inside a context are no longer
    needed (1 lane per context measured best).  Every batch is computed by one context exactly as Engine.forward does
    (bit-identical results, tests/test_gpu_api.py); the price is a second set of activations (9.9 GB at batch 64 of the
    288 GB) and one more batch of latency.  The reference has no counterpart (one nn.Module call per image,
    acr/main.py:92-96).  A non-Python host does the same with two acrmi_ctx and two streams.

        pool = EnginePool(0, n=2); pool.load_state_dict(sd, max_batch=64); pool.load_mano(tables)
        t = pool.submit(frames)          # queued on the context's stream, behind the caller's current stream
        out = pool.collect(t)            # the caller's current stream waits for that batch; dict of device tensors
    At most n tickets may be outstanding.
    The contexts run on plain HIP streams of the library (acrmi_stream_create): torch.cuda.Stream() would instantiate
    torch's whole stream pool, and with that many streams alive the few in use share hardware queues."""

    def __init__(self, device=0, n=2, first=None):
        """first: an existing Engine to use as context 0 (its program, if loaded, is shared with the others)."""
        if n < 1:
            raise ValueError('n must be >= 1')
        self.engines = ([first] if first is not None else []) + [Engine(device) for _ in range(n - (first is not None))]
        self.device = self.engines[0].device
        # plain HIP streams from the library (acrmi_stream_create), seen by torch as external streams
        self._raw = []
        for _ in range(n):
            st = C.c_void_p()
            _lib.check(self.engines[0].L.acrmi_stream_create(self.device.index, C.byref(st)))
            self._raw.append(st)
        self.streams = [torch.cuda.ExternalStream(st.value, device=self.device) for st in self._raw]
        self._turn = 0
        self._busy = [None] * n
        self._inflight = []      # released tickets whose batch may still be running: their tensors stay referenced
        self.table = None        # stream_table(): the One-Euro state the contexts share
        self.tracks = None       # track_table(): the tracks the contexts share

    def __len__(self):
        return len(self.engines)

    def close(self, keep_first=False):
        """Releases the streams and the contexts (keep_first: all but context 0, e.g. an Engine passed as `first`)."""
        if self._raw:
            with torch.cuda.device(self.device):
                torch.cuda.synchronize()
            self._inflight = []          # every batch has run: the tensors the tickets kept alive may go
            if self.table is not None:
                self.table.close()
                self.table = None
            if self.tracks is not None:
                self.tracks.close()
                self.tracks = None
            self.streams = []
            L = _lib.lib()
            for st in self._raw:
                L.acrmi_stream_destroy(st)
            self._raw = []
        for e in self.engines[1 if keep_first else 0:]:
            e.close()
        self.engines = []      # (keep_first: context 0 stays open and belongs to whoever passed it in)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_state_dict(self, sd, max_batch=1, lanes=1, precision='fp32', wino24='auto'):
        """sd = None: share the program context 0 already holds.  wino24 as Engine.load_state_dict (the same
        checkpoint at the same max_batch lowers to the same program on an Engine and on a pool: bit-equal results)."""
        if wino24 == 'auto':
            wino24 = None if max_batch >= 16 else False
        prog = self.engines[0].program if sd is None else packer.lower(sd, precision=precision, wino24=wino24,
                                                                       splitk=max_batch < 16)
        if prog is None:
            raise _lib.AcrmiError('no checkpoint loaded')
        holder = next((e for e in self.engines if e.program is prog), None)      # a context that already holds the blob
        for e in self.engines:
            if e.program is not prog:
                e.load_program(prog, max_batch, share_with=holder)      # one device copy of the weights for the pool
                holder = holder or e
            else:
                e.ensure_batch(max_batch)
            e.set_lanes(lanes)

    def load_mano(self, tables=None):
        """tables = None: context 0's tables."""
        for e in self.engines:
            if tables is not None:
                e.load_mano(tables)
            elif e is not self.engines[0]:
                for name, t in self.engines[0]._mano_tables.items():
                    e.load_mano_side(name, t)

    def configure(self, fn):
        """fn(engine) on every context (options: set_conf_thresh, set_center_idx, set_point_heads, ...)."""
        for e in self.engines:
            fn(e)

    def stream_table(self, capacity):
        """The pool's StreamTable (created on the first call): ONE table for all contexts, so a video stream's state follows
        its frames to whichever context takes the batch; the library applies the updates in the order of the submits."""
        if self.table is None:
            self.table = StreamTable(self.device, capacity)
        elif self.table.capacity != int(capacity):
            raise ValueError('the pool holds a table of %d streams (asked for %d)' % (self.table.capacity, int(capacity)))
        return self.table

    def track_table(self, capacity, max_hand, gate=8, max_miss=5):
        """The pool's TrackTable (created on the first call): ONE table for all contexts, as stream_table()."""
        want = (int(capacity), int(max_hand), int(gate), int(max_miss))
        if self.tracks is None:
            self.tracks = TrackTable(self.device, *want)
        elif (self.tracks.capacity, self.tracks.max_hand, self.tracks.gate, self.tracks.max_miss) != want:
            raise ValueError('the pool holds a track table of (capacity, max_hand, gate, max_miss) = %s (asked for %s)' % (
                (self.tracks.capacity, self.tracks.max_hand, self.tracks.gate, self.tracks.max_miss), want))
        return self.tracks

    def submit(self, img, offsets=None, project=False, out=None, streams=None, max_hand=1, tracks=None, smooth=True):
        """streams: the video stream of each frame (Engine.forward's `streams=`, on the pool's stream_table());
        max_hand: Engine.forward's; tracks / smooth: Engine.forward's `tracks=` on the pool's track_table()."""
        max_hand = check_max_hand(max_hand)
        if tracks is not None:      # (checked before the turn moves on)
            if self.tracks is None:
                raise ValueError('tracks= needs the pool\'s table: call track_table(capacity, max_hand) first')
            tracks = track_args(tracks, self.tracks, streams, None, max_hand, img.shape[0])
        if max_hand > 1 and streams is not None:
            raise ValueError('streams= follows one hand of each side through a video: not with max_hand=%d' % max_hand)
        if streams is not None and self.table is None:
            raise ValueError('streams= needs the pool\'s table: call stream_table(capacity) first')
        if streams is not None:      # (checked before the turn moves on)
            streams = stream_ids(streams, img.shape[0])
        i = self._turn
        if self._busy[i] is not None:
            raise RuntimeError('collect() the ticket submitted %d calls ago first' % len(self.engines))
        self._turn = (i + 1) % len(self.engines)
        # host-side conversions run on the caller's stream: they must be queued before `ready` is recorded
        img = self.engines[i]._check_img(img)
        if offsets is not None:
            offsets = offsets.to(self.device, torch.float32).contiguous()
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))   # the frames (and the out tensors) as the caller left them
        st = self.streams[i]
        st.wait_event(ready)
        # (no `with torch.cuda.stream(st)`: tensors must not come from the caching allocator's pool of a stream that
        # close() destroys; everything this call allocates belongs to the caller's stream, which collect() orders behind
        # the batch)
        table = self.table if streams is not None else None
        res = self.engines[i].forward(img, offsets=offsets, project=project, out=out, stream=self._raw[i].value,
                                      streams=streams, table=table, max_hand=max_hand, tracks=tracks,
                                      track_table=self.tracks if tracks is not None else None, smooth=smooth)
        done = torch.cuda.Event()
        done.record(st)
        # Everything the batch reads or writes stays referenced by the ticket until its event has completed: the call
        # runs on the pool's stream, so torch's caching allocator (which only knows the caller's stream) would hand a
        # dropped `img` / `offsets` block to the caller's next allocation while the kernels still read it.
        ticket = {'slot': i, 'event': done, 'out': res, 'img': img, 'offsets': offsets, 'table': table, 'tracks': self.tracks}
        self._busy[i] = ticket
        return ticket

    def _on_ticket(self, ticket, name, prepare, call, keep=None, caller_waits=False):
        """One more call on the ticket's batch, on the ticket's stream behind its forward and behind what the caller's
        current stream holds now.  prepare(engine) -> the tensors the call takes: the host-side conversions, which run on
        the caller's stream and so must be queued before `ready` is recorded; call(engine, raw stream, tensors) -> the
        result; keep: the Engine attribute that names what else the call touched.  collect() then also orders the caller's
        stream behind this call; caller_waits: it is made to wait for it now, on the device."""
        i = ticket['slot']
        if self._busy[i] is not ticket:
            raise RuntimeError('%s() belongs between submit() and collect() of its ticket' % name)
        eng = self.engines[i]
        tensors = prepare(eng)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))
        self.streams[i].wait_event(ready)
        res = call(eng, self._raw[i].value, tensors)
        done = torch.cuda.Event()
        done.record(self.streams[i])
        if caller_waits:
            torch.cuda.current_stream(self.device).wait_event(done)
        # as in submit: everything the call touches stays referenced by the ticket until its event has completed - appended,
        # so that a second call on the ticket does not drop what the kernels of the first may still be reading
        ticket['event'] = done
        ticket.setdefault('kept', []).append((res, tensors, getattr(eng, keep) if keep else None))
        return res

    def _view(self, ticket, name, keep, prepare, **kw):
        """Engine.<name> of the ticket's batch over the frames prepare() returns (as keyword arguments)."""
        return self._on_ticket(ticket, name, prepare, keep=keep,
                               call=lambda eng, raw, frames: getattr(eng, name)(ticket['out'], stream=raw, **frames, **kw))

    def _frames(self, images, offsets):
        def prepare(eng):
            return {'images': images.contiguous(),
                    'offsets': None if offsets is None else offsets.to(self.device, torch.float32).contiguous()}
        return prepare

    @staticmethod
    def _region_frames(ticket, frames, offsets, region_frame):
        def prepare(eng):
            f, o, rf = eng._regions(frames, offsets, region_frame, ticket['out']['slots'].shape[0])
            return {'frames': f, 'offsets': o, 'region_frame': rf}
        return prepare

    def render(self, ticket, images, offsets=None, **kw):
        """Engine.render of the ticket's batch on the ticket's stream, behind its forward: call between submit() (with
        project=True) and collect().  `images` (and offsets) as the caller's current stream left them.  collect() then
        also orders the caller's stream behind the drawing.  Returns what Engine.render returns."""
        return self._view(ticket, 'render', '_render_keep', self._frames(images, offsets), **kw)

    def overlay(self, ticket, images, what, offsets=None, **kw):
        """Engine.overlay of the ticket's batch on the ticket's stream, behind its forward: call between submit() (with
        project=True) and collect(), like render().  Returns what Engine.overlay returns."""
        return self._view(ticket, 'overlay', '_overlay_keep', self._frames(images, offsets), what=what, **kw)

    def render_regions(self, ticket, frames, offsets, region_frame, **kw):
        """Engine.render_regions of the ticket's batch (a forward on regions) on the ticket's stream, like render()."""
        return self._view(ticket, 'render_regions', '_render_keep', self._region_frames(ticket, frames, offsets, region_frame), **kw)

    def overlay_regions(self, ticket, frames, what, offsets, region_frame, **kw):
        """Engine.overlay_regions of the ticket's batch on the ticket's stream, like overlay()."""
        return self._view(ticket, 'overlay_regions', '_overlay_keep', self._region_frames(ticket, frames, offsets, region_frame),
                          what=what, **kw)

    def segment(self, ticket, images=None, offsets=None, ids=None, **kw):
        """Engine.segment of the ticket's batch on the ticket's stream, behind its forward: call between submit() and
        collect(), like overlay().  `images`, `offsets` and `ids` as the caller's current stream left them.  Returns what
        Engine.segment returns."""
        def prepare(eng):
            return {'images': None if images is None else images.contiguous(),
                    'offsets': None if offsets is None else offsets.to(self.device, torch.float32).contiguous(),
                    'ids': None if ids is None else ids.contiguous()}
        return self._view(ticket, 'segment', '_segment_keep', prepare, **kw)

    def contact(self, ticket, **kw):
        """Engine.contact of the ticket's batch on the ticket's stream, behind its forward: call between submit() (with
        project=True) and collect(), like render().  max_hand is the ticket's.  Returns what Engine.contact returns; collect()
        then also orders the caller's stream behind it."""
        out = ticket['out']
        K = out['slots'].shape[1] if out['slots'].dim() == 4 else 1

        def prepare(eng):
            ct = kw.get('cam_trans')
            return {} if ct is None else {'cam_trans': ct.to(self.device, torch.float32).contiguous()}

        rest = {k: v for k, v in kw.items() if k != 'cam_trans'}
        return self._on_ticket(ticket, 'contact', prepare, keep='_contact_keep',
                               call=lambda eng, raw, t: eng.contact(out, max_hand=K, stream=raw, **t, **rest))

    def score(self, ticket, gt, board=None, **kw):
        """Engine.score of the ticket's batch on the ticket's stream, behind its forward: call between submit() (with
        project=True) and collect(), like contact().  max_hand is the ticket's.  A board shared by the pool's contexts is
        updated in the order of the calls, as the stream table is.  Returns what Engine.score returns."""
        out = ticket['out']
        K = out['slots'].shape[1] if out['slots'].dim() == 4 else 1

        def prepare(eng):      # (every conversion here: Engine.score then queues nothing on the caller's stream)
            t = {'gt': score_truth(gt, tuple(out['slots'].shape[:-1]), self.device)}
            if kw.get('cam_trans') is not None:
                t['cam_trans'] = kw['cam_trans'].to(self.device, torch.float32).contiguous()
            return t

        rest = {k: v for k, v in kw.items() if k != 'cam_trans'}
        return self._on_ticket(ticket, 'score', prepare, keep='_score_keep',
                               call=lambda eng, raw, t: eng.score(out, board=board, max_hand=K, stream=raw, **t, **rest))

    def refine(self, ticket, **kw):
        """Engine.refine of the ticket's batch: call between submit() (with project=True) and collect().  max_hand is the
        ticket's.  The fit is mostly torch's own ops around two launches, so it runs on the CALLER's current stream, which is
        made to wait - on the device - for the ticket's forward; the ticket's stream is then ordered behind it, so that later
        calls on the ticket and collect() see it.  Returns what Engine.refine returns (a new dict: the ticket's own `out` is
        not changed)."""
        i = ticket['slot']
        if self._busy[i] is not ticket:
            raise RuntimeError('refine() belongs between submit() and collect() of its ticket')
        out = ticket['out']
        K = out['slots'].shape[1] if out['slots'].dim() == 4 else 1
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ticket['event'])
        res = self.engines[i].refine(out, max_hand=K, **kw)
        done = torch.cuda.Event()
        done.record(cur)
        self.streams[i].wait_event(done)
        after = torch.cuda.Event()
        after.record(self.streams[i])
        ticket['event'] = after
        ticket.setdefault('kept', []).append((res, kw, None))
        return res

    def match(self, ticket, gt, on='pj2d_org', board=None, **kw):
        """Engine.match of the ticket's batch on the ticket's stream, behind its forward: call between submit() (with
        project=True) and collect(), like score().  max_hand is the ticket's.  A board shared by the pool's contexts is updated
        in the order of the calls.  Returns what Engine.match returns; a score() of its rows on the same ticket runs behind it."""
        out = ticket['out']
        K = out['slots'].shape[1] if out['slots'].dim() == 4 else 1

        def prepare(eng):      # (every conversion here: Engine.match then converts nothing on the caller's stream)
            _, truth = match_truth(gt, on, out['slots'].shape[0], self.device)
            key = 'joints' if on == 'joints' else 'kp2d'
            t = {'gt': dict(gt, **{key: truth['points']}, **{k: truth[k] for k in ('joint_valid', 'valid', 'group') if truth[k] is not None})}
            if kw.get('cam_trans') is not None:
                t['cam_trans'] = kw['cam_trans'].to(self.device, torch.float32).contiguous()
            return t

        rest = {k: v for k, v in kw.items() if k != 'cam_trans'}
        return self._on_ticket(ticket, 'match', prepare, keep='_match_keep',
                               call=lambda eng, raw, t: eng.match(out, on=on, board=board, max_hand=K, stream=raw, **t, **rest))

    def track_boxes(self, ticket, frame_hw, scale=1.5, min_size=64, out=None):
        """ops.track_boxes of the ticket's batch on the ticket's stream, behind its forward: call between submit() (with
        project=True and offsets) and collect(), like render().  -> the boxes of the next frames, int32 on the device.  The
        caller's current stream is made to wait for them ON THE DEVICE, so they can go straight into
        ops.preprocess_rois_device and the submit() of the next batch while this ticket is still outstanding; the host waits
        for nothing."""
        def prepare(eng):
            res = ticket['out']
            if res.get('pj2d_org') is None:
                raise ValueError('the ticket holds no pj2d_org (submit(..., offsets=offsets, project=True))')
            n = res['slots'].shape[0]
            boxes = out if out is not None else torch.empty(n, 4, dtype=torch.int32, device=self.device)
            return ops_mod.frame_hw_device(frame_hw, n, self.device), boxes

        def call(eng, raw, hw_boxes):
            return ops_mod.track_boxes(ticket['out']['pj2d_org'], ticket['out']['slots'], hw_boxes[0], scale=scale,
                                       min_size=min_size, out=hw_boxes[1], stream=raw)

        return self._on_ticket(ticket, 'track_boxes', prepare, call, caller_waits=True)

    def _reap(self):
        self._inflight = [t for t in self._inflight if not t['event'].query()]

    def release(self, ticket):
        """Frees the ticket's context for the next submit without making any stream wait: for callers that order
        their consumers on ticket['event'] themselves (parallel.ShardedRunner queues the all-gather behind it)."""
        if self._busy[ticket['slot']] is ticket:
            self._busy[ticket['slot']] = None
            self._reap()
            self._inflight.append(ticket)      # kept until its event has completed (see submit)
        return ticket['event']

    def collect(self, ticket):
        self.release(ticket)
        torch.cuda.current_stream(self.device).wait_event(ticket['event'])
        return ticket['out']


class _DevArray(object):
    """__cuda_array_interface__ shim so torch can view library-owned HBM without copying."""

    def __init__(self, ptr, n, device, typestr='<f4'):
        self.__cuda_array_interface__ = {'shape': (n,), 'typestr': typestr, 'data': (int(ptr), False), 'version': 2}
        self.device = device
