"""acr.main.ACR: the demo-facing wrapper (acr/main.py:24-141) over the MI355X path.

    acr = ACR(args_set)                      # builds the model, loads the checkpoint + MANO tables
    results = acr(bgr_frame, path)           # {path: [per-hand dict of float16 arrays]}  or  {path: {}}
    results = acr.forward_batch(frames, paths)   # the batched form the reference never had
    results = acr.forward_batch(frames, paths, streams=camera_ids)   # -t: every frame smoothed with its camera's filters

Drawing (acr/visualization.py:100-218 with show_items=['mesh'], acr/renderer/*): with `renderer='hip'` the hand meshes
are rasterised over the frames on the GPU (csrc/render.hip; conventions in DESIGN.md "Rendering") -
    results = acr(bgr_frame, path); frame = acr.rendering['mesh_rendering_orgimgs'][0]      # uint8 [H,W,3] BGR, numpy
    results, frames = acr.forward_raw_batch(bgr_frames, paths, render=True)                # device tensors, original sizes
    results, frames = acr.forward_batch(rgb512, paths, render=rgb512)                      # the network input
'none' and the reference's 'pyrender' / 'pytorch3d' draw nothing; the results never depend on the renderer.

The other views of Visualizer.visulize_result_live (acr/visualization.py:228-254) are drawn on the GPU as well
(csrc/overlay.hip; rules in DESIGN.md "Key-point and heat-map views"): list them in `show_items` -
    acr.show_items = ['mesh', 'pj2d', 'centermap']         # default ['mesh']; also 'org_img'
    results = acr(bgr_frame, path); acr.rendering['pj2d'][0]; left, right = acr.rendering['centermap'][0]
    results, views = acr.forward_raw_batch(bgr_frames, paths, render=True, show_items=('mesh', 'pj2d', 'centermap'))
    views['pj2d'], views['centermap']                      # frames like the input; the centre view as [2 (left, right), ...]
'pj2d' = the 21 projected key points of each hand as a coloured skeleton, 'centermap' = the left and right centre heat
maps in false colour over the frame.  The 'j3d' plot and video or image files stay out of scope.
Two views the reference does not have colour the meshes per VERTEX: 'contact' (with contact=) by the
distance to the other hand, 'error' (with gt= that holds 'verts') by the error against truth -
    results, views = acr.forward_batch(rgb512, paths, contact=True, render=rgb512, show_items=('mesh', 'contact'))
The network's own hand-part segmentation is the view 'segm' - the part labels in colour over the frame -
and, with masks=True / masks='iou', three more keys of every hand dict: 'mask_area', 'mask_box', 'mask_iou' -
    results, views = acr.forward_raw_batch(bgr_frames, paths, render=True, show_items=('mesh', 'segm'), masks='iou')
"""
import logging

import numpy as np
import torch

from ..config import ConfigContext, args, parse_args, validate
from .mano_wrapper import MANOWrapper
from .model import ACR as ACR_v1
from .utils import (create_OneEuroFilter, get_remove_keys, img_preprocess, justify_detection_state, load_model,
                    reorganize_results, save_results, smooth_results)


# the views of acr/visualization.py:174-254 that are built, and the two per-vertex colour views
SHOW_ITEMS = ('mesh', 'pj2d', 'centermap', 'org_img', 'contact', 'error')
COLOR_ITEMS = ('contact', 'error')      # the meshes coloured per vertex: Engine.contact_colors / Engine.error_colors
MAP_ITEMS = ('segm',)                   # views of the network's other maps: the part segmentation (Engine.segment)


def check_color_items(items, contact=False, gt=None, where=None):
    """The two per-vertex colour views among `items` need what they show: 'contact' the contact measure (contact=True or
    'surface'), 'error' ground-truth vertices (gt= with 'verts').  where: the entry point that does not build them at all.
    ValueError before anything runs."""
    for name in items or ():
        if name not in COLOR_ITEMS:
            continue
        if where is not None:
            raise ValueError('show_items: %r is a view of forward_batch / forward_raw_batch without boxes=, not of %s' % (name, where))
        if name == 'contact' and not contact:
            raise ValueError("show_items: 'contact' colours the hands by the contact measure: it needs contact=True or contact='surface'")
        if name == 'error' and (not isinstance(gt, dict) or gt.get('verts') is None):
            raise ValueError("show_items: 'error' colours the hands by their vertex errors: it needs gt= with 'verts'")


def check_show_items(show_items):
    """None stays None; else the list of view names, ValueError for one that is not in SHOW_ITEMS or MAP_ITEMS."""
    if show_items is None:
        return None
    items = [show_items] if isinstance(show_items, str) else list(show_items)
    for name in items:
        if name not in SHOW_ITEMS and name not in MAP_ITEMS:
            raise ValueError('show_items: %r is not one of %s' % (name, SHOW_ITEMS + MAP_ITEMS))
    return items


def check_masks(masks, where=None):
    """masks= of forward_batch / forward_raw_batch: False, True or 'iou'; where: the entry point that does not build them."""
    if not isinstance(masks, bool) and not (isinstance(masks, str) and masks == 'iou'):
        raise ValueError("masks must be True, False or 'iou', not %r" % (masks,))
    if masks and where is not None:
        raise ValueError('masks= over regions is not built (%s): the part segmentation is a map per region, and overlapping '
                         'regions of a frame would need a winner rule' % where)
    return masks


def check_map_items(items, where):
    """'segm' among `items` over regions (`where`) is a ValueError before anything runs."""
    for name in items or ():
        if name in MAP_ITEMS:
            raise ValueError('show_items: %r over regions is not built (%s): the part segmentation is a map per region, and '
                             'overlapping regions of a frame would need a winner rule' % (name, where))


class ACR(object):
    def __init__(self, args_set=None, state_dict=None, mano_tables=None, device=0, max_batch=1):
        """args_set: namespace from config.parse_args (default: config.args()).  state_dict / mano_tables
        let callers inject in-memory assets (tests, synthetic runs) instead of model_path / mano_root files."""
        a = validate(args() if args_set is None else args_set)
        self.demo_cfg = {'mode': 'parsing', 'calc_loss': False}
        for k, v in vars(a).items():
            setattr(self, k, v)
        logging.basicConfig(level=logging.INFO)
        self._args = a
        self._device = device
        self.rendering = None      # renderer='hip': {'mesh_rendering_orgimgs': [frame]} of the last forward()
        self.show_items = ['mesh']      # the views `forward` leaves on `rendering` (SHOW_ITEMS); the reference's default
        self.stream_table = None        # forward_batch(..., streams=): One-Euro state per video stream (engine.StreamTable)
        self.track_table = None         # forward_batch(..., tracks=): the tracks per video stream (engine.TrackTable)
        self._build_model_(state_dict, mano_tables, device, max_batch)
        if self.temporal_optimization:
            # acr/main.py:45-47: one filter set per hand type; the state lives in the engine's context
            self.filter_dict = create_OneEuroFilter(a.smooth_coeff, engine=self.model.engine)

    def _build_model_(self, state_dict, mano_tables, device, max_batch):
        """acr/main.py:57-63"""
        with ConfigContext(self._args):
            model = ACR_v1(device=device, max_batch=max_batch).eval()
            if state_dict is not None:
                model.load_state_dict(state_dict)
            else:
                model = load_model(self.model_path, model, prefix='module.', drop_prefix='', fix_loaded=False)
            self.model = model.cuda(device)
            self.mano_regression = MANOWrapper(mano_root=self.mano_root, tables=mano_tables, device=device,
                                               engine=self.model.engine()).bind_model(self.model)

    @torch.no_grad()
    def process_results(self, outputs):
        """acr/main.py:66-89"""
        if self.temporal_optimization:
            pd = outputs['params_dict']
            if len(pd['poses']) != 2:
                raise ValueError('temporal optimisation expects exactly one frame (2 rows), as acr/main.py:77 asserts')
            # rows of a one-frame batch are [left, right] = the slot order: smooth the slots on the device and
            # refresh the rows the MANO stage reads (acr/main.py:69-83)
            from .. import _lib as S
            slots = smooth_results(self.filter_dict, outputs['slots'])
            pd['poses'].copy_(slots[0, :, S.SLOT_POSES:S.SLOT_POSES + 48])
            pd['betas'].copy_(slots[0, :, S.SLOT_BETAS:S.SLOT_BETAS + 10])
            pd['global_orient'], pd['hand_pose'] = pd['poses'][:, :3].contiguous(), pd['poses'][:, 3:].contiguous()
        outputs = self.mano_regression(outputs, outputs['meta_data'])
        reorganize_idx = outputs['reorganize_idx'].cpu().numpy()
        results = reorganize_results(outputs, outputs['meta_data']['imgpath'], reorganize_idx)
        return outputs, results

    @torch.no_grad()
    def single_image_forward(self, bgr_frame, path):
        """acr/main.py:126-141"""
        meta = img_preprocess(bgr_frame, path, input_size=self.input_size, single_img_input=True, device=self._device)
        ds_org, imgpath_org = get_remove_keys(meta, keys=['data_set', 'imgpath'])
        meta['batch_ids'] = torch.arange(len(meta['image']))
        outputs = self.model(meta, **self.demo_cfg)
        outputs['detection_flag'], outputs['reorganize_idx'] = justify_detection_state(outputs['detection_flag'],
                                                                                       outputs['reorganize_idx'])
        meta.update({'imgpath': imgpath_org, 'data_set': ds_org})
        outputs['meta_data']['imgpath'] = [path] * len(outputs['params_pred'])
        return outputs

    @torch.no_grad()
    def forward(self, bgr_frame, path):
        """acr/main.py:92-123 without the drawing: {path: [hand dicts]} or {path: {}} when nothing is detected.
        hands_per_side > 1 in the config: the frame goes through forward_raw_batch(max_hand=hands_per_side) instead - up to
        that many hands of each side, lefts in rank order then rights; `rendering` holds the same views."""
        if int(getattr(self, 'hands_per_side', 1)) > 1:
            return self._forward_multi_single(bgr_frame, path)
        outputs = self.single_image_forward(bgr_frame, path)
        if outputs is not None and outputs['detection_flag']:
            outputs, results = self.process_results(outputs)
            if self.save_dict_results and self.output_dir:
                save_results(results, self.output_dir.rstrip('/') + '/results.pkl')
        else:
            print('no hand detected!')
            results = {path: {}}
        if self.renderer == 'hip':
            items = check_show_items(self.show_items)
            check_color_items(items, where='forward')
            self.rendering = self._views_single(bgr_frame, outputs, items)
        return results

    def _forward_multi_single(self, bgr_frame, path):
        """`forward` with hands_per_side > 1: one frame through the batched path."""
        if self.temporal_optimization:
            raise ValueError('temporal optimisation follows one hand of each side: not with hands_per_side > 1')
        frame = torch.from_numpy(np.ascontiguousarray(np.asarray(bgr_frame, np.uint8)))[None].cuda(self._device)
        items = check_show_items(self.show_items) if self.renderer == 'hip' else None
        got = self.forward_raw_batch(frame, [path], render=bool(items), show_items=items or None)
        results, views = got if items else (got, None)
        if not results[path]:
            print('no hand detected!')
        elif self.save_dict_results and self.output_dir:
            save_results(results, self.output_dir.rstrip('/') + '/results.pkl')
        if self.renderer == 'hip':
            self.rendering = {}
            for name in items:
                v = views[name]
                if name == 'centermap':
                    self.rendering[name] = [(v[0, 0].cpu().numpy(), v[1, 0].cpu().numpy())]
                else:
                    self.rendering['mesh_rendering_orgimgs' if name == 'mesh' else name] = [v[0].cpu().numpy()]
        return results

    def _views_single(self, bgr_frame, outputs, items):
        """`rendering` of one forward(): 'mesh' -> 'mesh_rendering_orgimgs' (the reference's key), 'pj2d' -> [frame],
        'centermap' -> [(left, right)], 'segm' -> [frame], 'org_img' -> [frame]; uint8 [H,W,3] BGR numpy, original size."""
        from .. import ops
        views = {}
        frame = np.ascontiguousarray(np.asarray(bgr_frame, np.uint8))
        for name in items:
            if name == 'mesh':
                views['mesh_rendering_orgimgs'] = [self._render_single(bgr_frame, outputs)]
            elif name == 'org_img':
                views['org_img'] = [frame.copy()]
            elif name == 'pj2d':
                kps = None if outputs is None else outputs.get('pj2d_org')
                if kps is None or not len(kps):
                    views['pj2d'] = [frame.copy()]
                    continue
                img = torch.from_numpy(frame)[None].to(kps.device)
                drawn = ops.draw_skeletons(kps.float().contiguous(), img, hand_frame=torch.zeros(len(kps), dtype=torch.int32),
                                           bgr=True)
                views['pj2d'] = [drawn[0].cpu().numpy()]
            elif name == 'centermap':
                if outputs is None or outputs.get('l_center_map') is None:
                    views['centermap'] = [(frame.copy(), frame.copy())]
                    continue
                maps = torch.cat([outputs['l_center_map'][:1], outputs['r_center_map'][:1]], 1)      # [1,2,h,w]
                img = torch.from_numpy(frame)[None].to(maps.device)
                both = ops.draw_heatmaps(maps, img, view=ops.view_from_offsets(outputs['meta_data']['offsets'][:1]), bgr=True)
                views['centermap'] = [(both[0, 0].cpu().numpy(), both[1, 0].cpu().numpy())]
            elif name == 'segm':
                if outputs is None or outputs.get('segms') is None:
                    views['segm'] = [frame.copy()]
                    continue
                logits = outputs['segms'][:1].permute(0, 2, 3, 1).float().contiguous()      # NCHW -> [1,h,w,33]
                img = torch.from_numpy(frame)[None].to(logits.device)
                views['segm'] = [ops.draw_segm(logits, img, offsets=outputs['meta_data']['offsets'][:1], bgr=True)[0].cpu().numpy()]
        return views

    def _render_single(self, bgr_frame, outputs):
        """The reference's 'mesh_rendering_orgimgs' (acr/visualization.py:196-218): the original frame with the detected
        hands drawn over it - uint8 [H,W,3] BGR numpy.  No detection: a copy of the frame."""
        from .. import ops
        frame = np.ascontiguousarray(np.asarray(bgr_frame, np.uint8))
        if outputs is None or outputs.get('verts') is None or not len(outputs['verts']):
            return frame.copy()
        dev = outputs['verts'].device
        side = outputs['output_hand_type'].to(torch.int32)
        ml = self.mano_regression.mano_layer
        cols = torch.tensor([list(reversed(c)) for c in ops.HAND_COLORS_RGB])[side.long().cpu()]      # BGR
        n = len(side)
        img = ops.render_meshes(outputs['verts'], (ml['l'].th_faces, ml['r'].th_faces), torch.from_numpy(frame)[None].to(dev),
                                mesh_frame=torch.zeros(n, dtype=torch.int32), trans=outputs['cam_trans'], colors=cols,
                                view=ops.view_from_offsets(outputs['meta_data']['offsets'][:1]),
                                focal_length=float(self.focal_length), topo_index=side)
        return img[0].cpu().numpy()

    __call__ = forward

    @torch.no_grad()
    def reset_streams(self, ids=None):
        """The listed video streams of forward_batch(..., streams=) - all of them when ids is None - start a new sequence
        (a new video behind a camera id; the reference builds new filters per video, acr/main.py:50-53)."""
        if self.stream_table is not None:
            self.stream_table.reset(ids)

    def close_streams(self):
        """Frees the stream table; the next forward_batch(..., streams=) creates a new one (every stream fresh, and
        `max_streams` may differ)."""
        table, self.stream_table = self.stream_table, None
        if table is not None:
            table.close()

    @torch.no_grad()
    def reset_tracks(self, ids=None):
        """The listed video streams of forward_batch(..., tracks=) - all of them when ids is None - lose their tracks."""
        if self.track_table is not None:
            self.track_table.reset(ids)

    def close_tracks(self):
        """Frees the track table; the next forward_batch(..., tracks=) creates a new one."""
        table, self.track_table = self.track_table, None
        if table is not None:
            table.close()

    def _tracks_for(self, K, max_streams, gate, max_miss):
        """forward_batch's `tracks=`: the TrackTable this object owns (created on first use with the parameters of that call;
        like the stream table it is not the model's, so it survives load_state_dict)."""
        from ..engine import TrackTable
        want = (256 if max_streams is None else int(max_streams), K, 8 if gate is None else int(gate),
                5 if max_miss is None else int(max_miss))
        t = self.track_table
        if t is None:
            t = self.track_table = TrackTable(self._device, *want)
        elif t.max_hand != K or (max_streams is not None and t.capacity != want[0]) or \
                (gate is not None and t.gate != want[2]) or (max_miss is not None and t.max_miss != want[3]):
            raise ValueError('the track table holds (streams, max_hand, gate, max_miss) = %s (asked for %s): close_tracks() first'
                             % ((t.capacity, t.max_hand, t.gate, t.max_miss), want))
        return t

    def _streams_for(self, streams, max_streams, B):
        """forward_batch's `streams=`: the host ids and the table this object owns (created on first use; it is not the
        model's, so it survives load_state_dict)."""
        from ..engine import StreamTable, stream_ids
        if not self.temporal_optimization:
            raise ValueError('streams= smooths per video stream: it needs temporal_optimization (-t)')
        ids = stream_ids(streams, B)
        if self.stream_table is None:
            self.stream_table = StreamTable(self._device, 256 if max_streams is None else max_streams)
        elif max_streams is not None and int(max_streams) != self.stream_table.capacity:
            raise ValueError('the stream table holds %d streams (max_streams=%d)' % (self.stream_table.capacity, max_streams))
        return ids, self.stream_table

    @torch.no_grad()
    def forward_batch(self, rgb_u8_frames, paths, offsets=None, point_heads=True, batch_semantics=None, render=None,
                      render_bgr=False, show_items=None, streams=None, max_streams=None, max_hand=None, tracks=None,
                      track_gate=None, track_max_miss=None, multi_point_heads=False, contact=False, gt=None, board=None,
                      masks=False, match=None, match_gate=float('inf'), match_board=None, refine=None):
        """Batched throughput path: uint8 [B,512,512,3] RGB (already pre-processed) -> per-image results.
        One fused call (backbone, heads, decode, MANO, projection) + one D2H of the packed results.
        The head maps are not part of these results, so by default the params/cam/prior towers run only at the
        decoded centers (Engine.set_point_heads; same results within fp32 round-off) - point_heads=False runs the
        dense heads as `forward` does.
        batch_semantics: 'frame' | 'reference' (None = the model's ResultParser setting, args().batch_semantics): with
        'reference' the fused call applies the reference's batch-wide prior rules (acr/result_parser.py:42-47,102-145) on
        the device - decode, acrmi_prior_gate, gated decode - still ONE call (ACRMI_OPT_BATCH_PRIOR).
        render: frames to draw the meshes over (Engine.render) - uint8 device tensor [B,H,W,3], or a list of B frames
        [H_i,W_i,3] of different sizes (one render call per size, output order = input order): the network input itself
        when `offsets` is None, else the original frames the offsets rows describe; render_bgr: their channel order.
        The return value is then (results, rendered); `results` is what it is without `render`.
        show_items: names from SHOW_ITEMS - the views to draw over `render` instead of the meshes alone; the return value is
        then (results, {name: frames}): 'mesh' as above, 'pj2d' the key-point skeletons, 'centermap' the left and right centre
        heat maps as [2,B,H,W,3] (a list of [2,H_i,W_i,3] for a list of frames), 'org_img' the frames themselves; 'contact'
        (needs contact=) the meshes coloured per vertex by the distance to the nearest hand of the other side - near is hot, 0.02
        m and beyond blue, a vertex inside the other hand magenta - and 'error' (needs gt= with 'verts') by the root-aligned
        vertex error, 0.02 m and beyond red (Engine.contact_colors / error_colors; the 0.02 m are parameters of the picture;
        DESIGN.md section 22).  A hand without a partner, or without truth, keeps its flat colour.
        streams (needs -t): the video stream (camera) of each frame, ints in [0, max_streams), -1 = do not smooth this frame -
        every frame is smoothed with the One-Euro state of ITS stream (acr/main.py:69-83 per video) instead of the batch being
        one video; the state lives in a table of max_streams streams (default 256, fixed when the first such call creates
        it) that this object owns across load_state_dict; reset_streams() starts streams anew.
        max_hand (None = args().hands_per_side; 1..8): up to that many hands of EACH side per frame (Engine.forward's
        max_hand).  results[path] then lists the flagged left hands in rank order, then the flagged right
        hands in rank order.  With max_hand > 1 the dense heads run even with point_heads=True, unless multi_point_heads=True:
        then the towers run only at the max_hand best centres of each side (Engine.set_point_heads_multi; same results within
        fp32 round-off; a program without the point heads stays dense; DESIGN.md section 17 says at which max_hand it pays);
        batch_semantics='reference', streams= and temporal optimisation are a ValueError; 'mesh' and 'pj2d'
        are drawn as the views of max_hand regions per frame (Engine.render_regions / overlay_regions with the frame's own
        offsets row), 'centermap' and 'org_img' as always.
        tracks (any max_hand): the video stream (camera) of each frame, ints in [0, max_streams), -1 =
        leave the frame as decoded.  The hands of every frame are put into the order of their stream's TRACKS (this object owns
        the engine.TrackTable, created by the first such call: max_streams streams, track_gate map pixels, track_max_miss
        frames; reset_tracks() / close_tracks()), every hand dict gains 'track_id', and results[path] lists the flagged lefts
        then the flagged rights in SLOT order, so a hand keeps its place while its rank changes.  With -t every track is smoothed
        with its own One-Euro filter.  Not together with streams=.
        contact=True: Engine.contact runs behind the fused call, and every hand dict gains four keys
        (only then): 'contact_dist' - metres from the hand's nearest vertex to the nearest hand of the OTHER side in the same
        row (inf when there is none); 'contact_with' - the index of that hand in results[path] (-1: none; with max_hand > 1
        the partner is the pair with the smallest distance, the lower rank on a tie); 'contact_verts' - the hand's own vertex
        indices within ops.CONTACT_DIST of that hand's nearest vertex; 'penetration' - metres, the depth estimate of the
        hand's vertices inside the partner.  A nearest-vertex heuristic on two independently placed meshes, not a measurement.
        Pairs are formed inside a row only: hands of different frames - and, with boxes=, of different regions, each of
        which has its own camera - are never paired.
        contact='surface' (DESIGN.md section 20): the same four keys from the surface measure (Engine.contact(mode='surface')):
        'contact_dist' - metres between the two SURFACES, the square root of the smaller min_d2 of the pair's two directions;
        'contact_verts' - the hand's own vertices within ops.CONTACT_DIST of the partner's surface; 'penetration' - metres,
        the largest distance to the partner's surface among the hand's own vertices inside it (ray crossings).
        gt=: ground truth as Engine.score takes it - {'joints': [B,(K,)2,21,3], 'verts', 'joint_valid',
        'group'} - scored on the GPU behind the fused call.  Every hand dict gains 'mpjpe', 'pa_mpjpe', 'mpvpe', 'pa_mpvpe' (only
        then): the hand's mean root-aligned and Procrustes-aligned joint and vertex errors in metres, nan for a hand without
        truth (its group outside the board's, no counted point, no 'verts').  board= (needs gt=): an engine.ScoreBoard the
        batch is added to, on the device; its summary() is the data set's score.  With boxes= a region is a row.
        show_items 'segm' (DESIGN.md section 23): the network's hand-part segmentation in colour over the frames
        (Engine.segment), like 'centermap' a view of the frame, not of a hand.
        masks=True: every hand dict gains 'mask_area' - the pixels the segmentation gives the hand's SIDE - and 'mask_box' - the
        smallest (l, t, r, b) around them, r and b exclusive, zeros when there are none - at the resolution of the frames given
        to `render`, else on the 512 x 512 canvas.  The map has no instances: with max_hand > 1 every hand of a side carries its
        side's values.  masks='iou': also 'mask_iou', the intersection over union of the side's mask and the side's drawn
        silhouette (the rasteriser's ids over the same frames, or over a scratch canvas) - a check of the reconstruction against
        image evidence that needs no ground truth; nan when both are empty.
        match='kp2d' | 'joints' (needs gt=): the decoded hands are matched to the annotated ones on the
        GPU before they are scored (Engine.match): gt then leads with [B,G,2] for any G in 1..8, whatever max_hand is, and may
        hold 'kp2d' [B,G,2,21,2] in the pixels of pj2d_org and 'valid' [B,G,2].  'kp2d' matches on pj2d_org against gt['kp2d'],
        'joints' on joints + cam_trans against gt['joints']; match_gate is the largest mean distance of a pair (pixels /
        metres; default inf: a parameter, not a measurement).  Every hand dict gains 'gt_index' - the annotated hand it was
        matched to, -1 for a false positive - and 'match_cost'; the four score keys come from the matched truth, nan for an
        unmatched hand; board= receives the rows in TRUTH order, so its 'missed' are the annotated hands nothing was matched
        to and its MRRPE pairs are (left g, right g).  match_board=: an engine.MatchBoard the batch's TP / FP / FN are added to.
        The 'error' view and boxes= are not built with match=.
        refine=dict(kp2d=..., joints=..., weights=..., steps=..., lam_pose=..., lam_beta=..., lr=..., free=...) (DESIGN.md
        section 26): Engine.refine runs behind the fused call - every flagged hand is fitted on the GPU, in one launch, to
        kp2d [B,(K,)2,21,2] in the units of pj2d (the canvas, -1..1; 'kp2d_org' instead: pixels of the original frames, taken
        through the inverse of pj2d_org's formula with `offsets`) and / or root-aligned joints [B,(K,)2,21,3], with the network's
        own prediction as start and prior.  The pose, shape, camera and mesh keys of every hand dict then come from the refined
        hand - as do the views, contact, scores and masks - and it gains 'fit_loss' (first and last evaluated step).  Without
        refine= nothing changes by a byte."""
        _check_contact(contact)
        _check_score(gt, board)
        _check_match(match, gt, match_gate, match_board, show_items)
        check_masks(masks)
        show_items = check_show_items(show_items)
        if show_items is not None and render is None:
            raise ValueError('show_items needs the frames to draw over (render=)')
        check_color_items(show_items, contact, gt)
        K = int(self.hands_per_side if max_hand is None else max_hand)
        results, eng, out = self._fused_call(rgb_u8_frames, paths, offsets=offsets, point_heads=point_heads,
                                             batch_semantics=batch_semantics, streams=streams, max_streams=max_streams, K=K,
                                             tracks=tracks, track_gate=track_gate, track_max_miss=track_max_miss,
                                             multi_point_heads=multi_point_heads, contact=contact, gt=gt, board=board,
                                             masks=masks, mask_frames=render, mask_offsets=offsets, match=match,
                                             match_gate=match_gate, match_board=match_board, refine=refine)
        if render is None:
            return results
        _add_vertex_colors(eng, out, K, show_items, render_bgr)
        if K != 1 or tracks is not None:      # the [B,K,...] shapes: K pairs per frame
            return results, _multi_views(self, eng, out, render, offsets, render_bgr, show_items)

        def draw(name):
            if name == 'mesh' or name in COLOR_ITEMS:
                return self._render_batch(eng, out, render, offsets, render_bgr, vertex_colors=out.get(('vertex_colors', name)))
            if name in MAP_ITEMS:
                return self._segm_batch(eng, out, render, offsets, render_bgr)
            return self._overlay_batch(eng, out, render, name, offsets, render_bgr)

        return results, _views(show_items, render, draw)

    def _fused_call(self, frames, paths, *, offsets=None, point_heads=True, batch_semantics=None, streams=None, max_streams=None,
                    K=1, tracks=None, track_gate=None, track_max_miss=None, multi_point_heads=False, contact=False, gt=None,
                    board=None, masks=False, mask_frames=None, mask_offsets=None, match=None, match_gate=float('inf'),
                    match_board=None, refine=None):
        """The fused call of forward_batch and its packaging -> (results, the engine, what the engine returned).  K = 1 without
        tracks: one hand of each side, `point_heads` is the switch and multi_point_heads is checked and without effect.
        K > 1 or tracks=: Engine.forward(max_hand=K) on the dense heads, or with multi_point_heads (K > 1) at the K best centres.
        Everything that can be refused is refused before anything runs; the engine's options are back at their defaults
        afterwards, also after an exception."""
        from .. import ops
        from ..engine import check_max_hand
        K = check_max_hand(K)
        _check_multi_point_heads(multi_point_heads)
        multi = K != 1 or tracks is not None
        if multi:
            if tracks is not None and streams is not None:
                raise ValueError('tracks= smooths every track with its own filter: not together with streams=')
            if streams is not None:
                raise ValueError('streams= follows one hand of each side through a video: not with max_hand=%d' % K)
            if self.temporal_optimization and tracks is None:
                raise ValueError('temporal optimisation follows one hand of each side: not with max_hand=%d' % K)
            if (batch_semantics or self.model._result_parser.batch_semantics) != 'frame':
                raise ValueError("batch_semantics='reference' is the reference's rule for one hand of each side (it cannot run "
                                 'more: acr/result_parser.py:134): not with max_hand=%d' % K)
        B = frames.shape[0]
        ids, table = (None, None) if streams is None else self._streams_for(streams, max_streams, B)
        eng = self.model.engine(B)
        if offsets is None:
            offsets = _whole_frame_offsets(B)
        refine_kw = None if refine is None else _refine_args(refine, offsets)
        # coeff: smooth_coeff travels with a call that may smooth (a reloaded checkpoint builds a new context)
        if not multi:
            # frames of the batch = one video stream, in order; with `streams` the table holds the state and the frames are
            # not one stream
            heads, temporal, coeff = point_heads, bool(self.temporal_optimization) and ids is None, self._args.smooth_coeff
            semantics, heads_multi = batch_semantics or self.model._result_parser.batch_semantics, False
            kw = dict(streams=ids, table=table)
        else:
            heads, temporal, coeff, semantics, heads_multi = False, False, None, 'frame', multi_point_heads and K > 1
            kw = dict(max_hand=K)
            if tracks is not None:      # every track is smoothed by its own filter: ACRMI_OPT_TEMPORAL itself stays off
                coeff = self._args.smooth_coeff
                kw.update(tracks=tracks, track_table=self._tracks_for(K, max_streams, track_gate, track_max_miss),
                          smooth=bool(self.temporal_optimization))
        try:
            eng.set_point_heads(heads)
            eng.set_temporal(temporal, smooth_coeff=coeff)
            eng.set_batch_semantics(semantics)
            eng.set_point_heads_multi(heads_multi)
            out = eng.forward(frames, offsets=offsets, project=True, **kw)
        finally:
            eng.set_point_heads(False)
            eng.set_temporal(False)
            eng.set_batch_semantics('frame')
            eng.set_point_heads_multi(False)
        eng.check_range()      # 'fp16x3' only: an activation outside the f16 range is an error, not an empty result
        if refine is not None:      # the hands that go on are the refined ones (Engine.refine)
            out = eng.refine(out, max_hand=K, offsets=offsets, **refine_kw)
        # cam_trans for every slot (acr/utils.py:399-412): the device least-squares kernel on all hands
        out['cam_trans'] = ops.cam_trans(out['joints'].view(-1, 21, 3), out['pj2d'].view(-1, 21, 2),
                                         focal_length=self.focal_length).view(*out['slots'].shape[:-1], 3)
        if contact:
            _add_contact(eng, out, K, 'surface' if contact == 'surface' else 'vertex')
        if gt is not None and match is not None:
            _add_match(eng, out, K, gt, board, match, match_gate, match_board)
        elif gt is not None:
            _add_score(eng, out, K, gt, board)
        if masks:
            _add_masks(self, eng, out, masks == 'iou', mask_frames, mask_offsets)
        return results_from_out(out, paths), eng, out

    def _render_batch(self, eng, out, frames, offsets, bgr, vertex_colors=None):
        """The meshes over a tensor of frames (Engine.render) or a list of frames of different sizes; vertex_colors
        [B,2,778,3]: coloured per vertex."""
        src = out if vertex_colors is None else dict(out, vertex_colors=vertex_colors)

        def draw(imgs, idx, place):
            sub, off = _frames_of(src, offsets, idx, ('slots', 'verts', 'cam_trans', 'vertex_colors'))
            kw = {} if vertex_colors is None else {'vertex_colors': sub['vertex_colors']}
            return eng.render(sub, imgs, offsets=off, focal_length=float(self.focal_length), bgr=bgr, **kw)

        return _per_size(frames, draw, count=out['slots'].shape[0])

    def _overlay_batch(self, eng, out, frames, what, offsets, bgr):
        """'pj2d' / 'centermap' over a tensor of frames (Engine.overlay) or a list of frames of different sizes."""
        from .. import ops
        B = out['slots'].shape[0]
        whole = {}      # 'maps': the centre maps of the whole batch, fetched by the first group that needs them

        def draw(imgs, idx, place):
            if idx is None or what == 'pj2d':
                sub, off = _frames_of(out, offsets, idx, ('slots', 'pj2d', 'pj2d_org'))
                return eng.overlay(sub, imgs, what, offsets=off, bgr=bgr)
            # the context's maps are those of the whole batch: a subset goes through the stand-alone operator
            if not whole:
                whole['maps'] = eng.center_maps(B)
            sub, off = _frames_of(whole, offsets, idx, ('maps',))
            return ops.draw_heatmaps(sub['maps'], imgs, view=None if off is None else ops.view_from_offsets(off), bgr=bgr)

        return _per_size(frames, draw, count=B, pair=what == 'centermap')

    def _segm_batch(self, eng, out, frames, offsets, bgr):
        """'segm' over a tensor of frames (Engine.segment) or a list of frames of different sizes."""
        from .. import ops
        B = out['slots'].shape[0]

        def draw(imgs, idx, place):
            if idx is None:
                return eng.segment(B, images=imgs, offsets=offsets, bgr=bgr, labels=False)['view']
            # the context's map is that of the whole batch: a subset goes through the stand-alone operator
            sub, off = _frames_of({'logits': _segm_logits(eng, B)}, offsets, idx, ('logits',))
            return ops.draw_segm(sub['logits'], imgs, offsets=off, bgr=bgr)

        return _per_size(frames, draw, count=B)


def _refine_args(refine, offsets):
    """refine= of forward_batch / forward_raw_batch -> the keyword arguments of Engine.refine.  kp2d is in the units of pj2d (the
    canvas, -1..1); 'kp2d_org' - key points in pixels of the original frames - is taken through the inverse of pj2d_org's
    formula with the frames' offsets rows: pj2d = (org - (crop_left - pad_left, crop_top - pad_top)) * 2 / (pad_w, pad_h) - 1."""
    kw = dict(refine)
    unknown = set(kw) - {'kp2d', 'kp2d_org', 'joints', 'weights', 'steps', 'lam_pose', 'lam_beta', 'lr', 'free', 'dense'}
    if unknown:
        raise ValueError('refine= holds kp2d / kp2d_org / joints / weights / steps / lam_pose / lam_beta / lr / free / dense, not %s'
                         % sorted(unknown))
    org = kw.pop('kp2d_org', None)
    if org is not None:
        if kw.get('kp2d') is not None:
            raise ValueError('refine=: kp2d or kp2d_org, not both')
        org = torch.as_tensor(org)
        of = torch.as_tensor(offsets).to(org.device, torch.float32)
        of = of.reshape((of.shape[0],) + (1,) * (org.dim() - 2) + (10,))
        pad = of[..., 0:2]
        lt = torch.stack([of[..., 5] - of[..., 9], of[..., 2] - of[..., 6]], -1)
        kw['kp2d'] = (org.to(torch.float32) - lt) * 2.0 / pad - 1.0
    return kw


def _whole_frame_offsets(B):
    """The offsets rows of B frames that are the 512 x 512 network input itself."""
    return torch.tensor([[512., 512, 0, 0, 0, 0, 0, 0, 0, 0]]).repeat(B, 1)


def _per_size(frames, draw, count=None, pair=False):
    """draw(imgs [n,H,W,3], idx, place) over `frames`.  A tensor [N,H,W,3]: one call with idx = place = None, its result as it
    is.  A list of frames [H_i,W_i,3] of different sizes (`count` of them, where the caller expects a number): one call per
    size in the order the sizes appear, with idx = the positions in `frames` of the stacked imgs and place [len(frames)] =
    frame of the list -> frame of imgs, -1 = another group's; -> a list in input order.  pair: draw returns [2,n,H,W,3] (left,
    right - 'centermap') instead of [n,H,W,3], and the list holds [2,H_i,W_i,3]."""
    if not isinstance(frames, (list, tuple)):
        return draw(frames, None, None)
    if count is not None and len(frames) != count:
        raise ValueError('one frame to draw into per input frame')
    groups = {}
    for i, f in enumerate(frames):
        groups.setdefault(tuple(f.shape), []).append(i)
    drawn = [None] * len(frames)
    for idx in groups.values():
        place = torch.full((len(frames),), -1, dtype=torch.long)
        place[idx] = torch.arange(len(idx))
        got = draw(torch.stack([frames[i] for i in idx]), idx, place)
        for j, i in enumerate(idx):
            drawn[i] = got[:, j] if pair else got[j]
    return drawn


def _frames_of(out, offsets, idx, keys):
    """(the tensors `keys` of `out`, offsets) of the frames idx of a _per_size group (None: `out` and offsets as they are)."""
    if idx is None:
        return out, offsets
    sel = torch.tensor(idx, device=out[keys[0]].device)
    return ({k: out[k].index_select(0, sel) for k in keys if out.get(k) is not None},
            None if offsets is None else torch.as_tensor(offsets)[idx])


def _local_frames(frame_of, place):
    """frame_of [M] (the frame of each hand or region, -1 = none) in the frames of a _per_size group -> int32; -1 stays -1 and
    the frames of other groups become -1."""
    if place is not None:
        frame_of = torch.where(frame_of >= 0, place[frame_of.clamp(min=0)], torch.full_like(frame_of, -1))
    return frame_of.to(torch.int32)


def _views(items, frames, draw):
    """The views `items` over `frames`: None -> draw('mesh') alone, not in a dict; else {name: draw(name)}, with 'org_img' the
    frames as given."""
    def one(name):
        return frames if name == 'org_img' else draw(name)

    return one('mesh') if items is None else {name: one(name) for name in items}


def _check_multi_point_heads(value):
    if not isinstance(value, bool):
        raise ValueError('multi_point_heads must be True or False, not %r' % (value,))


def _check_contact(value):
    if not isinstance(value, bool) and not (isinstance(value, str) and value == 'surface'):
        raise ValueError("contact must be True, False or 'surface', not %r" % (value,))


def _check_score(gt, board):
    if gt is not None and (not isinstance(gt, dict) or gt.get('joints') is None):
        raise ValueError("gt must be a dict with 'joints' (Engine.score says what else it may hold)")
    if board is not None and gt is None:
        raise ValueError('board= accumulates the scores of gt=: it needs gt=')
    if board is not None and getattr(board, 'sets', None) != (21, 778):
        raise ValueError('board must be an engine.ScoreBoard of the default point sets (21 joints, 778 vertices)')


def _add_score(eng, out, K, gt, board):
    """out['score'] = the per-hand rows of Engine.score of `out` against gt ({'joints': row_f [N,4], 'verts': row_f or None}),
    added to `board` on the device when there is one."""
    res = eng.score(out, gt, board=board, max_hand=K, cam_trans=out['cam_trans'])
    out['score_result'] = res      # (the per-vertex errors: the 'error' view)
    out['score'] = {'joints': res['joints']['row_f'], 'verts': None if res['verts'] is None else res['verts']['row_f']}


def _check_match(match, gt, match_gate, match_board, show_items=None):
    """match= / match_gate= / match_board= of forward_batch: ValueError before anything runs."""
    if match is None:
        if match_board is not None:
            raise ValueError('match_board= accumulates the counts of match=: it needs match=')
        return
    if match not in ('kp2d', 'joints'):
        raise ValueError("match must be None, 'kp2d' or 'joints', not %r" % (match,))
    if gt is None:
        raise ValueError('match= matches the decoded hands to gt=: it needs gt=')
    if match == 'kp2d' and gt.get('kp2d') is None:
        raise ValueError("match='kp2d' compares pj2d_org with gt['kp2d']: gt does not hold it")
    if not float(match_gate) >= 0:
        raise ValueError('match_gate %r: finite and >= 0, or inf' % (match_gate,))
    if match_board is not None and not hasattr(match_board, 'words'):
        raise ValueError('match_board must be an engine.MatchBoard')
    if 'error' in (show_items or ()):
        raise ValueError("show_items: 'error' is not built with match=: the errors are in truth order")


def _add_match(eng, out, K, gt, board, match, gate, match_board):
    """Engine.match of `out` against gt, then Engine.score of the truth-ordered rows (added to `board` when there is one):
    out['match'] = {'match' [B,K,2], 'cost' [B,K,2], 'G'}, out['score'] = the per-hand rows in TRUTH order."""
    res = eng.match(out, gt, on='joints' if match == 'joints' else 'pj2d_org', gate=gate, max_hand=K, cam_trans=out['cam_trans'],
                    board=match_board)
    G = res['pred_of'].shape[1]
    sc = eng.score(res['out'], res['gt'], board=board, max_hand=G, cam_trans=res['out']['cam_trans'])
    out['match'] = {'match': res['match'], 'cost': res['cost'], 'G': G}
    out['match_result'] = res
    out['score'] = {'joints': sc['joints']['row_f'], 'verts': None if sc['verts'] is None else sc['verts']['row_f']}


def _segm_logits(eng, B):
    """The part logits of the last program run, NHWC [B,256,256,33]: a view of the context's buffer, not a copy."""
    return eng.buffer(eng.program['heads'].segm_buf, B, 33)


def _mask_ids(self, eng, out, imgs, offsets, idx, place):
    """The rasteriser's ids of the hands of `out` over imgs [n,H,W,3] (the frames idx of a _per_size group; drawn into a scratch
    copy): (2 * row + hand) * F + face, so the left hand of every pair is the even mesh."""
    focal = float(self.focal_length)
    if out['slots'].dim() == 3:
        sub, off = _frames_of(out, offsets, idx, ('slots', 'verts', 'cam_trans'))
        return eng.render(sub, imgs, offsets=off, focal_length=focal, return_ids=True)[1]
    B, K = out['slots'].shape[:2]      # K pairs per frame: pair k of frame b is region b * K + k with the frame's own row
    flat = {k: out[k].flatten(0, 1) for k in ('slots', 'verts', 'cam_trans')}
    region_frame = _local_frames(torch.arange(B).repeat_interleave(K), place)
    return eng.render_regions(flat, imgs, torch.as_tensor(offsets).to(torch.float32).repeat_interleave(K, 0), region_frame,
                              focal_length=focal, return_ids=True)[1]


def _add_masks(self, eng, out, iou, frames, offsets):
    """out['masks'] = the statistics of the part segmentation per frame, {'counts': [B,33], 'boxes': [B,2,4], 'agree': [B,2,3]
    or None} (ops.segm_stats): at the resolution of `frames` (a tensor [B,H,W,3] or a list of B frames) under their offsets
    rows, else on the 512 x 512 canvas; iou: with the rasteriser's ids of the same frames."""
    from .. import ops
    B = out['slots'].shape[0]
    offsets = _whole_frame_offsets(B) if offsets is None else offsets
    dev = out['slots'].device
    n_faces = eng._faces['left'].shape[0] if iou and eng._faces.get('left') is not None else None
    if iou and n_faces is None:
        raise ValueError("masks='iou' compares the masks with the drawn meshes: it needs the MANO faces (mano tables with 'faces')")

    def one(imgs, idx, place):
        if imgs is None and iou:
            imgs = torch.zeros(B, 512, 512, 3, dtype=torch.uint8, device=dev)      # a scratch canvas for the rasteriser
        ids = _mask_ids(self, eng, out, imgs, offsets, idx, place) if iou else None
        if idx is None:
            st = eng.segment(B, images=imgs, offsets=offsets, stats=True, ids=ids, labels=False, draw=False)
        else:
            sub, off = _frames_of({'logits': _segm_logits(eng, B)}, offsets, idx, ('logits',))
            st = ops.segm_stats(ops.segm_labels(sub['logits'], imgs.shape[1:3], offsets=off), 33, ids=ids, n_faces=n_faces)
        n = st['counts'].shape[0]
        agree = st['agree'].view(n, 6) if iou else torch.zeros(n, 6, dtype=torch.int32, device=dev)
        return torch.cat([st['counts'], st['boxes'].view(n, 8), agree], 1)      # one row per frame

    rows = one(None, None, None) if frames is None else _per_size(frames, one, count=B)
    rows = (torch.stack(list(rows)) if isinstance(rows, (list, tuple)) else rows).cpu().numpy()
    out['masks'] = {'counts': rows[:, :33], 'boxes': rows[:, 33:41].reshape(B, 2, 4), 'agree': rows[:, 41:].reshape(B, 2, 3) if iou else None}


def mask_keys(ms, b, h):
    """The mask keys of a hand of side h (0 left, 1 right) in frame b from out['masks']: its SIDE's values."""
    counts = ms['counts'][b]
    keys = {'mask_area': np.int32(counts[1:17].sum() if h == 1 else counts[17:33].sum()), 'mask_box': ms['boxes'][b, h].astype(np.int32)}
    if ms['agree'] is not None:
        inter, mask, sil = (int(v) for v in ms['agree'][b, h])
        union = mask + sil - inter
        keys['mask_iou'] = np.float32(inter / union) if union > 0 else np.float32(np.nan)
    return keys


def _add_contact(eng, out, K, mode='vertex'):
    """out['contact'] = Engine.contact of `out` at the package's default parameters, with the parameters beside it."""
    from .. import ops
    kw = {} if mode == 'vertex' else {'mode': mode}
    out['contact'] = dict(eng.contact(out, max_hand=K, cam_trans=out['cam_trans'], **kw), contact_dist=ops.CONTACT_DIST,
                          max_depth=ops.CONTACT_MAX_DEPTH)


def _add_vertex_colors(eng, out, K, items, bgr):
    """out[('vertex_colors', name)] [B,(K,)2,778,3] for the per-vertex colour views among `items`, at the package's default
    parameters, from what _add_contact / _add_score left on `out`."""
    for name in items or ():
        if name == 'contact':
            out[('vertex_colors', name)] = eng.contact_colors(out['contact'], out, max_hand=K, max_depth=out['contact']['max_depth'], bgr=bgr)
        elif name == 'error':
            out[('vertex_colors', name)] = eng.error_colors(out['score_result'], out, max_hand=K, bgr=bgr)


def _contact_keys(con, b, k, h, K, index_of):
    """The four contact keys of hand (row b, rank k, side h): its partner is the flagged hand of the other side in the row whose
    pair has the smallest min_d2, the lower rank on a tie.  con: out['contact'] as host arrays; index_of: (rank, side) -> the
    index in the row's list.  The surface measure (con has 'face', min_d2 is [n,2]): a pair's distance is the smaller min_d2 of
    its two directions; the hand's own direction is h."""
    surface = 'face' in con
    best, rank, pair = np.float32(np.inf), -1, -1
    for q in range(K):
        p = (b * K + k) * K + q if h == 0 else (b * K + q) * K + k
        d = con['min_d2'][p].min() if surface else con['min_d2'][p]
        if d < best:
            best, rank, pair = d, q, p
    if pair < 0:
        return {'contact_dist': np.float32(np.inf), 'contact_with': np.int32(-1), 'contact_verts': np.zeros(0, np.int32),
                'penetration': np.float32(0)}
    r = np.float32(con['contact_dist'])
    touching = (con['face' if surface else 'nn'][pair, h] >= 0) & (con['d2'][pair, h] <= r * r)
    return {'contact_dist': np.sqrt(best, dtype=np.float32), 'contact_with': np.int32(index_of.get((rank, 1 - h), -1)),
            'contact_verts': np.nonzero(touching)[0].astype(np.int32),
            'penetration': np.sqrt(con['depth2'][pair, h], dtype=np.float32)}


def results_from_out(out, paths):
    """What the fused call returned -> {path: [hand dicts]} ({} for a frame without a flagged hand).  out: 'slots' [B,2,176] or
    [B,K,2,176] and 'verts', 'joints', 'pj2d', 'pj2d_org', 'cam_trans' shaped alike (tensors or arrays: nothing here needs
    a device).  A frame lists its flagged left hands in rank order, then its flagged right hands in rank order - torch.cat((l,
    r)) of acr/result_parser.py:166-168; with one pair per frame that is left, right."""
    from .. import _lib as S
    host = {k: (out[k].detach().cpu().numpy() if hasattr(out[k], 'detach') else np.asarray(out[k]))
            for k in ('slots', 'verts', 'joints', 'pj2d', 'pj2d_org', 'cam_trans')}
    slots = host['slots']
    B = slots.shape[0]
    if slots.ndim == 3:
        host = {k: v[:, None] for k, v in host.items()}
        slots = host['slots']
    ids = out.get('track_ids')      # [B,K,2] with tracks=: every hand dict gains 'track_id'
    if ids is not None:
        ids = (ids.detach().cpu().numpy() if hasattr(ids, 'detach') else np.asarray(ids)).reshape(slots.shape[:3])
    if len(paths) != B:
        raise ValueError('one path per frame: %d paths, %d frames' % (len(paths), B))
    con = out.get('contact')      # with contact=True: every hand dict gains the four contact keys
    if con is not None:
        con = {k: (v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)) for k, v in con.items()}
    ms = out.get('masks')      # with masks=: every hand dict gains its side's mask keys
    fl = out.get('fit_loss')      # with refine=: every hand dict gains 'fit_loss' (first, last evaluated step)
    if fl is not None:
        fl = (fl.detach().cpu().numpy() if hasattr(fl, 'detach') else np.asarray(fl)).reshape(slots.shape[:3] + (2,))
    sc = out.get('score')      # with gt=: every hand dict gains the four score keys
    if sc is not None:
        from .. import score as score_mod
        sc = {k: (None if v is None else v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)) for k, v in sc.items()}
    mt = out.get('match')      # with match=: 'gt_index' and 'match_cost', and the score rows are in truth order
    if mt is not None:
        from .. import match as match_mod
        mt = {k: (v.detach().cpu().numpy() if hasattr(v, 'detach') else np.asarray(v)) for k, v in mt.items()}
    results = {}
    for b, path in enumerate(paths):
        hands = []
        where = []
        for h in (0, 1):
            for k in range(slots.shape[1]):
                if slots[b, k, h, S.SLOT_FLAG] > 0.5:
                    s = slots[b, k, h]
                    hands.append({'cam': s[S.SLOT_CAM:S.SLOT_CAM + 3].astype(np.float16),
                                  'cam_trans': host['cam_trans'][b, k, h].astype(np.float16),
                                  'poses': s[S.SLOT_POSES:S.SLOT_POSES + 48].astype(np.float16),
                                  'betas': s[S.SLOT_BETAS:S.SLOT_BETAS + 10].astype(np.float16),
                                  'j3d': host['joints'][b, k, h].astype(np.float16),
                                  'verts': host['verts'][b, k, h].astype(np.float16),
                                  'pj2d': host['pj2d'][b, k, h].astype(np.float16),
                                  'pj2d_org': host['pj2d_org'][b, k, h].astype(np.float16),
                                  'hand_type': np.int32(h), 'detection_flag_cache': True})
                    if ids is not None:
                        hands[-1]['track_id'] = np.int32(ids[b, k, h])
                    if fl is not None:
                        hands[-1]['fit_loss'] = fl[b, k, h].astype(np.float32)
                    row = (b * slots.shape[1] + k) * 2 + h
                    if mt is not None:
                        hands[-1].update(match_mod.hand_match_keys(mt['match'], mt['cost'], row))
                        g = int(mt['match'].reshape(-1)[row])      # the score row of the matched truth; none: nan
                        row = (b * int(mt['G']) + g) * 2 + h if g >= 0 else None
                    if sc is not None:
                        hands[-1].update(score_mod.hand_score_keys(sc if row is not None else {}, row))
                    if ms is not None:
                        hands[-1].update(mask_keys(ms, b, h))
                    where.append((k, h))
        if con is not None:
            index_of = {kh: n for n, kh in enumerate(where)}
            for hand, (k, h) in zip(hands, where):
                hand.update(_contact_keys(con, b, k, h, slots.shape[1], index_of))
        results[path] = hands if hands else {}
    return results


def _multi_views(self, eng, out, frames, offsets, bgr, items):
    """The views of a forward with max_hand = K > 1 over `frames` (a tensor [B,H,W,3] or a list of B frames): pair k of frame b
    is drawn as region b * K + k of frame b with the frame's own offsets row (offsets None: the 512 x 512 network input)."""
    B, K = out['slots'].shape[:2]
    if len(frames) != B:
        raise ValueError('one frame to draw into per input frame')
    rows = (_whole_frame_offsets(B) if offsets is None else torch.as_tensor(offsets).to(torch.float32)).repeat_interleave(K, 0)
    flat = {k: out[k].flatten(0, 1) for k in ('slots', 'verts', 'joints', 'pj2d', 'pj2d_org', 'cam_trans') +
            tuple(('vertex_colors', name) for name in COLOR_ITEMS) if out.get(k) is not None}
    # the centre maps are the frame's, not a pair's: drawn per frame, with pair 0's slots standing for the frame
    return _region_views(self, eng, flat, frames, rows, torch.arange(B).repeat_interleave(K), items, bgr=bgr,
                         centermap=lambda: self._overlay_batch(eng, {'slots': out['slots'][:, 0]}, frames, 'centermap', offsets, bgr),
                         segm=lambda: self._segm_batch(eng, out, frames, offsets, bgr))


def _forward_raw_batch(self, bgr_frames_dev, paths, render=False, show_items=None, streams=None, max_streams=None,
                       pixel_format='bgr', matrix='cv601', boxes=None, box_frame=None, render_format='bgr', region_views=False,
                       max_hand=None, tracks=None, track_gate=None, track_max_miss=None, multi_point_heads=False, contact=False,
                       gt=None, board=None, masks=False, match=None, match_gate=float('inf'), match_board=None, refine=None):
    """BASELINE.json config 4: raw BGR uint8 frames [n,H,W,3] resident in HBM (e.g. 1080p video) - or a LIST of device frames
    [H_i,W_i,3] of different sizes (a folder of images, acr/main.py:144-205) - -> per-image results.  Pre-processing (white square pad + bicubic resize to 512) runs on the GPU (ops.preprocess),
    then the fused path; `offsets` carry the pad geometry so pj2d_org lands in original-frame pixels.
    render=True: -> (results, frames with the hand meshes drawn over them: a tensor like the input, or a list in input order);
    with show_items (names from SHOW_ITEMS) -> (results, {name: frames}) as forward_batch.  streams / max_streams: as
    forward_batch.
    pixel_format='nv12': the frames are NV12 surfaces as a video decoder leaves them (ops.preprocess_nv12 says which layouts),
    converted by the integer rule `matrix` names (ops.nv12_matrix) inside the pre-processing kernel; the results are those
    of the BGR frames ops.nv12_to_bgr makes of them, and those BGR frames - a tensor [n,H,W,3] when all sizes agree, else a
    list - are what render=True / show_items draw over.
    boxes [n,4] = (l, t, r, b) with box_frame [n] (default: box i of frame i): the network sees n REGIONS of the frames at the
    resolution the frames have (ops.preprocess_rois; a person or hand detector's boxes, or acr.utils.boxes_from_keypoints of
    the frame before).  One path per region, results keyed by it, a stream id per region; pj2d_org is in the pixels of the
    ORIGINAL frame.  render=True then needs show_items of 'pj2d' / 'org_img': the skeletons of all regions of a frame are drawn
    over that frame, one drawn frame per source frame.  'mesh' and 'centermap' over regions are a ValueError (the
    rasteriser's viewport is per frame: DESIGN.md "Regions of interest") - unless region_views=True: then every view of
    SHOW_ITEMS is drawn over the source frames with one view per REGION (Engine.render_regions / overlay_regions, DESIGN.md
    "Views over regions"), the default view is 'mesh' as without boxes, and 'centermap' is [2,N,H,W,3] over the N frames.
    refine=: as forward_batch ('kp2d_org' is in the pixels of these frames); not built over regions (boxes=).
    render_format='nv12' (with render=True): the drawn views come back as NV12 surfaces for a video encoder - a tensor
    [n,H*3/2,W] when all sizes agree, else a list; 'centermap' keeps its leading pair.  With pixel_format='nv12' every view is
    composed onto its source surface (ops.nv12_compose: new bytes only where something was drawn) and 'org_img' is the
    surfaces as given; `matrix` is then a name or a pair (row6, row10).  With BGR frames the views go through
    ops.bgr_to_nv12, and `matrix` is a name, a pair or a row of ten integers; H and W must be even.
    max_hand: as forward_batch (None = args().hands_per_side).  With boxes= more than one hand of a side per REGION is a
    ValueError: the box is there because the caller has found the person.
    tracks / track_gate / track_max_miss: as forward_batch; with boxes= a ValueError (ops.track_boxes follows a region).
    multi_point_heads: as forward_batch (without effect with boxes=: a region has one hand of each side).
    contact: as forward_batch.  With boxes= the two hands of a REGION are paired: every region has its own camera, so hands of
    different regions are never paired, also when the regions lie in one frame.
    gt / board: as forward_batch.  With boxes= a region is a row: gt['joints'] is [n,2,21,3] for n regions.
    show_items 'contact' / 'error' (DESIGN.md section 22): as forward_batch, also with render_format='nv12'; with boxes= - and
    in track_raw_batch - a ValueError: the two views over regions are not built at this layer (Engine.render_regions takes
    vertex_colors=).
    show_items 'segm' and masks=: as forward_batch, the masks at the frames' own resolution with
    render=True, also with render_format='nv12'; with boxes= - and 'segm' in track_raw_batch - a ValueError: views and masks
    over regions are not built (several overlapping regions of a frame would need a winner rule).
    match / match_gate / match_board: as forward_batch, gt['kp2d'] in the pixels of the original frames;
    with boxes= a ValueError (a region is one person)."""
    from .utils import img_preprocess_gpu
    _check_multi_point_heads(multi_point_heads)
    _check_contact(contact)
    _check_score(gt, board)
    _check_match(match, gt, match_gate, match_board, check_show_items(show_items))
    if boxes is not None and match is not None:
        raise ValueError('match= with boxes= is not implemented: a region is one person (DESIGN.md section 24)')
    check_color_items(check_show_items(show_items), contact, gt, where=None if boxes is None else 'forward_raw_batch(boxes=)')
    check_masks(masks, where=None if boxes is None else 'forward_raw_batch(boxes=)')
    if boxes is not None:
        check_map_items(check_show_items(show_items), 'forward_raw_batch(boxes=)')
    if boxes is not None and tracks is not None:
        raise ValueError('tracks= with boxes= is not implemented: a region is one person (DESIGN.md section 18)')
    if boxes is not None and int(self.hands_per_side if max_hand is None else max_hand) != 1:
        raise ValueError('boxes= with max_hand > 1 is not implemented: a region is one person (DESIGN.md section 17)')
    to_nv12, matrix = _check_render_args(bgr_frames_dev, show_items, render, render_format, pixel_format, matrix)
    if region_views and boxes is None:
        raise ValueError('region_views=True draws the views of regions: it needs boxes=')
    if boxes is not None and refine is not None:
        raise ValueError('refine= over regions is not built (forward_raw_batch(boxes=))')
    if boxes is not None:
        got = _forward_regions(self, bgr_frames_dev, paths, boxes, box_frame, render, show_items, streams, max_streams,
                               pixel_format, matrix, region_views, contact, gt, board)
    else:
        if box_frame is not None:
            raise ValueError('box_frame says which frame each box is of: it needs boxes=')
        meta = img_preprocess_gpu(bgr_frames_dev, paths, pixel_format=pixel_format, matrix=matrix)
        canvas = None
        if render:
            from .. import ops
            canvas = ops.nv12_to_bgr(bgr_frames_dev, matrix) if pixel_format == 'nv12' else bgr_frames_dev
        got = self.forward_batch(meta['image'], paths, offsets=meta['offsets'], render=canvas,
                                 render_bgr=True, show_items=show_items, streams=streams, max_streams=max_streams,
                                 max_hand=max_hand, tracks=tracks, track_gate=track_gate, track_max_miss=track_max_miss,
                                 multi_point_heads=multi_point_heads, contact=contact, gt=gt, board=board, masks=masks,
                                 match=match, match_gate=match_gate, match_board=match_board, refine=refine)
    if to_nv12 is None:
        return got
    return got[0], _views_to_nv12(to_nv12, got[1])


def _check_render_args(frames, items, render, render_format, pixel_format, matrix):
    """The render arguments of forward_raw_batch / track_raw_batch, refused before anything runs -> (None, matrix), or with
    render_format='nv12' what _nv12_views returns."""
    if items is not None and not render:
        raise ValueError('show_items needs render=True')
    if render_format not in ('bgr', 'nv12'):
        raise ValueError("render_format: %r is not 'bgr' or 'nv12'" % (render_format,))
    if render_format != 'nv12':
        return None, matrix
    if not render:
        raise ValueError("render_format='nv12' needs render=True")
    return _nv12_views(frames, pixel_format, matrix)


def _views_to_nv12(to_nv12, views):
    """`to_nv12` of _nv12_views over a view of the meshes alone or over a dict of views."""
    if not isinstance(views, dict):
        return to_nv12('mesh', views)
    return {name: to_nv12(name, view) for name, view in views.items()}


def _nv12_views(frames, pixel_format, matrix):
    """render_format='nv12' of forward_raw_batch -> (the function that turns one drawn BGR view into NV12 surfaces, the matrix
    of the input side).  Everything that can be refused is refused here, before anything runs."""
    from .. import ops
    if pixel_format == 'nv12':
        row6, row10 = ops._nv12_matrix_pair(matrix)

        def one(drawn):
            return ops.nv12_compose(frames, drawn, matrix=(row6, row10), bgr=True)
    else:
        if isinstance(matrix, str) or (isinstance(matrix, (tuple, list)) and len(matrix) == 2):
            row10 = ops._nv12_matrix_pair(matrix)[1]
        else:
            row10 = ops.nv12_out_matrix(matrix)
        row6 = 'cv601'     # BGR frames pass no input rule: the pre-processing gets the default, not the caller's output row
        items = list(frames.unbind(0)) if isinstance(frames, torch.Tensor) and frames.dim() == 4 else list(frames)
        for i, f in enumerate(items):
            if f.dim() != 3 or f.shape[0] < 2 or f.shape[1] < 2 or f.shape[0] % 2 or f.shape[1] % 2:
                raise ValueError("render_format='nv12': frame %d: NV12 needs H and W even and >= 2, got %s" % (i, tuple(f.shape)))

        def one(drawn):
            return ops.bgr_to_nv12(drawn, matrix=row10, bgr=True)

    def view(name, drawn):
        if name == 'org_img' and pixel_format == 'nv12':
            return frames
        if name != 'centermap':
            return one(drawn)
        if isinstance(drawn, (list, tuple)):      # [2,H_i,W_i,3] per frame: left and right
            left, right = one([d[0] for d in drawn]), one([d[1] for d in drawn])
            return [torch.stack([a, b]) for a, b in zip(left, right)]
        return torch.stack([one(drawn[0]), one(drawn[1])])

    return view, row6


def _region_views(self, eng, out, canvas, offsets, box_frame, items, bgr=True, centermap=None, segm=None):
    """The views `items` (None: the meshes alone, not in a dict) of the n regions of `out` over their frames `canvas` - a
    tensor [N,H,W,3], or a list of frames of different sizes, drawn per size and returned in input order; 'centermap' is
    [2,N,H,W,3], respectively a list of [2,H_i,W_i,3].  offsets: the regions' rows, on the host or on the device.  bgr: the
    frames' channel order.  centermap: a function that draws that view instead of Engine.overlay_regions; segm: the function
    that draws 'segm' (a view of whole frames: there is none over regions)."""
    n = out['slots'].shape[0]
    frame_of = torch.arange(n) if box_frame is None else torch.as_tensor(np.asarray(box_frame)).long()

    def one(name):
        if name == 'centermap' and centermap is not None:
            return centermap()
        if name in MAP_ITEMS:
            if segm is None:
                check_map_items([name], 'region views')
            return segm()

        def draw(imgs, idx, place):
            region_frame = _local_frames(frame_of, place)
            if name == 'mesh' or name in COLOR_ITEMS:
                kw = {} if name == 'mesh' else {'vertex_colors': out[('vertex_colors', name)]}
                return eng.render_regions(out, imgs, offsets, region_frame, focal_length=float(self.focal_length), bgr=bgr, **kw)
            return eng.overlay_regions(out, imgs, name, offsets, region_frame, bgr=bgr)

        return _per_size(canvas, draw, pair=name == 'centermap')

    return _views(items, canvas, one)


def _forward_regions(self, frames, paths, boxes, box_frame, render, show_items, streams, max_streams, pixel_format, matrix,
                     region_views=False, contact=False, gt=None, board=None):
    """forward_raw_batch with boxes."""
    from .. import _lib as S
    from .. import ops
    from .utils import img_preprocess_gpu
    items = check_show_items(show_items)
    check_color_items(items, where='forward_raw_batch(boxes=)')
    if render and not region_views:
        bad = [name for name in (items or ['mesh']) if name not in ('pj2d', 'org_img')]
        if bad:
            raise ValueError('%s over regions is not implemented (the viewport of the rasteriser and of the heat maps is one row '
                             "per frame; two regions of a frame need two): use show_items=('pj2d',)" % ', '.join(repr(b) for b in bad))
    meta = img_preprocess_gpu(frames, paths, pixel_format=pixel_format, matrix=matrix, boxes=boxes, box_frame=box_frame)
    n = meta['image'].shape[0]
    if len(paths) != n:
        raise ValueError('one path per region: %d paths, %d regions' % (len(paths), n))
    results, eng, out = self._fused_call(meta['image'], paths, offsets=meta['offsets'], point_heads=True, streams=streams,
                                         max_streams=max_streams, contact=contact, gt=gt, board=board)
    if not render:
        return results
    canvas = ops.nv12_to_bgr(frames, matrix) if pixel_format == 'nv12' else frames
    if region_views:
        return results, _region_views(self, eng, out, canvas, meta['offsets'], box_frame, items)
    # hand h of region i goes into frame box_frame[i]; a slot without a detection is not drawn
    frame_of = torch.arange(n) if box_frame is None else torch.as_tensor(box_frame).cpu().long()
    flagged = (out['slots'][:, :, S.SLOT_FLAG] > 0.5).cpu()
    hand_frame = torch.where(flagged, frame_of[:, None].expand(n, 2), torch.full((n, 2), -1)).reshape(-1)
    kps = out['pj2d_org'].reshape(-1, 21, 2).float().contiguous()
    return results, _views(items, canvas, lambda name: _draw_over_frames(kps, canvas, hand_frame))


def _draw_over_frames(kps, canvas, hand_frame):
    """ops.draw_skeletons of hands [M,21,2] over a tensor of frames, or over a list of frames of different sizes (one call per
    size, output order = input order); hand_frame [M] = the frame of each hand, -1 = not drawn."""
    from .. import ops
    return _per_size(canvas, lambda imgs, idx, place: ops.draw_skeletons(kps, imgs, hand_frame=_local_frames(hand_frame, place),
                                                                          bgr=True))


def _track_raw_batch(self, frames, paths, boxes=None, box_frame=None, streams=None, max_streams=None, pixel_format='bgr',
                     matrix='cv601', scale=1.5, min_size=64, render=False, show_items=None, render_format='bgr'):
    """One step of a video loop on regions whose boxes stay on the device (DESIGN.md "Tracking on the device") ->
    (results, next_boxes).  frames, paths, box_frame, streams, pixel_format, matrix: as forward_raw_batch(boxes=); boxes: the
    int32 device tensor [n,4] the call before returned as next_boxes, or None for the first frames of a video: the whole
    frames.  results: the dicts forward_raw_batch(boxes=) gives for those boxes.  next_boxes: the regions of the next frames
    (ops.track_boxes: acr.utils.boxes_from_keypoints on the fp32 key points, scale and min_size as there), int32 on the
    device.  Packaging the dicts waits for the device, as it always has; the boxes never pass through the host.
    render=True: -> (results, next_boxes, views): the regions' views drawn over their source frames from the device `offsets`
    rows (DESIGN.md "Views over regions") - the frames with the meshes, or with show_items (names from SHOW_ITEMS)
    {name: frames} as forward_raw_batch(boxes=, region_views=True); a list of frames of different sizes is drawn per size
    and returned in input order.  render_format='nv12': as forward_raw_batch."""
    from .. import ops
    items = check_show_items(show_items)
    check_color_items(items, where='track_raw_batch')
    check_map_items(items, 'track_raw_batch')
    to_nv12, matrix = _check_render_args(frames, items, render, render_format, pixel_format, matrix)
    scale, min_size = ops.check_track_args(scale, min_size)
    frame_hw = ops.region_frame_sizes(frames, box_frame, pixel_format)
    if boxes is None:
        if box_frame is not None:
            raise ValueError('box_frame says which frame each box is of: it needs boxes=')
        boxes = ops.whole_frame_boxes(frames, pixel_format)
    rgb, offsets, _ = ops.preprocess_rois_device(frames, boxes, box_frame, pixel_format=pixel_format, matrix=matrix)
    n = rgb.shape[0]
    if len(paths) != n:
        raise ValueError('one path per region: %d paths, %d regions' % (len(paths), n))
    results, eng, out = self._fused_call(rgb, paths, offsets=offsets, point_heads=True, streams=streams, max_streams=max_streams)
    next_boxes = ops.track_boxes(out['pj2d_org'], out['slots'], frame_hw, scale=scale, min_size=min_size)
    if not render:
        return results, next_boxes
    canvas = ops.nv12_to_bgr(frames, matrix) if pixel_format == 'nv12' else frames
    views = _region_views(self, eng, out, canvas, offsets, box_frame, items)
    return results, next_boxes, views if to_nv12 is None else _views_to_nv12(to_nv12, views)


ACR.forward_raw_batch = _forward_raw_batch
ACR.track_raw_batch = _track_raw_batch


def main(argv=None):
    """python -m <package>.acr.main --demo_mode folder --inputs DIR : runs the path on .npy / image files it can
    read without cv2 (uint8 HxWx3 BGR arrays saved with numpy)."""
    import glob
    import os
    import sys
    a = parse_args(sys.argv[1:] if argv is None else argv)
    with ConfigContext(a):
        acr = ACR(args_set=a)
        files = sorted(glob.glob(os.path.join(a.inputs or '.', '*.npy')))
        for f in files:
            res = acr(np.load(f), f)
            print(f, {k: (len(v) if isinstance(v, list) else 0) for k, v in res.items()})


if __name__ == '__main__':
    main()
