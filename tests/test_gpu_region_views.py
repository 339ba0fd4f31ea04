"""GPU tests of the views over regions (DESIGN.md "Views over regions"): the rasteriser with one view per mesh and the heat-map
kernel that composes the maps of several regions into one frame, against the numpy restatement in tests/region_view_ref.py;
and the calls above them - Engine, EnginePool, ACR - against the stand-alone operators fed the same device data."""
import ctypes

import numpy as np
import pytest
import torch

import nv12_ref as N
import overlay_ref as O
import region_view_ref as V
import render_ref as R
import roi_ref
from conftest import pkg

pytestmark = pytest.mark.gpu

AMBIGUOUS_CAP = 0.01      # the project's: share of the covered pixels whose two nearest surfaces are within 1e-5 relative
FH, FW = 96, 160          # the dword path of the heat-map kernel
SH, SW = 37, 53           # its byte path
SCALE, MIN_SIZE = 1.0, 32      # tests/test_gpu_track.py's: at the defaults every box of the synthetic checkpoint is the whole frame
_cache = {}


def _images(n, h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3)).astype(np.uint8)


def _offsets(H, W, boxes):
    return np.stack([np.asarray(roi_ref.offsets(H, W, b), np.float32) for b in boxes])


# ---- meshes ---------------------------------------------------------------------------------------------------------------
MH, MW = 208, 240
# frame 0: a 100-pixel and a 200-pixel window that overlap (sx = 0.195 and 0.39) and one cut by the frame's corner (60 x 58
# pixels are left of a 120-pixel box: not square, pads not zero); frame 1: one region; the last mesh goes nowhere
MESH_BOXES = [(20, 20, 120, 120), (30, 4, 230, 204), (180, 150, 300, 270), (60, 40, 188, 168), (20, 20, 120, 120)]
MESH_FRAME = [0, 0, 0, 1, -1]


def _on_canvas(cx, cy, Z, focal=1265.0):
    """Camera-space centre that projects to canvas (cx, cy) at depth Z."""
    return ((cx - 256.0) * Z / focal, (cy - 256.0) * Z / focal, Z)


def _mesh_case():
    if 'mesh' not in _cache:
        offsets = _offsets(MH, MW, MESH_BOXES)
        views = np.stack([V.view_row(o) for o in offsets])
        assert abs(views[0][0] - 0.1953) < 1e-3 and abs(views[1][0] - 0.3906) < 1e-3
        assert offsets[2][6] > 0 and offsets[2][8] > 0 and views[2][0] == np.float32(60 / 512)      # padded above and below
        axes = (0.05, 0.09, 0.03)
        # region 0's mesh at Z = 0.8 in the middle of its window: frame (70, 70).  Region 1's at Z = 0.9 around frame (100, 90),
        # over the right part of it: canvas ((100 - 30) / 0.39, (90 - 4) / 0.39).  Plain 1/Z would order 1.25 before 1.11; sx/Z orders 0.244 behind 0.434.
        centres = [_on_canvas(256, 256, 0.8), _on_canvas(179, 220, 0.9), _on_canvas(200, 180, 0.85), _on_canvas(230, 270, 0.8),
                   _on_canvas(256, 256, 0.8)]
        verts = np.stack([R.ellipsoid(24, 32, axes, c)[0] for c in centres])
        faces = R.ellipsoid(24, 32, axes, centres[0])[1]
        images = _images(2, MH, MW, seed=3)
        colors = np.array([[0.46, 0.59, 0.64], [0.94, 0.71, 0.53], [0.3, 0.9, 0.4], [0.8, 0.2, 0.5], [1, 1, 1]], np.float32)
        ref = V.render(verts, faces, images, MESH_FRAME, views, colors=colors)
        alone = [V.render(verts, faces, images, [f if k == m else -1 for k, f in enumerate(MESH_FRAME)], views, colors=colors)['ids'] >= 0
                 for m in (0, 1)]
        _cache['mesh'] = dict(verts=verts, faces=faces, images=images, views=views, colors=colors, ref=ref, both=alone[0] & alone[1])
    return _cache['mesh']


def _compare(got_out, got_ids, ref, images, what=''):
    """The rules of tests/test_gpu_render.py's _compare."""
    cov = ref['ids'] >= 0
    amb = R.ambiguous(ref)
    n_cov, n_amb = int(cov.sum()), int(amb.sum())
    id_bad = int(((got_ids != ref['ids']) & cov & ~amb).sum())
    diff = np.abs(got_out.astype(np.int64) - ref['out'].astype(np.int64)).max(-1)
    col_worst = int(diff[cov & ~amb].max()) if (cov & ~amb).any() else 0
    print('%s: covered %d, ambiguous %d (%.4f %%), mask mismatches %d, id mismatches outside ambiguous %d, worst colour '
          'difference %d' % (what, n_cov, n_amb, 100.0 * n_amb / max(n_cov, 1), int(((got_ids >= 0) != cov).sum()), id_bad,
                             col_worst))
    assert ((got_ids >= 0) == cov).all(), 'covered mask differs from the integer rule'
    assert n_amb <= AMBIGUOUS_CAP * max(n_cov, 1)
    assert id_bad == 0
    assert col_worst <= 1
    assert (got_out[~cov] == images[~cov]).all(), 'an uncovered pixel changed'
    return n_cov


def _render(c, **kw):
    ops = pkg('ops')
    out, ids = ops.render_meshes(torch.from_numpy(c['verts']).cuda(), c['faces'], torch.from_numpy(c['images']).cuda(),
                                 colors=torch.from_numpy(c['colors']), return_ids=True, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ids.cpu().numpy()


def test_meshes_of_regions_against_the_restatement():
    c = _mesh_case()
    ref, F = c['ref'], len(c['faces'])
    got, ids = _render(c, mesh_frame=torch.tensor(MESH_FRAME), mesh_view=torch.from_numpy(c['views']))
    n_cov = _compare(got, ids, ref, c['images'], 'meshes of four regions in two frames')
    assert n_cov > 3000
    seen = sorted(np.unique(ids[ids >= 0] // F).tolist())
    assert seen == [0, 1, 2, 3], seen      # every drawn mesh is visible somewhere, the one with frame -1 nowhere
    assert (ids[1][ids[1] >= 0] // F == 3).all() and (ids[0][ids[0] >= 0] // F != 3).all()
    # where the meshes of the two overlapping regions both cover a pixel the LARGE region's is in front: sx / Z, not 1 / Z
    both = c['both'][0]
    assert both.sum() > 300
    assert (ref['ids'][0][both] // F == 1).all() and (ids[0][both] // F == 1).all()
    # the mesh of the small region is drawn outside its region's window too (it is not clipped), and some of it is visible
    assert (ids[0] // F == 0).any()


def test_per_mesh_view_reduces_to_the_per_frame_view():
    """One region per frame: mesh_view = view[mesh_frame] draws what view does - the same covered mask, ids and colours
    equal outside the pixels whose two nearest surfaces fp32 cannot be asked to order (the depth values differ by the
    factor sx, so their roundings do)."""
    c = _mesh_case()
    F = len(c['faces'])
    frames = [0, 1, 0, 1, -1]
    view = np.stack([c['views'][1], c['views'][3]])      # the view of frame 0 and of frame 1
    per_mesh = np.stack([view[max(f, 0)] for f in frames])
    ref = R.render(c['verts'], c['faces'], c['images'], mesh_frame=frames, colors=c['colors'], view=view)
    a_out, a_ids = _render(c, mesh_frame=torch.tensor(frames), view=torch.from_numpy(view))
    b_out, b_ids = _render(c, mesh_frame=torch.tensor(frames), mesh_view=torch.from_numpy(per_mesh))
    _compare(a_out, a_ids, ref, c['images'], 'per-frame view')
    amb = R.ambiguous(ref)
    assert ((a_ids >= 0) == (b_ids >= 0)).all()
    assert (a_ids[~amb] == b_ids[~amb]).all()
    assert np.abs(a_out.astype(int) - b_out.astype(int))[~amb].max() <= 1
    assert (a_ids >= 0).sum() > 3000 and sorted(np.unique(a_ids[a_ids >= 0] // F).tolist()) == [0, 1, 2, 3]
    with pytest.raises(ValueError, match='exclude each other'):
        _render(c, view=torch.from_numpy(view), mesh_view=torch.from_numpy(per_mesh))
    with pytest.raises(ValueError, match=r'mesh_view must be \[M,4\]'):
        _render(c, mesh_frame=torch.tensor(frames), mesh_view=torch.from_numpy(view))


# ---- heat maps ------------------------------------------------------------------------------------------------------------
def _heat_case(H, W):
    """Regions of two H x W frames: overlapping windows, a window across the tile borders at x = 128 and y = 32 (where the
    frame has them), a window of 3 x 5 pixels (its footprint is the whole map: the unstaged path), a region with an empty
    window, a NaN row, a zero row, frame indices -1 and 2."""
    key = ('heat', H, W)
    if key not in _cache:
        s = W / 160.0
        boxes = [(int(10 * s), 10 * H // 96, int(90 * s), 90 * H // 96), (int(50 * s), 20 * H // 96, int(140 * s), H),
                 (int(100 * s), 10 * H // 96, int(150 * s), 60 * H // 96), (int(20 * s), 70 * H // 96, int(20 * s) + 3, 70 * H // 96 + 5),
                 (-30, -20, int(60 * s), 50 * H // 96), (0, 0, W, H), (int(30 * s), 5, int(120 * s), H - 5)]
        frames = [0, 0, 0, 0, 1, 1, 0]
        offsets = _offsets(H, W, boxes)
        empty = offsets[0].copy(); empty[5] = W                      # the crop leaves no pixel
        nan_row = np.full(10, np.nan, np.float32)
        part_nan = offsets[1].copy(); part_nan[9] = np.nan              # the view's shift is NaN, the window is not
        zero = np.zeros(10, np.float32)
        offsets = np.concatenate([offsets, np.stack([empty, nan_row, part_nan, zero, offsets[0], offsets[1]])])
        frames = frames + [0, 0, 0, 1, -1, 2]
        maps = np.stack([O.gaussian_maps(len(frames), 64, 64, seed=5 + H, peaks=3), O.gaussian_maps(len(frames), 64, 64, seed=6 + H, peaks=3)], 1)
        maps[2, 0, 10, 10] = np.nan      # a NaN cell: index 0
        _cache[key] = dict(maps=maps, offsets=offsets, frames=np.array(frames, np.int32), images=_images(2, H, W, seed=H))
    return _cache[key]


def _draw(c, maps=None, **kw):
    ops = pkg('ops')
    maps = c['maps'] if maps is None else maps
    out = ops.draw_region_heatmaps(torch.from_numpy(maps).cuda(), torch.from_numpy(c['images']).cuda(), torch.from_numpy(c['offsets']),
                                   torch.from_numpy(c['frames']), **kw)
    torch.cuda.synchronize()
    return out


def _want(c, side, **kw):
    return V.draw_region_heatmaps(c['maps'][:, side], c['images'], c['offsets'], c['frames'], **kw)


@pytest.mark.parametrize('H,W', [(FH, FW), (SH, SW)])
def test_region_heat_maps_are_the_restatement_byte_for_byte(H, W):
    ops = pkg('ops')
    c = _heat_case(H, W)
    got = _draw(c)
    assert tuple(got.shape) == (2, 2, H, W, 3) and got.dtype == torch.uint8
    for side in (0, 1):
        want = _want(c, side)
        bad = int((got[side].cpu().numpy() != want).any(-1).sum())
        print('%d x %d side %d: %d pixels differ, %d tinted' % (H, W, side, bad, int((want != c['images']).any(-1).sum())))
        assert bad == 0
    idx = V.heatmap_indices(c['maps'][:, 0], c['offsets'], c['frames'], 2, H, W)
    assert (idx[0] < 0).any() and (idx[0] >= 0).any(), 'frame 0 has covered and uncovered pixels'
    assert (got[0].cpu().numpy()[idx < 0] == c['images'][idx < 0]).all(), 'an uncovered pixel changed'
    # one map per region; BGR; a table and a weight of the caller's
    one = _draw(c, maps=np.ascontiguousarray(c['maps'][:, 1]))
    assert tuple(one.shape) == (2, H, W, 3) and torch.equal(one, got[1])
    lut = np.random.default_rng(1).integers(0, 256, (256, 3)).astype(np.uint8)
    assert (_draw(c, bgr=True)[0].cpu().numpy() == _want(c, 0, bgr=True)).all()
    assert (_draw(c, lut=lut, weight=0.35)[1].cpu().numpy() == _want(c, 1, lut=lut, weight=0.35)).all()
    # two calls are bit-identical; in place equals out of place
    assert torch.equal(_draw(c), got)
    dst = torch.empty(2, 2, H, W, 3, dtype=torch.uint8, device='cuda')
    dst[0] = torch.from_numpy(c['images']).cuda()
    same = ops.draw_region_heatmaps(torch.from_numpy(c['maps']).cuda(), dst[0], torch.from_numpy(c['offsets']),
                                    torch.from_numpy(c['frames']), dst=dst)
    assert same.data_ptr() == dst.data_ptr() and torch.equal(dst, got)
    # a frame drawn alone equals the same frame drawn in the batch
    for f in (0, 1):
        alone = dict(c, images=c['images'][f:f + 1], frames=np.where(c['frames'] == f, 0, -1).astype(np.int32))
        assert torch.equal(_draw(alone)[:, 0], got[:, f])


def test_three_regions_of_300_belong_to_the_frame():
    """The 256-wide scan: regions 0, 257 and 299 are frame 0's, the others belong to frame 1 (small windows), to no frame or
    to a frame that does not exist."""
    g = np.random.default_rng(300)
    n = 300
    frames = np.where(np.arange(n) % 3 == 0, 1, np.where(np.arange(n) % 3 == 1, -1, 7)).astype(np.int32)
    boxes = []
    for i in range(n):
        l, t = int(g.integers(0, FW - 24)), int(g.integers(0, FH - 24))
        boxes.append((l, t, l + int(g.integers(8, 24)), t + int(g.integers(8, 24))))
    for i, box in ((0, (5, 5, 100, 90)), (257, (60, 20, 150, 96)), (299, (120, 0, 160, 40))):
        frames[i], boxes[i] = 0, box
    c = dict(maps=O.gaussian_maps(n, 64, 64, seed=9, peaks=2)[:, None].repeat(2, 1), offsets=_offsets(FH, FW, boxes), frames=frames,
             images=_images(2, FH, FW, seed=8))
    c['maps'][:, 1] = c['maps'][::-1, 0]
    got = _draw(c)
    for side in (0, 1):
        assert (got[side].cpu().numpy() == _want(c, side)).all()
    only = dict(c, frames=np.where(np.isin(np.arange(n), (0, 257, 299)), 0, -1).astype(np.int32))
    assert torch.equal(_draw(only)[:, 0], got[:, 0])
    assert not torch.equal(got[0, 0], torch.from_numpy(c['images'][0]).cuda())


@pytest.mark.parametrize('H,W', [(FH, FW), (SH, SW)])
def test_one_whole_frame_region_per_frame_is_draw_heatmaps(H, W):
    ops = pkg('ops')
    c = _heat_case(H, W)
    maps = torch.from_numpy(c['maps'][:2]).cuda()
    images = torch.from_numpy(c['images']).cuda()
    offsets = torch.from_numpy(_offsets(H, W, [(0, 0, W, H)] * 2))
    want = ops.draw_heatmaps(maps, images, view=ops.view_from_offsets(offsets))
    got = ops.draw_region_heatmaps(maps, images, offsets, [0, 1])
    assert torch.equal(got, want) and not torch.equal(got[0], images)


# ---- Engine, EnginePool, ACR ------------------------------------------------------------------------------------------------
BOXES = [(20, 10, 121, 90), (0, 0, 101, 61), (31, 7, 160, 96)]      # tests/test_gpu_track.py's three regions of two frames
BOX_FRAME = [1, 0, 1]


@pytest.fixture(scope='module')
def near_sd():
    return pkg('synth').make_state_dict(seed=10)      # the checkpoint of tests/test_gpu_track.py: it detects hands


def _video():
    """(the NV12 surfaces, their BGR frames as one tensor [2,96,160,3]): tests/test_gpu_track.py's two frames."""
    if 'video' not in _cache:
        nv12 = [torch.from_numpy(np.concatenate(N.random_nv12(FH, FW, s), 0)).cuda() for s in (11, 12)]
        _cache['video'] = (nv12, pkg('ops').nv12_to_bgr(nv12))
    return _cache['video']


def _dev_boxes(boxes):
    return torch.tensor([list(b) for b in boxes], dtype=torch.int32).cuda()


def _expected(out, frames, mano_tables, focal=1265.0):
    """The stand-alone operators fed what the engine's calls read: -> (mesh frames, ids, heat maps, skeletons)."""
    ops, L = pkg('ops'), pkg('_lib')
    n = out['slots'].shape[0]
    offsets = out['offsets'].cpu()
    region_frame = torch.tensor(BOX_FRAME)
    flags = (out['slots'][:, :, L.SLOT_FLAG] > 0.5).cpu()
    hand_frame = torch.where(flags, region_frame[:, None].expand(n, 2), torch.full((n, 2), -1)).reshape(-1)
    cam_trans = out.get('cam_trans')
    if cam_trans is None:
        cam_trans = ops.cam_trans(out['joints'].view(-1, 21, 3), out['pj2d'].view(-1, 21, 2), focal_length=focal)
    mesh, ids = ops.render_meshes(out['verts'].view(2 * n, 778, 3), (mano_tables['left']['faces'], mano_tables['right']['faces']),
                                  frames, mesh_frame=hand_frame, trans=cam_trans.reshape(-1, 3),
                                  colors=torch.tensor(ops.HAND_COLORS_RGB).flip(1).repeat(n, 1), focal_length=focal,
                                  mesh_view=ops.view_from_offsets(offsets).repeat_interleave(2, 0),
                                  topo_index=torch.tensor([0, 1]).repeat(n), return_ids=True)
    heat = ops.draw_region_heatmaps(out['center_maps'], frames, offsets, region_frame, bgr=True)
    skel = ops.draw_skeletons(out['pj2d_org'].reshape(-1, 21, 2), frames, hand_frame=hand_frame.to(torch.int32), bgr=True)
    return mesh, ids, heat, skel


def test_engine_views_over_the_regions_of_a_track_step(near_sd, mano_tables):
    L = pkg('_lib')
    eng = pkg('engine').Engine(0)
    eng.load_state_dict(near_sd, max_batch=3)
    eng.load_mano(mano_tables)
    frames = _video()[1]
    boxes = _dev_boxes(BOXES)
    region_frame = torch.tensor(BOX_FRAME, dtype=torch.int32).cuda()
    warm, _, _ = eng.track_step(frames, boxes, box_frame=BOX_FRAME, scale=SCALE, min_size=MIN_SIZE)
    eng.render_regions(warm, frames, warm['offsets'], region_frame)      # (the context's scratch is allocated at the first call)
    eng.overlay_regions(warm, frames, 'pj2d', warm['offsets'], region_frame)
    torch.cuda.synchronize()
    # the three calls behind a track step, under a mode in which torch raises on every call that waits for the device
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            boxes.sum().item()      # the mode is honoured by this build
        out, nxt, status = eng.track_step(frames, boxes, box_frame=BOX_FRAME, scale=SCALE, min_size=MIN_SIZE)
        mesh, ids = eng.render_regions(out, frames, out['offsets'], region_frame, bgr=True, return_ids=True)
        heat = eng.overlay_regions(out, frames, 'centermap', out['offsets'], region_frame, bgr=True)
        skel = eng.overlay_regions(out, frames, 'pj2d', out['offsets'], region_frame, bgr=True)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    out['center_maps'] = eng.center_maps(3)
    assert (out['slots'][:, :, L.SLOT_FLAG] > 0.5).any(), 'no hand detected'
    want_mesh, want_ids, want_heat, want_skel = _expected(out, frames, mano_tables)
    assert torch.equal(mesh, want_mesh) and torch.equal(ids, want_ids)
    assert torch.equal(heat, want_heat) and tuple(heat.shape) == (2, 2, FH, FW, 3)
    assert torch.equal(skel, want_skel)
    assert not torch.equal(heat[0], frames) and not torch.equal(skel, frames)
    # host lists are taken too; in place
    work = frames.clone()
    assert eng.overlay_regions(out, work, 'pj2d', out['offsets'].cpu(), BOX_FRAME, bgr=True, dst=work).data_ptr() == work.data_ptr()
    assert torch.equal(work, skel)
    with pytest.raises(ValueError, match=r'offsets must be \[n,10\]'):
        eng.render_regions(out, frames, out['offsets'][:2], region_frame)
    with pytest.raises(ValueError, match='one integer per region'):
        eng.overlay_regions(out, frames, 'centermap', out['offsets'], region_frame[:2])
    # a real context refuses bad arguments with ACRMI_EINVAL
    p = ctypes.c_void_p(frames.data_ptr())
    assert eng.L.acrmi_render_regions(eng.ctx, p, p, p, 0, p, p, None, 1265.0, 0.9, p, p, 2, FH, FW, None, None) == L.E_INVAL
    assert eng.L.acrmi_render_regions(eng.ctx, p, p, p, 3, None, p, None, 1265.0, 0.9, p, p, 2, FH, FW, None, None) == L.E_INVAL
    assert eng.L.acrmi_overlay_regions(eng.ctx, 2, p, p, 3, p, p, 1, p, p, None, 2, FH, FW, None) == L.E_INVAL
    assert eng.L.acrmi_overlay_regions(eng.ctx, L.OVERLAY_CENTERMAP, None, None, 3, p, p, 1, p, p, p, 2, FH, FW, None) == L.E_INVAL
    eng.close()
    # the same on a ticket of an EnginePool
    ops = pkg('ops')
    pool = pkg('engine').EnginePool(0, n=2)
    pool.load_state_dict(near_sd, max_batch=3)
    pool.load_mano(mano_tables)
    for _ in range(2):      # both contexts
        rgb, offsets, _ = ops.preprocess_rois_device(frames, boxes, BOX_FRAME)
        t = pool.submit(rgb, offsets=offsets, project=True)
        got_mesh, got_ids = pool.render_regions(t, frames, offsets, region_frame, bgr=True, return_ids=True)
        got_heat = pool.overlay_regions(t, frames, 'centermap', offsets, region_frame, bgr=True)
        got_skel = pool.overlay_regions(t, frames, 'pj2d', offsets, region_frame, bgr=True)
        pool.collect(t)
        assert torch.equal(got_mesh, mesh) and torch.equal(got_ids, ids) and torch.equal(got_heat, heat) and torch.equal(got_skel, skel)
    with pytest.raises(RuntimeError, match='between submit'):
        pool.render_regions(t, frames, offsets, region_frame)
    pool.close()


def test_acr_layer_draws_every_view_over_regions(near_sd, mano_tables):
    cfg, ops, utils = pkg('config'), pkg('ops'), pkg('acr.utils')
    acr = pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml', '--renderer', 'hip']),
                              state_dict=near_sd, mano_tables=mano_tables, max_batch=3)
    nv12, frames = _video()
    bgr = frames
    paths = ['a', 'b', 'c']
    items = ('mesh', 'pj2d', 'centermap', 'org_img')
    boxes = np.array(BOXES, np.int32)
    kw = dict(scale=SCALE, min_size=MIN_SIZE)
    res, nxt, views = acr.track_raw_batch(frames, paths, boxes=_dev_boxes(BOXES), box_frame=BOX_FRAME, render=True, show_items=items, **kw)
    plain, nxt0 = acr.track_raw_batch(frames, paths, boxes=_dev_boxes(BOXES), box_frame=BOX_FRAME, **kw)
    assert sorted(res) == sorted(plain) and torch.equal(nxt, nxt0) and sorted(views) == sorted(items)
    # the engine's calls on the same forward
    meta = utils.img_preprocess_gpu(frames, paths, boxes=boxes, box_frame=BOX_FRAME)
    eng = acr.model.engine(3)
    eng.set_point_heads(True)
    try:
        out = eng.forward(meta['image'], offsets=meta['offsets'], project=True)
    finally:
        eng.set_point_heads(False)
    focal = float(acr.focal_length)
    out['cam_trans'] = ops.cam_trans(out['joints'].view(-1, 21, 3), out['pj2d'].view(-1, 21, 2), focal_length=focal).view(3, 2, 3)
    want = {'mesh': eng.render_regions(out, frames, meta['offsets'], BOX_FRAME, focal_length=focal, bgr=True),
            'pj2d': eng.overlay_regions(out, frames, 'pj2d', meta['offsets'], BOX_FRAME, bgr=True),
            'centermap': eng.overlay_regions(out, frames, 'centermap', meta['offsets'], BOX_FRAME, bgr=True), 'org_img': frames}
    for name in items:
        assert torch.equal(views[name], want[name]), name
    assert not torch.equal(views['mesh'], frames) or not torch.equal(views['pj2d'], frames)
    # without show_items: the meshes alone
    _, _, mesh = acr.track_raw_batch(frames, paths, boxes=_dev_boxes(BOXES), box_frame=BOX_FRAME, render=True, **kw)
    assert torch.equal(mesh, want['mesh'])
    # forward_raw_batch draws the same views with the keyword, and refuses them without it as it always has
    res2, views2 = acr.forward_raw_batch(frames, paths, boxes=boxes, box_frame=BOX_FRAME, render=True, show_items=items, region_views=True)
    assert sorted(res2) == sorted(res) and all(torch.equal(views2[name], want[name]) for name in items)
    _, mesh2 = acr.forward_raw_batch(frames, paths, boxes=boxes, box_frame=BOX_FRAME, render=True, region_views=True)
    assert torch.equal(mesh2, want['mesh'])
    with pytest.raises(ValueError, match='over regions is not implemented'):
        acr.forward_raw_batch(frames, paths, boxes=boxes, box_frame=BOX_FRAME, render=True, show_items=('mesh',))
    with pytest.raises(ValueError, match='over regions is not implemented'):
        acr.forward_raw_batch(frames, paths, boxes=boxes, box_frame=BOX_FRAME, render=True)
    with pytest.raises(ValueError, match='needs boxes='):
        acr.forward_raw_batch(frames, ['a', 'b'], render=True, region_views=True)
    # NV12 out: the BGR views through ops.bgr_to_nv12; NV12 in and out: composed onto the source surfaces
    _, _, as_nv12 = acr.track_raw_batch(frames, paths, boxes=_dev_boxes(BOXES), box_frame=BOX_FRAME, render=True, show_items=items,
                                        render_format='nv12', **kw)
    for name in ('mesh', 'pj2d', 'org_img'):
        assert torch.equal(as_nv12[name], ops.bgr_to_nv12(want[name], bgr=True)), name
    assert torch.equal(as_nv12['centermap'], torch.stack([ops.bgr_to_nv12(want['centermap'][s], bgr=True) for s in (0, 1)]))
    _, _, composed = acr.track_raw_batch(nv12, paths, boxes=_dev_boxes(BOXES), box_frame=BOX_FRAME, pixel_format='nv12', render=True,
                                         show_items=('mesh', 'pj2d'), render_format='nv12', **kw)
    for name in ('mesh', 'pj2d'):
        assert torch.equal(torch.stack(list(composed[name])), torch.stack(list(ops.nv12_compose(nv12, want[name], bgr=True)))), name
    # frames of two sizes: drawn per size, returned in input order
    small = torch.from_numpy(_images(1, 64, 80, seed=4)[0]).cuda()
    mixed = [bgr[0], small, bgr[1]]
    boxes3 = [BOXES[1], (0, 0, 80, 64), BOXES[0]]
    _, _, per_size = acr.track_raw_batch(mixed, paths, boxes=_dev_boxes(boxes3), box_frame=[0, 1, 2], render=True,
                                         show_items=('mesh', 'centermap', 'pj2d'), **kw)
    assert [tuple(v.shape) for v in per_size['mesh']] == [(FH, FW, 3), (64, 80, 3), (FH, FW, 3)]
    assert [tuple(v.shape) for v in per_size['centermap']] == [(2, FH, FW, 3), (2, 64, 80, 3), (2, FH, FW, 3)]
    meta = utils.img_preprocess_gpu(mixed, paths, boxes=np.array(boxes3, np.int32), box_frame=[0, 1, 2])
    eng = acr.model.engine(3)
    eng.set_point_heads(True)
    try:
        out = eng.forward(meta['image'], offsets=meta['offsets'], project=True)
    finally:
        eng.set_point_heads(False)
    out['cam_trans'] = ops.cam_trans(out['joints'].view(-1, 21, 3), out['pj2d'].view(-1, 21, 2), focal_length=focal).view(3, 2, 3)
    big = eng.render_regions(out, torch.stack([bgr[0], bgr[1]]), meta['offsets'], [0, -1, 1], focal_length=focal, bgr=True)
    little = eng.overlay_regions(out, small[None], 'centermap', meta['offsets'], [-1, 0, -1], bgr=True)
    assert torch.equal(per_size['mesh'][0], big[0]) and torch.equal(per_size['mesh'][2], big[1])
    assert torch.equal(per_size['centermap'][1], little[:, 0]) and not torch.equal(little[0, 0], small)
