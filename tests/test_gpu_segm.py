"""GPU tests of the part segmentation as an output against the numpy restatement in tests/segm_ref.py:
labels, view bytes, counts, boxes and agree are EQUAL to it - no tolerance, no excluded pixels - on the staged and the unstaged
path of segm_kernel, the dword and the byte rows, whole cells in 16-byte pieces and class by class; then Engine.segment,
EnginePool.segment and the acr layer against the operators on the same forward."""
import ctypes

import numpy as np
import pytest
import torch

import overlay_ref as O
import region_view_ref as V
import segm_ref as SR
from conftest import pkg
from contact_cases import eng, frames3, near_sd      # (fixtures)

pytestmark = pytest.mark.gpu

F32 = np.float32
INF, NAN = float('inf'), float('nan')
WHOLE = [512., 512, 0, 0, 0, 0, 0, 0, 0, 0]      # the offsets row of a frame that is the 512 x 512 canvas


def _logits(n, h, w, ps, C, seed, quantum=None):
    """Smooth logits with noise, NHWC [n,h,w,ps]; channels beyond C hold 1e9 (a kernel that looked at them would show it);
    quantum: the values are multiples of it, so that interpolated values tie exactly."""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(n, C, max(h // 8, 2), max(w // 8, 2), generator=g) * 3
    x = torch.nn.functional.interpolate(low, size=(h, w), mode='bicubic', align_corners=False) + 0.3 * torch.randn(n, C, h, w, generator=g)
    x = x.permute(0, 2, 3, 1).numpy().astype(F32)
    if quantum:
        x = (np.round(x / quantum) * quantum).astype(F32)
    out = np.full((n, h, w, ps), 1e9, F32)
    out[..., :C] = x
    return out


def _images(n, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3)).astype(np.uint8)


def _gpu(logits, C, images=None, hw=None, **kw):
    """-> (view or None, labels) as numpy, through ops.draw_segm / ops.segm_labels on a [..., :C] slice of the padded buffer."""
    ops = pkg('ops')
    t = torch.from_numpy(logits).cuda()[..., :C]
    if images is None:
        return None, ops.segm_labels(t, hw, **kw).cpu().numpy()
    out, lab = ops.draw_segm(t, torch.from_numpy(images).cuda(), labels=True, **kw)
    return out.cpu().numpy(), lab.cpu().numpy()


CASES = {      # (n, h, w, pix_stride, C, H, W, view rows or None)
    'tiny3-byte': (1, 8, 8, 3, 3, 97, 203, None),
    'tiny5-dword': (3, 8, 8, 36, 5, 64, 128, None),
    'mid5-byte': (3, 40, 56, 5, 5, 97, 203, None),
    'mid33-dword': (1, 40, 56, 36, 33, 64, 128, None),
    'net-byte': (1, 256, 256, 36, 33, 97, 203, None),
    'net-scalar-cells': (3, 256, 256, 33, 33, 64, 128, None),
    'net-unstaged': (1, 256, 256, 36, 33, 16, 16, None),
    'net-unstaged-3': (3, 256, 256, 36, 3, 16, 16, None),
    'net-512': (1, 256, 256, 36, 33, 512, 512, None),
    'views': (3, 40, 56, 36, 33, 97, 203, [[0.4, 0.2, -3.25, 1.5], [0.11, 0.07, 30.5, 20.0], [1.0, 1.0, -400.0, -500.0]]),
}


@pytest.mark.parametrize('name', list(CASES))
def test_labels_and_view_equal_the_restatement(name):
    ops = pkg('ops')
    n, h, w, ps, C, H, W, view = CASES[name]
    logits, img = _logits(n, h, w, ps, C, seed=len(name)), _images(n, H, W, seed=n)
    v = None if view is None else np.array(view, F32)
    want = SR.labels(logits, C, H, W, v)
    want_view = SR.draw(img, want, C)
    kw = {} if v is None else {'view': torch.from_numpy(v)}
    out, lab = _gpu(logits, C, img, **kw)
    bad = int((lab != want).sum())
    print('%s: %d of %d labels differ, %d view bytes differ; labels present %d, uncovered %d' %
          (name, bad, want.size, int((out != want_view).sum()), len(np.unique(want)), int((want == SR.NONE).sum())))
    assert lab.dtype == np.uint8 and np.array_equal(lab, want)
    assert np.array_equal(out, want_view)
    assert ((want >= 1) & (want < C)).any() and (out != img).any()      # the case draws something
    # labels only, view only, in place, twice, and the frames one at a time: the same bytes
    t, im = torch.from_numpy(logits).cuda()[..., :C], torch.from_numpy(img).cuda()
    assert np.array_equal(_gpu(logits, C, None, (H, W), **kw)[1], lab)
    assert torch.equal(ops.draw_segm(t, im, **kw), torch.from_numpy(out).cuda())
    same = im.clone()
    assert ops.draw_segm(t, same, dst=same, **kw) is same and np.array_equal(same.cpu().numpy(), out)
    again = _gpu(logits, C, img, **kw)
    assert np.array_equal(again[0], out) and np.array_equal(again[1], lab)
    if n > 1:
        for i in range(n):
            one = _gpu(logits[i:i + 1], C, img[i:i + 1], **({} if v is None else {'view': torch.from_numpy(v[i:i + 1])}))
            assert np.array_equal(one[0][0], out[i]) and np.array_equal(one[1][0], lab[i]), i


def test_partial_canvas_and_views_that_draw_nothing():
    n, C, H, W = 5, 33, 64, 128
    logits, img = _logits(n, 40, 56, 36, C, seed=2), _images(n, H, W, seed=5)
    view = np.array([[0.5, 0.5, 40.0, 10.0],      # the canvas covers x in [40, 296), y in [10, 266): partial
                     [-0.25, 0.125, 0, 0],        # faces away
                     [NAN, 0.125, 0, 0], [0.25, 0.125, NAN, 0], [0.25, 0.0, 0, 0]], F32)
    want = SR.labels(logits, C, H, W, view)
    assert (want[0][:, :40] == SR.NONE).all() and (want[0][:10] == SR.NONE).all() and (want[0][10:, 40:] < C).all()
    assert (want[1:] == SR.NONE).all()
    out, lab = _gpu(logits, C, img, view=torch.from_numpy(view))
    assert np.array_equal(lab, want) and np.array_equal(out, SR.draw(img, want, C))
    assert np.array_equal(out[1:], img[1:]) and np.array_equal(out[0][:, :40], img[0][:, :40])      # untouched bytes
    # the same views as offsets rows: (o0 / 512, o1 / 512, o5 - o9, o2 - o6)
    off = np.zeros((n, 10), F32)
    off[:, 0], off[:, 1], off[:, 5], off[:, 2] = view[:, 0] * 512, view[:, 1] * 512, view[:, 2], view[:, 3]
    assert np.array_equal(SR.view_from_offsets(off), view, equal_nan=True)
    out2, lab2 = _gpu(logits, C, img, offsets=torch.from_numpy(off))
    assert np.array_equal(lab2, lab) and np.array_equal(out2, out)
    with pytest.raises(ValueError):
        _gpu(logits, C, img, offsets=torch.from_numpy(off), view=torch.from_numpy(view))


@pytest.mark.parametrize('h,w,H,W', [(8, 8, 97, 203), (256, 256, 64, 128), (256, 256, 16, 16)])
def test_ties_nan_inf_and_huge_logits(h, w, H, W):
    C = 5
    logits = _logits(2, h, w, 36, C, seed=7, quantum=0.5)      # multiples of 0.5 under dyadic weights: exact ties
    g = np.random.default_rng(8)
    cells = g.random((2, h, w, C))
    logits[..., :C][cells < 0.02] = NAN
    logits[..., :C][(cells >= 0.02) & (cells < 0.04)] = INF
    logits[..., :C][(cells >= 0.04) & (cells < 0.06)] = -INF
    logits[..., :C][(cells >= 0.06) & (cells < 0.08)] = 3e38      # two of them interpolate to inf
    logits[..., :C][(cells >= 0.08) & (cells < 0.10)] = -3e38
    logits[0, : h // 2, :, 0] = NAN      # a NaN in class 0 keeps label 0
    logits[1, h // 2:, :, 1:C] = logits[1, h // 2:, :, 1:2]      # classes 1 .. C-1 equal: the lowest of them wins
    img = _images(2, H, W, seed=3)
    want = SR.labels(logits, C, H, W)
    assert (want[0, : H // 4] == 0).all() and len(np.unique(want)) >= 3 and not np.isin(want[1, 3 * H // 4:], (2, 3, 4)).any()
    out, lab = _gpu(logits, C, img)
    print('%d x %d from %d x %d: %d of %d labels differ' % (H, W, h, w, int((lab != want).sum()), want.size))
    assert np.array_equal(lab, want) and np.array_equal(out, SR.draw(img, want, C))


def test_colour_table_weights_and_channel_order():
    C, H, W = 33, 97, 203
    logits, img = _logits(2, 40, 56, 36, C, seed=4), _images(2, H, W, seed=6)
    want = SR.labels(logits, C, H, W)
    table = np.random.default_rng(9).integers(0, 256, (C, 3)).astype(np.uint8)
    for weight in (0.0, 0.7, 1.0):
        for bgr in (False, True):
            out, lab = _gpu(logits, C, img, weight=weight, bgr=bgr)
            assert np.array_equal(lab, want) and np.array_equal(out, SR.draw(img, want, C, weight=weight, bgr=bgr)), (weight, bgr)
        out, _ = _gpu(logits, C, img, weight=weight, colors=table, bgr=True)      # the caller's table is taken as it is
        assert np.array_equal(out, SR.draw(img, want, C, colors=table, weight=weight)), weight
    assert np.array_equal(_gpu(logits, C, img, weight=0.0)[0], img)
    with pytest.raises(ValueError):
        _gpu(logits, C, img, colors=table[:5])
    with pytest.raises(ValueError):
        _gpu(logits, C, img, weight=1.5)


@pytest.mark.parametrize('H,W', [(1080, 1920), (480, 640)])
def test_video_frames_under_the_view_of_their_offsets_rows(H, W):
    """The frame padded to a square of its longer side and resized to 512: the row the pre-processing writes for it."""
    C, side = 33, max(H, W)
    pt, pl = (side - H) // 2, (side - W) // 2
    off = np.array([[side, side, 0, 0, 0, 0, pt, side - W - pl, side - H - pt, pl]], F32)
    logits, img = _logits(1, 256, 256, 36, C, seed=H), _images(1, H, W, seed=W)
    want = SR.labels(logits, C, H, W, SR.view_from_offsets(off))
    assert (want < C).all()      # the canvas covers the whole frame
    out, lab = _gpu(logits, C, img, offsets=torch.from_numpy(off), bgr=True)
    print('%d x %d: %d of %d labels differ' % (H, W, int((lab != want).sum()), want.size))
    assert np.array_equal(lab, want) and np.array_equal(out, SR.draw(img, want, C, bgr=True))


# ---- the map sampling the segmentation shares with the heat-map views (csrc/map_view_plan.h) ----------------------------------
@pytest.mark.parametrize('partial', [False, True])
@pytest.mark.parametrize('H,W', [(16, 16), (96, 158)])
def test_both_sides_of_the_staging_capacity(H, W, partial):
    """A 64 x 64 map (4096 cells: more than the heat maps' 48 * 48 and, at 33 classes, than the segmentation's 344) under
    draw_heatmaps, draw_region_heatmaps and draw_segm, byte for byte the restatements.  Over 16 x 16 the one tile's footprint is
    (nearly) the whole map: every tap is read from memory.  Over 96 x 158 the footprints fit and are staged; the width is no
    multiple of 4: the byte path.  partial: a view under which the canvas leaves part of the frame out - it zooms in at 16 x 16
    (canvas = 0.6 of the frame: still beyond the capacities) and out at 96 x 158 (1.5: still staged).  Already there at other
    shapes, no view: test_gpu_overlay's 128 x 128 map over 96 x 96 (from memory), this file's 'net-unstaged' (16 x 16)."""
    ops = pkg('ops')
    h = w = 64
    off = np.zeros((3, 10), F32)      # regions 0 and 1: one per frame; region 2 overlaps region 0 in frame 0
    span = (0.6 if H == 16 else 1.5) if partial else 1.0
    off[:, 0], off[:, 1] = span * W, span * H
    if partial:
        off[:, 5], off[:, 6] = W // 4, 3      # ox = W // 4, where the window starts too; oy = -3
    off[2, 5] += 2
    off[2, 3] = W // 8
    frames = [0, 1, 0]
    view = None if not partial else SR.view_from_offsets(off[:2])
    maps, img = O.gaussian_maps(3, h, w, seed=H, peaks=4), _images(2, H, W, seed=W)
    tm, ti = torch.from_numpy(maps).cuda(), torch.from_numpy(img).cuda()
    got = ops.draw_heatmaps(tm[:2], ti, view=None if view is None else torch.from_numpy(view)).cpu().numpy()
    want = O.draw_heatmaps(maps[:2], img, view)
    assert np.array_equal(got, want) and (want != img).any()
    if partial:
        assert np.array_equal(got[:, :, :W // 4], img[:, :, :W // 4])      # outside the canvas: the input
    got = ops.draw_region_heatmaps(tm, ti, torch.from_numpy(off), frames).cpu().numpy()
    want = V.draw_region_heatmaps(maps, img, off, frames)
    assert np.array_equal(got, want) and (want != img).any()
    C = 33
    logits = _logits(2, h, w, 36, C, seed=W)
    want = SR.labels(logits, C, H, W, view)
    out, lab = _gpu(logits, C, img, **({} if view is None else {'view': torch.from_numpy(view)}))
    assert np.array_equal(lab, want) and np.array_equal(out, SR.draw(img, want, C)) and (out != img).any()
    assert (want == SR.NONE).any() == partial


def test_the_three_views_agree_on_coverage():
    """A 40 x 56 map over a 97 x 203 zero image under a view that leaves part of the frame outside the canvas, weight 1 and a table
    of 255: the pixels draw_heatmaps changes are those segm_labels gives a label and those draw_region_heatmaps changes for the
    one region with that view's `offsets` row and a window that is the frame."""
    ops = pkg('ops')
    H, W = 97, 203
    off = np.array([[128, 64, 0, 0, 0, 0, 10, 0, 0, 20]], F32)      # the window: the whole frame
    view = SR.view_from_offsets(off)
    assert view.tolist() == [[0.25, 0.125, -20.0, -10.0]]      # the canvas: x in [-20, 108), y in [-10, 54) of the frame
    inside = np.zeros((H, W), bool)
    inside[:54, :108] = True
    img = torch.zeros(1, H, W, 3, dtype=torch.uint8).cuda()
    maps = torch.from_numpy(O.gaussian_maps(1, 40, 56, seed=3)).cuda()
    lut = torch.full((256, 3), 255, dtype=torch.uint8)
    heat = ops.draw_heatmaps(maps, img, view=torch.from_numpy(view), weight=1.0, lut=lut).cpu().numpy()[0]
    region = ops.draw_region_heatmaps(maps, img, torch.from_numpy(off), [0], weight=1.0, lut=lut).cpu().numpy()[0]
    lab = _gpu(_logits(1, 40, 56, 3, 3, seed=1), 3, None, (H, W), view=torch.from_numpy(view))[1][0]
    assert np.array_equal((heat != 0).any(-1), inside) and (heat[inside] == 255).all()
    assert np.array_equal((region != 0).any(-1), inside) and np.array_equal(lab != SR.NONE, inside)


# ---- statistics -------------------------------------------------------------------------------------------------------------
def _random_labels(n, H, W, C, seed):
    g = np.random.default_rng(seed)
    lab = g.integers(0, C, (n, H, W)).astype(np.uint8)
    lab[g.random(lab.shape) < 0.5] = 0
    lab[g.random(lab.shape) < 0.1] = SR.NONE
    lab[g.random(lab.shape) < 0.02] = C      # no label at all: not counted
    return lab


def _stats(lab, C, ids=None, F=None):
    res = pkg('ops').segm_stats(torch.from_numpy(lab).cuda(), C, ids=None if ids is None else torch.from_numpy(ids).cuda(), n_faces=F)
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize('n,H,W,C', [(1, 97, 203, 33), (3, 64, 128, 33), (3, 17, 5, 3), (2, 16, 16, 5), (1, 1, 1, 3)])
def test_statistics_equal_the_restatement(n, H, W, C):
    F = 1538
    lab = _random_labels(n, H, W, C, seed=H)
    if n > 1:
        lab[1][(lab[1] >= 1) & (lab[1] <= (C - 1) // 2)] = 0      # no right hand in frame 1
        lab[n - 1] = SR.NONE                                      # nothing at all in the last frame
    ids = np.random.default_rng(W).integers(-1, 6 * F, lab.shape).astype(np.int32)
    ids[np.random.default_rng(W + 1).random(lab.shape) < 0.4] = -1
    counts, boxes, agree = SR.stats(lab, C, ids, F)
    got = _stats(lab, C, ids, F)
    assert got['counts'].dtype == np.int32 and np.array_equal(got['counts'], counts)
    assert np.array_equal(got['boxes'], boxes) and np.array_equal(got['agree'], agree)
    plain = _stats(lab, C)
    assert set(plain) == {'counts', 'boxes'} and np.array_equal(plain['counts'], counts) and np.array_equal(plain['boxes'], boxes)
    none = _stats(lab, C, np.full_like(ids, -1), F)['agree']
    assert (none[:, :, 0] == 0).all() and (none[:, :, 2] == 0).all() and np.array_equal(none[:, :, 1], agree[:, :, 1])
    again = _stats(lab, C, ids, F)
    assert all(np.array_equal(again[k], got[k]) for k in got)
    for i in range(n):      # a frame alone equals the frame in the batch
        one = _stats(lab[i:i + 1], C, ids[i:i + 1], F)
        assert all(np.array_equal(one[k][0], got[k][i]) for k in got), i
    if n > 1:
        assert boxes[1, 1].tolist() == [0, 0, 0, 0] and not counts[n - 1].any() and not boxes[n - 1].any()


# ---- engine level ---------------------------------------------------------------------------------------------------------
def _by_operators(ops, eng, B, images, offsets, ids, n_faces, bgr=False):
    logits = eng.head_maps(B, nchw=False)['segms']
    assert tuple(logits.shape) == (B, 256, 256, 33) and logits.stride(2) == 36 and logits.dtype == torch.float32
    if images is None:
        lab = ops.segm_labels(logits, (512, 512))
        view = None
    else:
        view, lab = ops.draw_segm(logits, images, offsets=offsets, bgr=bgr, labels=True)
    return view, lab, ops.segm_stats(lab, 33, ids=ids, n_faces=n_faces)


def _check_engine(ops, e, frames, B, K, mano_tables):
    img = frames[:B]
    out = e.forward(img, project=True, **({} if K == 1 else {'max_hand': K}))
    n_faces = np.asarray(mano_tables['left']['faces']).shape[0]
    # the rasteriser's ids of the same frames: pair k of frame b as region b * K + k of frame b
    flat = {k: out[k].reshape(B * K, *out[k].shape[(1 if K == 1 else 2):]) for k in ('slots', 'verts', 'joints', 'pj2d')}
    if K == 1:
        ids = e.render(out, img, return_ids=True)[1]
    else:
        rows = torch.tensor([WHOLE]).repeat(B * K, 1).cuda()
        region_frame = torch.arange(B, dtype=torch.int32).repeat_interleave(K).cuda()
        ids = e.render_regions(flat, img, rows, region_frame, return_ids=True)[1]
    # in every order the engine draws, the left hand of a pair is the even mesh
    mesh = (ids[ids >= 0] // n_faces)
    flags = flat['slots'][:, :, pkg('_lib').SLOT_FLAG] > 0.5
    assert bool(flags.reshape(-1)[mesh.unique().long()].all())
    want_view, want_lab, want_st = _by_operators(ops, e, B, img, None, ids, n_faces)
    got = e.segment(out, images=img, stats=True, ids=ids)
    assert set(got) == {'labels', 'view', 'counts', 'boxes', 'agree'}
    assert torch.equal(got['labels'], want_lab) and torch.equal(got['view'], want_view)
    assert all(torch.equal(got[k], want_st[k]) for k in want_st)
    counts = got['counts'].cpu().numpy()
    print('B %d K %d: labels present %s, agree %s' % (B, K, (counts > 0).sum(1).tolist(), got['agree'].cpu().numpy().tolist()))
    assert (counts.sum(1) == 512 * 512).all()
    # without images: 512 x 512 under the identity view - the same labels, since these frames ARE 512 x 512
    plain = e.segment(B)
    assert set(plain) == {'labels'} and torch.equal(plain['labels'], want_lab)
    assert torch.equal(e.segment(out, offsets=torch.tensor([WHOLE]).repeat(B, 1))['labels'], want_lab)
    st = e.segment(B, labels=False, stats=True)
    assert set(st) == {'counts', 'boxes'} and torch.equal(st['counts'], want_st['counts']) and torch.equal(st['boxes'], want_st['boxes'])
    same = img.clone()
    assert e.segment(out, images=same, dst=same, labels=False)['view'] is same and torch.equal(same, want_view)
    bgr = e.segment(out, images=img, bgr=True, labels=False)['view']
    assert torch.equal(bgr, ops.draw_segm(e.head_maps(B, nchw=False)['segms'], img, bgr=True))
    # the same call queues without a host visit
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        quiet = e.segment(out, images=img, stats=True, ids=ids)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert all(torch.equal(quiet[k], got[k]) for k in got)
    return out, got, ids


@pytest.mark.parametrize('B,K', [(1, 1), (2, 1), (1, 2), (2, 2)])
def test_engine_segment_equals_the_operators(eng, mano_tables, frames3, B, K):
    _check_engine(pkg('ops'), eng, frames3, B, K, mano_tables)


def test_engine_segment_on_a_16_bit_storage_program(near_sd, mano_tables, frames3):
    e = pkg('engine').Engine(0)
    e.load_state_dict(near_sd, max_batch=2, precision='bf16')
    e.load_mano(mano_tables)
    _check_engine(pkg('ops'), e, frames3, 2, 1, mano_tables)      # (the segmentation buffer is fp32 in every storage type)
    e.close()


def test_segment_before_a_forward_and_at_another_batch_is_a_state_error(near_sd, mano_tables, frames3):
    L = pkg('_lib')
    e = pkg('engine').Engine(0)
    e.load_state_dict(near_sd, max_batch=2)
    e.load_mano(mano_tables)
    lab = torch.empty(2, 512, 512, dtype=torch.uint8, device='cuda')
    p = ctypes.c_void_p(lab.data_ptr())
    assert e.L.acrmi_segment(e.ctx, 2, None, 0.7, None, 0, None, None, p, 512, 512, None) == L.E_STATE
    with pytest.raises(L.AcrmiError, match='no program has run'):
        e.segment(2)
    out = e.forward(frames3[:2], project=True)
    assert e.segment(out)['labels'].shape == (2, 512, 512)
    assert e.L.acrmi_segment(e.ctx, 1, None, 0.7, None, 0, None, None, p, 512, 512, None) == L.E_STATE
    with pytest.raises(L.AcrmiError, match='batch of 2'):
        e.segment(1)
    with pytest.raises(ValueError):      # argument errors of the operator keep their kind
        e.segment(out, weight=2.0)
    e.close()


def test_pool_segment_equals_the_engine(eng, near_sd, mano_tables, frames3):
    img = frames3[:2]
    out = eng.forward(img, project=True)
    ids = eng.render(out, img, return_ids=True)[1]
    want = eng.segment(out, images=img, stats=True, ids=ids)
    pool = pkg('engine').EnginePool(0, n=2)
    pool.load_state_dict(near_sd, max_batch=2)
    pool.load_mano(mano_tables)
    for k in range(4):      # both contexts, twice
        t = pool.submit(img, project=True)
        got = pool.segment(t, images=img, stats=True, ids=ids)
        plain = pool.segment(t)
        pool.collect(t)
        assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
        assert torch.equal(plain['labels'], want['labels'])
    with pytest.raises(RuntimeError):
        pool.segment(t)
    pool.close()


# ---- the acr layer ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def acr(near_sd, mano_tables):
    cfg = pkg('config')
    return pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml']), state_dict=near_sd,
                               mano_tables=mano_tables, max_batch=2)


def _same_results(a, b, extra=()):
    assert list(a) == list(b)
    for path in a:
        assert len(a[path]) == len(b[path])
        for h0, h1 in zip(a[path], b[path]):
            assert set(h1) == set(h0) | set(extra)
            assert all(np.array_equal(h0[f], h1[f]) for f in h0)


def test_forward_batch_segm_view_and_masks(acr, frames3):
    ops = pkg('ops')
    img = frames3[:2]
    plain_res, plain = acr.forward_batch(img, ['a', 'b'], render=img, show_items=('mesh',))
    res, views = acr.forward_batch(img, ['a', 'b'], render=img, show_items=('mesh', 'segm'), masks='iou')
    assert list(views) == ['mesh', 'segm'] and views['segm'].shape == img.shape and views['segm'].dtype == torch.uint8
    assert torch.equal(views['mesh'], plain['mesh'])      # byte for byte what it is without the new view
    _same_results(plain_res, res, ('mask_area', 'mask_box', 'mask_iou'))
    # against the engine on the same forward
    e = acr.model.engine(2)
    seg = e.segment(2, images=img, offsets=torch.tensor([WHOLE]).repeat(2, 1), stats=True)
    assert torch.equal(views['segm'], seg['view'])
    assert torch.equal(views['segm'], ops.draw_segm(e.head_maps(2, nchw=False)['segms'], img))
    counts, boxes = seg['counts'].cpu().numpy(), seg['boxes'].cpu().numpy()
    area = np.stack([counts[:, 17:].sum(1), counts[:, 1:17].sum(1)], 1)      # [frame, side]
    seen = 0
    for b, path in enumerate(('a', 'b')):
        for hand in res[path]:
            s = int(hand['hand_type'])
            assert hand['mask_area'] == area[b, s] and hand['mask_box'].tolist() == boxes[b, s].tolist()
            assert np.isnan(hand['mask_iou']) or 0.0 <= hand['mask_iou'] <= 1.0
            seen += 1
    assert seen > 0
    # masks=True: the same two keys, no third; without frames: the 512 canvas, which these frames are
    for kw in (dict(render=img, show_items=('segm',)), dict()):
        got = acr.forward_batch(img, ['a', 'b'], masks=True, **kw)
        only = got[0] if kw else got
        _same_results(plain_res, only, ('mask_area', 'mask_box'))
        assert all(h1['mask_area'] == h0['mask_area'] and np.array_equal(h1['mask_box'], h0['mask_box'])
                   for p in res for h0, h1 in zip(res[p], only[p]))
    iou = acr.forward_batch(img, ['a', 'b'], masks='iou')      # on a scratch canvas
    assert all(np.array_equal(h1['mask_iou'], h0['mask_iou'], equal_nan=True) for p in res for h0, h1 in zip(res[p], iou[p]))
    # the iou against the statistics of the engine's own ids
    e.set_point_heads(True)      # (as the fused call runs)
    try:
        out = e.forward(img, offsets=torch.tensor([WHOLE]).repeat(2, 1), project=True)
    finally:
        e.set_point_heads(False)
    out['cam_trans'] = ops.cam_trans(out['joints'].view(-1, 21, 3), out['pj2d'].view(-1, 21, 2), focal_length=acr.focal_length).view(2, 2, 3)
    ids = e.render(out, img, offsets=torch.tensor([WHOLE]).repeat(2, 1), focal_length=float(acr.focal_length), return_ids=True)[1]
    agree = e.segment(out, images=img, offsets=torch.tensor([WHOLE]).repeat(2, 1), stats=True, ids=ids)['agree'].cpu().numpy()
    for b, path in enumerate(('a', 'b')):
        for hand in acr.forward_batch(img, ['a', 'b'], masks='iou')[path]:
            i, m, s = (int(v) for v in agree[b, int(hand['hand_type'])])
            want = np.float32(i / (m + s - i)) if m + s - i > 0 else np.float32(NAN)
            assert np.array_equal(hand['mask_iou'], want, equal_nan=True)
    two_res, two = acr.forward_batch(img, ['a', 'b'], render=img, show_items=('mesh', 'segm'), max_hand=2, masks='iou')
    assert torch.equal(two['segm'], e.segment(2, images=img, labels=False)['view'])      # the map is the frame's, not a pair's
    for path in two_res:      # every hand of a side carries the side's values
        for s in (0, 1):
            assert len({(int(h['mask_area']), tuple(h['mask_box'].tolist())) for h in two_res[path] if h['hand_type'] == s}) <= 1


def test_forward_raw_batch_segm_view_mixed_sizes_and_nv12(acr):
    ops, synth = pkg('ops'), pkg('synth')
    g = np.random.default_rng(12)
    small = torch.from_numpy(g.integers(0, 256, (96, 160, 3)).astype(np.uint8)).cuda()
    big = torch.from_numpy(np.ascontiguousarray(synth.make_frames(1, seed=3)[0][..., ::-1])).cuda()      # 512 x 512 BGR
    frames = [small, big]
    res, views = acr.forward_raw_batch(frames, ['a', 'b'], render=True, show_items=('mesh', 'segm'), masks=True)
    plain = acr.forward_raw_batch(frames, ['a', 'b'])
    _same_results(plain, res, ('mask_area', 'mask_box'))
    assert [tuple(v.shape) for v in views['segm']] == [(96, 160, 3), (512, 512, 3)]
    e = acr.model.engine(2)
    logits = e.head_maps(2, nchw=False)['segms']
    meta = pkg('acr.utils').img_preprocess_gpu(frames, ['a', 'b'])
    for i, f in enumerate(frames):      # every size through the operator on its own frame of the same forward
        want, lab = ops.draw_segm(logits[i:i + 1], f[None], offsets=meta['offsets'][i:i + 1], bgr=True, labels=True)
        assert torch.equal(views['segm'][i], want[0])
        st = ops.segm_stats(lab, 33)
        counts, boxes = st['counts'][0].cpu().numpy(), st['boxes'][0].cpu().numpy()
        for hand in res['ab'[i]]:
            s = int(hand['hand_type'])
            assert hand['mask_area'] == (counts[1:17].sum() if s == 1 else counts[17:].sum())
            assert hand['mask_box'].tolist() == boxes[s].tolist()
    both = torch.stack([big, big.flip(0)])
    _, bgr_views = acr.forward_raw_batch(both, ['a', 'b'], render=True, show_items=('mesh', 'segm'))
    _, nv = acr.forward_raw_batch(both, ['a', 'b'], render=True, show_items=('mesh', 'segm'), render_format='nv12')
    assert tuple(nv['segm'].shape) == (2, 768, 512) and torch.equal(nv['segm'], ops.bgr_to_nv12(bgr_views['segm'], bgr=True))
    assert not torch.equal(bgr_views['segm'], both)
    for kw in (dict(show_items=('segm',), render=True), dict(show_items=('segm',), render=True, region_views=True), dict(masks=True)):
        with pytest.raises(ValueError, match='over regions'):
            acr.forward_raw_batch(both, ['a', 'b'], boxes=[[0, 0, 256, 256], [10, 10, 300, 300]], **kw)
