"""GPU tests of the key-point skeleton and heat-map views (csrc/overlay.hip, DESIGN.md "Key-point and heat-map views")
against the numpy restatement of their rules in tests/overlay_ref.py: byte for byte, no tolerance, no excluded pixels."""
import ctypes

import numpy as np
import pytest
import torch

import overlay_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu


def _images(n, h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3)).astype(np.uint8)


def _skel(kps, images, **kw):
    ops = pkg('ops')
    hf = kw.pop('hand_frame', None)
    got = ops.draw_skeletons(torch.from_numpy(np.asarray(kps, np.float32)).cuda(), torch.from_numpy(images).cuda(),
                             hand_frame=None if hf is None else torch.as_tensor(np.asarray(hf)), **kw)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _same(got, want, what):
    bad = int((got != want).any(-1).sum())
    print('%s: %d of %d pixels differ, %d drawn' % (what, bad, want[..., 0].size, int((want != 0).any(-1).sum())))
    assert bad == 0, what


# ---- skeleton ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bgr', [False, True])
@pytest.mark.parametrize('hw', [(512, 512), (1080, 1920), (480, 640), (97, 203)])
def test_skeleton_random_hands(hw, bgr):
    H, W = hw
    N = 3
    kps = R.random_hands(2 * N, H, W, seed=H + W)
    kps[1] += (0.45 * W, 0.1 * H)            # partly off the image
    kps[2] -= (2.0 * W, 0.0)                 # wholly off it
    kps[3] += (-0.4 * W, 0.45 * H)
    images = _images(N, H, W, seed=1)
    want = R.draw_skeletons(kps, images, bgr=bgr)
    got = _skel(kps, images, bgr=bgr)
    drawn = int((want != images).any(-1).sum())
    assert drawn > 200
    _same(got, want, 'skeleton %dx%d bgr=%s (%d px drawn)' % (H, W, bgr, drawn))
    assert np.array_equal(got[(want == images).all(-1)], images[(want == images).all(-1)])      # every other pixel is the input


def test_skeleton_special_cases():
    H = W = 512
    images = _images(4, H, W, seed=2)
    kps = R.random_hands(10, H, W, seed=5)
    kps[1] = 200.5                                   # coincident joints: L2 = 0, discs only
    kps[2, 7, 0] = np.nan                            # a non-finite key point: the hand is not drawn
    kps[3, 12] = (20000.0, 100.0)                    # a coordinate beyond the limit: its primitives are dropped
    kps[4, 0] = (-16384.0, 3.0)                      # exactly at the limit (the wrist: every finger loses its last bone)
    kps[5, 3, 1] = -np.inf
    kps[6] = kps[6] * 40.0 - 8000.0                  # long bones crossing the image from far outside
    kps[7] = -kps[7]                                 # negative coordinates truncate toward zero
    kps[8, 1:] = kps[8, :1] + 0.9 * (kps[8, 1:] - kps[8, :1]) / 12.0      # a tiny hand: bones shorter than the discs
    hand_frame = np.array([0, 0, 1, 1, 2, 2, 0, -1, 0, 0], np.int32)      # five hands in frame 0; one not drawn; frame 3 empty
    want = R.draw_skeletons(kps, images, hand_frame=hand_frame)
    _same(_skel(kps, images, hand_frame=hand_frame), want, 'special cases')
    assert np.array_equal(want[3], images[3]) and not np.array_equal(want[0], images[0])
    # more than two hands of a frame, far apart in the index: the search keeps hand order (the last hand is on top)
    many = R.random_hands(300, H, W, seed=9)
    hf = np.full(300, -1, np.int32)
    hf[[3, 70, 150, 299]] = 1
    hf[[0, 64, 256]] = 2
    many[299] = many[3] + 2.0
    _same(_skel(many, images, hand_frame=hf), R.draw_skeletons(many, images, hand_frame=hf), 'sparse hand index')
    # widths, radii and colour tables other than the defaults
    col = np.random.default_rng(3).integers(0, 256, (21, 3)).astype(np.uint8)
    for lw, rad in ((1, 0), (2, 1), (5, 6), (11, 10), (3, 40)):
        want = R.draw_skeletons(kps[:2], images[:1], hand_frame=[0, 0], colors=col, line_width=lw, circle_rad=rad)
        got = _skel(kps[:2], images[:1], hand_frame=[0, 0], colors=torch.from_numpy(col), line_width=lw, circle_rad=rad)
        _same(got, want, 'line_width %d circle_rad %d' % (lw, rad))
    with pytest.raises(ValueError, match='line_width'):      # beyond what the int64 terms were bounded for
        _skel(kps[:2], images[:1], line_width=12)


# ---- heat maps --------------------------------------------------------------------------------------------------------
def _heat(maps, images, **kw):
    ops = pkg('ops')
    view = kw.pop('view', None)
    got = ops.draw_heatmaps(torch.from_numpy(maps).cuda(), torch.from_numpy(images).cuda(),
                            view=None if view is None else torch.from_numpy(np.asarray(view, np.float32)), **kw)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _heat_want(maps, images, **kw):
    return np.stack([R.draw_heatmaps(maps[:, s], images, **kw) for s in (0, 1)])


def test_heatmap_identity_view_and_torch_form():
    H = W = 512
    n = 4
    maps = R.gaussian_maps(2 * n, 64, 64, seed=11, peaks=3).reshape(n, 2, 64, 64)
    maps[0, 0, 5, 7] = 3.0            # above 1: the index clamps at 255
    maps[1, 1] -= 0.2                 # below 0: clamps at 0
    images = _images(n, H, W, seed=3)
    for bgr in (False, True):
        got = _heat(maps, images, bgr=bgr)
        assert got.shape == (2, n, H, W, 3)
        _same(got.reshape(-1, H, W, 3), _heat_want(maps, images, bgr=bgr).reshape(-1, H, W, 3), 'heat map 512 bgr=%s' % bgr)
    # one view; another weight
    one = _heat(np.ascontiguousarray(maps[:, 1]), images, weight=0.4)
    _same(one, R.draw_heatmaps(maps[:, 1], images, weight=0.4), 'one view, weight 0.4')
    # the torch form (make_heatmaps, acr/visualization.py:280-285) through a table that is its own index: at most 1e-5 of the
    # pixels may differ, and by at most 1 (weight 1 writes LUT[idx] itself)
    ident = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    idx = _heat(maps, images, weight=1.0, lut=torch.from_numpy(ident))[..., 0]
    want = torch.nn.functional.interpolate(torch.from_numpy(maps), size=(H, W), mode='bilinear').mul(255).clamp(0, 255).byte()
    d = np.abs(idx.astype(np.int32) - want.permute(1, 0, 2, 3).numpy().astype(np.int32))
    print('index against torch: %d of %d pixels differ, worst %d' % (int((d != 0).sum()), d.size, int(d.max())))
    assert d.max() <= 1 and (d != 0).sum() <= 1e-5 * d.size


@pytest.mark.parametrize('hw', [(1080, 1920), (480, 640)])
def test_heatmap_offsets_views(hw):
    ops = pkg('ops')
    H, W = hw
    n = 2
    raw = _images(n, H, W, seed=4)
    _, offsets = ops.preprocess(torch.from_numpy(raw).cuda())
    view = ops.view_from_offsets(offsets).cpu().numpy()
    maps = R.gaussian_maps(2 * n, 64, 64, seed=H, peaks=3).reshape(n, 2, 64, 64)
    got = _heat(maps, raw, view=view, bgr=True)
    _same(got.reshape(-1, H, W, 3), _heat_want(maps, raw, view=view, bgr=True).reshape(-1, H, W, 3), 'offsets view %dx%d' % (H, W))
    # a canvas that covers part of the frame only (and one that faces away): pixels outside it are untouched
    part = np.array([[0.5, 0.75, 100.25, 50.5], [-1.0, 1.0, 0.0, 0.0]], np.float32)
    got = _heat(maps, raw, view=part)
    want = _heat_want(maps, raw, view=part)
    _same(got.reshape(-1, H, W, 3), want.reshape(-1, H, W, 3), 'partial canvas %dx%d' % (H, W))
    inside = np.zeros((H, W), bool)
    inside[50:50 + 385, 100:100 + 257] = True
    assert np.array_equal(got[0, 0][~inside[:H, :W]], raw[0][~inside[:H, :W]]) and np.array_equal(got[1, 1], raw[1])
    assert (got[0, 0][60:400, 110:350] != raw[0][60:400, 110:350]).any()


def test_heatmap_other_map_and_image_shapes():
    for (h, w), (H, W), seed in (((40, 56), (333, 517), 1),      # not 64 x 64; a width not divisible by 4: the byte path
                                 ((128, 128), (96, 96), 2),       # more map cells under a tile than LDS holds: read from memory
                                 ((64, 64), (31, 1030), 3)):
        maps = R.gaussian_maps(2 * 2, h, w, seed=seed, peaks=4).reshape(2, 2, h, w)
        images = _images(2, H, W, seed=seed)
        got = _heat(maps, images)
        _same(got.reshape(-1, H, W, 3), _heat_want(maps, images).reshape(-1, H, W, 3), 'maps %dx%d on %dx%d' % (h, w, H, W))
    nanmap = R.gaussian_maps(2, 64, 64, seed=5).reshape(1, 2, 64, 64)
    nanmap[0, 0, 10:20, 10:20] = np.nan
    images = _images(1, 256, 256, seed=6)
    _same(_heat(nanmap, images).reshape(-1, 256, 256, 3), _heat_want(nanmap, images).reshape(-1, 256, 256, 3), 'NaN cells')


# ---- determinism ------------------------------------------------------------------------------------------------------
def test_determinism_batching_in_place():
    ops = pkg('ops')
    N, H, W = 64, 512, 512
    images = torch.from_numpy(_images(N, H, W, seed=7)).cuda()
    kps = torch.from_numpy(R.random_hands(2 * N, H, W, seed=8)).cuda()
    maps = torch.from_numpy(R.gaussian_maps(2 * N, 64, 64, seed=9).reshape(N, 2, 64, 64)).cuda()
    a, b = ops.draw_skeletons(kps, images), ops.draw_skeletons(kps, images)
    assert torch.equal(a, b) and not torch.equal(a, images)
    ha, hb = ops.draw_heatmaps(maps, images), ops.draw_heatmaps(maps, images)
    assert torch.equal(ha, hb)
    for i in range(N):      # a frame drawn alone = the frame drawn in the batch
        assert torch.equal(ops.draw_skeletons(kps[2 * i:2 * i + 2], images[i:i + 1])[0], a[i])
        assert torch.equal(ops.draw_heatmaps(maps[i:i + 1], images[i:i + 1])[:, 0], ha[:, i])
    work = images.clone()
    assert ops.draw_skeletons(kps, work, dst=work).data_ptr() == work.data_ptr() and torch.equal(work, a)
    # uncovered pixels are the input: against the restatement's mask of the first frames
    want = R.draw_skeletons(kps[:8].cpu().numpy(), images[:4].cpu().numpy())
    assert np.array_equal(a[:4].cpu().numpy(), want)
    keep = (want == images[:4].cpu().numpy()).all(-1)
    assert np.array_equal(a[:4].cpu().numpy()[keep], images[:4].cpu().numpy()[keep]) and 0 < (~keep).sum() < keep.size // 4


# ---- engine, pool, acr ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def near_sd():
    return pkg('synth').make_state_dict(seed=10)      # (the checkpoint tests/test_gpu_render.py uses: both hands detected)


def _engine(sd, mano_tables, max_batch=2):
    eng = pkg('engine').Engine(0)
    eng.load_state_dict(sd, max_batch=max_batch)
    eng.load_mano(mano_tables)
    return eng


def _expected_skeleton(ops, L, out, images, offsets=None, bgr=False):
    B = images.shape[0]
    kps = ((out['pj2d'] + 1) / 2 * 512) if offsets is None else out['pj2d_org']
    flags = out['slots'][:, :, L.SLOT_FLAG].reshape(-1) > 0.5
    frame = torch.arange(2 * B, device=flags.device) // 2
    return ops.draw_skeletons(kps.reshape(2 * B, 21, 2).contiguous(), images,
                              hand_frame=torch.where(flags, frame, torch.full_like(frame, -1)), bgr=bgr)


def _expected_centermap(ops, eng, images, offsets=None, bgr=False):
    hm = eng.head_maps(images.shape[0])
    maps = torch.cat([hm['l_center_map'], hm['r_center_map']], 1).float()
    assert torch.equal(maps, eng.center_maps(images.shape[0]))
    return ops.draw_heatmaps(maps, images, view=None if offsets is None else ops.view_from_offsets(offsets), bgr=bgr)


def test_overlay_before_a_forward_is_a_state_error(synth_sd, mano_tables, frames2):
    L = pkg('_lib')
    eng = _engine(synth_sd, mano_tables)
    img = torch.from_numpy(frames2).cuda()
    dst = torch.empty(2, *img.shape, dtype=torch.uint8, device='cuda')
    slots = torch.zeros(2, 2, L.SLOT, device='cuda')
    pj = torch.zeros(2, 2, 21, 2, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for what, a, b in ((L.OVERLAY_SKELETON, p(slots), p(pj)), (L.OVERLAY_CENTERMAP, None, None)):
        rc = eng.L.acrmi_overlay(eng.ctx, what, a, b, 2, None, 0, p(img), p(dst[0]), p(dst[1]), 512, 512, None)
        assert rc == L.E_STATE
    with pytest.raises(L.AcrmiError, match='no program has run'):
        eng.overlay({'slots': slots, 'pj2d': pj}, img, 'pj2d')
    out = eng.forward(img, project=True)
    assert eng.overlay(out, img, 'pj2d').shape == img.shape
    assert eng.overlay(out, img, 'centermap').shape == (2,) + tuple(img.shape)
    with pytest.raises(L.AcrmiError, match='batch of 2'):      # the resident maps are those of two frames
        eng.overlay({k: v[:1] for k, v in out.items()}, img[:1], 'centermap')
    with pytest.raises(ValueError):
        eng.overlay(out, img, 'j3d')
    eng.close()


@pytest.mark.parametrize('precision', ['fp32', 'fp16'])
def test_engine_overlay_matches_the_operators(precision, near_sd, mano_tables, frames2):
    ops, L = pkg('ops'), pkg('_lib')
    eng = pkg('engine').Engine(0)
    eng.load_state_dict(near_sd, max_batch=2, **({} if precision == 'fp32' else {'precision': precision}))
    eng.load_mano(mano_tables)
    img = torch.from_numpy(frames2).cuda()
    out = eng.forward(img, project=True)
    if precision == 'fp32':
        assert (out['slots'][:, :, L.SLOT_FLAG] > 0.5).all()
    # the network input
    got = eng.overlay(out, img, 'pj2d')
    assert torch.equal(got, _expected_skeleton(ops, L, out, img))
    print('%s: skeleton pixels on the network input: %d' % (precision, int((got != img).any(-1).sum())))
    work = img.clone()
    assert eng.overlay(out, work, 'pj2d', dst=work).data_ptr() == work.data_ptr() and torch.equal(work, got)
    both = eng.overlay(out, img, 'centermap')
    assert torch.equal(both, _expected_centermap(ops, eng, img)) and not torch.equal(both[0], img)
    # original frames through the offsets rows, BGR
    raw = torch.from_numpy(np.ascontiguousarray(np.kron(frames2, np.ones((1, 2, 2, 1), np.uint8))[:, 152:872, :, ::-1])).cuda()
    rgb, offsets = ops.preprocess(raw)
    out = eng.forward(rgb, offsets=offsets, project=True)
    got = eng.overlay(out, raw, 'pj2d', offsets=offsets, bgr=True)
    assert got.shape == raw.shape and torch.equal(got, _expected_skeleton(ops, L, out, raw, offsets=offsets, bgr=True))
    print('%s: skeleton pixels on the original frames: %d' % (precision, int((got != raw).any(-1).sum())))
    both = eng.overlay(out, raw, 'centermap', offsets=offsets, bgr=True)
    assert torch.equal(both, _expected_centermap(ops, eng, raw, offsets=offsets, bgr=True))
    # an undetected hand draws nothing
    half = dict(out, slots=out['slots'].clone())
    half['slots'][0, 1, L.SLOT_FLAG] = 0.0
    half['slots'][1, :, L.SLOT_FLAG] = 0.0
    got = eng.overlay(half, raw, 'pj2d', offsets=offsets, bgr=True)
    assert torch.equal(got, _expected_skeleton(ops, L, half, raw, offsets=offsets, bgr=True)) and torch.equal(got[1], raw[1])
    eng.set_conf_thresh(1e6)
    out = eng.forward(img, project=True)
    assert not (out['slots'][:, :, L.SLOT_FLAG] > 0.5).any() and torch.equal(eng.overlay(out, img, 'pj2d'), img)
    eng.close()


def test_pool_overlay_on_the_tickets_stream(near_sd, mano_tables, frames2):
    eng = _engine(near_sd, mano_tables)
    img = torch.from_numpy(frames2).cuda()
    out = eng.forward(img, project=True)
    want = eng.overlay(out, img, 'pj2d'), eng.overlay(out, img, 'centermap')
    pool = pkg('engine').EnginePool(0, n=2)
    pool.load_state_dict(near_sd, max_batch=2)
    pool.load_mano(mano_tables)
    for k in range(4):      # both contexts, twice
        t = pool.submit(img, project=True)
        skel = pool.overlay(t, img, 'pj2d')
        heat = pool.overlay(t, img, 'centermap')
        pool.collect(t)
        assert torch.equal(skel, want[0]) and torch.equal(heat, want[1])
    with pytest.raises(RuntimeError):
        pool.overlay(t, img, 'pj2d')
    pool.close()
    eng.close()


def test_acr_layer_views(near_sd, mano_tables, frames2):
    cfg, ops = pkg('config'), pkg('ops')
    acr = pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml', '--renderer', 'hip']),
                              state_dict=near_sd, mano_tables=mano_tables, max_batch=2)
    assert acr.show_items == ['mesh']
    rs = np.random.RandomState(7)
    big = np.clip(np.kron(rs.randint(0, 256, (135, 240, 3)).astype(np.float32), np.ones((8, 8, 1), np.float32)), 0, 255).astype(np.uint8)
    small = np.ascontiguousarray(frames2[0][:, :, ::-1])      # BGR 512 x 512
    frames = [torch.from_numpy(big).cuda(), torch.from_numpy(small).cuda()]
    items = ['mesh', 'pj2d', 'centermap']
    plain = acr.forward_raw_batch(frames, ['a', 'b'])
    res_m, drawn_m = acr.forward_raw_batch(frames, ['a', 'b'], render=True)
    res, views = acr.forward_raw_batch(frames, ['a', 'b'], render=True, show_items=items)
    assert sorted(views) == sorted(items)
    for r in (res_m, res):      # the result dicts are unchanged by the views
        assert sorted(r) == sorted(plain)
        for k in plain:
            assert len(r[k]) == len(plain[k])
            for a, b in zip(r[k], plain[k]):
                assert sorted(a) == sorted(b) and all(np.array_equal(a[f], b[f]) for f in b)
    for i, f in enumerate(frames):
        assert torch.equal(views['mesh'][i], drawn_m[i])
        assert views['pj2d'][i].shape == f.shape and views['centermap'][i].shape == (2,) + tuple(f.shape)
        assert not torch.equal(views['centermap'][i][0], f) and not torch.equal(views['centermap'][i][1], f)
    # what the list path drew = the operators on the same forward (frames of one size each: one group per frame)
    eng = acr.model.engine(2)
    meta = pkg('acr.utils').img_preprocess_gpu(frames, ['a', 'b'])
    eng.set_point_heads(True)      # as forward_batch runs it
    out = eng.forward(meta['image'], offsets=meta['offsets'], project=True)
    maps = eng.center_maps(2)
    for i, f in enumerate(frames):
        want = ops.draw_skeletons(out['pj2d_org'][i].contiguous(), f[None], hand_frame=torch.zeros(2, dtype=torch.int32), bgr=True)
        assert torch.equal(views['pj2d'][i], want[0])
        want = ops.draw_heatmaps(maps[i:i + 1], f[None], view=ops.view_from_offsets(meta['offsets'][i:i + 1]), bgr=True)
        assert torch.equal(views['centermap'][i], want[:, 0])
    # the network input itself, as one tensor
    img = torch.from_numpy(frames2).cuda()
    res2, drawn2 = acr.forward_batch(img, ['a', 'b'], render=img)
    assert drawn2.shape == img.shape                       # without show_items: exactly today's return value
    res3, views3 = acr.forward_batch(img, ['a', 'b'], render=img, show_items=('pj2d', 'centermap', 'org_img'))
    assert sorted(views3) == ['centermap', 'org_img', 'pj2d'] and views3['org_img'] is img
    assert views3['pj2d'].shape == img.shape and views3['centermap'].shape == (2,) + tuple(img.shape)
    out = eng.forward(img, offsets=torch.tensor([[512., 512, 0, 0, 0, 0, 0, 0, 0, 0]]).repeat(2, 1), project=True)
    assert torch.equal(views3['pj2d'], eng.overlay(out, img, 'pj2d'))
    assert torch.equal(views3['centermap'], eng.overlay(out, img, 'centermap'))
    eng.set_point_heads(False)
    with pytest.raises(ValueError):
        acr.forward_batch(img, ['a', 'b'], render=img, show_items=['mesh', 'tagmap'])
    with pytest.raises(ValueError):
        acr.forward_batch(img, ['a', 'b'], show_items=['pj2d'])
    # single image: default -> exactly the mesh key; listed views are added
    one = acr(small, 'b')
    assert sorted(one) == ['b'] and sorted(acr.rendering) == ['mesh_rendering_orgimgs']
    mesh = acr.rendering['mesh_rendering_orgimgs'][0]
    acr.show_items = items
    again = acr(small, 'b')
    assert sorted(again) == ['b'] and len(again['b']) == len(one['b'])
    for a, b in zip(again['b'], one['b']):
        assert all(np.array_equal(a[f], b[f]) for f in b)
    assert sorted(acr.rendering) == ['centermap', 'mesh_rendering_orgimgs', 'pj2d']
    assert np.array_equal(acr.rendering['mesh_rendering_orgimgs'][0], mesh)
    assert acr.rendering['pj2d'][0].shape == small.shape and acr.rendering['pj2d'][0].dtype == np.uint8
    left, right = acr.rendering['centermap'][0]
    assert left.shape == small.shape and (left != small).any() and (right != small).any()
    acr.show_items = ['mesh', 'j3d']
    with pytest.raises(ValueError):
        acr(small, 'b')
