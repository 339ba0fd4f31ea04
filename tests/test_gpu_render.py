"""GPU tests of the mesh overlay (csrc/render.hip, DESIGN.md "Rendering") against the numpy restatement of its rules
in tests/render_ref.py: exact coverage, ids outside the pixels an fp32 depth cannot order, colours within one count."""
import numpy as np
import pytest
import torch

import render_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

AMBIGUOUS_CAP = 0.01      # share of the covered pixels whose two nearest surfaces are within 1e-5 relative in 1/Z


def _images(n, h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3)).astype(np.uint8)


def _run(verts, faces, images, **kw):
    ops = pkg('ops')
    t = {k: kw.pop(k) for k in ('trans', 'view', 'mesh_frame', 'colors', 'topo_index') if k in kw}
    dev = {k: (None if v is None else torch.as_tensor(np.asarray(v))) for k, v in t.items()}
    out, ids = ops.render_meshes(torch.from_numpy(np.asarray(verts, np.float32)).cuda(), faces, torch.from_numpy(images).cuda(),
                                 return_ids=True, **dev, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ids.cpu().numpy()


def _compare(got_out, got_ids, ref, images, what=''):
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


def _ellipsoids():
    va, fa = R.ellipsoid(24, 32, (0.05, 0.09, 0.03), (-0.06, 0.01, 0.90))
    vb, _ = R.ellipsoid(24, 32, (0.05, 0.09, 0.03), (0.03, -0.02, 0.93))
    assert va.shape == (738, 3) and fa.shape == (1472, 3)
    return np.stack([va, vb]), fa


def _synth_hands(mano_tables, z=0.8):
    verts = np.stack([mano_tables['left']['v_template'] + np.float32([-0.05, 0, z]),
                      mano_tables['right']['v_template'] + np.float32([0.05, 0, z])]).astype(np.float32)
    return verts, [mano_tables['left']['faces'], mano_tables['right']['faces']]


def test_closed_meshes_coverage_ids_colours():
    verts, faces = _ellipsoids()
    img = _images(1, 512, 512)
    cols = [[0.46, 0.59, 0.64], [0.94, 0.71, 0.53]]
    out, ids = _run(verts, faces, img, mesh_frame=[0, 0], colors=cols)
    ref = R.render(verts, faces, img, mesh_frame=[0, 0], colors=cols)
    assert _compare(out, ids, ref, img, what='ellipsoids') == 53070


def test_synthetic_mano_tables_stress(mano_tables):
    """Random index triples: long, overlapping, degenerate triangles; two topologies in one depth-tested pass."""
    verts, faces = _synth_hands(mano_tables)
    img = _images(1, 512, 512, seed=1)
    cols = [[0.46, 0.59, 0.64], [0.94, 0.71, 0.53]]
    out, ids = _run(verts, faces, img, mesh_frame=[0, 0], colors=cols, topo_index=[0, 1])
    ref = R.render(verts, faces, img, mesh_frame=[0, 0], colors=cols)
    _compare(out, ids, ref, img, what='synthetic MANO')


def test_no_holes_at_shared_edges():
    """A flat 16 x 16 quad grid, split into triangles, turned 45 degrees against the pixel grid."""
    n = 16
    g = (np.arange(n + 1) - n / 2) * 0.01
    gx, gy = np.meshgrid(g, g)
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    v = np.stack([c * gx - s * gy, s * gx + c * gy, np.full_like(gx, 0.9)], -1).reshape(-1, 3).astype(np.float32)
    faces = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            faces += [[a, a + 1, a + n + 2], [a, a + n + 2, a + n + 1]]
    faces = np.array(faces, np.int64)
    img = _images(1, 512, 512, seed=2)
    out, ids = _run(v[None], faces, img)
    xi, yi, _, ok = R.snap(v, None, None, 1265.0)
    assert ok.all()
    # the outline is the square through the four snapped corners; "more than one pixel inside" = every edge function of
    # the outline (normalised to pixels) exceeds 1
    corners = [0, n, (n + 1) * (n + 1) - 1, n * (n + 1)]
    cx, cy = xi[corners].astype(np.float64) / 256, yi[corners].astype(np.float64) / 256
    ys, xs = np.mgrid[0:512, 0:512]
    px, py = xs + 0.5, ys + 0.5
    inside = np.ones((512, 512), bool)
    for k in range(4):
        x0, y0, x1, y1 = cx[k], cy[k], cx[(k + 1) % 4], cy[(k + 1) % 4]
        dist = ((x1 - x0) * (py - y0) - (y1 - y0) * (px - x0)) / np.hypot(x1 - x0, y1 - y0)
        inside &= dist > 1.0
    assert inside.sum() > 30000
    assert (ids[0][inside] >= 0).all(), 'hole inside the grid'
    cov = np.argwhere(ids[0] >= 0)
    for y, x in cov:
        assert R.contains(xi, yi, faces[ids[0, y, x]], int(x) * 256 + 128, int(y) * 256 + 128), (x, y)
    ref = R.render(v[None], faces, img)
    assert ((ids[0] >= 0) == (ref['ids'][0] >= 0)).all()      # every pixel exactly once: the integer rule's mask


def test_skips_and_degenerates(mano_tables):
    verts, faces = _ellipsoids()
    img = _images(2, 512, 512, seed=3)
    out, ids = _run(verts, faces, img, mesh_frame=[-1, -1])
    assert (out == img).all() and (ids == -1).all()
    # zero-area faces, a vertex in front of the near limit, a mesh wholly off the canvas, a mesh half off it
    f2 = faces.copy()
    f2[10] = [5, 5, 9]
    f2[11] = [7, 7, 7]
    v = verts.copy()
    v[0, 100, 2] = 0.01                       # Z < 0.05: every triangle at this vertex is dropped
    v[0, 200, 2] = -0.3                       # behind the camera
    v[1] += np.float32([0.13, 0, 0])          # half off the canvas to the right
    v3 = np.concatenate([v, (verts[:1] + np.float32([3.0, 0, 0]))])      # a third mesh wholly off the canvas
    mf = [0, 1, 1]
    out, ids = _run(v3, f2, img, mesh_frame=mf)
    ref = R.render(v3, f2, img, mesh_frame=mf)
    _compare(out, ids, ref, img, what='degenerates')
    assert (ref['ids'][1] >= 0).any() and not (ref['ids'] >= 2 * len(f2)).any()
    # 6 cm from the camera and 2 m wide: the outer vertices snap beyond +-2^22 and take their triangles with them
    far = (verts[:1] - np.float32([-0.06, 0.01, 0.90])) * np.float32([20, 20, 1e-3]) + np.float32([0, 0, 0.06])
    assert not R.snap(far[0], None, None, 1265.0)[3].all()
    out, ids = _run(far, faces, img[:1])
    ref = R.render(far, faces, img[:1])
    _compare(out, ids, ref, img[:1], what='snapped coordinates beyond the limit')


@pytest.mark.parametrize('hw', [(1080, 1920), (480, 640)])
def test_viewport_of_original_frames(hw, mano_tables):
    ops = pkg('ops')
    H, W = hw
    frames = _images(2, H, W, seed=4)
    _, offsets = ops.preprocess(torch.from_numpy(frames).cuda())
    view = ops.view_from_offsets(offsets).numpy()
    o = offsets.numpy()
    assert np.allclose(view[:, 0], o[:, 0] / 512) and np.allclose(view[:, 2], o[:, 5] - o[:, 9])
    verts, faces = _ellipsoids()
    hands, hfaces = _synth_hands(mano_tables, z=1.0)
    out, ids = _run(verts, faces, frames, mesh_frame=[0, 0], view=view)
    ref = R.render(verts, faces, frames, mesh_frame=[0, 0], view=view)
    _compare(out, ids, ref, frames, what='ellipsoids %dx%d' % (W, H))
    assert (ref['ids'][0] >= 0).sum() > 53070 * (max(H, W) / 512.0) ** 2 * 0.5
    out, ids = _run(hands, hfaces, frames, mesh_frame=[1, 1], view=view, topo_index=[0, 1])
    ref = R.render(hands, hfaces, frames, mesh_frame=[1, 1], view=view)
    _compare(out, ids, ref, frames, what='synthetic MANO %dx%d' % (W, H))


def test_determinism_batching_in_place(mano_tables):
    ops = pkg('ops')
    rng = np.random.default_rng(5)
    B = 64
    base, faces = _synth_hands(mano_tables)
    topo = [torch.from_numpy(ops.mesh_topology(f, 778)).cuda() for f in faces]
    verts = np.tile(base[None], (B, 1, 1, 1)).reshape(2 * B, 778, 3)
    trans = rng.uniform(-0.08, 0.08, (2 * B, 3)).astype(np.float32)
    mf = np.repeat(np.arange(B), 2).astype(np.int32)
    mf[rng.integers(0, 2 * B, 10)] = -1
    ti = np.tile([0, 1], B).astype(np.int32)
    img = torch.from_numpy(_images(B, 512, 512, seed=6)).cuda()
    v, t = torch.from_numpy(verts).cuda(), torch.from_numpy(trans).cuda()
    kw = dict(return_ids=True, topo_index=torch.from_numpy(ti))
    a, ia = ops.render_meshes(v, topo, img, mesh_frame=torch.from_numpy(mf), trans=t, **kw)
    b, ib = ops.render_meshes(v, topo, img, mesh_frame=torch.from_numpy(mf), trans=t, **kw)
    assert torch.equal(a, b) and torch.equal(ia, ib)
    assert (ia >= 0).any()
    for n in range(B):
        o, i = ops.render_meshes(v[2 * n:2 * n + 2], topo, img[n:n + 1], mesh_frame=torch.from_numpy(np.where(mf[2 * n:2 * n + 2] >= 0, 0, -1)),
                                 trans=t[2 * n:2 * n + 2], return_ids=True, topo_index=torch.tensor([0, 1]))
        assert torch.equal(o[0], a[n]), 'frame %d alone differs from the batch' % n
        keep = i[0] >= 0
        assert torch.equal(i[0][keep] + 2 * n * len(faces[0]), ia[n][keep]) and torch.equal(keep, ia[n] >= 0)
    work = img.clone()
    c = ops.render_meshes(v, topo, work, mesh_frame=torch.from_numpy(mf), trans=t, out=work, topo_index=torch.from_numpy(ti))
    assert c.data_ptr() == work.data_ptr() and torch.equal(c, a)


# ---- through the stack ---------------------------------------------------------------------------------------------------
# The camera of a synthetic checkpoint is as arbitrary as its weights: seed 0 puts both hands BEHIND the camera (cam_trans z =
# -15.6 / -20.5 m in tests/golden/e2e_batch1.npz), where nothing may be drawn.  Seed 10 ('both_near' of tests/golden/cases.py)
# detects both hands and puts the left one 4.5 m in front of it: that one is drawn from the network's own output.  The tests
# also hand in translations that put BOTH hands in front of the camera.
@pytest.fixture(scope='module')
def near_sd():
    return pkg('synth').make_state_dict(seed=10)


def _placed(B, seed=0):
    """cam_trans [B,2,3]: left hand left of the axis, right hand right of it, 0.8 - 1.1 m away."""
    b = np.arange(B, dtype=np.float32)[:, None] + 0.25 * seed
    h = np.arange(2, dtype=np.float32)[None, :]
    t = np.stack([-0.07 + 0.14 * h + 0.01 * b, 0.02 * b - 0.01 + 0 * h, 0.8 + 0.1 * h + 0.05 * b], -1).astype(np.float32)
    return torch.from_numpy(t).cuda()


def _engine(synth_sd, mano_tables, max_batch=2):
    eng = pkg('engine').Engine(0)
    eng.load_state_dict(synth_sd, max_batch=max_batch)
    eng.load_mano(mano_tables)
    return eng


def _expected(ops, L, out, mano_tables, images, offsets=None, bgr=False, cam_trans=None):
    """ops.render_meshes fed what Engine.render reads: verts, cam_trans, flags and hand types of the fused call."""
    B = images.shape[0]
    if cam_trans is None:
        cam_trans = ops.cam_trans(out['joints'].view(-1, 21, 3), out['pj2d'].view(-1, 21, 2), focal_length=1265.0)
    cam_trans = cam_trans.reshape(-1, 3)
    flags = out['slots'][:, :, L.SLOT_FLAG].reshape(-1) > 0.5
    frame = torch.arange(2 * B, device=flags.device) // 2
    cols = torch.tensor(ops.HAND_COLORS_RGB)
    if bgr:
        cols = cols.flip(1)
    return ops.render_meshes(out['verts'].view(2 * B, 778, 3), (mano_tables['left']['faces'], mano_tables['right']['faces']),
                             images, mesh_frame=torch.where(flags, frame, torch.full_like(frame, -1)), trans=cam_trans,
                             colors=cols.repeat(B, 1), view=None if offsets is None else ops.view_from_offsets(offsets),
                             topo_index=torch.tensor([0, 1]).repeat(B), return_ids=True)


def test_engine_render_matches_render_meshes(near_sd, mano_tables, frames2):
    ops, L = pkg('ops'), pkg('_lib')
    eng = _engine(near_sd, mano_tables)
    img = torch.from_numpy(frames2).cuda()
    out = eng.forward(img, project=True)
    flags = out['slots'][:, :, L.SLOT_FLAG] > 0.5
    assert flags.all()
    # the network's own camera (computed by Engine.render with the cam_trans kernel)
    got, ids = eng.render(out, img, return_ids=True)
    want, want_ids = _expected(ops, L, out, mano_tables, img)
    assert torch.equal(got, want) and torch.equal(ids, want_ids)
    assert (ids >= 0).any() and not torch.equal(got, img)
    # both hands in front of the camera; out of place and in place
    ct = _placed(2)
    got, ids = eng.render(out, img, cam_trans=ct, return_ids=True)
    want, want_ids = _expected(ops, L, out, mano_tables, img, cam_trans=ct)
    assert torch.equal(got, want) and torch.equal(ids, want_ids)
    F = len(mano_tables['left']['faces'])
    assert sorted(torch.unique(ids[ids >= 0] // F).tolist()) == [0, 1, 2, 3]      # all four hands are visible somewhere
    work = img.clone()
    assert eng.render(out, work, cam_trans=ct, dst=work).data_ptr() == work.data_ptr() and torch.equal(work, got)
    # original frames: the offsets rows of the pre-processing are the viewport
    raw = torch.from_numpy(np.ascontiguousarray(np.kron(frames2, np.ones((1, 2, 2, 1), np.uint8))[:, 152:872, :, ::-1])).cuda()
    assert tuple(raw.shape) == (2, 720, 1024, 3)
    rgb, offsets = ops.preprocess(raw)
    out = eng.forward(rgb, offsets=offsets, project=True)
    for ct in (None, _placed(2, seed=10)):
        got, ids = eng.render(out, raw, offsets=offsets, cam_trans=ct, bgr=True, return_ids=True)
        want, want_ids = _expected(ops, L, out, mano_tables, raw, offsets=offsets, bgr=True, cam_trans=ct)
        assert got.shape == raw.shape and torch.equal(got, want) and torch.equal(ids, want_ids)
    assert (ids >= 0).any()
    # a frame without a detection comes back untouched
    eng.set_conf_thresh(1e6)      # (synthetic center scores are not bounded by 1)
    out = eng.forward(img, project=True)
    assert not (out['slots'][:, :, L.SLOT_FLAG] > 0.5).any()
    got, ids = eng.render(out, img, cam_trans=_placed(2), return_ids=True)
    assert torch.equal(got, img) and (ids == -1).all()
    eng.close()


def test_render_before_faces_is_a_state_error(synth_sd, mano_tables, frames2):
    L = pkg('_lib')
    eng = pkg('engine').Engine(0)
    eng.load_state_dict(synth_sd, max_batch=2)
    eng.load_mano({s: {k: v for k, v in mano_tables[s].items() if k != 'faces'} for s in ('left', 'right')})
    assert not eng.have_faces
    img = torch.from_numpy(frames2).cuda()
    out = eng.forward(img, project=True)
    with pytest.raises(L.AcrmiError, match='faces'):
        eng.render(out, img)
    eng.load_faces('left', mano_tables['left']['faces'])
    eng.load_faces('right', mano_tables['right']['faces'])
    assert eng.have_faces and eng.render(out, img).shape == img.shape
    eng.close()


def test_pool_render_on_the_tickets_stream(near_sd, mano_tables, frames2):
    eng = _engine(near_sd, mano_tables)
    img = torch.from_numpy(frames2).cuda()
    out = eng.forward(img, project=True)
    ct = _placed(2)
    want = [eng.render(out, img, return_ids=True), eng.render(out, img, cam_trans=ct, return_ids=True)]
    assert (want[0][1] >= 0).any() and (want[1][1] >= 0).any()
    pool = pkg('engine').EnginePool(0, n=2)
    pool.load_state_dict(near_sd, max_batch=2)
    pool.load_mano(mano_tables)
    for k in range(4):      # both contexts, twice; the network's camera and the placed one
        t = pool.submit(img, project=True)
        got, ids = pool.render(t, img, return_ids=True, cam_trans=ct if k % 2 else None)
        pool.collect(t)
        assert torch.equal(got, want[k % 2][0]) and torch.equal(ids, want[k % 2][1])
    with pytest.raises(RuntimeError):
        pool.render(t, img)
    pool.close()
    eng.close()


def test_acr_layer_renders_and_leaves_results_alone(near_sd, mano_tables, frames2):
    cfg = pkg('config')
    synth_sd = near_sd
    acr = pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml', '--renderer', 'hip']),
                              state_dict=synth_sd, mano_tables=mano_tables, max_batch=2)
    rs = np.random.RandomState(7)
    big = np.clip(np.kron(rs.randint(0, 256, (135, 240, 3)).astype(np.float32), np.ones((8, 8, 1), np.float32)), 0, 255).astype(np.uint8)
    small = np.ascontiguousarray(frames2[0][:, :, ::-1])      # BGR 512 x 512
    frames = [torch.from_numpy(big).cuda(), torch.from_numpy(small).cuda()]
    plain = acr.forward_raw_batch(frames, ['a', 'b'])
    res, drawn = acr.forward_raw_batch(frames, ['a', 'b'], render=True)
    assert [tuple(d.shape) for d in drawn] == [(1080, 1920, 3), (512, 512, 3)]
    assert sorted(res) == sorted(plain)
    for k in plain:
        assert len(res[k]) == len(plain[k])
        for h1, h2 in zip(res[k], plain[k]):
            assert sorted(h1) == sorted(h2) and all(np.array_equal(h1[f], h2[f]) for f in h1)
    assert len(res['b']) == 2 and not torch.equal(drawn[1], frames[1])
    for d, f, k in zip(drawn, frames, 'ab'):
        changed = (d != f).any(-1)
        visible = [h for h in res[k] if float(h['cam_trans'][2]) > 0.1]      # (the others are behind the camera)
        assert bool(changed.any()) == bool(visible)
        for h in visible:      # the overlay sits where the projected joints are
            pj = h['pj2d_org'].astype(np.float32)
            lo, hi = pj.min(0) - 40, pj.max(0) + 40
            ys, xs = torch.nonzero(changed, as_tuple=True)
            assert len(xs) > 100
            inside = (xs >= lo[0]) & (xs <= hi[0]) & (ys >= lo[1]) & (ys <= hi[1])
            assert inside.any()
    # the network input itself, as one tensor
    img = torch.from_numpy(frames2).cuda()
    res2, drawn2 = acr.forward_batch(img, ['a', 'b'], render=img)
    assert drawn2.shape == img.shape and not torch.equal(drawn2, img)
    # single image: the reference's key, on the `rendering` attribute; the results dict is what it always was
    one = acr(small, 'b')
    assert sorted(one) == ['b'] and acr.rendering['mesh_rendering_orgimgs'][0].shape == small.shape
    assert (acr.rendering['mesh_rendering_orgimgs'][0] != small).any()
    off = pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml']), state_dict=synth_sd,
                              mano_tables=mano_tables, max_batch=2)
    off(small, 'b')
    assert off.rendering is None
