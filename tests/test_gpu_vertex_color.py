"""GPU tests of the per-vertex colour views against the numpy restatement in
tests/vertex_color_ref.py: the rasteriser with a colour per vertex (exact coverage, ids outside the pixels an fp32 depth cannot
order, colours within one count and - so that a systematic off-by-one cannot hide behind that bar - at most 0.1 % of the pixels
off by that count), acrmi_vertex_colors and acrmi_contact_values for equal bits, and the Engine / ACR calls against the
operators on the same tensors.

The four rasteriser scenes are 128 x 128 (view 0.25): 3261 covered pixels, none ambiguous, for the two ellipsoids, 7361 covered
with 38 ambiguous (0.52 %) for the synthetic MANO hands."""
import numpy as np
import pytest
import torch

import render_ref as R
import vertex_color_ref as VR
from conftest import pkg
from contact_cases import eng, frames3, near_sd      # (fixtures)

pytestmark = pytest.mark.gpu

AMBIGUOUS_CAP = 0.01      # share of the covered pixels whose two nearest surfaces are within 1e-5 relative in 1/Z
OFF_BY_ONE_CAP = 0.001    # share of the covered unambiguous pixels that may differ by one count (floor of fp32 against float64)
F32 = np.float32
VIEW = np.array([[0.25, 0.25, 0, 0]], F32)
CENTRES = ((-0.06, 0.01, 0.90), (0.03, -0.02, 0.93))      # those of tests/test_gpu_render.py's ellipsoids
_cache = {}


def _images(n, h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3)).astype(np.uint8)


def _scene(name, mano_tables):
    """-> (verts [2,V,3], faces per mesh, faces argument of the operator, topo_index, vcol [2,V,3], image [1,128,128,3])."""
    if name == 'mano':
        verts = np.stack([mano_tables['left']['v_template'] + F32([-0.05, 0, 0.8]),
                          mano_tables['right']['v_template'] + F32([0.05, 0, 0.8])]).astype(F32)
        faces = [np.asarray(mano_tables['left']['faces']), np.asarray(mano_tables['right']['faces'])]
        arg, ti = faces, [0, 1]
    else:
        va, fa = R.ellipsoid(12, 16, (0.05, 0.09, 0.03), CENTRES[0])
        vb, _ = R.ellipsoid(12, 16, (0.05, 0.09, 0.03), CENTRES[1])
        verts = np.stack([va, vb])
        if name == 'reversed':      # the second mesh wound the other way: the same picture, through the re-orientation bit
            faces, arg, ti = [fa, fa[:, ::-1].copy()], [fa, fa[:, ::-1].copy()], [0, 1]
        else:
            faces, arg, ti = [fa, fa], fa, None
    vcol = np.random.default_rng(7).uniform(0, 1, verts.shape).astype(F32)
    return verts, faces, arg, ti, vcol, _images(1, 128, 128, seed=11)


def _reference(name, mano_tables):
    """The restatement's picture of a scene, computed once ('mesh_view' and 'reversed' show the picture of 'ellipsoids')."""
    key = 'mano' if name == 'mano' else 'ellipsoids'
    if key not in _cache:
        verts, faces, _, _, vcol, img = _scene(key, mano_tables)
        ref = VR.render(verts, faces, img, vcol, mesh_frame=[0, 0], view=VIEW)
        for v in ref.values():
            v.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def _run(verts, faces, images, vcol, **kw):
    ops = pkg('ops')
    t = {k: (None if v is None else torch.as_tensor(np.asarray(v))) for k, v in kw.items()}
    out, ids = ops.render_meshes(torch.from_numpy(np.asarray(verts, F32)).cuda(), faces, torch.from_numpy(images).cuda(),
                                 return_ids=True, vertex_colors=None if vcol is None else torch.from_numpy(np.asarray(vcol, F32)).cuda(),
                                 **t)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ids.cpu().numpy()


def _compare(got_out, got_ids, ref, images, what=''):
    cov = ref['ids'] >= 0
    amb = R.ambiguous(ref)
    clear = cov & ~amb
    n_cov, n_amb, n_clear = int(cov.sum()), int(amb.sum()), int(clear.sum())
    id_bad = int(((got_ids != ref['ids']) & clear).sum())
    diff = np.abs(got_out.astype(np.int64) - ref['out'].astype(np.int64)).max(-1)
    col_worst = int(diff[clear].max()) if n_clear else 0
    n_off = int((diff[clear] == 1).sum())
    print('%s: covered %d, ambiguous %d (%.4f %%), mask mismatches %d, id mismatches outside ambiguous %d, worst colour '
          'difference %d, pixels off by one count %d of %d (%.4f %%)'
          % (what, n_cov, n_amb, 100.0 * n_amb / max(n_cov, 1), int(((got_ids >= 0) != cov).sum()), id_bad, col_worst, n_off,
             n_clear, 100.0 * n_off / max(n_clear, 1)))
    assert ((got_ids >= 0) == cov).all(), 'covered mask differs from the integer rule'
    assert (got_out[~cov] == images[~cov]).all(), 'an uncovered pixel changed'
    assert n_amb <= AMBIGUOUS_CAP * max(n_cov, 1)
    assert id_bad == 0
    assert col_worst <= 1
    assert n_off <= OFF_BY_ONE_CAP * max(n_clear, 1)
    return n_cov, n_amb


# ---- the rasteriser ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ellipsoids', 'mano', 'reversed', 'mesh_view'])
def test_rasteriser_matches_the_restatement(name, mano_tables):
    verts, faces, arg, ti, vcol, img = _scene(name, mano_tables)
    ref = _reference(name, mano_tables)
    kw = dict(mesh_frame=[0, 0], topo_index=ti)
    if name == 'mesh_view':      # one row per mesh; the depth value is 0.25 / Z for both: the same order, the same picture
        kw['mesh_view'] = np.repeat(VIEW, 2, 0)
    else:
        kw['view'] = VIEW
    out, ids = _run(verts, arg, img, vcol, **kw)
    n_cov, n_amb = _compare(out, ids, ref, img, what=name)
    assert (n_cov, n_amb) == ((7361, 38) if name == 'mano' else (3261, 0))
    flat, flat_ids = _run(verts, arg, img, None, **kw)
    assert (flat_ids == ids).all() and (flat != out).any()      # the colours reach the picture, and nothing else does


def test_batching_in_place_determinism_and_constant_colours(mano_tables):
    ops = pkg('ops')
    verts, faces, arg, ti, vcol, _ = _scene('mano', mano_tables)
    B = 4
    g = np.random.default_rng(3)
    v = torch.from_numpy(np.tile(verts[None], (B, 1, 1, 1)).reshape(2 * B, 778, 3)).cuda()
    t = torch.from_numpy(g.uniform(-0.04, 0.04, (2 * B, 3)).astype(F32)).cuda()
    vc = torch.from_numpy(g.uniform(0, 1, (2 * B, 778, 3)).astype(F32)).cuda()
    topo = [torch.from_numpy(ops.mesh_topology(f, 778)).cuda() for f in faces]
    img = torch.from_numpy(_images(B, 128, 128, seed=5)).cuda()
    view = torch.from_numpy(np.repeat(VIEW, B, 0))
    mf = torch.arange(2 * B, dtype=torch.int32) // 2
    mf[3] = -1
    ti = torch.tensor([0, 1] * B)
    a, ia = ops.render_meshes(v, topo, img, mesh_frame=mf, trans=t, view=view, topo_index=ti, vertex_colors=vc, return_ids=True)
    b, ib = ops.render_meshes(v, topo, img, mesh_frame=mf, trans=t, view=view, topo_index=ti, vertex_colors=vc, return_ids=True)
    assert torch.equal(a, b) and torch.equal(ia, ib) and (ia >= 0).any()
    for n in range(B):
        s = slice(2 * n, 2 * n + 2)
        o, i = ops.render_meshes(v[s], topo, img[n:n + 1], mesh_frame=torch.where(mf[s] >= 0, 0, -1).to(torch.int32), trans=t[s],
                                 view=view[:1], topo_index=ti[s], vertex_colors=vc[s], return_ids=True)
        keep = i[0] >= 0
        assert torch.equal(o[0], a[n]), 'frame %d alone differs from the batch' % n
        assert torch.equal(keep, ia[n] >= 0) and torch.equal(i[0][keep] + 2 * n * len(faces[0]), ia[n][keep])
    work = img.clone()
    c = ops.render_meshes(v, topo, work, mesh_frame=mf, trans=t, view=view, topo_index=ti, vertex_colors=vc, out=work)
    assert c.data_ptr() == work.data_ptr() and torch.equal(c, a)
    # the same colour at every vertex of a mesh: the flat call, within one count (base = (w0 c + w1 c + w2 c) / d, not c)
    cols = torch.from_numpy(g.uniform(0, 1, (2 * B, 3)).astype(F32))
    const = cols[:, None, :].repeat(1, 778, 1).cuda()
    flat = ops.render_meshes(v, topo, img, mesh_frame=mf, trans=t, view=view, topo_index=ti, colors=cols)
    got = ops.render_meshes(v, topo, img, mesh_frame=mf, trans=t, view=view, topo_index=ti, vertex_colors=const)
    assert (flat.int() - got.int()).abs().max().item() <= 1 and torch.equal(flat[ia < 0], got[ia < 0])


def test_wild_colours_stay_inside_the_picture(mano_tables):
    """NaN, infinities, negative and huge colours: the covered pixels take whatever the clamp makes of them, every other byte
    and every id stays, and the call comes back clean."""
    verts, faces, arg, ti, vcol, img = _scene('ellipsoids', mano_tables)
    ref = _reference('ellipsoids', mano_tables)
    wild = vcol.copy().reshape(-1)
    g = np.random.default_rng(9)
    wild[g.integers(0, wild.size, 400)] = np.tile(F32([np.nan, np.inf, -np.inf, -3.0, 7.5, 3e38, -3e38, 1e-42]), 50)
    wild = wild.reshape(vcol.shape)
    out, ids = _run(verts, arg, img, wild, mesh_frame=[0, 0], view=VIEW)
    cov = ref['ids'] >= 0
    assert (ids == ref['ids']).all() and (out[~cov] == img[~cov]).all()
    allnan, ids2 = _run(verts, arg, img, np.full_like(vcol, np.nan), mesh_frame=[0, 0], view=VIEW)
    assert (ids2 == ids).all() and (allnan[~cov] == img[~cov]).all()
    w = 0.9      # a NaN colour gives 0 through the clamp: not the background, and not the (1 - w) img term alone
    assert (allnan[cov] == 0).all()
    again, _ = _run(verts, arg, img, vcol, mesh_frame=[0, 0], view=VIEW)      # the next call is as good as ever
    assert np.abs(again.astype(int) - ref['out'].astype(int)).max() <= 1 and w == 0.9


# ---- values -> colours --------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize('shape', [(1, 5), (3, 64), (2, 257), (6, 778)])
def test_vertex_colors_bits(shape):
    ops = pkg('ops')
    M, V = shape
    g = np.random.default_rng(M * 1000 + V)
    lo, hi = 0.001, 0.02
    special = F32([lo, hi, np.nan, np.inf, -np.inf, 1e-42, -1e-42, 0.0, -0.0, np.nextafter(F32(hi), F32(0)), np.nextafter(F32(hi), F32(1)),
                   np.nextafter(F32(lo), F32(0)), 3e38, -3e38])
    values = g.uniform(-0.005, 0.03, (M, V)).astype(F32)
    values.reshape(-1)[g.permutation(M * V)[:min(len(special), M * V)]] = special[:M * V]
    flags = np.where(g.uniform(size=(M, V)) < 0.2, g.integers(-2 ** 31, 2 ** 31, (M, V)), 0).astype(np.int32)
    base = g.uniform(0, 1, (M, 3)).astype(F32)
    own = g.integers(0, 256, (256, 3)).astype(np.uint8)
    dv, df, db = torch.from_numpy(values).cuda(), torch.from_numpy(flags).cuda(), torch.from_numpy(base).cuda()
    for reverse in (False, True):
        for lut in (None, own):
            for bgr in (False, True):
                for fl in (None, flags):
                    got = ops.vertex_colors(dv, lo, hi, flags=None if fl is None else df, base=db, flag_color=(0.25, 1.0, 0.5), lut=lut,
                                            reverse=reverse, bgr=bgr).cpu().numpy()
                    want = VR.vertex_colors(values, lo, hi, flags=fl, base=base, flag_color=(0.25, 1.0, 0.5), lut=lut,
                                            reverse=reverse, bgr=bgr)
                    assert got.shape == (M, V, 3) and (_bits(got) == _bits(want)).all(), (reverse, lut is None, bgr, fl is None,
                                                                                          np.argwhere(_bits(got) != _bits(want))[:4])
    with pytest.raises(ValueError):
        ops.vertex_colors(dv, 0.02, 0.02)
    with pytest.raises(ValueError):
        ops.vertex_colors(dv, 0.0, float('nan'))


# ---- contact results -> values per hand ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', [5, 64, 257, 778])
def test_contact_values_bits(V):
    ops = pkg('ops')
    seen = np.zeros(4, bool)
    for K in (1, 2, 3):
        for B in (1, 3):
            g = np.random.default_rng(V * 100 + K * 10 + B)
            n = B * K * K
            d2 = g.uniform(0, 1e-3, (n, 2, V)).astype(F32)
            r = g.integers(0, 16, d2.shape)
            d2[r == 0] = np.inf
            d2[r == 1] = np.nan
            d2[r == 2] = F32(2.5e-4)      # ties between partners
            s = (g.uniform(-1, 1, d2.shape) * (r != 3)).astype(F32)
            cross = g.integers(0, 5, d2.shape).astype(np.int32)
            skipped = g.uniform(size=n) < 0.25      # whole skipped pairs, as the measures write them
            d2[skipped], s[skipped], cross[skipped] = np.inf, 0, 0
            dd, ds, dc = (torch.from_numpy(x).cuda() for x in (d2, s, cross))
            for surface in (False, True):
                for m in (0.02, 0.015, float('inf')):
                    con = {'d2': dd, 'cross': dc} if surface else {'d2': dd, 'side': ds}
                    got = ops.contact_values(con, B, K, max_depth=m)
                    val, flag = VR.contact_values(d2, cross if surface else s, B, K, m, surface=surface)
                    gv, gf = got['value'].cpu().numpy(), got['flag'].cpu().numpy()
                    assert gv.shape == (B, K, 2, V) and gf.dtype == np.int32
                    assert np.array_equal(np.isnan(gv), np.isnan(val)) and (_bits(gv)[~np.isnan(val)] == _bits(val)[~np.isnan(val)]).all()
                    assert np.array_equal(gf, flag), (V, K, B, surface, m)
                    for b in range(B):      # a row alone equals the row in the batch
                        rows = slice(b * K * K, (b + 1) * K * K)
                        one = ops.contact_values({k: v[rows] for k, v in con.items()}, 1, K, max_depth=m)
                        assert torch.equal(one['flag'][0], got['flag'][b])
                        assert np.array_equal(one['value'][0].cpu().numpy(), gv[b], equal_nan=True)
                    seen |= np.array([flag.any(), not flag.all(), np.isnan(val).any(), not np.isnan(val).all()])
    assert seen.all(), seen      # (over the cases of this V: flags set and not set, hands with and without a computed pair)


# ---- engine level ---------------------------------------------------------------------------------------------------------
def _placed(B, K):
    """cam_trans [B,K,2,3]: the hands of a row a few centimetres apart, the rows 0.8 to 1.0 m in front of the camera."""
    g = np.random.default_rng(22 * B + K)
    t = g.uniform(-0.02, 0.02, (B, K, 2, 3))
    t[..., 2] += g.uniform(0.82, 0.98, (B, 1, 1))
    return torch.from_numpy(t.astype(F32)).cuda()


def _truth(out, seed):
    g = torch.Generator().manual_seed(seed)
    noise = lambda t: t + (torch.randn(t.shape, generator=g) * 0.008).to(t.device)
    return {'joints': noise(out['joints']), 'verts': noise(out['verts'])}


def _engine_views(eng, mano_tables, frames, K):
    """The two colour views of B = 2 frames at K hands per side -> everything the engine returned, and the operators' results
    on the same tensors."""
    ops, L = pkg('ops'), pkg('_lib')
    B = 2
    out = eng.forward(frames[:B], project=True, **({} if K == 1 else {'max_hand': K}))
    out['slots'][..., L.SLOT_FLAG] = 1.0
    out['slots'][1, ..., 1, L.SLOT_FLAG] = 0.0      # the second row has no right hand: its left hands have no partner
    ct = _placed(B, K) if K > 1 else _placed(B, K)[:, 0]
    gt = _truth(out, K)
    faces = (mano_tables['left']['faces'], mano_tables['right']['faces'])
    n = B * K
    flat = {'slots': out['slots'].reshape(n, 2, L.SLOT), 'verts': out['verts'].reshape(n, 2, 778, 3)}
    flags = flat['slots'][:, :, L.SLOT_FLAG] > 0.5
    frame_of = torch.arange(B, device='cuda').repeat_interleave(K)
    mf = torch.where(flags, frame_of[:, None].expand(n, 2), torch.full_like(frame_of[:, None].expand(n, 2), -1)).reshape(-1).to(torch.int32)

    rows = torch.tensor([[512., 512, 0, 0, 0, 0, 0, 0, 0, 0]]).repeat(n, 1).cuda()      # the whole 512 x 512 frame, per region

    def both(draw_engine):
        res = {}
        for mode in ('vertex', 'surface'):
            con = eng.contact(out, max_hand=K, cam_trans=ct, mode=mode)
            res['contact_' + mode] = eng.contact_colors(con, out, max_hand=K)
            res['con_' + mode] = con
        sc = eng.score(out, gt, max_hand=K, cam_trans=ct)
        res['sc'] = sc
        for kind in ('ra', 'pa'):
            res['error_' + kind] = eng.error_colors(sc, out, max_hand=K, kind=kind, hi=0.015)
        res['drawn'] = draw_engine(res['contact_vertex'])
        return res

    def draw_engine(vcol):
        if K == 1:
            return eng.render(out, frames[:B], cam_trans=ct, vertex_colors=vcol)
        sub = dict(flat, cam_trans=ct.reshape(n, 2, 3))
        return eng.render_regions(sub, frames[:B], rows, frame_of.to(torch.int32), cam_trans=ct.reshape(n, 2, 3),
                                  vertex_colors=vcol.reshape(n, 2, 778, 3))

    def draw_ops(vcol):
        kw = {} if K == 1 else {'mesh_view': torch.tensor([[1., 1, 0, 0]]).repeat(2 * n, 1)}
        return ops.render_meshes(flat['verts'].reshape(2 * n, 778, 3), faces, frames[:B], mesh_frame=mf, trans=ct.reshape(2 * n, 3),
                                 topo_index=[0, 1] * n, vertex_colors=vcol.reshape(2 * n, 778, 3), **kw)

    return out, both, draw_engine, draw_ops


@pytest.mark.parametrize('K', [1, 2])
def test_engine_colour_views_match_the_operators(eng, mano_tables, frames3, K):
    ops = pkg('ops')
    B = 2
    out, both, draw_engine, draw_ops = _engine_views(eng, mano_tables, frames3, K)
    res = both(draw_engine)
    lead = tuple(out['slots'].shape[:-1])
    base = torch.tensor(ops.HAND_COLORS_RGB).repeat(B * K, 1).cuda()
    for mode in ('vertex', 'surface'):
        con = res['con_' + mode]
        cv = ops.contact_values(con, B, K)
        want = ops.vertex_colors(cv['value'].view(-1, 778), 0.0, 0.02, flags=cv['flag'].view(-1, 778), base=base, reverse=True)
        got = res['contact_' + mode]
        assert tuple(got.shape) == lead + (778, 3) and torch.equal(got.reshape(-1, 778, 3), want), mode
        value = cv['value'].view(B, K, 2, 778)
        assert torch.isnan(value[1]).all() and not torch.isnan(value[0]).any()      # row 1 has no pair, row 0 has them all
        assert torch.equal(got.reshape(B, K, 2, 778, 3)[1], base.view(B, K, 2, 1, 3)[1].expand(K, 2, 778, 3))
        assert (value[0] < 0.02).any(), 'no vertex within `far`: the scene shows nothing'
    sc = res['sc']
    for kind in ('ra', 'pa'):
        e = sc['verts']['e_' + kind]
        values = torch.where(e < 0, torch.full_like(e, float('nan')), e)
        want = ops.vertex_colors(values, 0.0, 0.015, base=base)
        assert torch.equal(res['error_' + kind].reshape(-1, 778, 3), want), kind
        assert torch.isnan(values).any() and not torch.isnan(values).all()      # (the unflagged hands of row 1 are not scored)
    assert not torch.equal(res['error_ra'], res['error_pa'])
    drawn = res['drawn']
    assert torch.equal(drawn, draw_ops(res['contact_vertex'])) and not torch.equal(drawn, frames3[:B])
    bgr = eng.contact_colors(res['con_vertex'], out, max_hand=K, bgr=True)      # the table and the base colours flipped
    assert torch.equal(bgr, res['contact_vertex'].flip(-1))
    # the same calls queue without a host visit
    ct = _placed(B, K) if K > 1 else _placed(B, K)[:, 0]      # (copied to the device before the mode is switched on)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        con = eng.contact(out, max_hand=K, cam_trans=ct)
        quiet = {'contact_vertex': eng.contact_colors(con, out, max_hand=K),
                 'error_ra': eng.error_colors(sc, out, max_hand=K, kind='ra', hi=0.015)}
        quiet['drawn'] = draw_engine(quiet['contact_vertex'])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for k, v in quiet.items():
        assert torch.equal(v, res[k]), k


def test_forward_batch_contact_view(near_sd, mano_tables, frames3):
    cfg = pkg('config')
    acr = pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml']), state_dict=near_sd,
                              mano_tables=mano_tables, max_batch=2)
    img = frames3[:2]
    plain_res, plain = acr.forward_batch(img, ['a', 'b'], contact=True, render=img, show_items=('mesh',))
    res, views = acr.forward_batch(img, ['a', 'b'], contact=True, render=img, show_items=('mesh', 'contact'))
    assert set(views) == {'mesh', 'contact'} and views['contact'].shape == img.shape and views['contact'].dtype == torch.uint8
    assert torch.equal(views['mesh'], plain['mesh'])      # byte for byte what it is without the new view
    assert all(np.array_equal(h0[f], h1[f]) for k in res for h0, h1 in zip(plain_res[k], res[k]) for f in h0)
    surf = acr.forward_batch(img, ['a', 'b'], contact='surface', render=img, show_items=('contact',))[1]['contact']
    assert surf.shape == img.shape
    # against the engine on what the fused call returned
    e = acr.model.engine(2)
    e.set_point_heads(True)
    try:
        out = e.forward(img, offsets=torch.tensor([[512., 512, 0, 0, 0, 0, 0, 0, 0, 0]]).repeat(2, 1), project=True)
    finally:
        e.set_point_heads(False)
    ct = pkg('ops').cam_trans(out['joints'].view(-1, 21, 3), out['pj2d'].view(-1, 21, 2), focal_length=acr.focal_length).view(2, 2, 3)
    vcol = e.contact_colors(e.contact(out, cam_trans=ct), out)
    want = e.render(out, img, cam_trans=ct, focal_length=float(acr.focal_length), vertex_colors=vcol)
    assert torch.equal(views['contact'], want)
    gt = {'joints': out['joints'] + 0.004, 'verts': out['verts'] * 1.05}
    both = acr.forward_batch(img, ['a', 'b'], contact=True, gt=gt, render=img, show_items=('error', 'contact', 'mesh'))[1]
    assert list(both) == ['error', 'contact', 'mesh'] and torch.equal(both['contact'], views['contact'])
    assert torch.equal(both['mesh'], plain['mesh'])
    two = acr.forward_batch(img, ['a', 'b'], contact=True, render=img, show_items=('mesh', 'contact'), max_hand=2)[1]
    assert two['contact'].shape == img.shape and two['mesh'].shape == img.shape
    raw = torch.from_numpy(np.ascontiguousarray(img.cpu().numpy()[..., ::-1])).cuda()
    _, nv = acr.forward_raw_batch(raw, ['a', 'b'], contact=True, render=True, show_items=('contact',), render_format='nv12')
    assert tuple(nv['contact'].shape) == (2, 768, 512)
    with pytest.raises(ValueError, match='contact=True'):
        acr.forward_batch(img, ['a', 'b'], render=img, show_items=('contact',))
