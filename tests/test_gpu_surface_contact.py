"""The surface contact measure on the GPU (csrc/contact.hip) against the numpy restatement
(tests/surface_contact_ref.py) FOR EQUALITY: face, cross, the bits of d2 and point, and the summaries.  There is no tolerance
anywhere in this file; the one thing not compared is the payload of a NaN (contact_ref.same_bits).  Then the engine level:
Engine.contact(mode='surface'), EnginePool.contact and forward_batch(contact='surface') against the stand-alone operator on the
same tensors, and the default mode left as it was."""
import numpy as np
import pytest
import torch

import contact_cases as C
import contact_ref
import surface_contact_ref as R
from conftest import pkg
from contact_cases import LATLON, PAIRS, eng, frames3, near_sd, placed, scene      # (eng, frames3, near_sd: fixtures)

pytestmark = pytest.mark.gpu

KEYS, OLD_KEYS = C.KEYS['surface'], C.KEYS['vertex']


def host(res, keys=KEYS):
    return C.host(res, keys)


def assert_equal(got, want, what=''):
    C.assert_equal('surface', got, want, what)


def by_operator(ops, L, out, K, cam_trans, mano_tables, **kw):
    return C.by_operator('surface', ops, L, None, out, K, cam_trans, mano_tables, **kw)


@pytest.mark.parametrize('V', sorted(LATLON))
def test_matches_the_restatement(V):
    ops = pkg('ops')
    verts, faces, ti = scene(V)
    g = np.random.default_rng(V)
    trans = g.uniform(-0.01, 0.01, (5, 3)).astype(np.float32)
    dv = torch.from_numpy(verts).cuda()
    pairs = PAIRS if V < 778 else PAIRS[:3]      # (the restatement takes a third of a second per direction at 778 x 1552)
    clean = None
    for tr in (None, trans):
        want = R.mesh_surface_contact(verts, faces, pairs, trans=tr, topo_index=ti, contact_dist=0.005, max_depth=0.02)
        clean = want if clean is None else clean
        for r, m in ((0.005, 0.02), (0.0, float('inf'))):
            got = host(ops.mesh_surface_contact(dv, faces, pairs, trans=None if tr is None else torch.from_numpy(tr),
                                                topo_index=ti, contact_dist=r, max_depth=m))
            assert_equal(got, want if m == 0.02 else R.with_params(want, r, m), (V, tr is not None, r, m))
    if V >= 257:      # the cases are not trivial: the overlapping spheres overlap, the ones 0.12 apart do not touch
        assert clean['n_inside'][0].min() > 0 and clean['n_inside'][1].sum() == 0 and clean['n_contact'][1].sum() == 0
    # one topology, no topo_index; a topology blob on the device instead of faces, and the pairs in a device tensor
    blob = torch.from_numpy(ops.mesh_topology(faces[0], V)).cuda()
    got = host(ops.mesh_surface_contact(dv[:3], blob, torch.tensor(PAIRS[:2], dtype=torch.int32).cuda()))
    assert_equal(got, {k: v[:2] for k, v in clean.items()}, (V, 'blob'))


def face_counts():
    T = pkg('ops').SURFACE_FACE_TILE
    return [1, T - 1, T, T + 1, 2 * T + 1]


@pytest.mark.parametrize('k', range(5))
def test_face_counts_around_the_tile(k):
    """Random triples over 64 vertices: one face, one face short of a tile, a tile, a tile and one face, two tiles and one."""
    ops = pkg('ops')
    F = face_counts()[k]
    g = np.random.default_rng(100 + F)
    verts = (g.uniform(-0.05, 0.05, (3, 64, 3)) + np.array((0, 0, 0.5))).astype(np.float32)
    f = g.integers(0, 64, (F, 3))
    kw = dict(contact_dist=0.004, max_depth=0.03)
    got = host(ops.mesh_surface_contact(torch.from_numpy(verts).cuda(), f, [[0, 1], [2, 0]], **kw))
    assert_equal(got, R.mesh_surface_contact(verts, f, [[0, 1], [2, 0]], **kw), F)
    assert (got['face'] >= 0).all() and got['face'].max() <= F - 1 and (F == 1 or got['face'].max() > F // 2)


def test_synthetic_mano_hands(mano_tables):
    """The 778-vertex templates of the synthetic tables over their 1538 faces (random triples): two topologies per call."""
    ops = pkg('ops')
    g = np.random.default_rng(3)
    tl, tr = (np.asarray(mano_tables[s]['v_template'], np.float32).reshape(778, 3) for s in ('left', 'right'))
    verts = np.stack([tl, tr, tl + g.normal(0, 0.002, tl.shape).astype(np.float32), tr * np.float32(1.05)])
    trans = np.array([[0, 0, 0.8], [0.03, 0.01, 0.81], [0.2, 0, 0.9], [0.21, 0.01, 0.9]], np.float32)
    faces = (mano_tables['left']['faces'], mano_tables['right']['faces'])
    pairs = [[0, 1], [2, 3], [0, 3]]
    got = host(ops.mesh_surface_contact(torch.from_numpy(verts).cuda(), faces, pairs, trans=torch.from_numpy(trans).cuda(),
                                        topo_index=[0, 1, 0, 1]))
    want = R.mesh_surface_contact(verts, faces, pairs, trans=trans, topo_index=[0, 1, 0, 1])
    assert_equal(got, want)
    assert want['n_contact'][:2].sum() > 0 and want['cross'].max() > 0


def test_edge_cases():
    ops = pkg('ops')
    V = 70
    g = np.random.default_rng(5)
    f = g.integers(0, V - 1, (90, 3))                     # vertex V - 1 is referenced by no face
    f[0] = (20, 21, 22)
    f[1:5] = [(3, 3, 9), (4, 9, 4), (9, 5, 5), (6, 6, 6)]  # faces with repeated indices
    verts = g.uniform(-0.05, 0.05, (6, V, 3)).astype(np.float32)
    verts[1, 10] = verts[1, 3]                            # duplicated vertices
    verts[1, 40] = verts[1, 3]
    verts[1, 20:23] = [(0, 0, 0), (0.25, 0, 0), (0, 0.25, 0)]      # face 0 of mesh 1 on a grid, so that the next three are exact:
    verts[0, 7] = verts[1, 20]                            # a vertex of mesh 0 exactly on a vertex of mesh 1,
    verts[0, 8] = (0.125, 0, 0)                           # ... on an edge
    verts[0, 9] = (0.0625, 0.0625, 0)                     # ... and on a face
    verts[2, 5, 1] = np.nan                               # a NaN vertex
    verts[3] = np.nan                                     # an all-NaN mesh
    verts[4, 0] = 3e19                                    # squares overflow: +inf never wins
    pairs = [[0, 1], [1, 0], [0, 0], [-1, 2], [0, 2], [2, 3], [3, 3], [1, -5], [4, 0], [0, 1]]      # mesh 0 in many pairs
    dv = torch.from_numpy(verts).cuda()
    kw = dict(contact_dist=0.0, max_depth=float('inf'))
    got = host(ops.mesh_surface_contact(dv, f, pairs, **kw))
    want = R.mesh_surface_contact(verts, f, pairs, **kw)
    assert_equal(got, want)
    assert not got['d2'][0, 0, 7:10].any() and got['n_contact'][0, 0] >= 3
    assert np.array_equal(got['point'][0, 0, 7:10], verts[0, 7:10])
    assert not got['d2'][2, :, :V - 1][:, np.isin(np.arange(V - 1), f[5:])].any()      # a mesh with itself: on its own faces
    assert got['face'][4, 1, 5] == -1 and np.isinf(got['d2'][4, 1, 5]) and not got['point'][4, 1, 5].any()
    assert (got['face'][5, 0] == -1).all() and (got['face'][6] == -1).all() and (got['closest'][6] == -1).all()
    assert not got['cross'][6].any() and not got['n_inside'][6].any()
    assert got['face'][8, 0, 0] == -1 and (got['face'][8, 1] >= 0).all()
    for p in (3, 7):                                      # skipped pairs between computed ones
        assert (got['face'][p] == -1).all() and np.isinf(got['d2'][p]).all() and not got['point'][p].any()
        assert not got['cross'][p].any() and not got['n_contact'][p].any() and not got['n_inside'][p].any()
        assert (got['closest'][p] == -1).all() and np.isinf(got['min_d2'][p]).all() and not got['depth2'][p].any()
    for k in KEYS:                                        # the same pair twice in one call
        assert np.array_equal(got[k][0], got[k][9], equal_nan=True)
    # no pair
    none = ops.mesh_surface_contact(dv, f, np.zeros((0, 2), np.int32))
    assert tuple(none['face'].shape) == (0, 2, V) and tuple(none['point'].shape) == (0, 2, V, 3)
    assert tuple(none['min_d2'].shape) == (0, 2) and tuple(none['closest'].shape) == (0, 2, 2)
    # pair indices beyond the meshes: refused for a host list, skipped for a device tensor (the kernel checks every index)
    with pytest.raises(ValueError):
        ops.mesh_surface_contact(dv, f, [[0, 6]])
    wild = torch.tensor([[0, 6], [2 ** 31 - 1, 0], [0, 1], [-2 ** 31, 1]], dtype=torch.int32).cuda()
    got = host(ops.mesh_surface_contact(dv, f, wild, **kw))
    assert_equal(got, R.mesh_surface_contact(verts, f, wild.cpu().numpy(), **kw))
    assert (got['face'][[0, 1, 3]] == -1).all() and (got['face'][2, 0] >= 0).all()
    with pytest.raises(ValueError):
        ops.mesh_surface_contact(dv, f, [[0, 1]], contact_dist=float('nan'))
    with pytest.raises(ValueError):      # beyond the stated limits: refused, not clamped
        ops.mesh_surface_contact(torch.zeros(2, 4001, 3).cuda(), np.array([[0, 1, 2]]), [[0, 1]])
    with pytest.raises(ValueError):
        ops.mesh_surface_contact(dv, g.integers(0, V, (ops.SURFACE_MAX_FACES + 1, 3)), [[0, 1]])


def test_determinism_and_batch_independence():
    ops = pkg('ops')
    verts, faces, ti = scene(257, seed=9)
    dv = torch.from_numpy(verts).cuda()
    a = host(ops.mesh_surface_contact(dv, faces, PAIRS, topo_index=ti))
    b = host(ops.mesh_surface_contact(dv, faces, PAIRS, topo_index=ti))
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    for p, pair in enumerate(PAIRS):      # a pair computed alone equals the same pair computed in the batch
        one = host(ops.mesh_surface_contact(dv, faces, [pair], topo_index=ti))
        for k in KEYS:
            assert one[k][0].tobytes() == a[k][p].tobytes(), (p, k)


# ---- engine level ---------------------------------------------------------------------------------------------------------
def test_engine_surface_contact_matches_the_operator(eng, mano_tables, frames3):
    ops, L = pkg('ops'), pkg('_lib')
    for B in (2, 3):
        out = eng.forward(frames3[:B], project=True)
        own = ops.cam_trans(out['joints'].view(-1, 21, 3), out['pj2d'].view(-1, 21, 2), focal_length=1265.0).view(B, 2, 3)
        got = host(eng.contact(out, mode='surface'))      # the network's own camera, computed by the call
        want, pairs = by_operator(ops, L, out, 1, own, mano_tables)
        assert_equal(got, want, (B, 'own'))
        ct = placed(B)[:, 0]
        got = host(eng.contact(out, cam_trans=ct, contact_dist=0.01, max_depth=float('inf'), mode='surface'))
        want, pairs = by_operator(ops, L, out, 1, ct, mano_tables, contact_dist=0.01, max_depth=float('inf'))
        assert_equal(got, want, (B, 'placed'))
        assert (pairs[:2] >= 0).all() and got['n_contact'].sum() > 0      # (both hands are detected in the first two frames)
    # the default mode is byte for byte what it was, before and after a surface call on the same context
    before = host(eng.contact(out, cam_trans=ct), OLD_KEYS)
    eng.contact(out, cam_trans=ct, mode='surface')
    after = eng.contact(out, cam_trans=ct, mode='vertex')
    assert set(after) == set(OLD_KEYS)
    n = out['slots'].shape[0]
    flags = out['slots'].reshape(n, 2, L.SLOT)[:, :, L.SLOT_FLAG].cpu().numpy()
    old = host(ops.mesh_contact(out['verts'].reshape(2 * n, 778, 3), (mano_tables['left']['faces'], mano_tables['right']['faces']),
                                contact_ref.frame_pairs(flags, 1), trans=ct.reshape(2 * n, 3), topo_index=[0, 1] * n,
                                sign=list(eng.contact_sign) * n), OLD_KEYS)
    for k in OLD_KEYS:
        assert before[k].tobytes() == after[k].cpu().numpy().tobytes() == old[k].tobytes(), k
    # an undetected side, and flags of arbitrary bytes: the skipped-pair row, decided on the device
    out = {k: v.clone() for k, v in out.items()}
    bits = torch.tensor([0x7fc00000, 0x3f000000, 0x7f800000, 0xff800000 - 2 ** 32, 0x3f000001, 0x00000001], dtype=torch.int32)
    out['slots'][:, :, L.SLOT_FLAG] = bits.view(torch.float32).view(3, 2).cuda()      # NaN 0.5 | inf -inf | 0.5+ denormal
    got = host(eng.contact(out, cam_trans=ct, mode='surface'))
    want, pairs = by_operator(ops, L, out, 1, ct, mano_tables)
    assert pairs.tolist() == [[-1, -1]] * 3               # NaN, exactly one half, -inf and a denormal are not flags
    assert_equal(got, want)
    assert (got['face'] == -1).all() and np.isinf(got['d2']).all() and not got['cross'].any() and not got['n_inside'].any()
    out['slots'][1, :, L.SLOT_FLAG] = torch.tensor([float('inf'), 1e30]).cuda()
    got = host(eng.contact(out, cam_trans=ct, mode='surface'))
    want, pairs = by_operator(ops, L, out, 1, ct, mano_tables)
    assert pairs.tolist() == [[-1, -1], [2, 3], [-1, -1]] and (got['face'][1] >= 0).all()
    assert_equal(got, want)
    with pytest.raises(ValueError):
        eng.contact(out, mode='faces')


def test_engine_surface_contact_max_hand_2(eng, mano_tables, frames3):
    ops, L = pkg('ops'), pkg('_lib')
    B, K = 2, 2
    out = eng.forward(frames3[:B], project=True, max_hand=K)
    ct = placed(B, K)
    out['slots'][:, :, :, L.SLOT_FLAG] = 1.0              # every rank a hand: all K * K pairs of every row, rows never mixed
    out['slots'][1, 1, 0, L.SLOT_FLAG] = 0.0              # ... but one: two skipped pairs between computed ones
    got = host(eng.contact(out, max_hand=K, cam_trans=ct, mode='surface'))
    want, pairs = by_operator(ops, L, out, K, ct, mano_tables)
    assert got['face'].shape == (B * K * K, 2, 778) and got['point'].shape == (B * K * K, 2, 778, 3)
    assert (pairs[:6] >= 0).all() and (pairs[6:] == -1).all() and (pairs[:6, 0] // (2 * K) == pairs[:6, 1] // (2 * K)).all()
    assert_equal(got, want)
    with pytest.raises(ValueError):
        eng.contact(out, max_hand=1, mode='surface')


def test_three_calls_queue_without_a_host_visit(eng, frames3):
    out = eng.forward(frames3[:2], project=True)
    ct = placed(2)[:, 0]
    want = host(eng.contact(out, cam_trans=ct, mode='surface'))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        res = [eng.contact(out, cam_trans=ct, mode='surface'), eng.contact(out, mode='surface'),
               eng.contact(out, cam_trans=ct, mode='surface')]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for k in KEYS:
        assert np.array_equal(res[0][k].cpu().numpy(), want[k], equal_nan=True) and torch.equal(res[0][k], res[2][k]), k


def test_pool_surface_contact_on_the_tickets_stream(eng, near_sd, mano_tables, frames3):
    img = frames3[:2]
    out = eng.forward(img, project=True)
    ct = placed(2)[:, 0]
    want = [host(eng.contact(out, mode='surface')), host(eng.contact(out, cam_trans=ct, mode='surface'))]
    pool = pkg('engine').EnginePool(0, n=2)
    pool.load_state_dict(near_sd, max_batch=2)
    pool.load_mano(mano_tables)
    for k in range(4):      # both contexts, twice; the network's camera and the placed one
        t = pool.submit(img, project=True)
        got = pool.contact(t, cam_trans=ct if k % 2 else None, mode='surface')
        pool.collect(t)
        assert_equal(host(got), want[k % 2], k)
    pool.close()


def test_forward_batch_surface_contact_keys(near_sd, mano_tables, frames3):
    ops, L, cfg = pkg('ops'), pkg('_lib'), pkg('config')
    acr = pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml']), state_dict=near_sd,
                              mano_tables=mano_tables, max_batch=2)
    img = frames3[:2]
    plain = acr.forward_batch(img, ['a', 'b'])
    res = acr.forward_batch(img, ['a', 'b'], contact='surface')
    new = {'contact_dist', 'contact_with', 'contact_verts', 'penetration'}
    for k in plain:                                       # the same four keys, and everything else as without them
        assert len(res[k]) == len(plain[k]) == 2
        for h0, h1 in zip(plain[k], res[k]):
            assert set(h1) == set(h0) | new and not new & set(h0)
            assert all(np.array_equal(h0[f], h1[f]) for f in h0)
    # against the operator on what the fused call returned
    e = acr.model.engine(2)
    e.set_point_heads(True)      # (as forward_batch runs it: the towers at the decoded centres)
    try:
        out = e.forward(img, offsets=torch.tensor([[512., 512, 0, 0, 0, 0, 0, 0, 0, 0]]).repeat(2, 1), project=True)
    finally:
        e.set_point_heads(False)
    ct = ops.cam_trans(out['joints'].view(-1, 21, 3), out['pj2d'].view(-1, 21, 2), focal_length=acr.focal_length).view(2, 2, 3)
    want, pairs = by_operator(ops, L, out, 1, ct, mano_tables)
    r2 = np.float32(ops.CONTACT_DIST) * np.float32(ops.CONTACT_DIST)
    for b, k in enumerate('ab'):
        for h, hand in enumerate(res[k]):
            assert int(hand['hand_type']) == h and int(hand['contact_with']) == 1 - h
            assert hand['contact_dist'] == np.sqrt(want['min_d2'][b].min(), dtype=np.float32)
            assert hand['penetration'] == np.sqrt(want['depth2'][b, h], dtype=np.float32)
            assert hand['contact_verts'].tolist() == np.nonzero((want['face'][b, h] >= 0) & (want['d2'][b, h] <= r2))[0].tolist()
    raw = acr.forward_raw_batch(torch.from_numpy(np.ascontiguousarray(img.cpu().numpy()[..., ::-1])).cuda(), ['a', 'b'],
                                contact='surface')
    assert all(new <= set(h) for k in raw for h in raw[k])
    for bad in (1, 'vertex', 'Surface'):
        with pytest.raises(ValueError):
            acr.forward_batch(img, ['a', 'b'], contact=bad)
