"""The contact / interpenetration measure on the GPU (csrc/contact.hip) against the numpy restatement
(tests/contact_ref.py) FOR EQUALITY: nn, the bits of d2 and side, and both summaries.  There is no tolerance anywhere in this
file; the one thing not compared is the payload of a NaN (contact_ref.same_bits).  Then the engine level: Engine.contact,
EnginePool.contact and forward_batch(contact=True) against the stand-alone operator on the same tensors."""
from functools import partial

import numpy as np
import pytest
import torch

import contact_cases as C
import contact_ref as R
from conftest import pkg
from contact_cases import LATLON, PAIRS, eng, frames3, near_sd, placed, scene      # (eng, frames3, near_sd: fixtures)

pytestmark = pytest.mark.gpu

KEYS = C.KEYS['vertex']
host = partial(C.host, keys=KEYS)
assert_equal = partial(C.assert_equal, 'vertex')
by_operator = partial(C.by_operator, 'vertex')


@pytest.mark.parametrize('V', sorted(LATLON))
def test_matches_the_restatement(V):
    ops = pkg('ops')
    verts, faces, ti = scene(V)
    g = np.random.default_rng(V)
    trans = g.uniform(-0.01, 0.01, (5, 3)).astype(np.float32)
    sign = [1, 1, 1, -1, 1]
    dv = torch.from_numpy(verts).cuda()
    for tr in (None, trans):
        for r, m in ((0.005, 0.02), (0.0, float('inf'))):
            got = host(ops.mesh_contact(dv, faces, PAIRS, trans=None if tr is None else torch.from_numpy(tr), topo_index=ti,
                                        sign=sign, contact_dist=r, max_depth=m))
            want = R.mesh_contact(verts, faces, PAIRS, trans=tr, topo_index=ti, sign=sign, contact_dist=r, max_depth=m)
            assert_equal(got, want, (V, tr is not None, r, m))
    if V >= 257:      # the cases are not trivial: the overlapping spheres overlap, the ones 0.12 apart do not touch
        clean = R.mesh_contact(verts, faces, PAIRS[:2], topo_index=ti)
        assert clean['n_inside'][0].min() > 0 and clean['n_inside'][1].sum() == 0 and clean['n_contact'][1].sum() == 0
    # one topology, no topo_index, no sign; a topology blob on the device instead of faces
    blob = torch.from_numpy(ops.mesh_topology(faces[0], V)).cuda()
    got = host(ops.mesh_contact(dv[:3], blob, torch.tensor([[0, 1], [1, 2]], dtype=torch.int32).cuda()))
    assert_equal(got, R.mesh_contact(verts[:3], faces[0], [[0, 1], [1, 2]]), (V, 'blob'))


def test_synthetic_mano_hands(mano_tables):
    """The 778-vertex templates of the synthetic tables over their faces (random triples): two topologies chosen per mesh."""
    ops = pkg('ops')
    g = np.random.default_rng(3)
    tl, tr = (np.asarray(mano_tables[s]['v_template'], np.float32).reshape(778, 3) for s in ('left', 'right'))
    verts = np.stack([tl, tr, tl + g.normal(0, 0.002, tl.shape).astype(np.float32), tr * np.float32(1.05)])
    trans = np.array([[0, 0, 0.8], [0.03, 0.01, 0.81], [0.2, 0, 0.9], [0.21, 0.01, 0.9]], np.float32)
    faces = (mano_tables['left']['faces'], mano_tables['right']['faces'])
    sign = [ops.mesh_orientation(tl, faces[0]), ops.mesh_orientation(tr, faces[1])] * 2
    pairs = [[0, 1], [2, 3], [0, 3]]
    got = host(ops.mesh_contact(torch.from_numpy(verts).cuda(), faces, pairs, trans=torch.from_numpy(trans).cuda(),
                                topo_index=[0, 1, 0, 1], sign=sign))
    want = R.mesh_contact(verts, faces, pairs, trans=trans, topo_index=[0, 1, 0, 1], sign=sign)
    assert_equal(got, want)
    assert want['n_contact'][:2].sum() > 0


def test_edge_cases():
    ops, L = pkg('ops'), pkg('_lib')
    V = 70
    g = np.random.default_rng(5)
    f = g.integers(0, V - 1, (90, 3))                     # vertex V - 1 is referenced by no face
    verts = g.uniform(-0.05, 0.05, (6, V, 3)).astype(np.float32)
    verts[1, 10] = verts[1, 3]                            # duplicated vertices: the lowest j
    verts[1, 40] = verts[1, 3]
    verts[0, 7] = verts[1, 3]                             # ... and a vertex of mesh 0 sits exactly on them
    verts[2, 5, 1] = np.nan                               # a NaN vertex (and NaN normals around it)
    verts[3] = np.nan                                     # an all-NaN mesh
    verts[4, 0] = 3e19                                    # squares overflow: +inf never wins
    pairs = [[0, 1], [1, 0], [0, 0], [-1, 2], [0, 2], [2, 3], [3, 3], [1, -5], [4, 0], [0, 1]]      # mesh 0 in many pairs
    dv = torch.from_numpy(verts).cuda()
    kw = dict(contact_dist=0.0, max_depth=float('inf'))
    got = host(ops.mesh_contact(dv, f, pairs, **kw))
    want = R.mesh_contact(verts, f, pairs, **kw)
    assert_equal(got, want)
    assert got['nn'][0, 0, 7] == 3 and got['d2'][0, 0, 7] == 0 and got['n_contact'][0].tolist() == [1, 3]
    assert got['nn'][2, 0].tolist() == list(range(V)) and not got['d2'][2].any()      # a mesh with itself
    assert got['nn'][4, 1, 5] == -1 and np.isinf(got['d2'][4, 1, 5]) and got['side'][4, 1, 5] == 0 and (got['nn'][4, 0] != 5).all()
    assert (got['nn'][5, 0] == -1).all() and (got['nn'][6] == -1).all() and got['closest'][6].tolist() == [-1, -1]
    assert got['nn'][8, 0, 0] == -1 and (got['nn'][8, 1] != 0).all()
    for p in (3, 7):                                      # skipped pairs between computed ones
        assert (got['nn'][p] == -1).all() and np.isinf(got['d2'][p]).all() and not got['side'][p].any()
        assert not got['n_contact'][p].any() and not got['n_inside'][p].any() and got['closest'][p].tolist() == [-1, -1]
    for k in KEYS:                                        # the same pair twice in one call
        assert np.array_equal(got[k][0], got[k][9], equal_nan=True)
    assert not got['side'][0, 1][got['nn'][0, 1] == V - 1].any()      # the unreferenced vertex has N = 0
    # sign = -1: side is negated bit for bit, everything but the inside figures stays
    neg = host(ops.mesh_contact(dv, f, pairs, sign=[-1] * 6, **kw))
    assert_equal(neg, R.mesh_contact(verts, f, pairs, sign=[-1] * 6, **kw))
    # (a sum of zeros of both signs is +0 under either sign, so a zero may stay as it is; everything else flips its sign bit)
    nz = ~np.isnan(got['side']) & (got['side'] != 0)
    assert nz.sum() > 400 and not neg['side'][~np.isnan(got['side']) & ~nz].any()
    assert np.array_equal(neg['side'].view(np.uint32)[nz] ^ np.uint32(0x80000000), got['side'].view(np.uint32)[nz])
    assert np.array_equal(neg['nn'], got['nn']) and R.same_bits(neg['d2'], got['d2']) and np.array_equal(neg['n_contact'], got['n_contact'])
    # no pair
    none = ops.mesh_contact(dv, f, np.zeros((0, 2), np.int32))
    assert tuple(none['nn'].shape) == (0, 2, V) and tuple(none['min_d2'].shape) == (0,)
    # pair indices beyond the meshes: refused for a host list, skipped for a device tensor (the kernel checks every index)
    with pytest.raises(ValueError):
        ops.mesh_contact(dv, f, [[0, 6]])
    wild = torch.tensor([[0, 6], [2 ** 31 - 1, 0], [0, 1], [-2 ** 31, 1]], dtype=torch.int32).cuda()
    got = host(ops.mesh_contact(dv, f, wild, **kw))
    assert_equal(got, R.mesh_contact(verts, f, wild.cpu().numpy(), **kw))
    assert (got['nn'][[0, 1, 3]] == -1).all() and (got['nn'][2, 0] >= 0).all()
    with pytest.raises(ValueError):
        ops.mesh_contact(dv, f, [[0, 1]], contact_dist=float('nan'))
    with pytest.raises(ValueError):
        ops.mesh_contact(torch.zeros(2, 4001, 3).cuda(), np.array([[0, 1, 2]]), [[0, 1]])      # beyond the stated limit


def test_determinism_and_batch_independence():
    ops = pkg('ops')
    verts, faces, ti = scene(257, seed=9)
    dv = torch.from_numpy(verts).cuda()
    sign = [1, -1, 1, 1, -1]
    a = host(ops.mesh_contact(dv, faces, PAIRS, topo_index=ti, sign=sign))
    b = host(ops.mesh_contact(dv, faces, PAIRS, topo_index=ti, sign=sign))
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    for p, pair in enumerate(PAIRS):      # a pair computed alone equals the same pair computed in the batch
        one = host(ops.mesh_contact(dv, faces, [pair], topo_index=ti, sign=sign))
        for k in KEYS:
            assert one[k][0].tobytes() == a[k][p].tobytes(), (p, k)


# ---- engine level ---------------------------------------------------------------------------------------------------------
def test_scratch_growth_and_the_two_modes_side_by_side(eng, mano_tables, frames3):
    """The context's two scratch buffers, from the module engine's first calls on: the modes in the order vertex, surface,
    vertex, surface at B = 1 (both allocate), B = 3 (both grow) and B = 1 again (both are reused, not shrunk), then once each
    at max_hand = 2 (another carve-up of the same buffers), all on the current stream.  Every result equals the stateless
    operator's on the same tensors - no tolerance: neither mode disturbs the other, and a regrown buffer serves as a first."""
    ops, L = pkg('ops'), pkg('_lib')
    for B, K in ((1, 1), (3, 1), (1, 1), (1, 2)):
        out = eng.forward(frames3[:B], project=True, **({} if K == 1 else {'max_hand': K}))
        ct = placed(B, K) if K > 1 else placed(B)[:, 0]
        for mode in ('vertex', 'surface') * (2 if K == 1 else 1):
            got = C.host(eng.contact(out, max_hand=K, cam_trans=ct, mode=mode), C.KEYS[mode])
            want, _ = C.by_operator(mode, ops, L, eng, out, K, ct, mano_tables)
            C.assert_equal(mode, got, want, (B, K, mode))


def test_engine_contact_matches_the_operator(eng, mano_tables, frames3):
    ops, L = pkg('ops'), pkg('_lib')
    for B in (2, 3):
        out = eng.forward(frames3[:B], project=True)
        own = ops.cam_trans(out['joints'].view(-1, 21, 3), out['pj2d'].view(-1, 21, 2), focal_length=1265.0).view(B, 2, 3)
        got = host(eng.contact(out))                      # the network's own camera, computed by the call
        want, pairs = by_operator(ops, L, eng, out, 1, own, mano_tables)
        assert_equal(got, want, (B, 'own'))
        ct = placed(B)[:, 0]
        got = host(eng.contact(out, cam_trans=ct, contact_dist=0.01, max_depth=float('inf')))
        want, pairs = by_operator(ops, L, eng, out, 1, ct, mano_tables, contact_dist=0.01, max_depth=float('inf'))
        assert_equal(got, want, (B, 'placed'))
        assert (pairs[:2] >= 0).all() and got['n_contact'].sum() > 0      # (both hands are detected in the first two frames)
    # an undetected side, and flags of arbitrary bytes: the skipped-pair row, decided on the device
    out = {k: v.clone() for k, v in out.items()}
    bits = torch.tensor([0x7fc00000, 0x3f000000, 0x7f800000, 0xff800000 - 2 ** 32, 0x3f000001, 0x00000001], dtype=torch.int32)
    out['slots'][:, :, L.SLOT_FLAG] = bits.view(torch.float32).view(3, 2).cuda()      # NaN 0.5 | inf -inf | 0.5+ denormal
    got = host(eng.contact(out, cam_trans=ct))
    want, pairs = by_operator(ops, L, eng, out, 1, ct, mano_tables)
    assert pairs.tolist() == [[-1, -1]] * 3               # NaN, exactly one half, -inf and a denormal are not flags
    assert_equal(got, want)
    assert (got['nn'] == -1).all() and np.isinf(got['d2']).all() and not got['side'].any() and not got['n_inside'].any()
    out['slots'][1, :, L.SLOT_FLAG] = torch.tensor([float('inf'), 1e30]).cuda()
    got = host(eng.contact(out, cam_trans=ct))
    want, pairs = by_operator(ops, L, eng, out, 1, ct, mano_tables)
    assert pairs.tolist() == [[-1, -1], [2, 3], [-1, -1]] and (got['nn'][1] >= 0).all()
    assert_equal(got, want)
    # the sign override reaches the kernel
    eng.set_contact_sign(-eng.contact_sign[0], eng.contact_sign[1])
    try:
        flipped = host(eng.contact(out, cam_trans=ct))
        want, _ = by_operator(ops, L, eng, out, 1, ct, mano_tables)
    finally:
        eng.set_contact_sign(None, None)
    assert_equal(flipped, want)
    assert not np.array_equal(flipped['side'][1, 1], got['side'][1, 1]) and R.same_bits(flipped['side'][1, 0], got['side'][1, 0])


def test_engine_contact_max_hand_2(eng, mano_tables, frames3):
    ops, L = pkg('ops'), pkg('_lib')
    B, K = 2, 2
    out = eng.forward(frames3[:B], project=True, max_hand=K)
    ct = placed(B, K)
    got = host(eng.contact(out, max_hand=K, cam_trans=ct))
    want, pairs = by_operator(ops, L, eng, out, K, ct, mano_tables)
    assert got['nn'].shape == (B * K * K, 2, 778)
    assert_equal(got, want)
    out['slots'][:, :, :, L.SLOT_FLAG] = 1.0              # every rank a hand: all K * K pairs of every row, rows never mixed
    got = host(eng.contact(out, max_hand=K, cam_trans=ct))
    want, pairs = by_operator(ops, L, eng, out, K, ct, mano_tables)
    assert (pairs >= 0).all() and sorted(set((pairs // (2 * K)).reshape(-1).tolist())) == [0, 1]
    assert (pairs[:, 0] // (2 * K) == pairs[:, 1] // (2 * K)).all()
    assert_equal(got, want)
    with pytest.raises(ValueError):
        eng.contact(out, max_hand=1)


def test_contact_before_faces_is_a_state_error(near_sd, mano_tables, frames3):
    L = pkg('_lib')
    e = pkg('engine').Engine(0)
    e.load_state_dict(near_sd, max_batch=2)
    e.load_mano({s: {k: v for k, v in mano_tables[s].items() if k != 'faces'} for s in ('left', 'right')})
    out = e.forward(frames3[:2], project=True)
    with pytest.raises(L.AcrmiError, match='faces'):
        e.contact(out)
    e.close()


def test_three_calls_queue_without_a_host_visit(eng, frames3):
    out = eng.forward(frames3[:2], project=True)
    ct = placed(2)[:, 0]
    want = host(eng.contact(out, cam_trans=ct))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        res = [eng.contact(out, cam_trans=ct), eng.contact(out), eng.contact(out, cam_trans=ct)]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for k in KEYS:
        assert np.array_equal(res[0][k].cpu().numpy(), want[k], equal_nan=True) and torch.equal(res[0][k], res[2][k]), k


def test_pool_contact_on_the_tickets_stream(eng, near_sd, mano_tables, frames3):
    img = frames3[:2]
    out = eng.forward(img, project=True)
    ct = placed(2)[:, 0]
    want = [host(eng.contact(out)), host(eng.contact(out, cam_trans=ct))]
    pool = pkg('engine').EnginePool(0, n=2)
    pool.load_state_dict(near_sd, max_batch=2)
    pool.load_mano(mano_tables)
    for k in range(4):      # both contexts, twice; the network's camera and the placed one
        t = pool.submit(img, project=True)
        got = pool.contact(t, cam_trans=ct if k % 2 else None)
        pool.collect(t)
        assert_equal(host(got), want[k % 2], k)
    with pytest.raises(RuntimeError):
        pool.contact(t)
    pool.close()


def test_forward_batch_contact_keys(near_sd, mano_tables, frames3):
    ops, L, cfg = pkg('ops'), pkg('_lib'), pkg('config')
    acr = pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml']), state_dict=near_sd,
                              mano_tables=mano_tables, max_batch=2)
    img = frames3[:2]
    plain = acr.forward_batch(img, ['a', 'b'])
    res = acr.forward_batch(img, ['a', 'b'], contact=True)
    again = acr.forward_batch(img, ['a', 'b'])
    new = {'contact_dist', 'contact_with', 'contact_verts', 'penetration'}
    for k in plain:                                       # without contact=True the dicts are what they were
        assert len(res[k]) == len(plain[k]) == len(again[k]) == 2
        for h0, h1, h2 in zip(plain[k], res[k], again[k]):
            assert set(h1) == set(h0) | new and set(h2) == set(h0) and not new & set(h0)
            assert all(np.array_equal(h0[f], h1[f]) and np.array_equal(h0[f], h2[f]) for f in h0)
    # against the operator on what the fused call returned
    e = acr.model.engine(2)
    e.set_point_heads(True)      # (as forward_batch runs it: the towers at the decoded centres)
    try:
        out = e.forward(img, offsets=torch.tensor([[512., 512, 0, 0, 0, 0, 0, 0, 0, 0]]).repeat(2, 1), project=True)
    finally:
        e.set_point_heads(False)
    ct = ops.cam_trans(out['joints'].view(-1, 21, 3), out['pj2d'].view(-1, 21, 2), focal_length=acr.focal_length).view(2, 2, 3)
    want, pairs = by_operator(ops, L, e, out, 1, ct, mano_tables)
    r2 = np.float32(ops.CONTACT_DIST) * np.float32(ops.CONTACT_DIST)
    for b, k in enumerate('ab'):
        for h, hand in enumerate(res[k]):
            assert int(hand['hand_type']) == h and int(hand['contact_with']) == 1 - h
            assert hand['contact_dist'] == np.sqrt(want['min_d2'][b], dtype=np.float32)
            assert hand['penetration'] == np.sqrt(want['depth2'][b, h], dtype=np.float32)
            assert hand['contact_verts'].tolist() == np.nonzero(want['d2'][b, h] <= r2)[0].tolist()
    raw = acr.forward_raw_batch(torch.from_numpy(np.ascontiguousarray(img.cpu().numpy()[..., ::-1])).cuda(), ['a', 'b'], contact=True)
    assert all(new <= set(h) for k in raw for h in raw[k])
    with pytest.raises(ValueError):
        acr.forward_batch(img, ['a', 'b'], contact=1)
