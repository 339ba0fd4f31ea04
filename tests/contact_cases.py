"""What the GPU tests of the two contact measures share (tests/test_gpu_contact.py: 'vertex', tests/test_gpu_surface_contact.py:
'surface'): the scene, the comparison FOR EQUALITY - there is no tolerance here; the one thing not compared is the payload of a
NaN (contact_ref.same_bits) -, the engine fixtures, and the stand-alone operator fed what Engine.contact reads."""
import numpy as np
import pytest
import torch

import contact_ref
from conftest import pkg
from render_ref import ellipsoid

KEYS = {'vertex': ('nn', 'd2', 'side', 'min_d2', 'closest', 'n_contact', 'n_inside', 'depth2'),
        'surface': ('face', 'd2', 'point', 'cross', 'min_d2', 'closest', 'n_contact', 'n_inside', 'depth2')}
INT_KEYS = ('nn', 'face', 'cross', 'closest', 'n_contact', 'n_inside')
# lat-long spheres with exactly V = 2 + (nlat - 1) * nlon vertices: 5 (less than a wave), 64 (a wave), 257 (two chunks of 128
# and one vertex), 778 (MANO's count: six chunks and ten vertices; 194 groups of four and two vertices in LDS; 1552 faces: six
# tiles of 256 and sixteen faces)
LATLON = {5: (2, 3), 64: (3, 31), 257: (16, 17), 778: (9, 97)}
PAIRS = [[0, 1], [0, 2], [3, 4], [0, 3], [4, 1], [2, 2]]


def host(res, keys):
    return {k: res[k].cpu().numpy() for k in keys}


def assert_equal(mode, got, want, what=''):
    for k in KEYS[mode]:
        if k in INT_KEYS:
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:4])
        else:
            assert contact_ref.same_bits(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:4])


def scene(V, seed=0):
    """Five meshes of V vertices: the two-sphere geometry of the issue (R = 0.05, centres (0, 0, 0.5) and (c, 0.003, 0.5) with
    c = 0.06 and 0.12) and two clouds of random vertices over random faces -> (verts [5,V,3], (sphere faces, random faces),
    topo_index)."""
    nlat, nlon = LATLON[V]
    g = np.random.default_rng(seed + V)
    a, f = ellipsoid(nlat, nlon, (0.05,) * 3, (0, 0, 0.5))
    b, _ = ellipsoid(nlat, nlon, (0.05,) * 3, (0.06, 0.003, 0.5))
    c, _ = ellipsoid(nlat, nlon, (0.05,) * 3, (0.12, 0.003, 0.5))
    assert a.shape[0] == V
    rnd = (g.uniform(-0.07, 0.07, (2, V, 3)) + np.array((0.02, 0, 0.5))).astype(np.float32)
    rf = g.integers(0, V, (len(f), 3))
    return np.stack([a, b, c, rnd[0], rnd[1]]), (f, rf), [0, 0, 0, 1, 1]


# ---- engine level (fixtures: import them by name) ----------------------------------------------------------------------
@pytest.fixture(scope='module')
def near_sd():
    return pkg('synth').make_state_dict(seed=10)      # (the checkpoint of tests/test_gpu_render.py: both hands are detected)


@pytest.fixture(scope='module')
def eng(near_sd, mano_tables):
    e = pkg('engine').Engine(0)
    e.load_state_dict(near_sd, max_batch=3)
    e.load_mano(mano_tables)
    yield e
    e.close()


@pytest.fixture(scope='module')
def frames3():
    return torch.from_numpy(pkg('synth').make_frames(3, seed=0)).cuda()


def placed(B, K=1):
    """cam_trans [B,K,2,3] that puts the hands of a row a few centimetres from each other, about 0.8 m from the camera."""
    g = np.random.default_rng(B * 10 + K)
    t = np.array((0, 0, 0.8), np.float32) + g.uniform(-0.03, 0.03, (B, K, 2, 3)).astype(np.float32)
    return torch.from_numpy(t).cuda()


def by_operator(mode, ops, L, eng, out, K, cam_trans, mano_tables, **kw):
    """ops.mesh_contact / ops.mesh_surface_contact fed what Engine.contact reads, with the pairs built from the flags on the
    host (the vertex measure with the engine's orientation signs)."""
    n = out['slots'].shape[0] * K
    flags = out['slots'].reshape(n, 2, L.SLOT)[:, :, L.SLOT_FLAG].cpu().numpy()
    pairs = contact_ref.frame_pairs(flags, K)
    if mode == 'vertex':
        kw['sign'] = list(eng.contact_sign) * n
    op = ops.mesh_contact if mode == 'vertex' else ops.mesh_surface_contact
    res = op(out['verts'].reshape(2 * n, 778, 3), (mano_tables['left']['faces'], mano_tables['right']['faces']), pairs,
             trans=cam_trans.reshape(2 * n, 3), topo_index=[0, 1] * n, **kw)
    return host(res, KEYS[mode]), pairs
