"""CPU-side checks of the mesh overlay's boundary: the host-only topology call, argument checks of the new C entry
points without a GPU, the renderer flag, and the no-fallback rule."""
import argparse
import copy
import ctypes

import numpy as np
import pytest
import torch

import render_ref as R
from conftest import pkg


def _topology(faces, n_verts):
    L = pkg('_lib')
    f = np.ascontiguousarray(np.asarray(faces, np.int32))
    n = L.lib().acrmi_mesh_topology(None, len(f), n_verts, None, 0)
    assert n == 2 + 3 * len(f) + n_verts + 1 + 3 * len(f)
    blob = np.full(n + 3, -7, np.int32)
    assert L.lib().acrmi_mesh_topology(f.ctypes.data_as(ctypes.c_void_p), len(f), n_verts, blob.ctypes.data_as(ctypes.c_void_p), n) == n
    assert (blob[n:] == -7).all(), 'wrote past the size it reported'
    return blob[:n]


def _check_blob(blob, faces, n_verts):
    F = len(faces)
    assert blob[0] == F and blob[1] == n_verts
    assert (blob[2:2 + 3 * F].reshape(F, 3) == faces).all()
    row, col = R.csr(faces, n_verts)
    assert (blob[2 + 3 * F:2 + 3 * F + n_verts + 1] == row).all()
    assert (blob[2 + 3 * F + n_verts + 1:] == col).all()
    return row, col


def test_mesh_topology_matches_numpy_csr(mano_tables):
    for side in ('left', 'right'):
        faces = mano_tables[side]['faces']
        blob = _topology(faces, 778)
        _check_blob(blob, faces, 778)
        assert (pkg('ops').mesh_topology(faces, 778) == blob).all()
        assert (pkg('ops').mesh_topology(torch.from_numpy(faces), 778) == blob).all()


def test_mesh_topology_unreferenced_vertex():
    faces = np.array([[0, 1, 2], [2, 1, 4], [4, 4, 0]], np.int64)      # vertex 3 is in no face; vertex 4 twice in one
    row, col = _check_blob(_topology(faces, 6), faces, 6)
    assert row.tolist() == [0, 2, 4, 6, 6, 9, 9] and col.tolist() == [0, 2, 0, 1, 0, 1, 1, 2, 2]


def test_bad_arguments_are_rejected_without_a_gpu():
    L = pkg('_lib')
    lib = L.lib()
    f = np.array([[0, 1, 2]], np.int32)
    fp = f.ctypes.data_as(ctypes.c_void_p)
    buf = np.zeros(64, np.int32)
    bp = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.acrmi_mesh_topology(None, -1, 3, None, 0) == L.E_INVAL
    assert lib.acrmi_mesh_topology(None, 1, 0, None, 0) == L.E_INVAL
    assert lib.acrmi_mesh_topology(None, 1, 3, bp, 64) == L.E_INVAL            # a blob to fill but no faces
    assert lib.acrmi_mesh_topology(fp, 1, 3, bp, 5) == L.E_INVAL               # blob too small
    assert lib.acrmi_mesh_topology(fp, 1, 2, bp, 64) == L.E_INVAL              # index 2 of a 2-vertex mesh
    assert b'acrmi_mesh_topology' in lib.acrmi_last_error(None)
    assert lib.acrmi_render_workspace(0, 10) == 0 and lib.acrmi_render_workspace(2, -1) == 0
    assert lib.acrmi_render_workspace(2, 1538) >= 2 * 1538 * 8
    assert lib.acrmi_rasterize(None, None, 1, 3, 1, None, None, None, None, None, None, 1265.0, 0.9, None, None, 1, 16, 16,
                               None, None, None) == L.E_INVAL
    one = ctypes.c_void_p(256)      # never dereferenced: the size checks come first
    assert lib.acrmi_rasterize(one, None, 0, 3, 1, one, None, None, one, one, None, 1265.0, 0.9, one, one, 1, 16, 16,
                               None, one, None) == L.E_INVAL
    assert lib.acrmi_rasterize(one, None, 1, 3, 1, one, None, None, one, one, None, -1.0, 0.9, one, one, 1, 16, 16,
                               None, one, None) == L.E_INVAL
    assert lib.acrmi_render(None, None, None, None, 1, None, None, 1265.0, 0.9, None, None, 512, 512, None, None) == L.E_INVAL
    assert lib.acrmi_load_faces(None, 0, None, 0) == L.E_INVAL


def test_renderer_flag():
    config = pkg('config')
    for r in ('hip', 'none', 'pyrender', 'pytorch3d'):
        ns = argparse.Namespace(**copy.deepcopy(config.DEFAULTS))
        ns.renderer = r
        assert config.validate(ns).renderer == r
        assert config.parse_args(['--renderer', r, '--configs_yml', '/nonexistent.yml']).renderer == r
    ns = argparse.Namespace(**copy.deepcopy(config.DEFAULTS))
    ns.renderer, ns.render_size = 'hip', 2048      # read and ignored: drawing happens at the frame's resolution
    config.validate(ns)
    ns.renderer = 'opengl'
    with pytest.raises(ValueError):
        config.validate(ns)


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_render_has_no_cpu_fallback(mano_tables):
    L = pkg('_lib')
    with pytest.raises(L.AcrmiError):
        pkg('ops').render_meshes(torch.zeros(1, 778, 3), mano_tables['left']['faces'], torch.zeros(1, 64, 64, 3, dtype=torch.uint8))


def test_restatement_is_self_consistent():
    """The yardstick's own invariants: two triangles that share an edge cover every pixel of their quad exactly once, and
    the drawn image is untouched where nothing is covered."""
    v = np.array([[[-0.02, -0.03, 0.9], [0.03, -0.02, 0.9], [0.025, 0.035, 0.9], [-0.03, 0.02, 0.9]]], np.float32)
    img = np.random.default_rng(0).integers(0, 256, (1, 512, 512, 3)).astype(np.uint8)
    a = R.render(v, np.array([[0, 1, 2], [0, 2, 3]]), img)
    b = R.render(v, np.array([[0, 1, 2]]), img)
    c = R.render(v, np.array([[2, 0, 3]]), img)      # the other half, other winding
    ca, cb, cc = a['ids'] >= 0, b['ids'] >= 0, c['ids'] >= 0
    assert cb.sum() > 1000 and cc.sum() > 1000
    assert not (cb & cc).any() and ((cb | cc) == ca).all()
    assert (a['out'][~ca] == img[~ca]).all() and (a['out'][ca] != img[ca]).any()
