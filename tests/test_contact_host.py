"""Host-side checks of the contact / interpenetration measure (acrmi_contact_workspace / acrmi_mesh_contact / acrmi_contact,
ops.mesh_contact / mesh_orientation, Engine.contact): the ABI surface and the argument checks that need
no device, the orientation sign, the rule itself on two spheres through the numpy restatement alone (tests/contact_ref.py),
the packaging of the four contact keys, and the host rules' stand-alone check program.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import contact_ref as R
from conftest import ROOT, pkg
from render_ref import ellipsoid

NEW = ('acrmi_contact_workspace', 'acrmi_mesh_contact', 'acrmi_contact')


def test_new_symbols_are_declared_exported_and_bound():
    L = pkg('_lib')
    lib = L.lib()
    header = open(os.path.join(ROOT, 'include', 'acrmi.h')).read()
    for name in NEW:
        assert name + '(' in header and name in L.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.acrmi_mesh_contact.argtypes) == 20 and len(lib.acrmi_contact.argtypes) == 15
    assert lib.acrmi_contact_workspace.restype is ctypes.c_size_t
    assert lib.acrmi_version() == L.VERSION == 303      # additive: the ABI version stays
    # the rule stands in the header and in the design document
    assert 'nearest-VERTEX half-space heuristic' in header and 'NOT normalised' in header
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '## 19.' in design and 'not a point-to-triangle distance' in design


def test_workspace_size():
    lib = pkg('_lib').lib()
    for m, v in ((0, 778), (2, 0), (-1, 5), (3, -2), (0, 0)):
        assert lib.acrmi_contact_workspace(m, v) == 0
    assert lib.acrmi_contact_workspace(2, 778) == 2 * 778 * 32 and lib.acrmi_contact_workspace(128, 4000) == 128 * 4000 * 32


def test_bad_arguments_are_rejected_before_any_device_call():
    L = pkg('_lib')
    lib = L.lib()
    p = ctypes.c_void_p(256)      # never read: the checks come first
    good = dict(verts=p, trans=None, M=2, V=778, F=1538, topo=p, topo2=None, mesh_topo=None, sign=None, pairs=p, n=1, r=0.005,
                m=0.02, nn=p, d2=p, s=p, sf=p, si=p, ws=p, stream=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        rc = lib.acrmi_mesh_contact(*a.values())
        return rc, lib.acrmi_last_error(None)

    for bad in (dict(verts=None), dict(topo=None), dict(pairs=None), dict(nn=None), dict(d2=None), dict(s=None), dict(sf=None),
                dict(si=None), dict(ws=None), dict(ws=ctypes.c_void_p(264)), dict(M=0), dict(M=-1), dict(V=0), dict(V=4001),
                dict(F=0), dict(n=-1), dict(r=-0.001), dict(r=float('inf')), dict(r=float('nan')), dict(m=-1.0),
                dict(m=float('nan')), dict(n=1380200), dict(M=2760400)):
        rc, msg = call(**bad)
        assert rc == L.E_INVAL and msg.startswith(b'acrmi_mesh_contact:'), (bad, rc, msg)
    # no pair: success, nothing is touched (also on a machine without a GPU)
    assert call(n=0)[0] == 0
    assert call(n=0, verts=None, pairs=None, nn=None, ws=None)[0] == 0
    assert call(n=0, V=4001)[0] == L.E_INVAL
    if not torch.cuda.is_available():      # well-formed arguments reach the device: a loud failure, no host path
        assert call(V=4000, m=float('inf'), r=0.0)[0] == L.E_HIP
    # the context form
    args = [None, p, p, p, 2, 1, None, 0.005, 0.02, p, p, p, p, p, None]
    assert lib.acrmi_contact(*args) == L.E_INVAL and lib.acrmi_last_error(None).startswith(b'acrmi_contact:')
    # the operator refuses host tensors and malformed arguments before it looks at the device
    ops = pkg('ops')
    with pytest.raises(L.AcrmiError):
        ops.mesh_contact(torch.zeros(2, 5, 3), np.zeros((4, 3), np.int64), [[0, 1]])
    for r, m in ((-1, 0.02), (float('inf'), 0.02), (float('nan'), 0.02), (0.005, -1), (0.005, float('nan'))):
        with pytest.raises(ValueError):
            ops.check_contact_params(r, m)
    assert ops.check_contact_params(0, float('inf')) == (0.0, float('inf'))
    assert (ops.CONTACT_DIST, ops.CONTACT_MAX_DEPTH) == (0.005, 0.02)


def test_mesh_orientation():
    ops = pkg('ops')
    v, f = ellipsoid(12, 24, (0.05, 0.04, 0.03), (0.1, -0.2, 0.5))
    assert ops.mesh_orientation(v, f) == 1
    assert ops.mesh_orientation(v, f[:, ::-1]) == -1
    assert ops.mesh_orientation(torch.from_numpy(v), torch.from_numpy(f[:, [0, 2, 1]])) == -1
    flat = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    tet = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
    assert ops.mesh_orientation(flat, tet) == 1 and ops.mesh_orientation(flat, tet[:, ::-1]) == 1      # volume exactly 0
    with pytest.raises(ValueError):
        ops.mesh_orientation(flat, np.array([[0, 1, 4]]))
    with pytest.raises(ValueError):
        ops.mesh_orientation(flat[:, :2], tet)
    # the restatement's normals point outwards on an outward-wound sphere, and flip with the sign
    n = R.vertex_normals(v, f)
    c = np.array((0.1, -0.2, 0.5), np.float32)
    assert ((n * (v - c)).sum(1) > 0).all()
    assert R.same_bits(R.vertex_normals(v, f, -1), -n)


def test_engine_sign_and_contact_arguments():
    """The parts of Engine.contact that run before the context is touched (a stub stands for the context)."""
    E, ops, synth = pkg('engine'), pkg('ops'), pkg('synth')
    eng = E.Engine.__new__(E.Engine)
    eng._mano_tables, eng._faces, eng._contact_sign, eng._contact_sign_set = {}, {}, [1, 1], None
    v, f = ellipsoid(20, 38, (0.05, 0.05, 0.05), (0, 0, 0))
    assert v.shape[0] <= 778
    vt = np.zeros((778, 3), np.float32)
    vt[:v.shape[0]] = v
    eng._faces['left'], eng._faces['right'] = f.astype(np.int32), f[:, ::-1].astype(np.int32)
    eng._derive_contact_sign('left')
    assert eng.contact_sign == (1, 1)                       # no template vertices yet: +1
    eng._mano_tables['left'] = eng._mano_tables['right'] = {'v_template': vt.reshape(-1)}
    eng._derive_contact_sign('left')
    eng._derive_contact_sign('right')
    assert eng.contact_sign == (1, -1)
    eng.set_contact_sign(-1, 1)
    assert eng.contact_sign == (-1, 1)
    for bad in ((0, 1), (1, 2), (None, 1), (1.5, 1)):
        with pytest.raises(ValueError):
            eng.set_contact_sign(*bad)
    eng.set_contact_sign(None, None)
    assert eng.contact_sign == (1, -1)
    out = {'slots': torch.zeros(2, 2, 176), 'verts': torch.zeros(2, 2, 778, 3)}
    for kw in (dict(max_hand=0), dict(max_hand=9), dict(max_hand=2), dict(contact_dist=-1.0), dict(max_depth=float('nan'))):
        with pytest.raises(ValueError):
            eng.contact(out, **kw)
    with pytest.raises(ValueError):
        eng.contact({'slots': torch.zeros(2, 2, 2, 176), 'verts': torch.zeros(2, 2, 2, 778, 3)}, max_hand=1)
    eng.ctx = None      # (so that __del__ has nothing to close)


SPHERES = [(nlat, nlon, c) for nlat, nlon in ((12, 24), (20, 38)) for c in (0.12, 0.06, 0.03)]
EXPECTED_INSIDE = {(12, 24, 0.12): 0, (12, 24, 0.06): 41, (12, 24, 0.03): 80, (20, 38, 0.12): 0, (20, 38, 0.06): 107,
                   (20, 38, 0.03): 212}
EXPECTED_MIN_MM = {(20, 38, 0.12): 20.2, (20, 38, 0.06): 2.0, (20, 38, 0.03): 0.55}


def two_spheres(nlat, nlon, c, R_=0.05):
    va, f = ellipsoid(nlat, nlon, (R_, R_, R_), (0, 0, 0.5))
    vb, _ = ellipsoid(nlat, nlon, (R_, R_, R_), (c, 0.003, 0.5))
    return np.stack([va, vb]), f, (np.array((0, 0, 0.5)), np.array((c, 0.003, 0.5)))


@pytest.mark.parametrize('nlat,nlon,c', SPHERES)
def test_rule_on_two_spheres(nlat, nlon, c):
    """The heuristic against geometry, through the restatement alone: every vertex well inside the other sphere (< 0.9 R from
    its centre) is inside, none well outside (> 1.1 R) is; the band between is a condition of the heuristic and is not
    judged.  At c = 0.12 the spheres are apart: nothing is inside and the closest pair is the facing vertices."""
    Rr = 0.05
    verts, f, centres = two_spheres(nlat, nlon, c)
    got = R.mesh_contact(verts, f, [[0, 1]], max_depth=np.inf)
    violations = 0
    for k in (0, 1):
        dist = np.sqrt(((verts[k].astype(np.float64) - centres[1 - k]) ** 2).sum(1))
        inside = (got['side'][0, k] < 0) & (got['nn'][0, k] >= 0)
        violations += int((~inside[dist < 0.9 * Rr]).sum()) + int(inside[dist > 1.1 * Rr].sum())
    assert violations == 0
    assert got['n_inside'][0].tolist() == [EXPECTED_INSIDE[(nlat, nlon, c)]] * 2      # the count of each side
    assert got['n_inside'][0].tolist() == [int(((got['side'][0, k] < 0)).sum()) for k in (0, 1)]
    # the summary's closest pair is the brute-force one
    d = np.sqrt(((verts[0][:, None].astype(np.float64) - verts[1][None].astype(np.float64)) ** 2).sum(2))
    assert abs(np.sqrt(float(got['min_d2'][0])) - d.min()) < 1e-7
    i, j = got['closest'][0]
    assert abs(d[i, j] - d.min()) < 1e-7
    if (nlat, nlon, c) in EXPECTED_MIN_MM:
        assert abs(1000 * d.min() - EXPECTED_MIN_MM[(nlat, nlon, c)]) < 0.06
    if c == 0.12:
        assert got['n_inside'].sum() == 0 and got['depth2'].sum() == 0 and got['n_contact'].sum() == 0
        # the facing vertices: the ones of a with the largest x, of b with the smallest
        assert verts[0][i, 0] == verts[0][:, 0].max() and verts[1][j, 0] == verts[1][:, 0].min()
    else:
        assert (got['depth2'][0] > 0).all()
        for k in (0, 1):
            ins = got['side'][0, k] < 0
            assert got['depth2'][0, k] == got['d2'][0, k][ins].max()


def test_restatement_edge_cases():
    v = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, 5, 5]],
                  [[0, 0, 0], [0, 0, 0], [np.nan, 0, 0], [2, 0, 0], [1, 0, 0]]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])      # vertex 4 is referenced by no face
    got = R.mesh_contact(v, f, [[0, 1], [-1, 0], [0, 0], [1, 2]], contact_dist=0.0, max_depth=np.inf)
    assert got['nn'][0, 0].tolist() == [0, 4, 0, 0, 3]               # duplicates: the lowest j; the NaN vertex never wins
    assert got['nn'][0, 1].tolist() == [0, 0, -1, 1, 1] and got['d2'][0, 1, 2] == np.inf and got['side'][0, 1, 2] == 0
    assert got['n_contact'][0].tolist() == [2, 3]                    # contact_dist 0: the coincident vertices
    assert got['closest'][0].tolist() == [0, 0] and got['min_d2'][0] == 0
    for p in (1, 3):                                                 # skipped: an index < 0, an index >= M
        assert (got['nn'][p] == -1).all() and np.isinf(got['d2'][p]).all() and not got['side'][p].any()
        assert got['closest'][p].tolist() == [-1, -1] and np.isinf(got['min_d2'][p]) and not got['n_contact'][p].any()
    assert got['nn'][2, 0].tolist() == [0, 1, 2, 3, 4] and not got['d2'][2].any()      # a mesh with itself
    assert not R.vertex_normals(v[0], f)[4].any()                    # unreferenced: N = 0
    assert R.frame_pairs(np.array([[[1, 0.4], [0.6, 1]]], np.float32), 2).tolist() == [[-1, -1], [0, 3], [-1, -1], [2, 3]]


def test_contact_keys_are_packaged_into_the_hand_dicts():
    from importlib import import_module
    main = import_module(pkg().__name__ + '.acr.main')
    g = np.random.default_rng(0)
    B, K, V = 2, 2, 778
    out = {'slots': g.normal(size=(B, K, 2, 176)).astype(np.float32), 'verts': np.zeros((B, K, 2, V, 3), np.float32),
           'joints': np.zeros((B, K, 2, 21, 3), np.float32), 'pj2d': np.zeros((B, K, 2, 21, 2), np.float32),
           'pj2d_org': np.zeros((B, K, 2, 21, 2), np.float32), 'cam_trans': np.zeros((B, K, 2, 3), np.float32)}
    flags = np.array([[[1, 1], [1, 0]], [[0, 1], [0, 0]]], np.float32)      # row 0: lefts 0, 1 and right 0; row 1: right 0 alone
    out['slots'][..., 0] = flags
    plain = main.results_from_out(out, ['a', 'b'])
    keys = set(plain['a'][0])
    pairs = R.frame_pairs(flags, K)
    n = B * K * K
    con = {'nn': np.full((n, 2, V), -1, np.int32), 'd2': np.full((n, 2, V), np.inf, np.float32), 'side': np.zeros((n, 2, V), np.float32),
           'min_d2': np.full(n, np.inf, np.float32), 'closest': np.full((n, 2), -1, np.int32), 'n_contact': np.zeros((n, 2), np.int32),
           'n_inside': np.zeros((n, 2), np.int32), 'depth2': np.zeros((n, 2), np.float32), 'contact_dist': 0.005, 'max_depth': 0.02}
    assert pairs[:, 0].tolist() == [0, -1, 2, -1, -1, -1, -1, -1]
    # pair 0 = (left 0, right 0) at 3 mm, pair 2 = (left 1, right 0) at 1 mm with two touching vertices and a 4 mm depth
    for p, d, touch in ((0, 0.003, [5]), (2, 0.001, [7, 9])):
        con['nn'][p], con['d2'][p] = 0, np.float32(1.0)
        con['d2'][p, :, touch] = np.float32(d) ** 2
        con['min_d2'][p] = np.float32(d) ** 2
    con['depth2'][2] = (np.float32(0.004) ** 2, np.float32(0.002) ** 2)
    out['contact'] = con
    res = main.results_from_out(out, ['a', 'b'])
    a = res['a']
    assert [(int(h['hand_type'])) for h in a] == [0, 0, 1]
    assert all(set(h) == keys | {'contact_dist', 'contact_with', 'contact_verts', 'penetration'} for h in a + res['b'])
    assert [int(h['contact_with']) for h in a] == [2, 2, 1]          # the right hand's partner is the nearer left hand
    assert np.allclose([h['contact_dist'] for h in a], [0.003, 0.001, 0.001], rtol=1e-6)
    assert [h['contact_verts'].tolist() for h in a] == [[5], [7, 9], [7, 9]]
    assert np.allclose([h['penetration'] for h in a], [0, 0.004, 0.002], rtol=1e-6)
    assert a[0]['contact_verts'].dtype == np.int32 and a[0]['contact_dist'].dtype == np.float32
    lone = res['b'][0]
    assert np.isinf(lone['contact_dist']) and lone['contact_with'] == -1 and lone['contact_verts'].size == 0 and lone['penetration'] == 0
    del out['contact']                                               # without contact=True nothing is added
    assert all(set(h) == keys for h in main.results_from_out(out, ['a', 'b'])['a'])


def test_host_rules_stand_alone_program(tmp_path):
    """tools/contact_check.cpp: csrc/contact_plan.h against a plain restatement as a program of its own.  The plain build must
    pass; the build with the address and undefined-behaviour sanitizers must pass as well where the host compiler can make
    one that starts - which of the two ran is printed."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        assert os.path.exists(hipcc), 'no C++ compiler'
        cmd = [hipcc, '-x', 'c++']
    else:
        cmd = [cxx]
    src = os.path.join(ROOT, 'tools', 'contact_check.cpp')
    cmd += ['-std=c++17', '-O1', '-g', src, '-o']
    plain = str(tmp_path / 'contact_check')
    subprocess.run(cmd + [plain], check=True, capture_output=True)
    run = subprocess.run([plain], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    ran = None
    for label, extra in (('static', san + ['-static-libasan', '-static-libubsan']), ('shared', san)):
        exe = str(tmp_path / ('contact_check_' + label))
        if subprocess.run(cmd + [exe] + extra, capture_output=True).returncode != 0:
            continue
        run = subprocess.run([exe], capture_output=True, text=True)
        if 'does not come first in initial library list' in run.stderr:
            continue
        ran = label
        assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
        break
    print('sanitizer variant that ran: %s' % ran)
