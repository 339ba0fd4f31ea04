"""Host-side checks of the surface contact measure (acrmi_surface_contact_workspace / acrmi_mesh_surface_contact /
acrmi_surface_contact, ops.mesh_surface_contact, Engine.contact(mode='surface')): the ABI surface and the
argument checks that need no device, the rule itself through the numpy restatement alone (tests/surface_contact_ref.py) - exact
cases, two spheres against geometry, and the case the nearest-vertex measure gets wrong -, the packaging of the contact keys,
and the rule's stand-alone check program.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import contact_ref
import surface_contact_ref as R
from conftest import ROOT, pkg
from render_ref import ellipsoid

NEW = ('acrmi_surface_contact_workspace', 'acrmi_mesh_surface_contact', 'acrmi_surface_contact')
F32 = np.float32


def test_new_symbols_are_declared_exported_and_bound():
    L = pkg('_lib')
    lib = L.lib()
    header = open(os.path.join(ROOT, 'include', 'acrmi.h')).read()
    for name in NEW:
        assert name + '(' in header and name in L.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.acrmi_mesh_surface_contact.argtypes) == 20 and len(lib.acrmi_surface_contact.argtypes) == 15
    assert lib.acrmi_surface_contact_workspace.restype is ctypes.c_size_t
    assert lib.acrmi_version() == L.VERSION == 303      # additive: the ABI version stays
    # the rule stands in the header, in the plan header and in the design document
    plan = open(os.path.join(ROOT, pkg().__name__, 'csrc', 'surface_contact_plan.h')).read()
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    for text in (header, plan, design, R.__doc__):
        assert 'd1/(d1-d3)' in text and 'e43/(e43+e56)' in text and '(va+vb)+vc' in text
        assert '(hi.x-lo.x)*(p.y-lo.y) - (hi.y-lo.y)*(p.x-lo.x)' in text
    assert '## 20.' in design
    ops = pkg('ops')      # the constants the Python layer repeats are the plan's
    for name, value in (('SURFACE_FACE_TILE', ops.SURFACE_FACE_TILE), ('SURFACE_MAX_FACES', ops.SURFACE_MAX_FACES)):
        assert re.search(r'constexpr int %s = (\d+);' % name, plan).group(1) == str(value)


def test_workspace_size():
    lib = pkg('_lib').lib()
    for m, v, f in ((0, 778, 1538), (2, 0, 1538), (2, 778, 0), (-1, 5, 5), (3, -2, 1), (0, 0, 0)):
        assert lib.acrmi_surface_contact_workspace(m, v, f) == 0
    assert lib.acrmi_surface_contact_workspace(2, 778, 1538) == 2 * (778 * 16 + 1538 * 48)
    assert lib.acrmi_surface_contact_workspace(128, 4000, 8000) == 128 * (4000 * 16 + 8000 * 48)


def test_bad_arguments_are_rejected_before_any_device_call():
    L = pkg('_lib')
    lib = L.lib()
    p = ctypes.c_void_p(256)      # never read: the checks come first
    good = dict(verts=p, trans=None, M=2, V=778, F=1538, topo=p, topo2=None, mesh_topo=None, pairs=p, n=1, r=0.005, m=0.02,
                face=p, d2=p, point=p, cross=p, sf=p, si=p, ws=p, stream=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        rc = lib.acrmi_mesh_surface_contact(*a.values())
        return rc, lib.acrmi_last_error(None)

    # limits are refused, not clamped: 4001 vertices, 8001 faces, and the 2^31 - 1 element limits
    for bad in (dict(verts=None), dict(topo=None), dict(pairs=None), dict(face=None), dict(d2=None), dict(point=None),
                dict(cross=None), dict(sf=None), dict(si=None), dict(ws=None), dict(ws=ctypes.c_void_p(264)), dict(M=0), dict(M=-1),
                dict(V=0), dict(V=4001), dict(F=0), dict(F=8001), dict(n=-1), dict(r=-0.001), dict(r=float('inf')),
                dict(r=float('nan')), dict(m=-1.0), dict(m=float('nan')), dict(n=460100), dict(M=2760400), dict(M=465500)):
        rc, msg = call(**bad)
        assert rc == L.E_INVAL and msg.startswith(b'acrmi_mesh_surface_contact:'), (bad, rc, msg)
    # no pair: success, nothing is touched (also on a machine without a GPU)
    assert call(n=0)[0] == 0
    assert call(n=0, verts=None, pairs=None, face=None, ws=None)[0] == 0
    assert call(n=0, V=4001)[0] == L.E_INVAL and call(n=0, F=8001)[0] == L.E_INVAL
    if not torch.cuda.is_available():      # well-formed arguments reach the device: a loud failure, no host path
        assert call(V=4000, F=8000, m=float('inf'), r=0.0)[0] == L.E_HIP
    # the context form
    args = [None, p, p, p, 2, 1, 0.005, 0.02, p, p, p, p, p, p, None]
    assert lib.acrmi_surface_contact(*args) == L.E_INVAL and lib.acrmi_last_error(None).startswith(b'acrmi_surface_contact:')
    # the operator refuses host tensors before it looks at the device
    with pytest.raises(L.AcrmiError):
        pkg('ops').mesh_surface_contact(torch.zeros(2, 5, 3), np.zeros((4, 3), np.int64), [[0, 1]])


def test_engine_and_batch_arguments():
    """What Engine.contact and forward_batch refuse before the context is touched (a stub stands for the context)."""
    E = pkg('engine')
    eng = E.Engine.__new__(E.Engine)
    out = {'slots': torch.zeros(2, 2, 176), 'verts': torch.zeros(2, 2, 778, 3)}
    for mode in ('Surface', 'triangle', None, 1, True):
        with pytest.raises(ValueError, match='mode'):
            eng.contact(out, mode=mode)
    for kw in (dict(max_hand=2), dict(contact_dist=-1.0), dict(max_depth=float('nan'))):
        with pytest.raises(ValueError):
            eng.contact(out, mode='surface', **kw)
    eng.ctx = None      # (so that __del__ has nothing to close)
    from importlib import import_module
    main = import_module(pkg().__name__ + '.acr.main')
    for ok in (True, False, 'surface'):
        main._check_contact(ok)
    for bad in (1, 0, None, 'vertex', 'Surface', b'surface', 1.0):
        with pytest.raises(ValueError):
            main._check_contact(bad)


TRI = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], F32)
# one point per branch of the closest-point rule, with its D2 and the point on the triangle
BRANCH_POINTS = [((-1, -1, 2), 6, (0, 0, 0)), ((5, -1, 0), 2, (4, 0, 0)), ((2, -3, 0), 9, (2, 0, 0)), ((-1, 5, 2), 6, (0, 4, 0)),
                 ((-2, 2, 0), 4, (0, 2, 0)), ((3, 3, 0), 2, (2, 2, 0)), ((1, 1, 3), 9, (1, 1, 0))]


def test_exact_cases():
    cols = lambda rows: [np.asarray(rows, F32)[..., k] for k in range(3)]
    pts = np.array([p for p, _, _ in BRANCH_POINTS], F32)
    br, q, D2 = R.closest(cols(pts), *(cols(TRI[c][None]) for c in range(3)))
    assert br.tolist() == [1, 2, 3, 4, 5, 6, 7]
    assert D2.tolist() == [6, 2, 9, 6, 4, 2, 9] and D2.dtype == F32
    assert np.stack(q, 1).tolist() == [list(map(float, w)) for _, _, w in BRANCH_POINTS]
    # a point on the triangle: 0, through the whole measure; the vertex sits below the face it is nearest to
    verts = np.zeros((2, 4, 3), F32)
    verts[0, :3] = TRI
    verts[0, 3] = (1.5, 1.25, 5)                                                # (the apex is not over any of the points below)
    verts[1] = [(1, 1, 0), (1, 1, -2), (9, 9, -1), (0.5, 0.5, 7)]
    f = np.array([[0, 1, 2], [0, 1, 3], [1, 2, 3], [2, 0, 3]])                 # a closed tetrahedron on the triangle
    got = R.mesh_surface_contact(verts, f, [[1, 0]], contact_dist=0.0, max_depth=np.inf)
    assert got['d2'][0, 0, 0] == 0 and got['face'][0, 0, 0] == 0 and got['point'][0, 0, 0].tolist() == [1, 1, 0]
    assert got['closest'][0, 0].tolist() == [0, 0] and got['min_d2'][0, 0] == 0 and got['n_contact'][0, 0] == 1
    # (1, 1, -2) is below the closed tetrahedron: two crossings; (9, 9, -1) is beside it: none; (0.5, 0.5, 7) above: none
    assert got['cross'][0, 0].tolist()[1:] == [2, 0, 0]
    assert got['d2'][0, 0, 1] == 4 and got['point'][0, 0, 1].tolist() == [1, 1, 0]
    # a face with a repeated index never counts as a crossing, whatever lies above the point
    rep = np.array([[0, 0, 1], [1, 2, 2], [2, 0, 2], [0, 1, 0]])
    assert not R.crossings(verts[1], verts[0], rep).any()
    assert R.crossings(verts[1][1:2], verts[0], f[:1]).all()                 # ... the proper base does
    # an all-NaN face never wins, and does not cross
    nan = verts.copy()
    nan[0, 3] = np.nan
    nan_faces = np.array([[3, 3, 3], [0, 1, 2], [3, 3, 3]])
    got = R.mesh_surface_contact(nan, nan_faces, [[1, 0]])
    assert (got['face'][0, 0] == 1).all() and np.isfinite(got['d2'][0, 0]).all()
    only = R.mesh_surface_contact(nan, nan_faces[[0, 2]], [[1, 0]])
    assert (only['face'][0, 0] == -1).all() and np.isinf(only['d2'][0, 0]).all() and not only['point'][0, 0].any()
    assert not only['cross'][0, 0].any() and only['closest'][0, 0].tolist() == [-1, -1] and not only['n_contact'][0].any()
    # a skipped pair
    skip = R.mesh_surface_contact(verts, f, [[-1, 0], [0, 2]])
    assert (skip['face'] == -1).all() and np.isinf(skip['d2']).all() and not skip['point'].any() and not skip['cross'].any()
    assert not skip['n_contact'].any() and not skip['n_inside'].any() and (skip['closest'] == -1).all()


SPHERES = [(nlat, nlon, c) for nlat, nlon in ((12, 24), (20, 38), (9, 97)) for c in (0.12, 0.06, 0.03)]
# inside vertices of the first sphere at c = 0.12 / 0.06 / 0.03, as an independent fp32 prototype of the rule counted them
EXPECTED_INSIDE = {(12, 24): (0, 41, 78), (20, 38): (0, 107, 208), (9, 97): (0, 128, 252)}


@pytest.mark.parametrize('nlat,nlon,c', SPHERES)
def test_rule_on_two_spheres(nlat, nlon, c):
    """The measure against geometry, through the restatement alone.  r_in = the smallest distance from the sphere's centre to a
    face plane (the polyhedron is convex and inscribed: its in-radius), r_max = the largest vertex radius, both in float64
    from the mesh itself.  Every vertex closer than r_in to the other centre is inside, none farther than r_max is; the band
    between belongs to the geometry.  The distance to the surface lies between the distances to the two spheres; 1e-6 m
    covers a few dozen fp32 roundings at coordinates below 1 m (an ulp is 6e-8).  0 violations."""
    va, f = ellipsoid(nlat, nlon, (0.05,) * 3, (0, 0, 0.5))
    vb, _ = ellipsoid(nlat, nlon, (0.05,) * 3, (c, 0.003, 0.5))
    verts, centres = np.stack([va, vb]), (np.array((0, 0, 0.5)), np.array((c, 0.003, 0.5)))
    got = R.mesh_surface_contact(verts, f, [[0, 1]], max_depth=np.inf)
    violations = 0
    for k in (0, 1):
        other = verts[1 - k].astype(np.float64) - centres[1 - k]
        n = np.cross(other[f[:, 1]] - other[f[:, 0]], other[f[:, 2]] - other[f[:, 0]])
        r_in = np.abs((other[f[:, 0]] * n).sum(1) / np.linalg.norm(n, axis=1)).min()
        r_max = np.linalg.norm(other, axis=1).max()
        assert 0.9 * 0.05 < r_in < r_max < 0.05 + 1e-7
        r = np.linalg.norm(verts[k].astype(np.float64) - centres[1 - k], axis=1)
        inside = (got['cross'][0, k] % 2 == 1) & (got['face'][0, k] >= 0)
        d = np.sqrt(got['d2'][0, k].astype(np.float64))
        far, deep = r > r_max, r < r_in
        violations += int(inside[far].sum()) + int((~inside[deep]).sum())
        violations += int(((d < r - r_max - 1e-6) | (d > r - r_in + 1e-6))[far].sum())
        violations += int(((d < r_in - r - 1e-6) | (d > r_max - r + 1e-6))[deep].sum())
        assert got['n_inside'][0, k] == inside.sum() and (far.sum() > 0 or deep.sum() > 0)
        if inside.any():
            assert got['depth2'][0, k] == got['d2'][0, k][inside].max()
    print('inside per side', got['n_inside'][0].tolist(), 'min mm', (1000 * np.sqrt(got['min_d2'][0])).tolist())
    assert violations == 0
    assert got['n_inside'][0, 0] == EXPECTED_INSIDE[(nlat, nlon)][(0.12, 0.06, 0.03).index(c)]
    if c == 0.12:
        assert not got['n_inside'].any() and not got['depth2'].any() and not got['n_contact'].any()
    else:
        assert (got['n_inside'][0] > 0).all()


def test_a_vertex_over_the_flat_of_a_large_triangle():
    """Why the feature exists: a vertex 1 mm above the centroid of a triangle of 0.1 m edges is 1 mm from the surface and in
    contact at the default 5 mm; the nearest-vertex measure reports more than 50 mm and no contact."""
    h = 0.1 * np.sqrt(3) / 2
    tri = np.array([[0, 0, 0.5], [0.1, 0, 0.5], [0.05, h, 0.5]], F32)
    centroid = tri.astype(np.float64).mean(0)
    verts = np.stack([tri, np.tile((centroid - (0, 0, 0.001)).astype(F32), (3, 1))])
    f = np.array([[0, 1, 2]])
    got = R.mesh_surface_contact(verts, f, [[1, 0]])
    assert abs(np.sqrt(float(got['d2'][0, 0, 0])) - 0.001) < 1e-6 and got['face'][0, 0, 0] == 0
    assert got['n_contact'][0, 0] == 3 and abs(np.sqrt(float(got['min_d2'][0, 0])) - 0.001) < 1e-6
    assert np.abs(got['point'][0, 0, 0] - centroid).max() < 1e-6
    old = contact_ref.mesh_contact(verts, f, [[1, 0]])
    assert np.sqrt(float(old['min_d2'][0])) > 0.05 and not old['n_contact'][0].any()


def test_surface_keys_are_packaged_into_the_hand_dicts():
    from importlib import import_module
    main = import_module(pkg().__name__ + '.acr.main')
    g = np.random.default_rng(0)
    B, K, V = 1, 2, 778
    out = {'slots': g.normal(size=(B, K, 2, 176)).astype(F32), 'verts': np.zeros((B, K, 2, V, 3), F32),
           'joints': np.zeros((B, K, 2, 21, 3), F32), 'pj2d': np.zeros((B, K, 2, 21, 2), F32),
           'pj2d_org': np.zeros((B, K, 2, 21, 2), F32), 'cam_trans': np.zeros((B, K, 2, 3), F32)}
    flags = np.array([[[1, 1], [1, 0]]], F32)      # lefts 0, 1 and right 0
    out['slots'][..., 0] = flags
    n = B * K * K
    con = {'face': np.full((n, 2, V), -1, np.int32), 'd2': np.full((n, 2, V), np.inf, F32), 'point': np.zeros((n, 2, V, 3), F32),
           'cross': np.zeros((n, 2, V), np.int32), 'min_d2': np.full((n, 2), np.inf, F32), 'closest': np.full((n, 2, 2), -1, np.int32),
           'n_contact': np.zeros((n, 2), np.int32), 'n_inside': np.zeros((n, 2), np.int32), 'depth2': np.zeros((n, 2), F32),
           'contact_dist': 0.005, 'max_depth': 0.02}
    # pair 0 = (left 0, right 0): 3 mm seen from the left, 2 mm seen from the right; pair 2 = (left 1, right 0): 1 mm / 4 mm
    for p, d, touch in ((0, (0.003, 0.002), ([5], [6, 8])), (2, (0.001, 0.004), ([7, 9], [1]))):
        con['face'][p], con['d2'][p] = 0, F32(1.0)
        for k in (0, 1):
            con['d2'][p, k, touch[k]] = F32(d[k]) ** 2
            con['min_d2'][p, k] = F32(d[k]) ** 2
    con['depth2'][2] = (F32(0.004) ** 2, F32(0.002) ** 2)
    out['contact'] = con
    a = main.results_from_out(out, ['a'])['a']
    assert [int(h['hand_type']) for h in a] == [0, 0, 1]
    assert [int(h['contact_with']) for h in a] == [2, 2, 1]          # the right hand's partner is the nearer left hand
    assert np.allclose([h['contact_dist'] for h in a], [0.002, 0.001, 0.001], rtol=1e-6)      # the smaller of both directions
    assert [h['contact_verts'].tolist() for h in a] == [[5], [7, 9], [1]]                     # the hand's own direction
    assert np.allclose([h['penetration'] for h in a], [0, 0.004, 0.002], rtol=1e-6)
    assert a[0]['contact_verts'].dtype == np.int32 and a[0]['contact_dist'].dtype == F32


def test_rule_stand_alone_program(tmp_path):
    """tools/surface_contact_check.cpp: the functions of csrc/surface_contact_plan.h on the exact cases, on random vertex-face
    pairs against a plain restatement in the same file, and the plan's limits - as a program of its own.  The plain build must
    pass; the build with the address and undefined-behaviour sanitizers must pass as well where the host compiler can make
    one that starts - which of the two ran is printed."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        assert os.path.exists(hipcc), 'no C++ compiler'
        cmd = [hipcc, '-x', 'c++']
    else:
        cmd = [cxx]
    src = os.path.join(ROOT, 'tools', 'surface_contact_check.cpp')
    cmd += ['-std=c++17', '-O1', '-g', '-ffp-contract=off', src, '-o']
    plain = str(tmp_path / 'surface_contact_check')
    subprocess.run(cmd + [plain], check=True, capture_output=True)
    run = subprocess.run([plain], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    ran = None
    for label, extra in (('static', san + ['-static-libasan', '-static-libubsan']), ('shared', san)):
        exe = str(tmp_path / ('surface_contact_check_' + label))
        if subprocess.run(cmd + [exe] + extra, capture_output=True).returncode != 0:
            continue
        run = subprocess.run([exe], capture_output=True, text=True)
        if 'does not come first in initial library list' in run.stderr:
            continue
        ran = label
        assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
        break
    print('sanitizer variant that ran: %s' % ran)
