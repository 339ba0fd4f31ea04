"""Host-side checks of the per-vertex colour views (acrmi_vertex_colors / acrmi_contact_values / acrmi_rasterize_colored /
acrmi_render_colored / acrmi_render_regions_colored, ops.vertex_colors / contact_values / render_meshes(vertex_colors=),
Engine.contact_colors / error_colors, show_items 'contact' / 'error'): the ABI surface and the argument
checks that need no device, the restatement's own edge rows (tests/vertex_color_ref.py), and the rule's stand-alone check
program.  No GPU."""
import ctypes
import os
import shutil
import subprocess
from importlib import import_module

import numpy as np
import pytest
import torch

import vertex_color_ref as VR
from conftest import ROOT, pkg

NEW = ('acrmi_vertex_colors', 'acrmi_contact_values', 'acrmi_rasterize_colored', 'acrmi_render_colored',
       'acrmi_render_regions_colored')
F32 = np.float32
INF, NAN = float('inf'), float('nan')


def test_new_symbols_are_declared_exported_and_bound():
    L = pkg('_lib')
    lib = L.lib()
    header = open(os.path.join(ROOT, 'include', 'acrmi.h')).read()
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW:
        assert name + '(' in header and name in L.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is ctypes.c_int, name
        assert '`%s`' % name in integration, name
    # the old entry points' arguments + vcol (+ the switch between per-frame and per-mesh view rows)
    assert len(lib.acrmi_rasterize_colored.argtypes) == len(lib.acrmi_rasterize.argtypes) + 2
    assert len(lib.acrmi_render_colored.argtypes) == len(lib.acrmi_render.argtypes) + 1
    assert len(lib.acrmi_render_regions_colored.argtypes) == len(lib.acrmi_render_regions.argtypes) + 1
    assert len(lib.acrmi_vertex_colors.argtypes) == 13 and len(lib.acrmi_contact_values.argtypes) == 10
    assert lib.acrmi_version() == L.VERSION == 303      # additive: the ABI version stays
    plan = open(os.path.join(ROOT, pkg().__name__, 'csrc', 'vertex_color_plan.h')).read()
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'ACRMI_HD' in plan and '__global__' not in plan and 'hip/' not in plan      # plain C++
    assert '## 22.' in design
    for text in (header, design):
        assert '((w_0 * vcol[v0][c] + w_1 * vcol[v1][c]) + w_2 * vcol[v2][c]) / d' in text
    main = import_module(pkg().__name__ + '.acr.main')
    assert main.SHOW_ITEMS[:4] == ('mesh', 'pj2d', 'centermap', 'org_img') and set(main.SHOW_ITEMS[4:]) == {'contact', 'error'}


def test_vertex_colors_arguments_are_checked_before_any_device_call():
    L = pkg('_lib')
    lib = L.lib()
    p = ctypes.c_void_p(256)      # never read: the checks come first
    rgb = (ctypes.c_float * 3)(1, 0, 1)
    good = dict(values=p, flags=None, base=p, M=2, V=778, lo=0.0, hi=0.02, reverse=0, flag_rgb=rgb, lut=None, bgr=0, vcol=p, stream=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.acrmi_vertex_colors(*a.values()), lib.acrmi_last_error(None)

    for bad in (dict(values=None), dict(base=None), dict(flag_rgb=None), dict(vcol=None), dict(M=-1), dict(V=0), dict(V=-3),
                dict(lo=0.02), dict(lo=0.03), dict(lo=NAN), dict(hi=NAN), dict(hi=INF), dict(lo=-INF), dict(lo=INF, hi=INF),
                dict(M=920100), dict(M=715827883, V=1), dict(M=1 << 30, V=1 << 30)):
        rc, msg = call(**bad)
        assert rc == L.E_INVAL and msg.startswith(b'acrmi_vertex_colors:'), (bad, rc, msg)
    assert call(M=0)[0] == 0 and call(M=0, values=None, vcol=None)[0] == 0      # nothing to do: success, nothing touched
    assert call(M=0, hi=0.0)[0] == L.E_INVAL
    if not torch.cuda.is_available():      # well-formed arguments reach the device: a loud failure, no host path
        assert call()[0] == L.E_HIP
    ops = pkg('ops')
    with pytest.raises(L.AcrmiError):
        ops.vertex_colors(torch.zeros(2, 5), 0, 1)
    for lo, hi in ((0, 0), (1, 0), (NAN, 1), (0, INF), (0, 1e39)):
        with pytest.raises(ValueError):
            ops.check_color_range(lo, hi)
    assert ops.check_color_range(0, 0.02) == (0.0, 0.02)
    with pytest.raises(ValueError, match='lut'):
        ops._lut_arg(np.zeros((256, 4), np.uint8))
    with pytest.raises(ValueError, match='lut'):
        ops._lut_arg(np.zeros((256, 3), np.float32))


def test_contact_values_arguments_are_checked_before_any_device_call():
    L = pkg('_lib')
    lib = L.lib()
    p = ctypes.c_void_p(256)
    good = dict(d2=p, s=p, cross=None, B=2, K=1, V=778, m=0.02, value=p, flag=p, stream=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.acrmi_contact_values(*a.values()), lib.acrmi_last_error(None)

    for bad in (dict(d2=None), dict(s=None), dict(cross=p), dict(value=None), dict(flag=None), dict(B=-1), dict(K=0), dict(K=9),
                dict(V=0), dict(m=-0.1), dict(m=NAN), dict(B=1381000), dict(B=21600, K=8)):
        rc, msg = call(**bad)
        assert rc == L.E_INVAL and msg.startswith(b'acrmi_contact_values:'), (bad, rc, msg)
    assert call(B=0)[0] == 0 and call(B=0, d2=None, value=None, flag=None)[0] == 0
    assert call(s=None, cross=p, B=0)[0] == 0
    if not torch.cuda.is_available():
        assert call(m=INF)[0] == L.E_HIP
    ops = pkg('ops')
    with pytest.raises(L.AcrmiError):
        ops.contact_values({'d2': torch.zeros(1, 2, 5), 'side': torch.zeros(1, 2, 5)}, 1)
    with pytest.raises(ValueError):
        ops.contact_values({'d2': torch.zeros(1, 2, 5)}, 1)


def test_colored_rasteriser_arguments_are_checked_before_any_device_call():
    L = pkg('_lib')
    lib = L.lib()
    p = ctypes.c_void_p(256)
    good = dict(verts=p, trans=None, M=2, V=778, F=1538, topo=p, topo2=None, mesh_topo=None, mesh_frame=p, rgb=p, vcol=p, view=None,
                per_mesh=0, focal=1265.0, w=0.9, img=p, out=p, N=1, H=64, W=64, ids=None, ws=p, stream=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.acrmi_rasterize_colored(*a.values()), lib.acrmi_last_error(None)

    for bad in (dict(vcol=None), dict(verts=None), dict(topo=None), dict(mesh_frame=None), dict(rgb=None), dict(img=None),
                dict(out=None), dict(ws=None), dict(per_mesh=1), dict(M=0), dict(V=4001), dict(F=0), dict(N=0), dict(H=0),
                dict(W=16385), dict(focal=0.0), dict(w=1.5), dict(w=NAN)):
        rc, msg = call(**bad)
        assert rc == L.E_INVAL and msg.startswith(b'acrmi_rasterize_colored:'), (bad, rc, msg)
    if not torch.cuda.is_available():
        assert call()[0] == L.E_HIP and call(per_mesh=1, view=p)[0] == L.E_HIP
    # the context forms: no context, and no colours
    args = [None, p, p, p, 2, None, None, p, 1265.0, 0.9, p, p, 64, 64, None, None]
    assert lib.acrmi_render_colored(*args) == L.E_INVAL and lib.acrmi_last_error(None).startswith(b'acrmi_render_colored:')
    args = [None, p, p, p, 2, p, p, None, p, 1265.0, 0.9, p, p, 1, 64, 64, None, None]
    assert lib.acrmi_render_regions_colored(*args) == L.E_INVAL
    assert lib.acrmi_last_error(None).startswith(b'acrmi_render_regions_colored:')
    with pytest.raises(L.AcrmiError):      # host tensors are refused before the device is looked at
        pkg('ops').render_meshes(torch.zeros(1, 5, 3), np.zeros((4, 3), np.int64), torch.zeros(1, 8, 8, 3, dtype=torch.uint8),
                                 vertex_colors=torch.zeros(1, 5, 3))


def test_engine_and_batch_arguments():
    """What the Engine calls and the acr layer refuse before the context is touched (a stub stands for the context)."""
    E = pkg('engine')
    eng = E.Engine.__new__(E.Engine)
    eng.ctx = None      # (so that __del__ has nothing to close)
    out = {'slots': torch.zeros(2, 2, 176), 'verts': torch.zeros(2, 2, 778, 3)}
    con = {'d2': torch.zeros(2, 2, 778), 'side': torch.zeros(2, 2, 778)}
    for kw in (dict(max_hand=2), dict(max_hand=0), dict(far=0.0), dict(far=NAN), dict(far=-1.0), dict(far=INF)):
        with pytest.raises(ValueError):
            eng.contact_colors(con, out, **kw)
    sc = {'verts': {'e_ra': torch.zeros(4, 778), 'e_pa': torch.zeros(4, 778)}}
    for kw in (dict(kind='mean'), dict(kind=None), dict(max_hand=2), dict(hi=0.0), dict(hi=NAN)):
        with pytest.raises(ValueError):
            eng.error_colors(sc, out, **kw)
    with pytest.raises(ValueError, match="gt\\['verts'\\]"):
        eng.error_colors({'verts': None}, out)
    with pytest.raises(ValueError):      # host tensors, and rows of another batch
        eng.error_colors(sc, out)
    main = import_module(pkg().__name__ + '.acr.main')
    assert main.check_show_items(('mesh', 'contact', 'error')) == ['mesh', 'contact', 'error']
    gt = {'joints': 1, 'verts': 1}
    main.check_color_items(['mesh', 'contact', 'error'], True, gt)
    main.check_color_items(['contact'], 'surface', None)
    main.check_color_items(['mesh', 'pj2d'], False, None, where='forward')
    main.check_color_items(None)
    with pytest.raises(ValueError, match='contact=True'):
        main.check_color_items(['mesh', 'contact'], False, gt)
    with pytest.raises(ValueError, match="gt= with 'verts'"):
        main.check_color_items(['error'], True, {'joints': 1})
    with pytest.raises(ValueError, match="gt= with 'verts'"):
        main.check_color_items(['error'], True, None)
    for name in ('contact', 'error'):
        with pytest.raises(ValueError, match='boxes='):
            main.check_color_items([name], True, gt, where='forward_raw_batch(boxes=)')
    # the entry points refuse before they touch the model (a stub stands for it)
    acr = main.ACR.__new__(main.ACR)
    acr.hands_per_side = 1
    frames = torch.zeros(1, 512, 512, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match='contact=True'):
        acr.forward_batch(frames, ['a'], render=frames, show_items=('mesh', 'contact'))
    with pytest.raises(ValueError, match="gt= with 'verts'"):
        acr.forward_batch(frames, ['a'], render=frames, show_items=('error',), contact=True, gt={'joints': torch.zeros(1, 2, 21, 3)})
    with pytest.raises(ValueError, match='contact=True'):
        acr.forward_raw_batch(frames, ['a'], render=True, show_items=('contact',))
    with pytest.raises(ValueError, match='boxes='):
        acr.forward_raw_batch(frames, ['a'], render=True, show_items=('contact',), contact=True, boxes=[[0, 0, 64, 64]])
    with pytest.raises(ValueError, match='track_raw_batch'):
        acr.track_raw_batch(frames, ['a'], render=True, show_items=('error',))


def test_restatement_edge_rows():
    lut = VR.default_lut()
    L = pkg('_lib').lib()
    for bgr in (0, 1):      # the default table is the heat-map views'
        buf = (ctypes.c_uint8 * 768)()
        assert L.acrmi_overlay_tables(bgr, None, buf) == 0
        assert (np.frombuffer(buf, np.uint8).reshape(256, 3) == VR.default_lut(bool(bgr))).all()
    lo, hi = 0.0, 0.02
    v = np.array([[-1, 0, -0.0, hi, 2 * hi, INF, -INF, NAN, 1e-42, hi / 2, np.nextafter(F32(hi), F32(0))]], F32)
    c = VR.vertex_colors(v, lo, hi, base=[0.1, 0.2, 0.3])
    assert c.dtype == F32 and c.shape == (1, 11, 3)
    i = [0, 0, 0, 255, 255, 255, 0, None, 0, 127, 254]
    for k, idx in enumerate(i):
        want = np.array([0.1, 0.2, 0.3], F32) if idx is None else lut[idx].astype(F32) / F32(255)
        assert (c[0, k] == want).all(), (k, idx)
    r = VR.vertex_colors(v, lo, hi, base=[0.1, 0.2, 0.3], reverse=True)
    assert (r[0, 3] == lut[0].astype(F32) / F32(255)).all() and (r[0, 0] == lut[255].astype(F32) / F32(255)).all()
    f = VR.vertex_colors(v, lo, hi, flags=np.array([[0, 5, -1, 0, 0, 0, 0, 1, 0, 0, 1 << 31 - 1]]), flag_color=(1, 0, 1))
    assert f[0, 1].tolist() == [1, 0, 1] and f[0, 7].tolist() == [1, 0, 1] and (f[0, 0] == c[0, 0]).all()
    assert (VR.vertex_colors(v, lo, hi, bgr=True)[0, 3] == lut[255, ::-1].astype(F32) / F32(255)).all()
    # contact values: the partner lists, NaN / +inf never win, no pair -> NaN, the two inside rules
    K, V = 2, 3
    d2 = np.full((4, 2, V), INF, F32)
    s = np.zeros((4, 2, V), F32)
    d2[0, 0] = [4e-4, NAN, INF]; d2[1, 0] = [1e-4, 9e-4, INF]          # left rank 0 against right ranks 0, 1
    s[0, 0] = [-1, -1, -1]; s[1, 0] = [1, -1, -1]
    d2[0, 1] = [1e-6, 1e-6, 1e-6]; d2[2, 1] = [4e-6, NAN, 0]           # right rank 0 against left ranks 0, 1
    val, flag = VR.contact_values(d2, s, 1, K, 0.02)
    assert np.array_equal(val[0, 0, 0], np.sqrt(np.array([1e-4, 9e-4, NAN], F32)), equal_nan=True)
    assert flag[0, 0, 0].tolist() == [1, 0, 0]       # (NaN <= m*m is false; +inf is beyond it)
    assert np.array_equal(val[0, 0, 1], np.sqrt(np.array([1e-6, 1e-6, 0], F32))) and flag[0, 0, 1].tolist() == [0, 0, 0]
    assert np.isnan(val[0, 1, 0]).all() and np.isnan(val[0, 1, 1]).all() and not flag[0, 1].any()
    cross = np.zeros((4, 2, V), np.int32)
    cross[1, 0] = [1, 2, 3]
    val2, flag2 = VR.contact_values(d2, cross, 1, K, 0.02, surface=True)
    assert np.array_equal(val2, val, equal_nan=True) and flag2[0, 0, 0].tolist() == [1, 0, 0]
    assert VR.contact_values(d2, cross, 1, K, 0.01, surface=True)[1][0, 0, 0].tolist() == [1, 0, 0]
    assert not VR.contact_values(d2, cross, 1, K, 0.009, surface=True)[1].any()      # 1e-4 > 0.009^2


def test_plan_stand_alone_program(tmp_path):
    """tools/vertex_color_check.cpp: csrc/vertex_color_plan.h against a plain restatement as a program of its own.  The plain
    build must pass; the build with the address and undefined-behaviour sanitizers must pass as well where the host compiler can
    make one that starts - which of the two ran is printed."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        assert os.path.exists(hipcc), 'no C++ compiler'
        cmd = [hipcc, '-x', 'c++']
    else:
        cmd = [cxx]
    src = os.path.join(ROOT, 'tools', 'vertex_color_check.cpp')
    cmd += ['-std=c++17', '-O1', '-g', '-ffp-contract=off', src, '-o']
    plain = str(tmp_path / 'vertex_color_check')
    subprocess.run(cmd + [plain], check=True, capture_output=True)
    run = subprocess.run([plain], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    ran = None
    for label, extra in (('static', san + ['-static-libasan', '-static-libubsan']), ('shared', san)):
        exe = str(tmp_path / ('vertex_color_check_' + label))
        if subprocess.run(cmd + [exe] + extra, capture_output=True).returncode != 0:
            continue
        run = subprocess.run([exe], capture_output=True, text=True)
        if 'does not come first in initial library list' in run.stderr:
            continue
        ran = label
        assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
        break
    print('sanitizer variant that ran: %s' % ran)
