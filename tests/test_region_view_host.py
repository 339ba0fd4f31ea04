"""CPU-side checks of the views over regions (DESIGN.md "Views over regions"): the rule of csrc/region_view_plan.h through its
stand-alone check program - plain, under the address and undefined-behaviour sanitizers, and as plain C++ through hipcc -
against the numpy restatement in tests/region_view_ref.py; the additive ABI; the argument checks that return before HIP is
touched; the Python layer's refusals.  None of it needs a GPU."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import region_view_ref as V
import roi_ref as R
from conftest import ROOT, pkg

NEW_SYMBOLS = ('acrmi_rasterize_views', 'acrmi_draw_region_heatmaps', 'acrmi_render_regions', 'acrmi_overlay_regions')
NAN, INF = float('nan'), float('inf')
H, W = 96, 160


def _rows():
    """(H, W, n_frames, frame, row): whole frames, windows clamped at each edge, crops that leave no pixel, negative, NaN and
    infinite entries, zero padded sizes, frame indices outside the batch, and seeded boxes through roi_ref.offsets."""
    rows = []
    for Hf, Wf in ((96, 160), (37, 53), (1080, 1920)):
        rows.append((Hf, Wf, 2, 0, R.offsets(Hf, Wf, (0, 0, Wf, Hf))))      # whole frames
    for box in ((0, 10, 50, 60), (110, 10, 160, 60), (30, 0, 80, 50), (30, 46, 80, 96), (-20, -10, 60, 70), (120, 60, 200, 140),
                (30, 20, 130, 90), (7, 9, 8, 10), (0, 0, 3, 5), (5, 0, 6, 96)):
        rows.append((H, W, 3, 1, R.offsets(H, W, box)))
    base = np.asarray(R.offsets(H, W, (30, 20, 130, 90)), np.float32)
    for at, value in ((5, 160.0), (5, 200.0), (3, 160.0), (3, 130.0), (2, 96.0), (4, 96.0), (4, 76.0), (2, 95.5), (5, 29.5), (5, 30.5),
                      (3, 0.5), (3, 29.5)):      # crops that leave no pixel, and fractional edges
        row = base.copy()
        row[at] = value
        rows.append((H, W, 3, 1, row))
    for at in range(10):
        for value in (-7.0, NAN, INF, -INF, 0.0, 1e30, -1e30):      # negative, NaN, infinite and zero entries, one at a time
            row = base.copy()
            row[at] = value
            rows.append((H, W, 3, 1, row))
    rows.append((H, W, 3, 1, np.full(10, NAN, np.float32)))
    rows.append((H, W, 3, 1, np.zeros(10, np.float32)))
    for frame in (-1, 3, 2 ** 31 - 1, -2 ** 31, 2):
        rows.append((H, W, 3, frame, base))
    rows.append((H, W, 0, 0, base))
    g = np.random.default_rng(20261019)
    for _ in range(200):
        l, t = int(g.integers(-40, W)), int(g.integers(-40, H))
        box = (l, t, l + int(g.integers(1, 200)), t + int(g.integers(1, 200)))
        if R.window(H, W, box) is not None:
            rows.append((H, W, 4, int(g.integers(-1, 5)), R.offsets(H, W, box)))
    return [(a, b, c, d, np.asarray(row, np.float32)) for a, b, c, d, row in rows]


def _num(v):
    return '%.9g' % v      # nine digits carry an fp32 value exactly; nan, inf, -inf as strtof reads them


def _f32(word):
    return struct.unpack('<f', struct.pack('<I', int(word, 16)))[0]


def test_the_restatement_on_known_rows():
    whole = V.region_view(R.offsets(H, W, (0, 0, W, H)), 0, 1, H, W)
    assert whole['window'] == (0, W, 0, H) and whole['draws']
    assert whole['view'].tolist() == [160 / 512, 160 / 512, 0.0, -32.0]      # 160 x 96 padded to 160 x 160: 32 rows above
    cut = V.region_view(R.offsets(H, W, (120, 60, 200, 140)), 1, 2, H, W)      # cut by the right and the bottom edge
    assert cut['window'] == (120, 160, 60, 96) and cut['draws']
    assert not V.region_view(R.offsets(H, W, (30, 20, 130, 90)), 2, 2, H, W)['draws']
    assert not V.region_view(np.full(10, NAN), 0, 1, H, W)['draws']
    assert not V.region_view(np.zeros(10), 0, 1, H, W)['draws']      # zero padded sizes: sx is not > 0


def _compiler():
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        assert os.path.exists(hipcc), 'no C++ compiler'
        return [hipcc, '-x', 'c++']
    return [cxx]


def _check_program(exe):
    rows = _rows()
    lines = ''.join('%d %d %d %d %s\n' % (a, b, c, d, ' '.join(_num(v) for v in row)) for a, b, c, d, row in rows)
    run = subprocess.run([exe], input=lines, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    got = run.stdout.strip().split('\n')
    assert len(got) == len(rows)
    kinds = set()
    for line, (Hf, Wf, n_frames, frame, row) in zip(got, rows):
        w = line.split()
        assert w[0] == 'view' and w[5] == 'window' and w[10] == 'draws' and len(w) == 12, line
        want = V.region_view(row, frame, n_frames, Hf, Wf)
        view = np.array([_f32(x) for x in w[1:5]], np.float32)
        assert np.array_equal(view, want['view'], equal_nan=True), (row.tolist(), line, want)
        assert tuple(int(x) for x in w[6:10]) == want['window'], (row.tolist(), line, want)
        assert int(w[11]) == int(want['draws']), (row.tolist(), line, want)
        x0, x1, y0, y1 = want['window']
        assert 0 <= x0 <= x1 <= Wf and 0 <= y0 <= y1 <= Hf      # no row leads outside the frame
        kinds.add((want['draws'], x0 < x1 and y0 < y1))
    assert kinds == {(True, True), (False, True), (False, False)}
    for bad in ('96 160 1 0 1 2 3\n', '0 160 1 0' + ' 0' * 10 + '\n', '96 99999 1 0' + ' 0' * 10 + '\n', '96 160 1 0' + ' 0' * 9 + ' x\n',
                '96 160 1 0.5' + ' 0' * 10 + '\n'):
        assert subprocess.run([exe], input=bad, capture_output=True, text=True).returncode == 2, bad
    assert subprocess.run([exe, 'other'], input='', capture_output=True, text=True).returncode == 2


def test_region_view_stand_alone_program(tmp_path):
    """tools/region_view_check.cpp: csrc/region_view_plan.h as a program of its own (a host program with its own main), once as
    a plain build and once with the address and undefined-behaviour sanitizers.  How this compiler links a sanitized program
    that starts is found with an empty program first; nothing here skips."""
    base = _compiler() + ['-std=c++17', '-O1', '-g', '-ffp-contract=off']
    src = os.path.join(ROOT, 'tools', 'region_view_check.cpp')
    plain = str(tmp_path / 'region_view_check')
    built = subprocess.run(base + [src, '-o', plain], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    _check_program(plain)
    empty = tmp_path / 'empty.cpp'
    empty.write_text('int main() { return 0; }\n')
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    flags = None
    for extra in (san + ['-static-libasan', '-static-libubsan'], san):
        exe = str(tmp_path / 'empty')
        if subprocess.run(base + [str(empty), '-o', exe] + extra, capture_output=True).returncode == 0 and \
                subprocess.run([exe], capture_output=True).returncode == 0:
            flags = extra
            break
    assert flags is not None, 'this compiler makes no address/undefined sanitizer build that starts'
    checked = str(tmp_path / 'region_view_check_san')
    built = subprocess.run(base + [src, '-o', checked] + flags, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    _check_program(checked)


def test_region_view_header_compiles_as_plain_cxx_through_hipcc(tmp_path):
    src = os.path.join(ROOT, 'tools', 'region_view_check.cpp')
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc)
    exe = str(tmp_path / 'by_hipcc')
    built = subprocess.run([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-ffp-contract=off', src, '-o', exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    _check_program(exe)


def test_the_kernels_use_the_header():
    csrc = os.path.join(ROOT, pkg().__name__, 'csrc')
    for name in ('render.hip', 'overlay.hip'):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "region_view_plan.h"' in text and 'region_view_row(' in text and 'region_view(' in text, name
        assert '/ 512.f' not in text.split('namespace acrmi', 1)[1].replace('(float)a.w / 512.f', '').replace('(float)a.h / 512.f', ''), \
            '%s restates the view' % name
    assert 'region_view_plan.h' in pkg('ops').view_from_offsets.__doc__
    offsets = torch.from_numpy(np.stack([R.offsets(H, W, (120, 60, 200, 140)), R.offsets(37, 53, (0, 0, 53, 37))]).astype(np.float32))
    got = pkg('ops').view_from_offsets(offsets).numpy()
    assert np.array_equal(got, np.stack([V.view_row(r) for r in offsets.numpy()]))


def test_abi_is_additive():
    L = pkg('_lib')
    src = open(os.path.join(ROOT, 'include', 'acrmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, src), '%s is not declared' % name
        assert name in L.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is ctypes.c_int
    assert [len(getattr(lib, name).argtypes) for name in NEW_SYMBOLS] == [21, 18, 17, 15]
    assert lib.acrmi_version() == L.VERSION == 303
    assert '#define ACRMI_VERSION 303' in open(os.path.join(ROOT, 'include', 'acrmi.h')).read()


def test_bad_arguments_are_rejected_without_a_gpu():
    L = pkg('_lib')
    lib = L.lib()
    p, q, r = ctypes.c_void_p(1024), ctypes.c_void_p(2048), ctypes.c_void_p(4096)      # (never dereferenced)

    def heat(maps=p, maps_r=None, stride=64 * 64, n=2, h=64, w=64, offsets=p, frames=p, weight=0.7, img=p, out=q, out_r=None,
             n_frames=2, Hf=H, Wf=W):
        return lib.acrmi_draw_region_heatmaps(maps, maps_r, stride, n, h, w, offsets, frames, weight, None, 0, img, out, out_r,
                                              n_frames, Hf, Wf, None)

    for kw in (dict(maps=None), dict(offsets=None), dict(frames=None), dict(img=None), dict(out=None), dict(maps_r=p),
               dict(out_r=r), dict(maps_r=p, out_r=q), dict(maps_r=p, out_r=p), dict(n=0), dict(n=-1), dict(n_frames=0),
               dict(n_frames=65536), dict(Hf=0), dict(Wf=0), dict(Hf=16385), dict(Wf=16385), dict(h=0), dict(w=0), dict(h=16385),
               dict(stride=64 * 64 - 1), dict(weight=-0.1), dict(weight=1.5), dict(weight=NAN)):
        assert heat(**kw) == L.E_INVAL, kw
        assert b'acrmi_draw_region_heatmaps' in lib.acrmi_last_error(None)

    def raster(view=p, verts=p, n_meshes=2, n_verts=10, n_faces=10, topo=p, mesh_frame=p, rgb=p, focal=1265.0, vw=0.9, img=p,
               out=q, n_frames=1, ws=p):
        return lib.acrmi_rasterize_views(verts, None, n_meshes, n_verts, n_faces, topo, None, None, mesh_frame, rgb, view, focal, vw,
                                         img, out, n_frames, H, W, None, ws, None)

    for kw in (dict(view=None), dict(verts=None), dict(n_meshes=0), dict(n_verts=4001), dict(n_faces=0), dict(topo=None),
               dict(mesh_frame=None), dict(rgb=None), dict(focal=0.0), dict(vw=1.5), dict(img=None), dict(out=None),
               dict(n_frames=0), dict(ws=None)):
        assert raster(**kw) == L.E_INVAL, kw
        assert b'acrmi_rasterize_views' in lib.acrmi_last_error(None)

    # the context calls refuse before they look at the context's state: a null context is enough to show it
    def render(ctx=None, verts=p, trans=p, slots=p, n=2, offsets=p, frames=p, focal=1265.0, vw=0.9, img=p, out=q, n_frames=2,
               Hf=H, Wf=W):
        return lib.acrmi_render_regions(ctx, verts, trans, slots, n, offsets, frames, None, focal, vw, img, out, n_frames, Hf, Wf,
                                        None, None)

    def overlay(what, ctx=None, slots=p, pj=p, n=2, offsets=p, frames=p, img=p, out=q, out2=r, n_frames=2, Hf=H, Wf=W):
        return lib.acrmi_overlay_regions(ctx, what, slots, pj, n, offsets, frames, 1, img, out, out2, n_frames, Hf, Wf, None)

    assert render() == L.E_INVAL and overlay(L.OVERLAY_SKELETON) == L.E_INVAL and overlay(L.OVERLAY_CENTERMAP) == L.E_INVAL


def test_python_layer_refuses_bad_arguments_without_a_gpu():
    ops, engine = pkg('ops'), pkg('engine')
    verts, faces = torch.zeros(2, 4, 3), np.array([[0, 1, 2], [0, 2, 3]])
    images = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match='view .* and mesh_view .* exclude each other'):
        ops.render_meshes(verts, faces, images, view=torch.ones(1, 4), mesh_view=torch.ones(2, 4))
    maps = torch.zeros(3, 2, 8, 8)
    good = torch.zeros(3, 10)
    for bad in (torch.zeros(3, 9), torch.zeros(10), torch.zeros(2, 10), torch.zeros(0, 10), [[0.0] * 10] * 4):
        with pytest.raises(ValueError, match=r'offsets must be \[n,10\]'):
            ops.draw_region_heatmaps(maps, images, bad, [0, 0, 0])
    for bad in ([0, 0], [0, 0, 0, 0], torch.zeros(3, 1, dtype=torch.int32), [0.0, 0.0, 0.0], torch.zeros(3)):
        with pytest.raises(ValueError, match='region_frame must hold one integer per region'):
            ops.draw_region_heatmaps(maps, images, good, bad)
    with pytest.raises(ValueError, match='maps must be a float tensor'):
        ops.draw_region_heatmaps(torch.zeros(3, 3, 8, 8), images, good, [0, 0, 0])
    with pytest.raises(ValueError, match='uint8'):
        ops.draw_region_heatmaps(maps, images.float(), good, [0, 0, 0])
    # Engine.render_regions / overlay_regions check their regions with the same function, before anything is queued
    assert ops.check_regions(good, [0, 1, 2], 3)[0] == 3
    for name in ('render_regions', 'overlay_regions', '_regions'):
        assert hasattr(engine.Engine, name)
    for name in ('render_regions', 'overlay_regions'):
        assert hasattr(engine.EnginePool, name)
    main = pkg('acr.main')
    with pytest.raises(ValueError, match='region_views=True .* needs boxes='):
        main._forward_raw_batch(None, None, ['a'], render=True, region_views=True)
    with pytest.raises(ValueError, match='show_items needs render=True'):
        main._track_raw_batch(None, None, ['a'], show_items=('mesh',))
    with pytest.raises(ValueError, match="render_format='nv12' needs render=True"):
        main._track_raw_batch(None, None, ['a'], render_format='nv12')


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_no_cpu_fallback():
    ops, L = pkg('ops'), pkg('_lib')
    with pytest.raises(L.AcrmiError):
        ops.draw_region_heatmaps(torch.zeros(1, 2, 8, 8), torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 10), [0])
