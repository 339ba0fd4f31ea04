"""CPU-side checks of tracking on the device (DESIGN.md "Tracking on the device"): the box rule of csrc/track_plan.h through
the C ABI (acrmi_track_box) against known answers and against acr.utils.boxes_from_keypoints, exactly; its stand-alone check
program, plain and under the address and undefined-behaviour sanitizers, with the roi_plan_or_frame rows the window kernels
compute on the device; the ABI and the argument checks that return before HIP is touched.  None of it needs a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import roi_ref as R
import track_ref as T
from conftest import ROOT, pkg

NEW_SYMBOLS = ('acrmi_track_box', 'acrmi_track_boxes', 'acrmi_preprocess_rois_dev', 'acrmi_preprocess_rois_nv12_dev')
FH, FW = 96, 160
NAN, INF = float('nan'), float('inf')
# (points, min_size, box) in a 96 x 160 frame at scale 1.5
KNOWN = [
    ([(80.25, 40.5)], 64, (48, 8, 113, 73)),
    ([(80.25, 40.5)], 1, (79, 40, 81, 41)),
    ([(-30, 20), (10, 50)], 64, (0, 3, 64, 67)),
    ([(1e6, 40)], 64, (96, 8, 160, 72)),
    ([(NAN, 1), (20, 30), (25.5, 33.25)], 64, (0, 0, 65, 65)),
    ([(INF, 1)], 64, (0, 0, 160, 96)),
    ([], 64, (0, 0, 160, 96)),
]
# tests/test_roi_host.py's cases
H, W = 48, 64
INT_CASES = [
    (H, W, (10, 5, 40, 30)),
    (H, W, (0, 5, 40, 30)), (H, W, (10, 0, 40, 30)),
    (H, W, (10, 5, 64, 30)), (H, W, (10, 5, 40, 48)),
    (H, W, (-7, 5, 40, 30)), (H, W, (10, -3, 40, 30)),
    (H, W, (10, 5, 70, 30)), (H, W, (10, 5, 40, 99)),
    (H, W, (-20, -10, 30, 20)),
    (H, W, (-5, -5, 100, 100)), (H, W, (0, 0, 64, 48)),
    (H, W, (10, 5, 21, 42)), (H, W, (10, 5, 22, 42)),
    (H, W, (3, 20, 50, 27)), (H, W, (3, 20, 50, 28)),
    (H, W, (63, 47, 64, 48)), (H, W, (5, 0, 6, 48)),
    (37, 53, (9, 11, 18, 16)),
    (H, W, (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1)),
]
EMPTY = [(H, W, (30, 5, 30, 30)), (H, W, (10, 20, 40, 20)),
         (H, W, (40, 5, 10, 30)), (H, W, (10, 30, 40, 5)),
         (H, W, (64, 5, 80, 30)), (H, W, (10, 48, 40, 60)),
         (H, W, (-30, 5, 0, 30)), (H, W, (10, -30, 40, 0)), (H, W, (-9, -9, -1, -1))]


def _abi_box(pts, Hf, Wf, scale, min_size):
    L = pkg('_lib')
    a = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 2))
    box = (ctypes.c_int32 * 4)()
    rc = L.lib().acrmi_track_box(a.ctypes.data_as(ctypes.c_void_p) if len(a) else None, len(a), Hf, Wf, scale, min_size, box)
    assert rc == 0, L.lib().acrmi_last_error(None)
    return tuple(box)


@pytest.mark.parametrize('pts,min_size,want', KNOWN)
def test_known_answers(pts, min_size, want):
    assert _abi_box(pts, FH, FW, 1.5, min_size) == want
    assert T.boxes([np.asarray(pts, np.float32).reshape(-1, 2)], (FH, FW), 1.5, min_size)[0][0].tolist() == list(want)


def test_a_box_without_pixels_is_the_whole_frame():
    """The side is lost against the centre in the 53 bits of a double: numpy answers with a box that has no pixels, the
    device rule with the whole frame."""
    f = pkg('acr.utils').boxes_from_keypoints
    assert f([np.array([[3e38, 40]], np.float32)], (FH, FW)).tolist() == [[0, 8, 0, 72]]
    assert f([np.array([[-3e38, -3e38]], np.float32)], (FH, FW)).tolist() == [[0, 0, 0, 0]]
    assert _abi_box([(3e38, 40)], FH, FW, 1.5, 64) == (0, 0, 160, 96)
    assert _abi_box([(-3e38, -3e38)], FH, FW, 1.5, 64) == (0, 0, 160, 96)


def _seeded():
    return T.items(20261019, 500)


def test_seeded_items_equal_the_numpy_rule_exactly():
    replaced = 0
    kinds = set()
    for i, (pts, (Hf, Wf), scale, min_size) in enumerate(_seeded()):
        want, empty = T.boxes([pts], (Hf, Wf), scale, min_size)
        replaced += int(empty[0])
        got = _abi_box(pts, Hf, Wf, scale, min_size)
        assert list(got) == want[0].tolist(), (i, pts.tolist(), (Hf, Wf), scale, min_size, got, want[0].tolist())
        kinds.add(((Hf, Wf), scale, min_size))
        assert R.window(Hf, Wf, got) == got      # every box is a legal region of its frame
    print('%d of 500 rows had no pixels and were replaced by the whole frame' % replaced)
    assert 1 <= replaced <= 25      # the clause is exercised, and at most 5 % of the items need it
    assert len(kinds) == 27         # every frame with every scale and min_size


def _compiler():
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        assert os.path.exists(hipcc), 'no C++ compiler'
        return [hipcc, '-x', 'c++']
    return [cxx]


def _num(v):
    return '%.9g' % v      # nine digits carry an fp32 value exactly; nan, inf, -inf as strtof reads them


def _check_program(exe):
    seeded = _seeded()
    lines = ''.join('%d %d %.17g %d %s\n' % (Hf, Wf, scale, min_size, ' '.join(_num(v) for v in pts.reshape(-1)))
                    for pts, (Hf, Wf), scale, min_size in seeded)
    lines += ''.join('%d %d 1.5 %d %s\n' % (FH, FW, m, ' '.join(_num(v) for p in pts for v in p)) for pts, m, _ in KNOWN)
    run = subprocess.run([exe], input=lines, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    got = [tuple(int(w) for w in line.split()[1:]) for line in run.stdout.strip().split('\n')]
    assert len(got) == len(seeded) + len(KNOWN) and run.stdout.count('box ') == len(got)
    for row, (pts, (Hf, Wf), scale, min_size) in zip(got, seeded):
        assert row == _abi_box(pts, Hf, Wf, scale, min_size)
    assert got[len(seeded):] == [want for _, _, want in KNOWN]
    # roi_plan_or_frame: what the window kernels do with a box read from device memory
    cases = INT_CASES + EMPTY
    run = subprocess.run([exe, 'plan'], input=''.join('%d %d %d %d %d %d\n' % ((Hf, Wf) + box) for Hf, Wf, box in cases),
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    rows = run.stdout.strip().split('\n')
    assert len(rows) == len(cases)
    for line, (Hf, Wf, box) in zip(rows, cases):
        words = line.split()
        assert words[0] == 'window' and words[5] == 'offsets' and words[16] == 'status' and len(words) == 18, line
        empty = R.window(Hf, Wf, box) is None
        assert empty == ((Hf, Wf, box) in EMPTY)
        ref = (0, 0, Wf, Hf) if empty else box
        assert tuple(int(w) for w in words[1:5]) == R.window(Hf, Wf, ref), (box, line)
        assert [int(w) for w in words[6:16]] == R.offsets(Hf, Wf, ref).astype(int).tolist(), (box, line)
        assert int(words[17]) == int(empty), (box, line)
    for bad in ('8 8 1.5\n', '8 8 1.5 64 1\n', '0 8 1.5 64\n', '8 8 0 64\n', '8 8 nan 64\n', '8 8 inf 64\n', '8 8 1.5 0\n', '8 8 1.5 64 1 x\n'):
        assert subprocess.run([exe], input=bad, capture_output=True, text=True).returncode == 2, bad
    for bad in ('8 8 0 0 4\n', '8 0 0 0 4 4\n', '8 8 0 0 4 x\n'):
        assert subprocess.run([exe, 'plan'], input=bad, capture_output=True, text=True).returncode == 2, bad
    assert subprocess.run([exe, 'other'], input='', capture_output=True, text=True).returncode == 2


def test_track_plan_stand_alone_program(tmp_path):
    """tools/track_plan_check.cpp: csrc/track_plan.h and csrc/roi_plan.h as a program of its own (a host program with its own
    main), once as a plain build and once with the address and undefined-behaviour sanitizers.  How this compiler links a
    sanitized program that starts is found with an empty program first; nothing here skips."""
    base = _compiler() + ['-std=c++17', '-O1', '-g', '-ffp-contract=off']
    src = os.path.join(ROOT, 'tools', 'track_plan_check.cpp')
    plain = str(tmp_path / 'track_plan_check')
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
    checked = str(tmp_path / 'track_plan_check_san')
    built = subprocess.run(base + [src, '-o', checked] + flags, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    _check_program(checked)


def test_roi_plan_header_still_compiles_alone_both_ways(tmp_path):
    """csrc/roi_plan.h and csrc/track_plan.h carry a host / device macro now: as plain C++ it must expand to nothing, with the
    system compiler and with hipcc -x c++."""
    src = os.path.join(ROOT, 'tools', 'track_plan_check.cpp')
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc)
    exe = str(tmp_path / 'by_hipcc')
    built = subprocess.run([hipcc, '-x', 'c++', '-std=c++17', '-O1', src, '-o', exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], input='96 160 1.5 64 80.25 40.5\n', capture_output=True, text=True)
    assert run.stdout == 'box 48 8 113 73\n'


def test_abi_is_additive():
    L = pkg('_lib')
    src = open(os.path.join(ROOT, 'include', 'acrmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, src), '%s is not declared' % name
        assert name in L.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is ctypes.c_int
    assert [len(getattr(lib, name).argtypes) for name in NEW_SYMBOLS] == [7, 8, 9, 10]
    assert lib.acrmi_version() == L.VERSION == 303
    kernels = open(os.path.join(ROOT, pkg().__name__, 'csrc', 'kernels.h')).read()
    assert 'constexpr int ROIS_PER_LAUNCH = 64;' in kernels
    assert 'track.hip' in pkg('build').SOURCES


def _bgr(L, n=1, Hf=8, Wf=8, ptr=256):
    fr = (L.Frame * n)()
    for i in range(n):
        fr[i].bgr_dev, fr[i].H, fr[i].W = ptr, Hf, Wf      # (never dereferenced: the checks come first)
    return fr


def _nv12(L, n=1, Hf=8, Wf=8):
    fr = (L.NV12Frame * n)()
    for i in range(n):
        fr[i].y_dev, fr[i].uv_dev, fr[i].H, fr[i].W, fr[i].y_pitch, fr[i].uv_pitch = 256, 512, Hf, Wf, Wf, Wf
    return fr


def test_bad_arguments_are_rejected_without_a_gpu():
    L = pkg('_lib')
    lib = L.lib()
    p = ctypes.c_void_p(1024)      # (never dereferenced)
    bad = (L.E_INVAL, L.E_INVAL)

    def both(frames_bgr, frames_nv12, n_frames, roi_frame, boxes, n, dst=p, coef=None):
        return (lib.acrmi_preprocess_rois_dev(frames_bgr, n_frames, roi_frame, boxes, n, dst, p, p, None),
                lib.acrmi_preprocess_rois_nv12_dev(frames_nv12, n_frames, roi_frame, boxes, n, coef, dst, p, p, None))

    def idx(*v):
        return (ctypes.c_int32 * len(v))(*v)

    assert both(None, None, 1, None, p, 1) == bad
    assert both(_bgr(L), _nv12(L), 1, None, None, 1) == bad
    assert both(_bgr(L), _nv12(L), 1, None, p, 1, dst=None) == bad
    assert both(_bgr(L), _nv12(L), 1, None, p, 0) == bad
    assert both(_bgr(L), _nv12(L), 1, None, p, -1) == bad
    assert both(_bgr(L), _nv12(L), 0, None, p, 1) == bad
    # without roi_frame_host there is one region per frame
    assert both(_bgr(L, 2), _nv12(L, 2), 2, None, p, 3) == bad
    assert b'one region per frame' in lib.acrmi_last_error(None)
    # a bad frame
    assert both(_bgr(L, ptr=None), _nv12(L, Wf=7), 1, None, p, 1) == bad
    assert b'frame 0' in lib.acrmi_last_error(None)
    assert lib.acrmi_preprocess_rois_dev(_bgr(L, Hf=0), 1, None, p, 1, p, p, p, None) == L.E_INVAL
    # a frame index outside [0, n_frames): the message names the region
    for index in (-1, 2, 2 ** 31 - 1):
        assert both(_bgr(L, 2), _nv12(L, 2), 2, idx(0, 1, index), p, 3) == bad
        msg = lib.acrmi_last_error(None)
        assert b'region 2' in msg and b'frame index' in msg and b'acrmi_preprocess_rois_nv12_dev' in msg
    # the NV12 coefficient row is checked as acrmi_preprocess_nv12 checks it
    overflow = (ctypes.c_int32 * 6)(-(1 << 24), 0, 0, 0, 0, 16)
    assert lib.acrmi_preprocess_rois_nv12_dev(_nv12(L), 1, None, p, 1, overflow, p, p, p, None) == L.E_INVAL
    assert b'overflow' in lib.acrmi_last_error(None)
    # acrmi_track_boxes / acrmi_track_box
    assert lib.acrmi_track_boxes(None, p, p, 1, 1.5, 64, p, None) == L.E_INVAL
    assert lib.acrmi_track_boxes(p, None, p, 1, 1.5, 64, p, None) == L.E_INVAL
    assert lib.acrmi_track_boxes(p, p, None, 1, 1.5, 64, p, None) == L.E_INVAL
    assert lib.acrmi_track_boxes(p, p, p, 1, 1.5, 64, None, None) == L.E_INVAL
    assert lib.acrmi_track_boxes(p, p, p, 0, 1.5, 64, p, None) == L.E_INVAL
    box = (ctypes.c_int32 * 4)()
    pts = (ctypes.c_float * 2)(1, 2)
    for scale, min_size in ((0.0, 64), (-1.0, 64), (NAN, 64), (INF, 64), (1.5, 0), (1.5, -3)):
        assert lib.acrmi_track_boxes(p, p, p, 1, scale, min_size, p, None) == L.E_INVAL
        assert b'scale' in lib.acrmi_last_error(None) and b'min_size' in lib.acrmi_last_error(None)
        assert lib.acrmi_track_box(pts, 1, 8, 8, scale, min_size, box) == L.E_INVAL
    assert lib.acrmi_track_box(None, 1, 8, 8, 1.5, 64, box) == L.E_INVAL
    assert lib.acrmi_track_box(pts, -1, 8, 8, 1.5, 64, box) == L.E_INVAL
    assert lib.acrmi_track_box(pts, 1, 0, 8, 1.5, 64, box) == L.E_INVAL
    assert lib.acrmi_track_box(pts, 1, 8, 8, 1.5, 64, None) == L.E_INVAL
    assert lib.acrmi_track_box(None, 0, 8, 8, 1.5, 64, box) == 0 and tuple(box) == (0, 0, 8, 8)


def test_python_layer_refuses_bad_arguments_without_a_gpu():
    ops = pkg('ops')
    frames = [torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(6, 10, 3, dtype=torch.uint8)]
    good = torch.zeros(2, 4, dtype=torch.int32)      # (a CPU tensor: refused last, after everything else has been looked at)
    for boxes in ([[0, 0, 4, 4], [0, 0, 4, 4]], np.zeros((2, 4), np.int32), torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int64),
                  torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), torch.zeros(0, 4, dtype=torch.int32),
                  torch.zeros(2, 8, dtype=torch.int32)[:, ::2], good):
        with pytest.raises(ValueError, match=r'int32 CUDA tensor \[n,4\].*ops\.preprocess_rois'):
            ops.preprocess_rois_device(frames, boxes)
    with pytest.raises(ValueError, match='box_frame is needed'):
        ops.preprocess_rois_device(frames, torch.zeros(3, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match='region 1: frame index 2'):
        ops.preprocess_rois_device(frames, good, box_frame=[0, 2])
    with pytest.raises(ValueError, match='region 0: frame index -1'):
        ops.preprocess_rois_device(frames, good, box_frame=[-1, 0])
    with pytest.raises(ValueError, match='one integer per box'):
        ops.preprocess_rois_device(frames, good, box_frame=[0.0, 1.0])
    with pytest.raises(ValueError, match='one integer per box'):
        ops.preprocess_rois_device(frames, good, box_frame=[0])
    with pytest.raises(ValueError, match='pixel_format'):
        ops.preprocess_rois_device(frames, good, pixel_format='i420')
    with pytest.raises(ValueError, match='uint8'):
        ops.preprocess_rois_device([torch.zeros(8, 8, 3)], good[:1])
    with pytest.raises(ValueError, match='unknown NV12 matrix'):
        ops.preprocess_rois_device(torch.zeros(6, 4, dtype=torch.uint8), good[:1], pixel_format='nv12', matrix='bt2020')
    with pytest.raises(ValueError, match='even'):
        ops.preprocess_rois_device(torch.zeros(6, 5, dtype=torch.uint8), good[:1], pixel_format='nv12')
    pj, slots = torch.zeros(2, 2, 21, 2), torch.zeros(2, 2, 176)
    for kw in (dict(scale=0), dict(scale=-1.5), dict(scale=NAN), dict(scale=INF), dict(scale='1.5'), dict(min_size=0),
               dict(min_size=64.0), dict(min_size=-1)):
        with pytest.raises(ValueError, match='scale' if 'scale' in kw else 'min_size'):
            ops.track_boxes(pj, slots, (8, 8), **kw)
    for hw in ((8,), (8, 8, 8), (0, 8), (8.0, 8.0), [(8, 8)] * 3):
        with pytest.raises(ValueError, match='frame_hw'):
            ops.track_boxes(pj, slots, hw)
    with pytest.raises(ValueError, match='pj2d_org'):
        ops.track_boxes(torch.zeros(2, 2, 21, 3), slots, (8, 8))
    with pytest.raises(ValueError, match='pj2d_org'):
        ops.track_boxes(pj, torch.zeros(3, 2, 176), (8, 8))


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_no_cpu_fallback():
    ops, L = pkg('ops'), pkg('_lib')
    with pytest.raises(L.AcrmiError):
        ops.track_boxes(torch.zeros(2, 2, 21, 2), torch.zeros(2, 2, 176), (8, 8))
