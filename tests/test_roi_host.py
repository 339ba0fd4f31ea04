"""CPU-side checks of region-of-interest pre-processing (DESIGN.md "Regions of interest"): the host rule of csrc/roi_plan.h
through the C ABI, the Python layer and its stand-alone check program against the numpy statement in tests/roi_ref.py,
argument checks that return before HIP is touched, the struct layout, and boxes_from_keypoints - none of it needs a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import roi_ref as R
from conftest import ROOT, pkg

NEW_SYMBOLS = ('acrmi_roi_offsets', 'acrmi_preprocess_rois', 'acrmi_preprocess_rois_nv12')
H, W = 48, 64
# (frame H, frame W, box): integer boxes
INT_CASES = [
    (H, W, (10, 5, 40, 30)),                                   # interior
    (H, W, (0, 5, 40, 30)), (H, W, (10, 0, 40, 30)),           # touching the left / top edge
    (H, W, (10, 5, 64, 30)), (H, W, (10, 5, 40, 48)),          # touching the right / bottom edge
    (H, W, (-7, 5, 40, 30)), (H, W, (10, -3, 40, 30)),         # overhanging each edge: clamped
    (H, W, (10, 5, 70, 30)), (H, W, (10, 5, 40, 99)),
    (H, W, (-20, -10, 30, 20)),                                # negative origin
    (H, W, (-5, -5, 100, 100)), (H, W, (0, 0, 64, 48)),        # the whole frame, overhanging and exact
    (H, W, (10, 5, 21, 42)), (H, W, (10, 5, 22, 42)),          # taller than wide: differences 26 and 25 (pad 12 left, 13 right)
    (H, W, (3, 20, 50, 27)), (H, W, (3, 20, 50, 28)),          # wider than tall: differences 40 and 39 (pad 19 top, 20 bottom)
    (H, W, (63, 47, 64, 48)), (H, W, (5, 0, 6, 48)),           # 1 x 1, a 1-pixel column
    (37, 53, (9, 11, 18, 16)),                                 # an odd frame
    (H, W, (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1)),    # the int32 extremes
]
FLOAT_CASES = [
    (200, 200, (10.0, 20.0, 100.7, 150.2)),                    # r = 100.7 of 200 crops int(99.3) = 99 on the right
    (200, 200, (10.9, 20.5, 100.0, 150.0)),                    # l, t truncate towards zero
    (H, W, (-3.5, -0.2, 40.5, 30.49)),
    (H, W, (0.999, 0.001, 63.001, 47.999)),
    (H, W, (5.5, 5.5, 1e12, 1e12)),
]
EMPTY = [(H, W, (30, 5, 30, 30)), (H, W, (10, 20, 40, 20)),                      # no width, no height
         (H, W, (40, 5, 10, 30)), (H, W, (10, 30, 40, 5)),                       # inverted
         (H, W, (64, 5, 80, 30)), (H, W, (10, 48, 40, 60)),                      # beyond the right / bottom edge
         (H, W, (-30, 5, 0, 30)), (H, W, (10, -30, 40, 0)), (H, W, (-9, -9, -1, -1))]      # before the left / top edge


def _abi_row(L, Hf, Wf, box):
    roi = L.Roi(0, *box)
    win = (ctypes.c_int32 * 4)()
    row = (ctypes.c_float * 10)()
    rc = L.lib().acrmi_roi_offsets(Hf, Wf, ctypes.byref(roi), win, row)
    return rc, tuple(win), np.array(row[:], np.float32)


def test_the_rule_by_hand():
    """Known answers, so that the reference statement and the library cannot be wrong together.  In a 48 x 64 frame the box
    (10, 5, 40, 30) crops 5 / 24 / 18 / 10 (t, r, b, l) and leaves 25 x 30, padded by 2 rows above and 3 below; (10, 5, 35, 35)
    leaves 30 x 25, padded by 2 columns left and 3 right.  In a 200 x 200 frame (10, 20, 100.7, 150.2) crops int(99.3) = 99 on
    the right and int(49.8) = 49 below: the window is [20:151, 10:101], 131 x 91, padded by 20 columns on either side."""
    for fn in (R.offsets, pkg('ops').roi_offsets):
        assert fn(H, W, (10, 5, 40, 30)).tolist() == [30, 30, 5, 24, 18, 10, 2, 0, 3, 0]
        assert fn(H, W, (10, 5, 35, 35)).tolist() == [30, 30, 5, 29, 13, 10, 0, 3, 0, 2]
        assert fn(200, 200, (10, 20, 100.7, 150.2)).tolist() == [131, 131, 20, 99, 49, 10, 0, 20, 0, 20]
    assert R.window(200, 200, (10, 20, 100.7, 150.2)) == (10, 20, 101, 151)


@pytest.mark.parametrize('Hf,Wf,box', INT_CASES)
def test_offsets_equal_the_reference_statement(Hf, Wf, box):
    L, ops = pkg('_lib'), pkg('ops')
    want, win = R.offsets(Hf, Wf, box), R.window(Hf, Wf, box)
    assert want is not None
    rc, got_win, got = _abi_row(L, Hf, Wf, box)
    assert rc == 0 and got_win == win and (got == want).all(), (got_win, got, win, want)
    row = ops.roi_offsets(Hf, Wf, box)
    assert row.dtype == np.float32 and (row == want).all()
    assert (ops.roi_offsets(Hf, Wf, np.array(box, np.int64)) == want).all()
    roi = L.Roi(0, *box)
    assert L.lib().acrmi_roi_offsets(Hf, Wf, ctypes.byref(roi), None, None) == 0      # either output may be left out


@pytest.mark.parametrize('Hf,Wf,box', FLOAT_CASES)
def test_float_boxes_truncate_like_the_reference(Hf, Wf, box):
    ops = pkg('ops')
    want = R.offsets(Hf, Wf, box)
    for given in (box, list(box), np.array(box, np.float64), torch.tensor(box, dtype=torch.float64)):
        assert (ops.roi_offsets(Hf, Wf, given) == want).all(), (given, want)
    # the integer box the Python layer hands to the library is the clamped window
    assert ops._roi_int_box(Hf, Wf, box) == R.window(Hf, Wf, box)


@pytest.mark.parametrize('Hf,Wf,box', EMPTY)
def test_empty_and_inverted_boxes_are_refused(Hf, Wf, box):
    L, ops = pkg('_lib'), pkg('ops')
    assert R.window(Hf, Wf, box) is None
    rc, _, _ = _abi_row(L, Hf, Wf, box)
    assert rc == L.E_INVAL and b'leaves no pixel' in L.lib().acrmi_last_error(None)
    with pytest.raises(ValueError, match='leaves no pixel'):
        ops.roi_offsets(Hf, Wf, box)


def test_roi_offsets_bad_arguments():
    L, ops = pkg('_lib'), pkg('ops')
    lib = L.lib()
    roi = L.Roi(0, 0, 0, 4, 4)
    row = (ctypes.c_float * 10)()
    assert lib.acrmi_roi_offsets(8, 8, None, None, row) == L.E_INVAL
    assert lib.acrmi_roi_offsets(0, 8, ctypes.byref(roi), None, row) == L.E_INVAL
    assert lib.acrmi_roi_offsets(8, -1, ctypes.byref(roi), None, row) == L.E_INVAL
    for bad in ((1, 2, 3), (1, 2, 3, 4, 5), 'abcd', (0, 0, float('nan'), 4), (0, 0, float('inf'), 4), [[0, 0, 4, 4]]):
        with pytest.raises(ValueError):
            ops.roi_offsets(8, 8, bad)
    with pytest.raises(ValueError):
        ops.roi_offsets(0, 8, (0, 0, 4, 4))


def test_abi_is_additive():
    L = pkg('_lib')
    assert ctypes.sizeof(L.Roi) == 20 and L.Roi.frame.offset == 0 and L.Roi.l.offset == 4 and L.Roi.b.offset == 16
    src = open(os.path.join(ROOT, 'include', 'acrmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, src), '%s is not declared' % name
        assert name in L.EXPORTS and hasattr(L.lib(), name)
        assert getattr(L.lib(), name).argtypes is not None and getattr(L.lib(), name).restype is ctypes.c_int
    assert 'typedef struct acrmi_roi' in src
    assert len(L.lib().acrmi_preprocess_rois.argtypes) == 7 and len(L.lib().acrmi_preprocess_rois_nv12.argtypes) == 8
    assert L.lib().acrmi_version() == L.VERSION == 303


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


def _rois(L, *rows):
    arr = (L.Roi * len(rows))()
    for i, row in enumerate(rows):
        arr[i] = L.Roi(*row)
    return arr


def test_bad_arguments_are_rejected_without_a_gpu():
    L = pkg('_lib')
    lib = L.lib()
    out = ctypes.c_void_p(1024)
    ok = (0, 1, 1, 5, 5)

    def both(frames_bgr, frames_nv12, n_frames, rois, n, dst=out):
        return (lib.acrmi_preprocess_rois(frames_bgr, n_frames, rois, n, dst, None, None),
                lib.acrmi_preprocess_rois_nv12(frames_nv12, n_frames, rois, n, None, dst, None, None))

    bad = (L.E_INVAL, L.E_INVAL)
    # null pointers, n = 0, no frames
    assert both(None, None, 1, _rois(L, ok), 1) == bad
    assert both(_bgr(L), _nv12(L), 1, None, 1) == bad
    assert both(_bgr(L), _nv12(L), 1, _rois(L, ok), 1, dst=None) == bad
    assert both(_bgr(L), _nv12(L), 1, _rois(L, ok), 0) == bad
    assert both(_bgr(L), _nv12(L), 1, _rois(L, ok), -1) == bad
    assert both(_bgr(L), _nv12(L), 0, _rois(L, ok), 1) == bad
    # a bad frame
    assert both(_bgr(L, ptr=None), _nv12(L, Wf=7), 1, _rois(L, ok), 1) == bad
    assert b'frame 0' in lib.acrmi_last_error(None)
    assert lib.acrmi_preprocess_rois(_bgr(L, Hf=0), 1, _rois(L, ok), 1, out, None, None) == L.E_INVAL
    # a frame index outside [0, n_frames): the message names the region
    for index in (-1, 2, 2 ** 31 - 1):
        rois = _rois(L, ok, (1, 0, 0, 4, 4), (index, 0, 0, 4, 4))
        for rc in both(_bgr(L, 2), _nv12(L, 2), 2, rois, 3):
            assert rc == L.E_INVAL
        assert b'region 2' in lib.acrmi_last_error(None) and b'frame index' in lib.acrmi_last_error(None)
    # an empty or inverted window, wherever it stands in the list, before anything is queued
    for _, _, box in EMPTY:
        small = tuple(min(max(v, -100), 100) for v in box)      # the same boxes against the 8 x 8 frame: still empty or outside
        if R.window(8, 8, small) is not None:
            continue
        rois = _rois(L, ok, (0,) + small, ok)
        assert both(_bgr(L), _nv12(L), 1, rois, 3) == bad
        msg = lib.acrmi_last_error(None)
        assert b'region 1' in msg and b'leaves no pixel' in msg and b'acrmi_preprocess_rois_nv12' in msg
    assert both(_bgr(L), _nv12(L), 1, _rois(L, ok, (0, 5, 2, 5, 6)), 2) == bad
    assert b'region 1' in lib.acrmi_last_error(None)
    # the NV12 coefficient row is checked as acrmi_preprocess_nv12 checks it
    overflow = (ctypes.c_int32 * 6)(-(1 << 24), 0, 0, 0, 0, 16)
    assert lib.acrmi_preprocess_rois_nv12(_nv12(L), 1, _rois(L, ok), 1, overflow, out, None, None) == L.E_INVAL


def test_python_layer_refuses_bad_arguments_without_a_gpu():
    ops, utils = pkg('ops'), pkg('acr.utils')
    frames = [torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(6, 10, 3, dtype=torch.uint8)]
    with pytest.raises(ValueError, match='box_frame is needed'):
        ops.preprocess_rois(frames, [[0, 0, 4, 4]])
    with pytest.raises(ValueError, match='region 1: frame index 2'):
        ops.preprocess_rois(frames, [[0, 0, 4, 4], [0, 0, 4, 4]], box_frame=[0, 2])
    with pytest.raises(ValueError, match='region 0: frame index -1'):
        ops.preprocess_rois(frames, [[0, 0, 4, 4]], box_frame=[-1])
    with pytest.raises(ValueError):
        ops.preprocess_rois(frames, [[0, 0, 4, 4]], box_frame=[0.0])
    with pytest.raises(ValueError):
        ops.preprocess_rois(frames, [[0, 0, 4, 4]], box_frame=[0, 1])
    with pytest.raises(ValueError):
        ops.preprocess_rois(frames, [[0, 0, 4]], box_frame=[0])
    with pytest.raises(ValueError):
        ops.preprocess_rois(frames, [], box_frame=[])
    with pytest.raises(ValueError):
        ops.preprocess_rois([], [[0, 0, 4, 4]], box_frame=[0])
    with pytest.raises(ValueError, match='pixel_format'):
        ops.preprocess_rois(frames, [[0, 0, 4, 4]], box_frame=[0], pixel_format='i420')
    with pytest.raises(ValueError, match='uint8'):
        ops.preprocess_rois([torch.zeros(8, 8, 3)], [[0, 0, 4, 4]])
    with pytest.raises(ValueError, match='even'):
        ops.preprocess_rois(torch.zeros(6, 5, dtype=torch.uint8), [[0, 0, 4, 4]], pixel_format='nv12')
    with pytest.raises(ValueError, match='unknown NV12 matrix'):
        ops.preprocess_rois(torch.zeros(6, 4, dtype=torch.uint8), [[0, 0, 4, 4]], pixel_format='nv12', matrix='bt2020')
    # NV12 as BGR: the boxes and frame indices are looked at before the device is
    surface = torch.zeros(6, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match='region 1: frame index 1'):
        ops.preprocess_rois(surface, [[0, 0, 4, 4], [0, 0, 4, 4]], box_frame=[0, 1], pixel_format='nv12')
    with pytest.raises(ValueError, match='box_frame is needed'):
        ops.preprocess_rois(surface, [[0, 0, 4, 4], [0, 0, 2, 2]], pixel_format='nv12')
    with pytest.raises(ValueError, match='boxes must be'):
        ops.preprocess_rois(surface, [[0, 0, 4]], pixel_format='nv12')
    with pytest.raises(ValueError, match='box_frame'):
        utils.img_preprocess_gpu(frames, box_frame=[0, 1])
    # img_preprocess(image, bbox=): the frame's layout and the box are looked at before the device is
    image = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match='leaves no pixel'):
        utils.img_preprocess(image, bbox=(5, 5, 5, 7))
    with pytest.raises(ValueError):
        utils.img_preprocess(image, bbox=(1, 2, 3))
    with pytest.raises(ValueError, match='uint8'):
        utils.img_preprocess(image.astype(np.float32), bbox=(0, 0, 4, 4))
    with pytest.raises(ValueError, match='input_size'):
        utils.img_preprocess(image, input_size=256, bbox=(0, 0, 4, 4))


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_no_cpu_fallback():
    ops, utils, L = pkg('ops'), pkg('acr.utils'), pkg('_lib')
    with pytest.raises(L.AcrmiError):
        ops.preprocess_rois([torch.zeros(8, 8, 3, dtype=torch.uint8)], [[0, 0, 4, 4]])
    with pytest.raises(L.AcrmiError):
        ops.preprocess_rois(torch.zeros(6, 4, dtype=torch.uint8), [[0, 0, 4, 4]], pixel_format='nv12')
    with pytest.raises(L.AcrmiError):
        utils.img_preprocess(np.zeros((8, 8, 3), np.uint8), bbox=(0, 0, 4, 4))


def _check_program_rows(exe):
    cases = INT_CASES + EMPTY
    args = [str(v) for Hf, Wf, box in cases for v in (Hf, Wf) + tuple(box)]
    run = subprocess.run([exe] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().split('\n')
    assert len(lines) == len(cases)
    for line, (Hf, Wf, box) in zip(lines, cases):
        want = R.offsets(Hf, Wf, box)
        if want is None:
            assert line == 'empty', (box, line)
            continue
        words = line.split()
        assert words[0] == 'window' and words[5] == 'offsets' and len(words) == 16, line
        assert tuple(int(w) for w in words[1:5]) == R.window(Hf, Wf, box), (box, line)
        assert [int(w) for w in words[6:]] == want.astype(int).tolist(), (box, line)
    assert subprocess.run([exe, '1', '2', '3'], capture_output=True).returncode == 2
    assert subprocess.run([exe, '8', '8', '0', '0', '4', 'x'], capture_output=True).returncode == 2


# the sizes at which the pad rule can go wrong (an odd pad on one axis, a one-pixel pad, an even pad), and 1080p both ways
FRAME_SIZES = [(1, 1), (1, 7), (7, 1), (2, 3), (3, 2), (5, 9), (9, 5), (1080, 1920), (1920, 1080)]


def _check_full_frame_rows(exe):
    """`frames`: the plan of the whole frame, which acrmi_preprocess, acrmi_preprocess_frames and acrmi_preprocess_nv12 take
    their offsets rows from, against the offsets of oracle.preprocess.img_preprocess for a frame of that size."""
    from oracle import preprocess as opre
    run = subprocess.run([exe, 'frames'], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().split('\n')
    assert len(lines) == len(FRAME_SIZES)
    for line, (Hf, Wf) in zip(lines, FRAME_SIZES):
        words = line.split()
        assert [words[i] for i in (0, 3, 8, 13, 18, 20)] == ['frame', 'window', 'crop', 'pad', 'side', 'offsets'] and len(words) == 31, line
        nums = {k: [int(w) for w in words[i:j]] for k, i, j in (('frame', 1, 3), ('window', 4, 8), ('crop', 9, 13), ('pad', 14, 18),
                                                               ('side', 19, 20), ('offsets', 21, 31))}
        _, want = opre.img_preprocess(np.zeros((Hf, Wf, 3), np.uint8))
        want = want.astype(int).tolist()
        assert nums['offsets'] == want, (Hf, Wf, line, want)
        assert nums['frame'] == [Hf, Wf] and nums['window'] == [0, 0, Wf, Hf] and nums['crop'] == [0, 0, 0, 0] == want[2:6]
        assert nums['pad'] == want[6:] and nums['side'] == [max(Hf, Wf)] == want[:1]
    assert want == [1920, 1920, 0, 0, 0, 0, 0, 420, 0, 420]      # 1920 x 1080 (H x W), by hand
    given = subprocess.run([exe, 'frames', '2', '3', '1', '7'], capture_output=True, text=True)
    assert given.returncode == 0 and [l.split()[21:] for l in given.stdout.strip().split('\n')] == \
        ['3 3 0 0 0 0 0 0 1 0'.split(), '7 7 0 0 0 0 3 0 3 0'.split()]
    assert subprocess.run([exe, 'frames', '8'], capture_output=True).returncode == 2


def test_roi_plan_stand_alone_program(tmp_path):
    """tools/roi_plan_check.cpp: csrc/roi_plan.h as a program of its own, its rows against tests/roi_ref.py - once as a plain
    build and once built with the address and undefined-behaviour sanitizers.  How this compiler links a sanitized program
    that starts (runtimes static or shared) is found with an empty program first; the check program must then build and
    pass that way, and nothing here skips.  Both builds also print the plans of whole frames (`frames`), which are compared
    with the pre-processing oracle's offsets rows."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        assert os.path.exists(hipcc), 'no C++ compiler'
        base = [hipcc, '-x', 'c++']
    else:
        base = [cxx]
    base += ['-std=c++17', '-O1', '-g']
    src = os.path.join(ROOT, 'tools', 'roi_plan_check.cpp')
    plain = str(tmp_path / 'roi_plan_check')
    subprocess.run(base + [src, '-o', plain], check=True, capture_output=True)
    _check_program_rows(plain)
    _check_full_frame_rows(plain)
    assert subprocess.run([plain], capture_output=True, text=True).stdout.count('\n') == 4      # the built-in list
    # the toolchain question, asked of a program without the code under test
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
    print('sanitizer flags: %s' % ' '.join(flags))
    checked = str(tmp_path / 'roi_plan_check_san')
    built = subprocess.run(base + [src, '-o', checked] + flags, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    _check_program_rows(checked)
    _check_full_frame_rows(checked)


def _hand(x0, y0, x1, y1):
    """21 points on the diagonal of the rectangle: its corners are among them."""
    s = np.linspace(0, 1, 21)[:, None]
    return np.array([x0, y0]) + s * np.array([x1 - x0, y1 - y0])


def test_boxes_from_keypoints_known_answers():
    f = pkg('acr.utils').boxes_from_keypoints
    hw = (480, 640)
    # one hand: 40 x 60 around (120, 230) -> side 60 * 1.5 = 90 -> [75, 165) x [185, 275)
    one = f([_hand(100, 200, 140, 260)[None]], hw)
    assert one.dtype == np.int32 and one.tolist() == [[75, 185, 165, 275]]
    # two hands: the box of both, 200 x 100 around (300, 150) -> side 300 -> [150, 450) x [0, 300)
    two = f([np.stack([_hand(200, 100, 260, 200), _hand(340, 120, 400, 180)])], hw)
    assert two.tolist() == [[150, 0, 450, 300]]
    # nothing detected -> the whole frame; the forms forward_batch returns
    assert f([np.zeros((0, 21, 2)), {}, []], hw).tolist() == [[0, 0, 640, 480]] * 3
    hands = [{'pj2d_org': _hand(100, 200, 140, 260).astype(np.float16), 'hand_type': np.int32(0)}]
    assert f([hands], hw).tolist() == [[75, 185, 165, 275]]
    # pushed back inside the frame: 90 wide around (630, 470) would end at (675, 515) -> moved by (-35, -35)
    assert f([_hand(610, 440, 650, 500)[None]], hw).tolist() == [[550, 390, 640, 480]]
    assert f([_hand(-10, -20, 30, 40)[None]], hw).tolist() == [[0, 0, 90, 90]]
    # min_size: a 4 x 6 hand gets 64 pixels around (102, 203), and more on request
    assert f([_hand(100, 200, 104, 206)[None]], hw).tolist() == [[70, 171, 134, 235]]
    assert f([_hand(100, 200, 104, 206)[None]], hw, min_size=100).tolist() == [[52, 153, 152, 253]]
    assert f([_hand(100, 200, 140, 260)[None]], hw, scale=1.0).tolist() == [[88, 198, 152, 262]]      # 60 < 64: min_size
    # a box larger than the frame is cut to it; one (H, W) per item
    big = f([_hand(10, 10, 90, 50)[None], _hand(10, 10, 90, 50)[None]], [(60, 100), (480, 640)], scale=2.0)
    assert big.tolist() == [[0, 0, 100, 60], [0, 0, 160, 160]]
    # every box is a legal region of its frame
    for row, (Hf, Wf) in zip(big.tolist(), [(60, 100), (480, 640)]):
        assert R.window(Hf, Wf, row) == tuple(row)
    with pytest.raises(ValueError):
        f([np.zeros((0, 2))], (0, 640))
    with pytest.raises(ValueError):
        f([np.zeros((0, 2))], [(480, 640), (480, 640)])
