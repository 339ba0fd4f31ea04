"""CPU-side checks of the NV12 input path (DESIGN.md "NV12 input"): known answers of the numpy reference, the coefficient
tables and struct layout of the C ABI, argument checks that return before HIP is touched, and the layout rules of the Python
layer - none of it needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import nv12_ref as N
from conftest import ROOT, pkg

KNOWN_CV601 = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((81, 90, 240), (254, 0, 0)),
               ((145, 54, 34), (0, 255, 1)), ((41, 240, 110), (0, 0, 255)), ((0, 0, 0), (0, 154, 0)),
               ((255, 255, 255), (255, 125, 255)), ((255, 0, 0), (74, 255, 20))]
NEW_SYMBOLS = ('acrmi_nv12_matrix', 'acrmi_preprocess_nv12', 'acrmi_nv12_to_rgb')
WHICH = ('cv601', 'bt601', 'bt601-full', 'bt709', 'bt709-full')      # ACRMI_NV12_* in order


@pytest.mark.parametrize('yuv,rgb', KNOWN_CV601)
def test_reference_known_answers_cv601(yuv, rgb):
    assert tuple(int(c) for c in N.yuv_to_rgb(*yuv, 'cv601')) == rgb


def test_reference_known_answers_bt709():
    assert tuple(int(c) for c in N.yuv_to_rgb(81, 90, 240, 'bt709')) == (255, 24, 0)
    assert tuple(int(c) for c in N.yuv_to_rgb(81, 90, 240, 'bt709-full')) == (255, 36, 10)


def test_reference_frame_layout():
    """Nearest chroma: the 2x2 block shares one pair; BGR order; both uv shapes."""
    y = np.array([[81, 16], [235, 81]], np.uint8)
    uv = np.array([[90, 240]], np.uint8)
    bgr = N.nv12_to_bgr(y, uv)
    assert bgr.shape == (2, 2, 3) and bgr[0, 0].tolist() == [0, 0, 254] and (bgr[1, 1] == bgr[0, 0]).all()
    assert (N.nv12_to_bgr(y, uv.reshape(1, 1, 2)) == bgr).all()
    rgb, off = N.preprocess(y, uv)
    assert rgb.shape == (512, 512, 3) and off.tolist() == [2, 2, 0, 0, 0, 0, 0, 0, 0, 0]


def test_matrix_tables_match_the_reference_copy():
    L = pkg('_lib')
    lib = L.lib()
    for which, name in enumerate(WHICH):
        row = (ctypes.c_int32 * 6)()
        assert lib.acrmi_nv12_matrix(which, row) == 0
        assert tuple(row) == N.MATRICES[name]
        assert L.NV12_MATRICES[name] == which
        assert tuple(pkg('ops').nv12_matrix(name).tolist()) == N.MATRICES[name]
    row = (ctypes.c_int32 * 6)()
    assert lib.acrmi_nv12_matrix(5, row) == L.E_INVAL and lib.acrmi_nv12_matrix(-1, row) == L.E_INVAL
    assert lib.acrmi_nv12_matrix(0, None) == L.E_INVAL
    got = pkg('ops').nv12_matrix([1, 2, 3, 4, 5, 6])
    assert got.dtype == np.int32 and got.tolist() == [1, 2, 3, 4, 5, 6]


def test_abi_is_additive():
    L = pkg('_lib')
    assert ctypes.sizeof(L.NV12Frame) == 32 and L.NV12Frame.H.offset == 16 and L.NV12Frame.y_pitch.offset == 24
    assert ctypes.sizeof(L.Frame) == 16
    src = open(os.path.join(ROOT, 'include', 'acrmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, src), '%s is not declared' % name
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    assert 'typedef struct acrmi_nv12_frame' in src
    for which, name in enumerate(('CV601', 'BT601', 'BT601_FULL', 'BT709', 'BT709_FULL')):
        assert re.search(r'#define ACRMI_NV12_%s (\d+)' % name, src).group(1) == str(which)
    assert L.lib().acrmi_version() == L.VERSION == 303


def _frame(L, H=4, W=4, y_pitch=None, uv_pitch=None, y=256, uv=512):
    fr = (L.NV12Frame * 1)()
    fr[0].y_dev, fr[0].uv_dev, fr[0].H, fr[0].W = y, uv, H, W      # (never dereferenced: the checks come first)
    fr[0].y_pitch = W if y_pitch is None else y_pitch
    fr[0].uv_pitch = W if uv_pitch is None else uv_pitch
    return fr


def test_bad_arguments_are_rejected_without_a_gpu():
    L = pkg('_lib')
    lib = L.lib()
    out = ctypes.c_void_p(1024)
    dst = (ctypes.c_void_p * 1)(2048)
    overflow = (ctypes.c_int32 * 6)(-(1 << 24), 0, 0, 0, 0, 16)    # 255 * 2^24 >= 2^31, on the negative side too
    edge = (ctypes.c_int32 * 6)(0, 0, 1 << 23, -((1 << 23) - 4096), 0, 0)      # 128 * (2^24 - 4096) + 2^19 = 2^31
    y_off = (ctypes.c_int32 * 6)(1220542, 2116026, -409993, -852492, 1673527, 256)

    def both(fr, coef=None):
        return (lib.acrmi_preprocess_nv12(fr, 1, coef, out, None, None), lib.acrmi_nv12_to_rgb(fr, 1, coef, 1, dst, None))

    assert lib.acrmi_preprocess_nv12(None, 1, None, out, None, None) == L.E_INVAL
    assert lib.acrmi_preprocess_nv12(_frame(L), 1, None, None, None, None) == L.E_INVAL
    assert lib.acrmi_preprocess_nv12(_frame(L), 0, None, out, None, None) == L.E_INVAL
    assert lib.acrmi_nv12_to_rgb(None, 1, None, 1, dst, None) == L.E_INVAL
    assert lib.acrmi_nv12_to_rgb(_frame(L), 1, None, 1, None, None) == L.E_INVAL
    assert lib.acrmi_nv12_to_rgb(_frame(L), 1, None, 1, (ctypes.c_void_p * 1)(None), None) == L.E_INVAL
    assert b'frame 0' in lib.acrmi_last_error(None)
    for fr in (_frame(L, W=5, y_pitch=8, uv_pitch=8),      # odd W
               _frame(L, H=3), _frame(L, H=0), _frame(L, W=-2),
               _frame(L, y_pitch=2), _frame(L, uv_pitch=3),   # pitch below W
               _frame(L, uv=None), _frame(L, y=None)):
        assert both(fr) == (L.E_INVAL, L.E_INVAL)
        assert b'frame 0' in lib.acrmi_last_error(None)
    for coef in (overflow, edge, y_off):
        assert both(_frame(L), coef) == (L.E_INVAL, L.E_INVAL)
    assert b'acrmi_nv12_to_rgb' in lib.acrmi_last_error(None)
    # the bad frame is found wherever it stands, before anything is queued
    fr = (L.NV12Frame * 3)()
    for i in range(3):
        fr[i].y_dev, fr[i].uv_dev, fr[i].H, fr[i].W, fr[i].y_pitch, fr[i].uv_pitch = 256, 512, 4, 4, 4, 4
    fr[2].W = 6
    assert lib.acrmi_preprocess_nv12(fr, 3, None, out, None, None) == L.E_INVAL
    assert b'frame 2' in lib.acrmi_last_error(None)


def test_python_layer_refuses_bad_layouts_without_a_gpu():
    ops = pkg('ops')
    for fn in (ops.preprocess_nv12, ops.nv12_to_bgr):
        ok = torch.zeros(6, 4, dtype=torch.uint8)
        with pytest.raises(ValueError, match='unknown NV12 matrix'):
            fn(ok, matrix='bt2020')
        with pytest.raises(ValueError):
            fn(ok, matrix=[1, 2, 3])
        with pytest.raises(ValueError, match='innermost stride'):
            fn(torch.zeros(4, 6, dtype=torch.uint8).t())                          # column-major surface
        with pytest.raises(ValueError, match='innermost stride'):
            fn(torch.zeros(6, 8, dtype=torch.uint8)[:, ::2])                      # every other byte
        with pytest.raises(ValueError, match='innermost stride'):
            fn((torch.zeros(4, 8, dtype=torch.uint8)[:, ::2], torch.zeros(2, 4, dtype=torch.uint8)))
        with pytest.raises(ValueError, match='interleaved'):
            fn((torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(2, 2, 4, dtype=torch.uint8)[:, :, ::2]))
        with pytest.raises(ValueError, match='even'):
            fn(torch.zeros(6, 5, dtype=torch.uint8))                              # odd W
        with pytest.raises(ValueError, match='even'):
            fn((torch.zeros(3, 4, dtype=torch.uint8), torch.zeros(1, 4, dtype=torch.uint8)))      # odd H
        with pytest.raises(ValueError):
            fn(torch.zeros(7, 4, dtype=torch.uint8))                              # rows not a multiple of 3
        with pytest.raises(ValueError):
            fn((torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.uint8)))      # uv of the wrong shape
        with pytest.raises(ValueError):
            fn(torch.zeros(6, 4, dtype=torch.float32))
        with pytest.raises(ValueError):
            fn([])
    with pytest.raises(ValueError, match='pixel_format'):
        pkg('acr.utils').img_preprocess_gpu(torch.zeros(6, 4, dtype=torch.uint8), pixel_format='i420')


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_no_cpu_fallback():
    ops, L = pkg('ops'), pkg('_lib')
    for fn in (ops.preprocess_nv12, ops.nv12_to_bgr):
        with pytest.raises(L.AcrmiError):
            fn(torch.zeros(6, 4, dtype=torch.uint8))
