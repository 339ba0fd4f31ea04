"""GPU tests of the NV12 input path (preprocess_rois_nv12_kernel of csrc/preprocess.hip, which ops.preprocess_nv12 runs with
the window (0, 0, W, H) of each surface, and nv12_to_rgb_kernel of csrc/nv12.hip; DESIGN.md "NV12 input") against the numpy
statement of its rule in tests/nv12_ref.py and the pre-processing oracle: everything is integer, so everything is compared
byte for byte.  All inputs are seeded random bytes over the full 0..255 range: both clamps and the negative-shift path are
hit."""
import numpy as np
import pytest
import torch

import nv12_ref as N
from conftest import pkg

pytestmark = pytest.mark.gpu

# (H, W): 2x2; pad on either side with an upscale; small odd-ish shapes; a strided view (see _device_frame); a downscale
# whose taps skip source pixels, so odd and even tap columns both occur; 1080p once
SIZES = [(2, 2), (4, 6), (6, 4), (18, 32), (34, 20), (130, 96), (540, 960), (1080, 1920)]
PITCHED = {(130, 96): 256}
CUSTOM_ROW = (1200000, 2000003, -400001, -800003, 1600001, 7)
_cache = {}


def _host_frame(H, W, seed=None):
    return N.random_nv12(H, W, 1000 * H + W if seed is None else seed)


def _device_frame(y, uv, pitch=None, fill=0):
    """One [H*3/2, W] device tensor; with `pitch`, a strided view of a [H*3/2, pitch] buffer whose bytes between W and the
    pitch hold `fill`."""
    H, W = y.shape
    surf = np.concatenate([y, uv], 0)
    if pitch is None:
        return torch.from_numpy(surf).cuda()
    buf = np.full((H * 3 // 2, pitch), fill, np.uint8)
    buf[:, :W] = surf
    return torch.from_numpy(buf).cuda()[:, :W]


def _reference(H, W, row='cv601'):
    """(rgb512, offsets) of the seeded frame of this size, computed once and shared."""
    key = (H, W, row)
    if key not in _cache:
        _cache[key] = N.preprocess(*_host_frame(H, W), row)
    return _cache[key]


def _mixed_batch(fill=0):
    return [_device_frame(*_host_frame(H, W), pitch=PITCHED.get((H, W)), fill=fill) for H, W in SIZES]


def test_fused_path_equals_reference_on_mixed_sizes():
    ops = pkg('ops')
    frames = _mixed_batch(fill=255)
    assert frames[5].stride() == (256, 1) and not frames[5].is_contiguous()
    rgb, offsets = ops.preprocess_nv12(frames)
    torch.cuda.synchronize()
    assert tuple(rgb.shape) == (len(SIZES), 512, 512, 3) and rgb.dtype == torch.uint8 and tuple(offsets.shape) == (len(SIZES), 10)
    got = rgb.cpu().numpy()
    for i, (H, W) in enumerate(SIZES):
        want, off = _reference(H, W)
        bad = int((got[i] != want).sum())
        print('%dx%d: %d differing bytes' % (H, W, bad))
        assert bad == 0, 'frame %d (%dx%d)' % (i, H, W)
        assert (offsets[i].numpy() == off).all()
    # the bytes between W and the pitch are not read: another filler, same result (0 and 255 would both change a tap)
    again, _ = ops.preprocess_nv12(_device_frame(*_host_frame(130, 96), pitch=256, fill=0))
    assert torch.equal(again[0], rgb[5])


@pytest.mark.parametrize('matrix', ['bt601', 'bt601-full', 'bt709', 'bt709-full', CUSTOM_ROW])
def test_fused_path_other_matrices(matrix):
    ops = pkg('ops')
    y, uv = _host_frame(18, 32)
    rgb, offsets = ops.preprocess_nv12(_device_frame(y, uv), matrix=matrix)
    want, off = N.preprocess(y, uv, matrix)
    assert (rgb[0].cpu().numpy() == want).all() and (offsets[0].numpy() == off).all()
    assert not (want == _reference(18, 32)[0]).all(), 'the matrix must matter'


def test_both_input_forms_give_identical_bytes():
    ops = pkg('ops')
    for H, W in ((18, 32), (2, 2), (4, 6)):
        y, uv = _host_frame(H, W)
        whole = _device_frame(y, uv)
        yd, uvd = torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()
        a, oa = ops.preprocess_nv12(whole)
        b, ob = ops.preprocess_nv12((yd, uvd.view(H // 2, W // 2, 2)))
        c, _ = ops.preprocess_nv12([(yd, uvd)])
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(oa, ob)
        assert (a[0].cpu().numpy() == _reference(H, W)[0]).all()
        assert torch.equal(ops.nv12_to_bgr(whole), ops.nv12_to_bgr((yd, uvd.view(H // 2, W // 2, 2))))
    stacked = torch.stack([_device_frame(*_host_frame(18, 32, seed=s)) for s in (1, 2)])      # [n, H*3/2, W]
    got, _ = ops.preprocess_nv12(stacked)
    each, _ = ops.preprocess_nv12([stacked[0], stacked[1]])
    assert got.shape[0] == 2 and torch.equal(got, each) and not torch.equal(got[0], got[1])


def test_more_frames_than_one_launch_holds():
    ops = pkg('ops')
    sizes = [((2, 2), (4, 6), (8, 4))[i % 3] for i in range(66)]
    host = [_host_frame(H, W, seed=i) for i, (H, W) in enumerate(sizes)]
    frames = [_device_frame(y, uv) for y, uv in host]
    rgb, offsets = ops.preprocess_nv12(frames)
    bgr = ops.nv12_to_bgr(frames)
    got = rgb.cpu().numpy()
    assert isinstance(bgr, list) and len(bgr) == 66
    for i, (y, uv) in enumerate(host):
        want, off = N.preprocess(y, uv)
        assert (got[i] == want).all(), 'frame %d' % i
        assert (offsets[i].numpy() == off).all()
        assert (bgr[i].cpu().numpy() == N.nv12_to_bgr(y, uv)).all(), 'frame %d' % i


def _pitched(plane, pitch, fill):
    """A strided device view of `plane` inside a buffer whose bytes between the width and the pitch hold `fill`."""
    buf = np.full((plane.shape[0], pitch), fill, np.uint8)
    buf[:, :plane.shape[1]] = plane
    return torch.from_numpy(buf).cuda()[:, :plane.shape[1]]


def test_frames_through_the_window_path_at_the_smallest_sizes():
    """acrmi_preprocess_nv12 hands the plan of the whole frame to the window path: the smallest surfaces with a pad on either
    axis, 10 x 4 once tight and once with y_pitch 11, uv_pitch 13 and a filler that would show, in one call."""
    ops = pkg('ops')
    sizes = [(2, 2), (2, 6), (6, 2), (10, 4)]
    host = [_host_frame(H, W) for H, W in sizes]
    y, uv = host[3]
    view = (_pitched(y, 11, 255), _pitched(uv, 13, 255))
    assert view[0].stride() == (11, 1) and view[1].stride() == (13, 1)
    rgb, offsets = ops.preprocess_nv12([_device_frame(*f) for f in host] + [view])
    assert tuple(rgb.shape) == (5, 512, 512, 3) and tuple(offsets.shape) == (5, 10)
    got = rgb.cpu().numpy()
    for i, (H, W) in enumerate(sizes + [(10, 4)]):
        want, off = _reference(H, W)
        bad = int((got[i] != want).sum())
        print('%dx%d: %d differing bytes, offsets %s' % (H, W, bad, offsets[i].tolist()))
        assert bad == 0, 'surface %d (%dx%d)' % (i, H, W)
        assert (offsets[i].numpy() == off).all()
    assert torch.equal(rgb[4], rgb[3]) and torch.equal(offsets[4], offsets[3])      # pitched and tight: equal bytes
    # 65 surfaces: the first, the last of the first launch and the one of the second against the reference, all against
    # the conversion followed by the BGR frame path
    many = [_host_frame(4, 4, seed=100 + i) for i in range(65)]
    frames = [_device_frame(*f) for f in many]
    rgb, offsets = ops.preprocess_nv12(frames)
    assert rgb.shape[0] == 65
    for i in (0, 63, 64):
        want, off = N.preprocess(*many[i])
        assert (rgb[i].cpu().numpy() == want).all(), 'surface %d' % i
        assert (offsets[i].numpy() == off).all()
    two, off2 = ops.preprocess_frames(ops.nv12_to_bgr(frames))
    assert torch.equal(rgb, two) and torch.equal(offsets, off2)


def test_plain_conversion_equals_reference():
    ops = pkg('ops')
    cases = [((2, 2), None), ((6, 10), 64), ((540, 960), None)]
    host = [_host_frame(H, W) for (H, W), _ in cases]
    frames = [_device_frame(y, uv, pitch=p, fill=255) for (y, uv), (_, p) in zip(host, cases)]
    got = ops.nv12_to_bgr(frames)
    assert isinstance(got, list) and [tuple(g.shape) for g in got] == [(2, 2, 3), (6, 10, 3), (540, 960, 3)]
    for g, (y, uv) in zip(got, host):
        assert (g.cpu().numpy() == N.nv12_to_bgr(y, uv)).all()
    flipped = ops.nv12_to_bgr(frames, rgb=True)
    for g, f in zip(got, flipped):
        assert torch.equal(f, g.flip(-1))
    same = ops.nv12_to_bgr([frames[1], frames[1]], matrix='bt709')
    assert isinstance(same, torch.Tensor) and tuple(same.shape) == (2, 6, 10, 3)
    assert (same[1].cpu().numpy() == N.nv12_to_bgr(*host[1], 'bt709')).all()
    one = ops.nv12_to_bgr(frames[0])
    assert tuple(one.shape) == (1, 2, 2, 3) and torch.equal(one[0], got[0])


def test_conversion_then_preprocess_equals_the_fused_path():
    """The composition property: the tap-wise conversion is the whole-frame conversion."""
    ops = pkg('ops')
    frames = _mixed_batch(fill=255)
    bgr = ops.nv12_to_bgr(frames)
    two, off2 = ops.preprocess_frames(bgr)
    one, off1 = ops.preprocess_nv12(frames)
    assert torch.equal(one, two) and torch.equal(off1, off2)


def _same_results(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert len(a[k]) == len(b[k])
        for h1, h2 in zip(a[k], b[k]):
            assert sorted(h1) == sorted(h2) and all(np.array_equal(h1[f], h2[f]) for f in h1)


@pytest.fixture(scope='module')
def near_sd():
    return pkg('synth').make_state_dict(seed=10)      # the checkpoint of tests/test_gpu_render.py: it detects both hands


def test_end_to_end_results_and_drawn_frames(near_sd, mano_tables):
    cfg, ops = pkg('config'), pkg('ops')
    acr = pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml', '--renderer', 'hip']),
                              state_dict=near_sd, mano_tables=mano_tables, max_batch=2)
    nv12 = [_device_frame(*_host_frame(96, 160, seed=s)) for s in (11, 12)]
    paths = ['a', 'b']
    bgr = ops.nv12_to_bgr(nv12)
    assert tuple(bgr.shape) == (2, 96, 160, 3)
    want = acr.forward_raw_batch(bgr, paths)
    _same_results(acr.forward_raw_batch(nv12, paths, pixel_format='nv12'), want)
    res_bgr, drawn_bgr = acr.forward_raw_batch(bgr, paths, render=True)
    res_nv12, drawn_nv12 = acr.forward_raw_batch(nv12, paths, render=True, pixel_format='nv12')
    _same_results(res_nv12, want)
    _same_results(res_bgr, want)
    assert tuple(drawn_nv12.shape) == (2, 96, 160, 3) and torch.equal(drawn_nv12, drawn_bgr)
    # without pixel_format a BGR call is what it was: pre-processing of the frames as they are, then forward_batch
    meta = pkg('acr.utils').img_preprocess_gpu(bgr, paths)
    assert torch.equal(meta['image'], ops.preprocess(bgr)[0])
    _same_results(acr.forward_batch(meta['image'], paths, offsets=meta['offsets']), want)
    _same_results(acr.forward_raw_batch(list(bgr), paths), want)
    print('hands per frame:', {k: len(v) for k, v in want.items()})
