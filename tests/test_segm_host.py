"""Host-side checks of the part segmentation as an output (acrmi_segm_tables / acrmi_segm_labels / acrmi_segm_stats /
acrmi_segment, ops.segm_labels / draw_segm / segm_stats, Engine.segment, show_items 'segm', masks=): the
numpy restatement (tests/segm_ref.py) against torch's bilinear interpolation + argmax and against plain numpy statistics, its
edge rows, the colour table, the ABI surface and the argument checks that need no device, and the rule's stand-alone check
program.  No GPU."""
import ctypes
import os
import shutil
import subprocess
from importlib import import_module

import numpy as np
import pytest
import torch

import segm_ref as SR
from conftest import ROOT, pkg

NEW = ('acrmi_segm_tables', 'acrmi_segm_labels', 'acrmi_segm_stats_ws_ints', 'acrmi_segm_stats', 'acrmi_segment')
F32 = np.float32
INF, NAN = float('inf'), float('nan')
MISMATCH_CAP = 1e-5      # share of the pixels whose label may differ from interpolate + argmax: the heat-map index test's cap


def smooth_logits(h, w, C, seed):
    """Smooth C-class logits with noise, NCHW [1,C,h,w]."""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(1, C, max(h // 16, 2), max(w // 16, 2), generator=g) * 3
    x = torch.nn.functional.interpolate(low, size=(h, w), mode='bicubic', align_corners=False)
    return (x + 0.3 * torch.randn(1, C, h, w, generator=g)).float()


@pytest.mark.parametrize('h,w,H,W', [(256, 256, 512, 512), (256, 256, 256, 256), (256, 256, 97, 203), (256, 256, 480, 640),
                                     (256, 256, 1080, 1920), (40, 56, 333, 517)])
def test_restatement_against_interpolate_and_argmax(h, w, H, W):
    """Under no view the rule is torch's bilinear resize (align_corners=False) followed by argmax, up to the rounding of the
    two interpolations.  Seen here: 0 pixels differ at every size of this list (one earlier probe of 1080p saw 1 of 2.07 M)."""
    x = smooth_logits(h, w, 33, 5)
    want = torch.nn.functional.interpolate(x, size=(H, W), mode='bilinear', align_corners=False).argmax(1)[0].numpy()
    got = SR.labels(x.permute(0, 2, 3, 1).contiguous().numpy(), 33, H, W)[0]
    bad = int((got != want).sum())
    print('%d x %d from %d x %d: %d of %d pixels differ (%.2e)' % (H, W, h, w, bad, got.size, bad / got.size))
    assert got.dtype == np.uint8 and got.shape == (H, W) and got.max() < 33
    assert bad <= MISMATCH_CAP * got.size
    assert len(np.unique(got)) > 8      # (the logits give a real mixture of labels)


def test_restatement_edge_rows():
    x = smooth_logits(256, 256, 33, 9).permute(0, 2, 3, 1).contiguous().numpy()
    # a 256 x 256 image without a view: the pixel is the cell (l1 = 0), the label the plain argmax
    assert np.array_equal(SR.labels(x, 33, 256, 256)[0], x[0].argmax(-1).astype(np.uint8))
    # more channels than classes: the tail of a cell is not looked at
    wide = np.concatenate([x, np.full((1, 256, 256, 3), 1e9, F32)], -1)
    assert np.array_equal(SR.labels(wide, 33, 64, 64), SR.labels(x, 33, 64, 64))
    # ties go to the lower class; a NaN in class 0 keeps label 0; a NaN elsewhere never wins
    cell = np.zeros((1, 2, 2, 5), F32)
    assert (SR.labels(cell, 5, 4, 4) == 0).all()
    cell[..., 3] = cell[..., 4] = 2
    assert (SR.labels(cell, 5, 4, 4) == 3).all()
    cell[..., 0] = NAN
    assert (SR.labels(cell, 5, 4, 4) == 0).all()
    cell[..., 0] = 1
    cell[..., 3] = NAN
    assert (SR.labels(cell, 5, 4, 4) == 4).all()
    cell[..., 4] = NAN
    assert (SR.labels(cell, 5, 4, 4) == 0).all()
    cell[..., 1] = INF      # an infinite cell under a weight of zero is NaN (2 x 2 pixels from 2 x 2 cells: l1 = 0): it does not win
    assert (SR.labels(cell, 5, 2, 2) == 0).all()
    assert (SR.labels(cell, 5, 8, 8)[0, 2:6, 2:6] == 1).all()      # between the cells both weights are > 0: inf wins
    # views: a partial canvas, a view that faces away, NaN
    o = np.array([[1024, 1024, 0, 0, 0, 100, 0, 0, 0, 0]], F32)      # scale 2, the canvas starts at x = 100
    v = SR.view_from_offsets(o)
    assert v.tolist() == [[2.0, 2.0, 100.0, 0.0]]
    lab = SR.labels(x, 33, 64, 200, v)[0]
    assert (lab[:, :100] == SR.NONE).all() and (lab[:, 100:] < 33).all()
    for bad in ([[-1, 1, 0, 0]], [[1, 0, 0, 0]], [[NAN, 1, 0, 0]], [[1, 1, NAN, 0]], [[1, 1, 0, INF]]):
        assert (SR.labels(x, 33, 8, 8, np.array(bad, F32)) == SR.NONE).all(), bad
    # the view: only the hands' pixels change, by the stated blend
    img = np.random.default_rng(1).integers(0, 256, (1, 64, 200, 3)).astype(np.uint8)
    col = SR.default_colors(33)
    drawn = SR.draw(img, lab[None], 33)
    hand = (lab >= 1) & (lab < 33)
    assert hand.any() and (~hand).any() and (drawn[0][~hand] == img[0][~hand]).all()
    y, xx = np.argwhere(hand)[0]
    want = np.floor(F32(0.7) * col[lab[y, xx]].astype(F32) + (F32(1) - F32(0.7)) * img[0, y, xx].astype(F32))
    assert (drawn[0, y, xx] == want.astype(np.uint8)).all()
    assert (SR.draw(img, lab[None], 33, weight=0.0) == img).all()
    assert (SR.draw(img, lab[None], 33, weight=1.0)[0][hand] == col[lab[hand]]).all()


def test_colour_table():
    L = pkg('_lib').lib()
    jet = (ctypes.c_uint8 * 768)()
    assert L.acrmi_overlay_tables(0, None, jet) == 0
    jet = np.frombuffer(jet, np.uint8).reshape(256, 3)
    assert np.array_equal(SR.jet(), jet)
    for C in (3, 5, 33, 63):
        for bgr in (0, 1):
            buf = (ctypes.c_uint8 * (3 * C))()
            assert L.acrmi_segm_tables(bgr, C, buf) == 0
            got = np.frombuffer(buf, np.uint8).reshape(C, 3)
            assert np.array_equal(got, SR.default_colors(C, bool(bgr))), (C, bgr)
            assert np.array_equal(got, pkg('ops').segm_colors(C, bool(bgr)))
    tab = SR.default_colors(33)
    for label in range(1, 33):      # the stated formula, on the heat maps' own table
        assert np.array_equal(tab[label], jet[128 + 8 * (label - 1)] if label <= 16 else jet[127 - 8 * (label - 17)]), label
    assert np.array_equal(SR.default_colors(33, True), tab[:, ::-1])
    assert not tab[0].any()
    right, left = {tuple(c) for c in tab[1:17]}, {tuple(c) for c in tab[17:]}
    assert len(right) == 16 and len(left) == 16 and not (right & left)      # 32 colours, the sides disjoint
    assert (tab[1:17, 0].astype(int) >= tab[1:17, 2]).all() and (tab[17:, 2].astype(int) >= tab[17:, 0]).all()      # right warm, left cold
    for bad in (4, 1, 65, 0, -3):
        assert L.acrmi_segm_tables(0, bad, (ctypes.c_uint8 * 256)()) == pkg('_lib').E_INVAL
    assert L.acrmi_segm_tables(0, 33, None) == pkg('_lib').E_INVAL


def test_statistics_restatement():
    g = np.random.default_rng(4)
    C, F = 33, 1538
    lab = g.integers(0, C, (3, 37, 53)).astype(np.uint8)
    lab[g.random(lab.shape) < 0.5] = 0
    lab[g.random(lab.shape) < 0.1] = SR.NONE
    lab[1][(lab[1] >= 1) & (lab[1] <= 16)] = 0      # frame 1 has no right hand
    lab[2] = 0                                      # frame 2 has no hand
    lab[2, 5, 7] = 20                               # ... but one left pixel
    ids = g.integers(-1, 6 * F, lab.shape).astype(np.int32)
    ids[g.random(lab.shape) < 0.5] = -1
    counts, boxes, agree = SR.stats(lab, C, ids, F)
    for f in range(3):
        assert np.array_equal(counts[f], np.bincount(lab[f].ravel(), minlength=256)[:C])
        assert counts[f].sum() == (lab[f] != SR.NONE).sum()      # label 255 is not counted
        for s, (lo, hi) in enumerate(((17, 32), (1, 16))):
            mask = (lab[f] >= lo) & (lab[f] <= hi)
            ys, xs = np.nonzero(mask)
            want = [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1] if len(xs) else [0, 0, 0, 0]
            assert boxes[f, s].tolist() == want, (f, s)
            sil = (ids[f] >= 0) & ((ids[f] // F) % 2 == s)
            assert agree[f, s].tolist() == [(mask & sil).sum(), mask.sum(), sil.sum()]
    assert boxes[1, 1].tolist() == [0, 0, 0, 0] and boxes[2, 0].tolist() == [7, 5, 8, 6] and boxes[2, 1].tolist() == [0, 0, 0, 0]
    none = np.full_like(ids, -1)
    a = SR.stats(lab, C, none, F)[2]
    assert (a[:, :, 0] == 0).all() and (a[:, :, 2] == 0).all() and np.array_equal(a[:, :, 1], agree[:, :, 1])      # ids = -1 everywhere
    assert SR.stats(lab, C)[2] is None
    alone = SR.stats(lab[1:2], C, ids[1:2], F)      # a frame alone is the frame in the batch
    assert np.array_equal(alone[0][0], counts[1]) and np.array_equal(alone[1][0], boxes[1]) and np.array_equal(alone[2][0], agree[1])


def test_new_symbols_are_declared_exported_and_bound():
    L = pkg('_lib')
    lib = L.lib()
    header = open(os.path.join(ROOT, 'include', 'acrmi.h')).read()
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW:
        assert name + '(' in header and name in L.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
        assert '`%s`' % name in integration, name
    assert lib.acrmi_segm_stats_ws_ints.restype is ctypes.c_size_t and lib.acrmi_segm_labels.restype is ctypes.c_int
    assert lib.acrmi_version() == L.VERSION == 303      # additive: the ABI version stays
    assert '#define ACRMI_SEGM_NONE 255' in header and L.SEGM_NONE == 255 == SR.NONE
    plan = open(os.path.join(ROOT, pkg().__name__, 'csrc', 'segm_plan.h')).read()
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'ACRMI_HD' in plan and '__global__' not in plan and 'hip/' not in plan      # plain C++
    assert '## 23.' in design
    main = import_module(pkg().__name__ + '.acr.main')
    assert main.SHOW_ITEMS == ('mesh', 'pj2d', 'centermap', 'org_img', 'contact', 'error') and main.MAP_ITEMS == ('segm',)
    assert main.check_show_items(('mesh', 'segm')) == ['mesh', 'segm'] and main.check_show_items('segm') == ['segm']
    with pytest.raises(ValueError, match='segms'):
        main.check_show_items(('segms',))


def test_labels_arguments_are_checked_before_any_device_call():
    L = pkg('_lib')
    lib = L.lib()
    p, q = ctypes.c_void_p(256), ctypes.c_void_p(4096)      # never read: the checks come first
    good = dict(logits=p, fs=256 * 256 * 36, ps=36, n=2, h=256, w=256, C=33, view=None, offsets=None, weight=0.7, colors=None, bgr=0,
                img=p, out=q, labels=q, H=64, W=64, stream=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.acrmi_segm_labels(*a.values()), lib.acrmi_last_error(None)

    for bad in (dict(C=32), dict(C=34), dict(C=1), dict(C=65), dict(C=0), dict(C=-33), dict(ps=32), dict(ps=0), dict(ps=5, C=7),
                dict(out=None, labels=None), dict(img=None), dict(logits=None), dict(view=p, offsets=p), dict(H=16385),
                dict(W=16385), dict(h=16385, fs=1 << 40), dict(w=16385, fs=1 << 40), dict(H=0), dict(W=-1), dict(h=0), dict(w=0),
                dict(n=-1), dict(n=65536), dict(fs=256 * 256 * 36 - 1), dict(weight=1.5), dict(weight=-0.1), dict(weight=NAN)):
        rc, msg = call(**bad)
        assert rc == L.E_INVAL and msg.startswith(b'acrmi_segm_labels:'), (bad, rc, msg)
    assert call(n=0)[0] == 0 and call(n=0, logits=None, img=None, out=None)[0] == 0      # nothing to do: success, nothing touched
    assert call(n=0, C=32)[0] == L.E_INVAL and call(n=0, out=None, labels=None)[0] == L.E_INVAL
    if not torch.cuda.is_available():      # well-formed arguments reach the device: a loud failure, no host path
        assert call()[0] == L.E_HIP and call(img=None, out=None)[0] == L.E_HIP and call(labels=None)[0] == L.E_HIP
    ops = pkg('ops')
    with pytest.raises(L.AcrmiError):      # host tensors are refused before the device is looked at
        ops.segm_labels(torch.zeros(1, 8, 8, 33))
    with pytest.raises(ValueError):
        ops.segm_labels(torch.zeros(1, 8, 8, 33, dtype=torch.float16))
    with pytest.raises(ValueError):
        ops.draw_segm(torch.zeros(1, 8, 8, 33), None)
    with pytest.raises(L.AcrmiError):
        ops.segm_stats(torch.zeros(1, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.segm_stats(torch.zeros(1, 8, 8))
    # the context form: no context
    assert lib.acrmi_segment(None, 1, None, 0.7, None, 0, None, None, q, 512, 512, None) == L.E_INVAL
    assert lib.acrmi_last_error(None).startswith(b'acrmi_segment:')


def test_stats_arguments_are_checked_before_any_device_call():
    L = pkg('_lib')
    lib = L.lib()
    p = ctypes.c_void_p(256)
    good = dict(labels=p, ids=p, n_faces=1538, n=2, H=64, W=64, C=33, counts=p, boxes=p, agree=p, ws=p, stream=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.acrmi_segm_stats(*a.values()), lib.acrmi_last_error(None)

    for bad in (dict(C=32), dict(C=65), dict(C=1), dict(labels=None), dict(counts=None), dict(boxes=None), dict(ws=None),
                dict(agree=None), dict(ids=None), dict(n_faces=0), dict(n_faces=-5), dict(H=0), dict(W=16385), dict(H=16385),
                dict(n=-1), dict(n=65536)):
        rc, msg = call(**bad)
        assert rc == L.E_INVAL and msg.startswith(b'acrmi_segm_stats:'), (bad, rc, msg)
    assert call(n=0)[0] == 0 and call(n=0, labels=None, counts=None, boxes=None, ws=None)[0] == 0
    if not torch.cuda.is_available():
        assert call()[0] == L.E_HIP and call(ids=None, agree=None, n_faces=0)[0] == L.E_HIP
    ws = lib.acrmi_segm_stats_ws_ints
    assert ws(2, 512, 512) == 2 * 32 * 80 and ws(1, 1, 1) == 80 and ws(1, 17, 5) == 160 and ws(0, 64, 64) == 0
    assert ws(1, 0, 64) == 0 and ws(1, 64, 16385) == 0 and ws(-1, 64, 64) == 0 and ws(65536, 64, 64) == 0


def test_engine_and_batch_arguments():
    """What Engine.segment and the acr layer refuse before the context is touched (a stub stands for the context)."""
    E = pkg('engine')
    eng = E.Engine.__new__(E.Engine)
    eng.ctx = None      # (so that __del__ has nothing to close)
    img = torch.zeros(2, 64, 64, 3, dtype=torch.uint8)
    for kw in (dict(images=img), dict(ids=torch.zeros(2, 512, 512, dtype=torch.int32)), dict(dst=img), dict(labels=False)):
        with pytest.raises(ValueError):
            eng.segment(2, **kw)
    main = import_module(pkg().__name__ + '.acr.main')
    for ok in (True, False, 'iou'):
        assert main.check_masks(ok) == ok
    for bad in (1, None, 'IoU', 'area', 0.5):
        with pytest.raises(ValueError, match='masks must be'):
            main.check_masks(bad)
    with pytest.raises(ValueError, match='over regions'):
        main.check_masks(True, where='forward_raw_batch(boxes=)')
    assert main.check_masks(False, where='forward_raw_batch(boxes=)') is False
    main.check_map_items(['mesh', 'pj2d'], 'anywhere')
    with pytest.raises(ValueError, match='over regions'):
        main.check_map_items(['mesh', 'segm'], 'forward_raw_batch(boxes=)')
    ms = {'counts': np.arange(66, dtype=np.int32).reshape(2, 33), 'boxes': np.arange(16, dtype=np.int32).reshape(2, 2, 4),
          'agree': np.array([[[2, 4, 6], [0, 0, 0]], [[0, 5, 0], [3, 3, 3]]], np.int32)}
    k = main.mask_keys(ms, 0, 0)
    assert k['mask_area'] == sum(range(17, 33)) and k['mask_box'].tolist() == [0, 1, 2, 3] and k['mask_iou'] == np.float32(2 / 8)
    k = main.mask_keys(ms, 1, 1)
    assert k['mask_area'] == sum(range(34, 50)) and k['mask_box'].tolist() == [12, 13, 14, 15] and k['mask_iou'] == 1.0
    assert np.isnan(main.mask_keys(ms, 0, 1)['mask_iou']) and main.mask_keys(ms, 1, 0)['mask_iou'] == 0.0
    assert 'mask_iou' not in main.mask_keys(dict(ms, agree=None), 0, 0)
    # the entry points refuse before they touch the model (a stub stands for it)
    acr = main.ACR.__new__(main.ACR)
    acr.hands_per_side = 1
    frames = torch.zeros(1, 512, 512, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match='masks must be'):
        acr.forward_batch(frames, ['a'], masks='yes')
    with pytest.raises(ValueError, match='render='):
        acr.forward_batch(frames, ['a'], show_items=('segm',))
    with pytest.raises(ValueError, match='over regions'):
        acr.forward_raw_batch(frames, ['a'], render=True, show_items=('pj2d', 'segm'), boxes=[[0, 0, 64, 64]])
    with pytest.raises(ValueError, match='over regions'):
        acr.forward_raw_batch(frames, ['a'], render=True, show_items=('segm',), boxes=[[0, 0, 64, 64]], region_views=True)
    with pytest.raises(ValueError, match='over regions'):
        acr.forward_raw_batch(frames, ['a'], masks=True, boxes=[[0, 0, 64, 64]])
    with pytest.raises(ValueError, match='over regions'):
        acr.forward_raw_batch(frames, ['a'], masks='iou', boxes=[[0, 0, 64, 64]])
    with pytest.raises(ValueError, match='over regions'):
        acr.track_raw_batch(frames, ['a'], render=True, show_items=('segm',))


def test_plan_stand_alone_program(tmp_path):
    """tools/segm_check.cpp: csrc/segm_plan.h against a plain restatement as a program of its own.  The plain build must pass;
    the build with the address and undefined-behaviour sanitizers must pass as well where the host compiler can make one that
    starts - which of the two ran is printed."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        assert os.path.exists(hipcc), 'no C++ compiler'
        cmd = [hipcc, '-x', 'c++']
    else:
        cmd = [cxx]
    src = os.path.join(ROOT, 'tools', 'segm_check.cpp')
    cmd += ['-std=c++17', '-O1', '-g', '-ffp-contract=off', src, '-o']
    plain = str(tmp_path / 'segm_check')
    subprocess.run(cmd + [plain], check=True, capture_output=True)
    run = subprocess.run([plain], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    ran = None
    for label, extra in (('static', san + ['-static-libasan', '-static-libubsan']), ('shared', san)):
        exe = str(tmp_path / ('segm_check_' + label))
        if subprocess.run(cmd + [exe] + extra, capture_output=True).returncode != 0:
            continue
        run = subprocess.run([exe], capture_output=True, text=True)
        if 'does not come first in initial library list' in run.stderr:
            continue
        ran = label
        assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
        break
    print('sanitizer variant that ran: %s' % ran)
