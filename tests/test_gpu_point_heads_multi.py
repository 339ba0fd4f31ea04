"""GPU: the point heads at the K best centres of each side (ACRMI_OPT_POINT_HEADS_MULTI, acrmi_point_heads_multi; DESIGN.md
section 17).  The towers run at the pixels of csrc/point_plan.h - tests/point_ref.py restates them - and the top-K decode of
what they wrote is the decode of the dense maps: flags, centres and scores exactly, the rest within the bounds
tests/test_gpu_network.py uses for the same towers against the same dense maps (the arithmetic per point is the same).
`pytest -m gpu`."""
import numpy as np
import pytest
import torch

import multi_ref as M
import point_ref as P
from conftest import pkg

pytestmark = pytest.mark.gpu

NAN = float('nan')


def bits(t):
    return t.contiguous().cpu().view(torch.int32)


@pytest.fixture(scope='module')
def engine4(synth_sd, mano_tables, frames2):
    """One fp32 W32 engine for batches of 4, four synthetic frames and their offsets rows."""
    e = pkg('engine').Engine(0)
    e.load_state_dict(synth_sd, max_batch=4)
    e.load_mano(mano_tables)
    img = torch.from_numpy(np.stack([frames2[0], frames2[1], frames2[1], frames2[0]])).cuda()
    offsets = torch.tensor([[512., 512, 0, 0, 0, 0, 0, 0, 0, 0], [640., 512, 64, 64, 0, 0, 0, 0, 0, 0]]).repeat(2, 1)
    assert e.has_point_heads
    yield e, img, offsets
    e.close()


def _poison(eng, B):
    hl = eng.program['heads']
    for s in (0, 1):      # whatever the point variant does not write must not be read either
        eng.buffer(hl.params_buf[s], B).fill_(NAN)
        eng.buffer(hl.prior_buf[s], B).fill_(NAN)


# ---- 1: planted peaks ------------------------------------------------------------------------------------------------------------
# per scene two frames of (left peaks, right peaks), (y, x, height): distinct heights above the threshold, >= 3 px apart
SCENES = {
    'corners, borders, close lefts, a shared right, a far left, fewer rights than K': [
        ([(0, 0, 0.95), (0, 63, 0.9), (63, 0, 0.85), (63, 63, 0.8)], [(0, 30, 0.95), (31, 0, 0.9), (63, 33, 0.85), (30, 63, 0.8)]),
        # lefts 3 px apart (their 9 x 9 windows overlap), both nearest to the one right; a left > 32 px from it
        ([(20, 20, 0.9), (20, 23, 0.8), (60, 60, 0.7)], [(22, 30, 0.9)]),
    ],
    'no peak on one side, a flagged peak at pixel 0 with placeholders': [
        ([], [(0, 0, 0.9)]),
        ([(0, 0, 0.9), (10, 10, 0.8)], [(5, 5, 0.7)]),
    ],
}


def _planted(scene):
    maps = np.zeros((2, 2, M.MAP, M.MAP), np.float32)      # [frame, side]
    for b, sides in enumerate(scene):
        for s, peaks in enumerate(sides):
            for i, (y, x, a) in enumerate(peaks):
                assert a > M.CONF_THRESH and all(max(abs(y - q[0]), abs(x - q[1])) >= 3 and a != q[2] for q in peaks[:i])
                maps[b, s, y, x] = a
    return maps


@pytest.mark.parametrize('name', sorted(SCENES))
def test_planted_peaks(engine4, name):
    eng, img, _ = engine4
    L = pkg('_lib')
    hl = eng.program['heads']
    maps = _planted(SCENES[name])
    B = eng.backbone_heads(img[:2])
    assert eng.conf_thresh == M.CONF_THRESH
    for s in (0, 1):
        eng.buffer(hl.center_buf[s], B, 1).copy_(torch.from_numpy(maps[:, s, :, :, None]).cuda())
    dense = [(eng.buffer(hl.params_buf[s], B).clone(), eng.buffer(hl.prior_buf[s], B).clone()) for s in (0, 1)]
    kinds = set()
    for K in (2, 3, 8):
        for s in (0, 1):
            eng.buffer(hl.params_buf[s], B).copy_(dense[s][0])
            eng.buffer(hl.prior_buf[s], B).copy_(dense[s][1])
        want = eng.decode(B, max_hand=K).clone()
        _poison(eng, B)
        eng.run_point_heads(B, max_hand=K)
        got = eng.decode(B, max_hand=K)
        torch.cuda.synchronize()
        want, got = want.cpu().numpy(), got.cpu().numpy()
        for key in (L.SLOT_FLAG, L.SLOT_FLATIND, L.SLOT_SCORE):
            np.testing.assert_array_equal(got[..., key], want[..., key])
        assert not np.isnan(got).any()
        np.testing.assert_allclose(got, want, rtol=5e-5, atol=5e-5)
        for b in range(B):
            flag, flat, partner, plan = P.plan_of_maps(maps[b, 0], maps[b, 1], K)
            np.testing.assert_array_equal(want[b, :, :, L.SLOT_FLAG] > 0.5, flag)
            np.testing.assert_array_equal(want[b, :, :, L.SLOT_FLATIND], flat)
            for s in (0, 1):
                # the pixels that are no longer NaN are the lists, whole: nothing else was written
                par = eng.buffer(hl.params_buf[s], B, 109)[b].reshape(4096, 109).isnan().cpu().numpy()
                pri = eng.buffer(hl.prior_buf[s], B, 106)[b].reshape(4096, 106).isnan().cpu().numpy()
                assert np.flatnonzero(~par.all(1)).tolist() == sorted(plan['own'][s]), (K, b, s)
                assert np.flatnonzero(~par.any(1)).tolist() == sorted(plan['own'][s]), (K, b, s)
                assert np.flatnonzero(~pri.all(1)).tolist() == sorted(plan['prior'][s]), (K, b, s)
                assert np.flatnonzero(~pri.any(1)).tolist() == sorted(plan['prior'][s]), (K, b, s)
                if flag[:, s].any() and not flag[:, s].all():
                    kinds.add('fewer peaks than K')
                if not flag[:, s].any():
                    kinds.add('no peak')
                if (flag[:, s] & (flat[:, s] == 0)).any() and not flag[:, s].all():
                    kinds.add('flagged pixel 0 with placeholders')
                if len(plan['prior'][s]) < (partner[:, s] >= 0).sum():
                    kinds.add('shared partner')
                if (flag[:, s] & (partner[:, s] < 0)).any() and flag[:, 1 - s].any():
                    kinds.add('nobody within 32 px')
    expected = {'fewer peaks than K', 'shared partner', 'nobody within 32 px'} if name.startswith('corners') else \
        {'fewer peaks than K', 'no peak', 'flagged pixel 0 with placeholders', 'shared partner'}
    assert kinds >= expected, kinds
    # K = 1 of the plan writes the bits of the classic point heads
    _poison(eng, B)
    eng.run_point_heads(B)
    classic = eng.decode(B).clone()
    _poison(eng, B)
    pkg('_lib').check(eng.L.acrmi_point_heads_multi(eng.ctx, B, 1, None), eng.ctx)
    torch.cuda.synchronize()
    assert torch.equal(bits(eng.decode(B)), bits(classic))


# ---- 2 - 4: the fused calls ------------------------------------------------------------------------------------------------------
def _threshold(eng, img, K):
    """A threshold under the K-th survivor of one map and over the K-th of another: ranks with and without a detection."""
    B = eng.backbone_heads(img)
    cm = eng.center_maps(B).cpu().numpy()
    kth = sorted(float(np.sort(M.nms_det(cm[b, h]).reshape(-1))[::-1][K - 1]) for b in range(B) for h in (0, 1))
    assert kth[0] < kth[-1], 'the maps of the synthetic checkpoint do not separate'
    return float(np.float32((kth[0] + kth[-1]) / 2))


def _assert_point_matches_dense(pt, dense):
    L = pkg('_lib')
    ps, ds = pt['slots'].cpu().numpy(), dense['slots'].cpu().numpy()
    for key in (L.SLOT_FLAG, L.SLOT_FLATIND, L.SLOT_SCORE):
        np.testing.assert_array_equal(ps[..., key], ds[..., key])
    np.testing.assert_allclose(ps[..., L.SLOT_PARAMS:L.SLOT_PARAMS + 109], ds[..., L.SLOT_PARAMS:L.SLOT_PARAMS + 109],
                               rtol=5e-5, atol=5e-5)
    assert not torch.isnan(pt['verts']).any() and not torch.isnan(pt['slots']).any()
    assert (pt['verts'] - dense['verts']).abs().max().item() < 2e-5
    assert (pt['joints'] - dense['joints']).abs().max().item() < 2e-5


@pytest.mark.parametrize('K', (2, 4))
def test_fused_calls_match_the_dense_heads(engine4, K):
    eng, img, offsets = engine4
    E, L = pkg('engine'), pkg('_lib')
    B = 4
    old = eng.conf_thresh
    eng.set_conf_thresh(_threshold(eng, img, K))
    tables = [E.TrackTable(0, 2, K, gate=128) for _ in range(2)]
    tracks = [0, 1, 0, -1]
    try:
        dense = {k: v.clone() for k, v in eng.forward(img, offsets=offsets, project=True, max_hand=K).items()}
        dense_t = {k: v.clone() for k, v in eng.forward(img, offsets=offsets, project=True, max_hand=K, tracks=tracks,
                                                        track_table=tables[0]).items()}
        flags = dense['slots'][..., L.SLOT_FLAG] > 0.5
        assert flags.any() and not flags.all()
        assert eng.set_point_heads_multi(True) is True and eng.point_heads_multi is True
        try:
            _poison(eng, B)
            pt = {k: v.clone() for k, v in eng.forward(img, offsets=offsets, project=True, max_hand=K).items()}
            _poison(eng, B)
            pt_t = {k: v.clone() for k, v in eng.forward(img, offsets=offsets, project=True, max_hand=K, tracks=tracks,
                                                         track_table=tables[1]).items()}
            torch.cuda.synchronize()
        finally:
            assert eng.set_point_heads_multi(False) is False
        assert sorted(pt) == sorted(dense) and tuple(pt['slots'].shape) == (B, K, 2, L.SLOT)
        _assert_point_matches_dense(pt, dense)
        _assert_point_matches_dense(pt_t, dense_t)
        assert torch.equal(pt_t['track_ids'], dense_t['track_ids'])
        again = eng.forward(img, offsets=offsets, project=True, max_hand=K)      # the dense program repairs the poisoned maps
        for k in dense:
            assert torch.equal(bits(again[k]), bits(dense[k])), k
    finally:
        eng.set_conf_thresh(old)
        for t in tables:
            t.close()


def _forward_multi(eng, img, offsets, K):
    """acrmi_forward_multi itself (Engine.forward takes acrmi_forward at max_hand = 1)."""
    B = img.shape[0]
    shape = (B, K, 2)
    got = {'slots': torch.empty(shape + (176,)), 'verts': torch.empty(shape + (778, 3)), 'joints': torch.empty(shape + (21, 3)),
           'verts_camed': torch.empty(shape + (778, 3)), 'pj2d': torch.empty(shape + (21, 2)), 'pj2d_org': torch.empty(shape + (21, 2))}
    got = {k: v.cuda() for k, v in got.items()}
    off_dev = offsets.cuda()
    pkg('_lib').check(eng.L.acrmi_forward_multi(eng.ctx, img.data_ptr(), B, K, off_dev.data_ptr(),
                                                *[got[k].data_ptr() for k in ('slots', 'verts', 'joints', 'verts_camed', 'pj2d',
                                                                              'pj2d_org')], None), eng.ctx)
    torch.cuda.synchronize()
    return got


def test_bit_equalities(engine4):
    eng, img, offsets = engine4
    kw = dict(offsets=offsets, project=True)
    # one hand per side through acrmi_forward_multi with the option = acrmi_forward with ACRMI_OPT_POINT_HEADS
    eng.set_point_heads(True)
    try:
        classic = {k: v.clone().unsqueeze(1) for k, v in eng.forward(img, **kw).items()}
        dense2 = {k: v.clone() for k, v in eng.forward(img, max_hand=2, **kw).items()}      # ACRMI_OPT_POINT_HEADS is not looked at
    finally:
        eng.set_point_heads(False)
    want2 = eng.forward(img, max_hand=2, **kw)
    for k in want2:
        assert torch.equal(bits(dense2[k]), bits(want2[k])), k
    eng.set_point_heads_multi(True)
    try:
        one = _forward_multi(eng, img, offsets, 1)
        for k in classic:
            assert torch.equal(bits(one[k]), bits(classic[k])), k
        first = {k: v.clone() for k, v in eng.forward(img, max_hand=3, **kw).items()}
        second = {k: v.clone() for k, v in eng.forward(img, max_hand=3, **kw).items()}
        eng.set_lanes(1)
        try:
            single = {k: v.clone() for k, v in eng.forward(img, max_hand=3, **kw).items()}
        finally:
            eng.set_lanes(0)
        torch.cuda.synchronize()
    finally:
        eng.set_point_heads_multi(False)
    for k in first:
        assert torch.equal(bits(second[k]), bits(first[k])), k
        assert torch.equal(bits(single[k]), bits(first[k])), k
    eng.forward(img, **kw)


def test_queued_calls_do_not_wait_for_the_device(engine4):
    eng, img, offsets = engine4
    K = 2
    off_dev = offsets.cuda()
    eng.set_point_heads_multi(True)
    try:
        warm = eng.forward(img, offsets=off_dev, project=True, max_hand=K)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            with pytest.raises(RuntimeError):
                warm['slots'].sum().item()      # the mode is honoured by this build
            outs = [eng.forward(img, offsets=off_dev, project=True, max_hand=K) for _ in range(3)]
        finally:
            torch.cuda.set_sync_debug_mode('default')
        torch.cuda.synchronize()
    finally:
        eng.set_point_heads_multi(False)
    for o in outs:
        assert torch.equal(bits(o['slots']), bits(warm['slots']))
    eng.forward(img, offsets=off_dev)


# ---- 5: programs without point-heads ops ---------------------------------------------------------------------------------------
def test_a_program_without_point_heads_stays_dense(synth_sd, mano_tables, frames2):
    E, L, cfg = pkg('engine'), pkg('_lib'), pkg('config')
    eng = E.Engine(0)
    eng.load_state_dict(synth_sd, max_batch=2, precision='fp16')
    try:
        assert not eng.has_point_heads
        assert eng.set_point_heads_multi(True) is False and eng.point_heads_multi is False
        assert eng.L.acrmi_set_option(eng.ctx, L.OPT_POINT_HEADS_MULTI, 1) == L.E_INVAL
        assert b'no point-heads ops' in eng.L.acrmi_last_error(eng.ctx)
        assert eng.L.acrmi_set_option(eng.ctx, L.OPT_POINT_HEADS_MULTI, 0) == 0
        B = eng.backbone_heads(torch.from_numpy(frames2).cuda())
        assert eng.L.acrmi_point_heads_multi(eng.ctx, B, 2, None) == L.E_INVAL
        assert b'acrmi_point_heads_multi' in eng.L.acrmi_last_error(eng.ctx)
        with pytest.raises(ValueError, match='acrmi_point_heads_multi: the program has no point-heads ops'):
            eng.run_point_heads(B, max_hand=2)
    finally:
        eng.close()
    acr = pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml', '--model_precision', 'fp16']),
                              state_dict=synth_sd, mano_tables=mano_tables, max_batch=2)
    x = torch.from_numpy(frames2).cuda()
    want = acr.forward_batch(x, ['a', 'b'], max_hand=2)
    got = acr.forward_batch(x, ['a', 'b'], max_hand=2, multi_point_heads=True)
    assert sorted(got) == sorted(want)
    n = 0
    for path in want:
        assert len(got[path]) == len(want[path])
        for g, w in zip(got[path], want[path]):
            assert sorted(g) == sorted(w)
            for k in w:
                np.testing.assert_array_equal(np.asarray(g[k]), np.asarray(w[k]))
            n += 1
    assert n > 0
