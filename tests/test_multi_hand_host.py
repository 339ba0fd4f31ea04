"""Several hands of each side per frame, the parts that need no GPU: the numpy statement of the top-K
rule (tests/multi_ref.py) against the reference's own parser (decode_topk.npz) and against the oracle at K = 1, the partner
rule on hand-made cases, the new C entry points, the config key and the packaging of the result dicts."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cases
import multi_ref as mr
from conftest import ROOT, golden, pkg
from oracle import decode as odec


# ---- 1. the reference's parser with K = max_hand ----------------------------------------------------------------------------
@pytest.mark.parametrize('K', mr.TOPK_KS)
def test_numpy_rule_equals_reference_topk(K):
    """CenterMap.parse_centermap_heatmap_adaptive_scale_batch(train_flag=True, max_hand=K) on the seeded maps: its batch_ids,
    flat indices and scores are the flagged ranks of the rule, frame by frame in rank order - exactly."""
    g = golden('decode_topk.npz')
    seen = set()
    for name in mr.TOPK_CASES:
        maps, counts = mr.topk_case_maps(name)
        ids, inds, scores = [], [], []
        for b, m in enumerate(maps):
            flag, flat, score = mr.topk(m[0], K)
            assert int(flag.sum()) == min(counts[b], K)
            assert not flat[~flag].any() and ((flat >= 0) & (flat < 4096)).all()
            ids += [b] * int(flag.sum())
            inds += flat[flag].tolist()
            scores += score[flag].tolist()
            seen.add('none' if counts[b] == 0 else 'fewer' if counts[b] < K else 'exactly' if counts[b] == K else 'more')
        np.testing.assert_array_equal(np.asarray(ids, np.int64), g['%s_k%d_batch_ids' % (name, K)])
        np.testing.assert_array_equal(np.asarray(inds, np.int64), g['%s_k%d_inds' % (name, K)])
        np.testing.assert_array_equal(np.asarray(scores, np.float32), g['%s_k%d_scores' % (name, K)])
    # the maps hold every regime: no detection, 1..K-1 (there is no such count for K = 1), exactly K, more than K
    assert seen == ({'none', 'exactly', 'more'} | ({'fewer'} if K > 1 else set()))


# ---- 2. K = 1 is the per-frame decode -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(cases.DECODE_CASES))
def test_numpy_rule_at_k1_equals_oracle_decode(name):
    maps = cases.decode_maps(name)
    want = odec.decode({k: torch.from_numpy(v) for k, v in maps.items()})
    got = mr.decode_multi(maps, 1)
    np.testing.assert_array_equal(got['flag'][:, 0], want['flag'])
    np.testing.assert_array_equal(got['flat_ind'][:, 0], want['flat_ind'])
    np.testing.assert_array_equal(got['score'][:, 0], want['score'])
    np.testing.assert_array_equal(got['params_pred'][:, 0], want['params_pred'])


# ---- 3. the partner rule ------------------------------------------------------------------------------------------------------
def _yx(*pts):
    return [y * 64 + x for y, x in pts]


def _partners(left, right, K):
    """left / right: lists of (y, x) in rank order -> partner [K,2] as (y, x) tuples or None."""
    flag = np.zeros((K, 2), bool)
    flat = np.zeros((K, 2), np.int64)
    for h, pts in enumerate((left, right)):
        flag[:len(pts), h] = True
        flat[:len(pts), h] = _yx(*pts)
    p = mr.partners(flag, flat)
    return [[None if p[k, h] < 0 else (int(p[k, h]) // 64, int(p[k, h]) % 64) for h in (0, 1)] for k in range(K)]


def test_partner_rule_on_hand_made_cases():
    # a distance of exactly 32 keeps the prior; d^2 = 1025 (32, 1) does not
    assert _partners([(0, 0)], [(0, 32)], 1) == [[(0, 32), (0, 0)]]
    assert _partners([(0, 0)], [(1, 32)], 1) == [[None, None]]
    # the nearest of two, whatever its rank
    assert _partners([(10, 10)], [(40, 40), (12, 14)], 2) == [[(12, 14), None], [None, (10, 10)]]
    # a tie in distance: the lower rank
    assert _partners([(20, 20)], [(20, 25), (20, 15)], 2)[0][0] == (20, 25)
    assert _partners([(20, 20)], [(20, 15), (20, 25)], 2)[0][0] == (20, 15)
    # asymmetric: L0's partner is R0, R0's partner is L1 (nearer to it), and R1 is too far from every left hand
    got = _partners([(10, 10), (10, 30)], [(10, 22), (60, 60)], 2)
    assert got[0] == [(10, 22), (10, 30)] and got[1] == [(10, 22), None]
    # one side empty: nobody has a partner; an unflagged rank never has one
    assert _partners([(5, 5), (30, 30)], [], 2) == [[None, None], [None, None]]
    assert _partners([(5, 5)], [(6, 6)], 3)[1:] == [[None, None], [None, None]]


def test_prior_is_added_at_the_partner_centre():
    """decode_multi on planted peaks: the own params at the own centre, plus the own prior map at the partner's centre in
    params[3:] - and nothing for the hand whose nearest partner is 33 pixels away."""
    cl = np.zeros((1, 1, 64, 64), np.float32)
    cr = np.zeros((1, 1, 64, 64), np.float32)
    cl[0, 0, 10, 10], cl[0, 0, 50, 5] = 0.9, 0.8
    cr[0, 0, 10, 20], cr[0, 0, 50, 38] = 0.7, 0.6
    maps = mr.head_maps(cl, cr, seed=5)
    d = mr.decode_multi(maps, 2)
    assert d['flag'].all()
    assert d['flat_ind'][0].tolist() == [_yx((10, 10), (10, 20)), _yx((50, 5), (50, 38))]
    assert d['partner'][0].tolist() == [_yx((10, 20), (10, 10)), [-1, -1]]
    own = maps['l_params_maps'][0, :, 10, 10]
    np.testing.assert_array_equal(d['params_pred'][0, 0, 0, :3], own[:3])
    np.testing.assert_array_equal(d['params_pred'][0, 0, 0, 3:], own[3:] + maps['l_prior_maps'][0, :, 10, 20])
    np.testing.assert_array_equal(d['params_pred'][0, 1, 1], maps['r_params_maps'][0, :, 50, 38])


# ---- 4. the C boundary --------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_additive():
    L = pkg('_lib')
    src = open(os.path.join(ROOT, 'include', 'acrmi.h')).read()
    for name in ('acrmi_decode_multi', 'acrmi_decode_maps_multi', 'acrmi_forward_multi'):
        assert re.search(r'\b%s\s*\(' % name, src) and name in L.EXPORTS and hasattr(L.lib(), name)
    assert re.search(r'#define ACRMI_MAX_HAND (\d+)', src).group(1) == str(L.MAX_HAND) == '8'
    assert re.search(r'#define ACRMI_VERSION (\d+)', src).group(1) == '303' and L.lib().acrmi_version() == L.VERSION == 303


def test_bad_arguments_are_refused_without_a_gpu():
    """Nothing here reaches a HIP call.  (ACRMI_OPT_BATCH_PRIOR / ACRMI_OPT_TEMPORAL with max_hand > 1 need a context, and a
    context needs a device: tests/test_gpu_multi_hand.py.)"""
    L = pkg('_lib')
    lib = L.lib()
    p = ctypes.c_void_p(64)      # never read: max_hand is checked first
    for K in (0, 9, -1):
        assert lib.acrmi_decode_maps_multi(p, p, 1, p, p, 109, p, p, 106, 1, K, 0.35, p, None) == L.E_INVAL
        assert b'max_hand' in lib.acrmi_last_error(None)
    assert lib.acrmi_decode_maps_multi(None, None, 1, None, None, 109, None, None, 106, 1, 2, 0.35, None, None) == L.E_INVAL
    assert lib.acrmi_decode_maps_multi(p, p, 1, p, p, 109, p, p, 106, 1, 2, 0.35, None, None) == L.E_INVAL      # no slots
    assert lib.acrmi_decode_maps_multi(p, p, 1, p, p, 108, p, p, 106, 1, 2, 0.35, p, None) == L.E_INVAL         # params_cs < 109
    assert lib.acrmi_decode_multi(None, 1, 2, None, None) == L.E_INVAL
    assert lib.acrmi_forward_multi(None, None, 1, 2, None, None, None, None, None, None, None, None) == L.E_INVAL
    ops, engine = pkg('ops'), pkg('engine')
    for K in (0, 9, 1.5):
        with pytest.raises(ValueError):
            engine.check_max_hand(K)
    assert engine.check_max_hand(8) == 8
    z = torch.zeros(1, 64, 64, 1)
    with pytest.raises((ValueError, pkg('_lib').AcrmiError)):      # host tensors: refused before the library is called
        ops.decode_maps_multi(z, z, z, z, z, z, 2)


# ---- 5. config and packaging --------------------------------------------------------------------------------------------------
def test_hands_per_side_is_validated_and_max_hand_stays_unread():
    cfg = pkg('config')
    base = ['--configs_yml', '/nonexistent.yml']
    assert cfg.parse_args(base).hands_per_side == 1
    assert cfg.parse_args(base + ['--hands_per_side', '8']).hands_per_side == 8
    for bad in ('0', '9', '-1'):
        with pytest.raises(ValueError):
            cfg.parse_args(base + ['--hands_per_side', bad])
    import argparse
    for bad in (2.0, True, '2', None):
        ns = argparse.Namespace(**copy.deepcopy(cfg.DEFAULTS))
        ns.hands_per_side = bad
        with pytest.raises(ValueError):
            cfg.validate(ns)
    ns = cfg.parse_args(base + ['--max_hand', '4'])      # the reference's training-time key: parsed, carried, not wired
    assert ns.max_hand == 4 and ns.hands_per_side == 1


def _fabricated_out(B, K, flags, multi=True):
    g = mr.rng(3)
    L = pkg('_lib')
    lead = (B, K, 2) if multi else (B, 2)
    out = {'slots': g.normal(0, 1, lead + (L.SLOT,)).astype(np.float32),
           'verts': g.normal(0, 1, lead + (778, 3)).astype(np.float32), 'joints': g.normal(0, 1, lead + (21, 3)).astype(np.float32),
           'pj2d': g.normal(0, 1, lead + (21, 2)).astype(np.float32), 'pj2d_org': g.normal(0, 100, lead + (21, 2)).astype(np.float32),
           'cam_trans': g.normal(0, 1, lead + (3,)).astype(np.float32)}
    out['slots'][..., L.SLOT_FLAG] = np.asarray(flags, np.float32).reshape(lead)
    return out


def test_result_dicts_list_lefts_then_rights_in_rank_order():
    """acr.main.results_from_out on a fabricated result: the flagged lefts by rank, then the flagged rights by rank
    (torch.cat((l, r)) of the reference), fp16 casts of the slots and the MANO outputs; {} for an empty frame."""
    L = pkg('_lib')
    main = pkg('acr.main')
    #         pair 0      pair 1      pair 2      (left, right)
    flags = [[[1, 0], [0, 1], [1, 1]],      # frame 0: L0 L2 R1 R2
             [[0, 0], [0, 0], [0, 0]],      # frame 1: nothing
             [[0, 1], [1, 0], [0, 0]]]      # frame 2: L1 R0
    out = _fabricated_out(3, 3, flags)
    res = main.results_from_out({k: torch.from_numpy(v) for k, v in out.items()}, ['a', 'b', 'c'])
    assert res['b'] == {}
    want = {'a': [(0, 0), (2, 0), (1, 1), (2, 1)], 'c': [(1, 0), (0, 1)]}
    for b, path in ((0, 'a'), (2, 'c')):
        assert [int(h['hand_type']) for h in res[path]] == [h for _, h in want[path]]
        for hand, (k, h) in zip(res[path], want[path]):
            s = out['slots'][b, k, h]
            np.testing.assert_array_equal(hand['cam'], s[L.SLOT_CAM:L.SLOT_CAM + 3].astype(np.float16))
            np.testing.assert_array_equal(hand['poses'], s[L.SLOT_POSES:L.SLOT_POSES + 48].astype(np.float16))
            np.testing.assert_array_equal(hand['betas'], s[L.SLOT_BETAS:L.SLOT_BETAS + 10].astype(np.float16))
            for key, src in (('verts', 'verts'), ('j3d', 'joints'), ('pj2d', 'pj2d'), ('pj2d_org', 'pj2d_org'), ('cam_trans', 'cam_trans')):
                np.testing.assert_array_equal(hand[key], out[src][b, k, h].astype(np.float16))
            assert hand[key].dtype == np.float16 and hand['detection_flag_cache'] is True
    # one pair per frame in the old [B,2,...] shape: left, right
    one = _fabricated_out(2, 1, [[1, 1], [0, 1]], multi=False)
    res = main.results_from_out(one, ['p', 'q'])
    assert [int(h['hand_type']) for h in res['p']] == [0, 1] and [int(h['hand_type']) for h in res['q']] == [1]
    np.testing.assert_array_equal(res['q'][0]['verts'], one['verts'][1, 1].astype(np.float16))
    with pytest.raises(ValueError):
        main.results_from_out(one, ['p'])
