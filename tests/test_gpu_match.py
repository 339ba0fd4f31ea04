"""Matching decoded hands to ground truth on the GPU (csrc/match.hip) against the numpy restatement
(tests/match_ref.py) FOR EQUALITY: match, pred_of, the bits of cost, counts, group, the gathered rows and the board - there is
no tolerance here.  Then the engine level: Engine.match + Engine.score, EnginePool.match and forward_batch(match=) against the
operators on the same tensors."""
import itertools

import numpy as np
import pytest
import torch

import match_ref as R
from conftest import pkg
from contact_cases import eng, frames3, near_sd, placed      # (fixtures)
from test_gpu_score import by_operator

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
INF = float('inf')
KEYS = ('match', 'pred_of', 'cost', 'counts', 'group')


def cuda(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def assert_equal(got, want, what=''):
    for k in KEYS:
        a = got[k].cpu().numpy() if hasattr(got[k], 'cpu') else got[k]
        b = want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (what, k, np.argwhere(a.view(np.int32) != b.view(np.int32))[:4])


def make_case(seed, B, K, G, n, D, variant):
    """The inputs of one operator call as host arrays.  Truths are clouds around random centres 0..100 apart; the predictions
    are the truths in another order - some exactly, some moved by noise - and clouds of their own.  variant (a counter) decides
    which optional arrays there are, the gate and min_points; from B >= 3 on there are NaN / inf / 3e19 coordinates and trans
    and flags of arbitrary bit patterns."""
    g = np.random.default_rng(seed)
    centre = g.uniform(0, 100, (B, G, 2, 1, D))
    truth = (centre + g.normal(0, 2, (B, G, 2, n, D))).astype(np.float32)
    pred = (g.uniform(0, 100, (B, K, 2, 1, D)) + g.normal(0, 2, (B, K, 2, n, D))).astype(np.float32)
    trans = g.normal(0, 3, (B, K, 2, D)).astype(np.float32) if variant & 4 else None
    for b, s in itertools.product(range(B), range(2)):
        order = g.permutation(G)
        for i in range(min(K, G)):
            kind = g.integers(0, 4)
            if kind == 0:
                continue      # a prediction of its own
            pred[b, i, s] = truth[b, order[i], s]
            if kind == 1:     # moved by noise; else an exact copy (the only pairs gate 0 allows)
                pred[b, i, s] += g.normal(0, 1, (n, D)).astype(np.float32)
            elif trans is not None and kind == 2:
                trans[b, i, s] = 0
    c = dict(pred=pred, truth=truth, flags=(g.random((B, K, 2)) < 0.8).astype(np.float32), trans=trans,
             valid=g.choice(np.array([0, 1, 1, 1, 7, 255], np.uint8), (B, G, 2, n)) if variant & 1 else None,
             truth_valid=g.choice(np.array([0, 1, 1, 255], np.uint8), (B, G, 2)) if variant & 2 else None,
             group=g.integers(-3, 20, (B, G, 2)).astype(np.int32) if variant & 8 else None,
             gate=(INF, 30.0, 0.0)[variant % 3], min_points=1 if (variant // 3) % 2 == 0 else n)
    if c['valid'] is not None:
        c['valid'][:, 0] = 1      # (a truth whose every point may count: min_points = n leaves something)
    if variant & 16:
        c['flags'] = None
    if B >= 3:
        pred[0, 0, 0, g.integers(0, n), 1] = np.nan
        truth[1, 0, 1, g.integers(0, n), 0] = np.inf
        pred[2, K - 1, 1, g.integers(0, n), D - 1] = -np.inf
        pred[1, 0, 0] = pred[1, 0, 0] * np.float32(3e17)      # finite: counted, the cost is finite
        truth[2, G - 1, 0] = np.float32(3e19)
        if trans is not None:
            trans[0, K - 1, 1, 0] = np.nan
            trans[1, K - 1, 1, D - 1] = np.inf
            trans[2, 0, 0] = np.float32(3e19)
        if c['flags'] is not None:
            raw = g.integers(0, 256, 4 * B * K * 2, dtype=np.uint8).view(np.float32).reshape(B, K, 2)      # arbitrary bytes
            c['flags'][B // 2:] = raw[B // 2:]
            special = np.array([0x7fc00000, 0x3f000000, 0x7f800000, 0xff800000, 0x3f000001, 0x00000001, 0x3f800000, 0xbf800000],
                               np.uint32).view(np.float32)      # NaN, 0.5, inf, -inf, just above 0.5, a denormal, 1, -1
            flat = c['flags'].reshape(-1)
            flat[:min(8, flat.size)] = special[:min(8, flat.size)]
    return c


def run(c):
    return pkg('ops').match_hands(cuda(c['pred']), cuda(c['truth']), flags=cuda(c['flags']), valid=cuda(c['valid']),
                                  truth_valid=cuda(c['truth_valid']), trans=cuda(c['trans']), group=cuda(c['group']), gate=c['gate'],
                                  min_points=c['min_points'])


def reference(c):
    return R.match_hands(c['pred'], c['truth'], flags=c['flags'], valid=c['valid'], truth_valid=c['truth_valid'], trans=c['trans'],
                         group=c['group'], gate=c['gate'], min_points=c['min_points'])


KG = [(1, 1), (1, 8), (8, 1), (2, 3), (4, 4), (5, 8), (8, 8)]


@pytest.mark.parametrize('B', [1, 3, 67])
@pytest.mark.parametrize('K,G', KG)
def test_operator_equals_the_rule(K, G, B):
    matched = 0
    for idx, (n, D) in enumerate(itertools.product((1, 21, 64, 65, 256), (2, 3))):
        variant = idx * 7 + K + 3 * G + B      # walks through the optional arrays, the three gates and both min_points
        c = make_case(1000 * K + 100 * G + B + idx, B, K, G, n, D, variant)
        got, want = run(c), reference(c)
        assert_equal(got, want, (K, G, B, n, D, variant))
        matched += int((want['match'] >= 0).sum())
        tp = want['counts'][:, :, 0]
        assert np.array_equal(tp, (want['match'] >= 0).sum(1)) and np.array_equal(tp, (want['pred_of'] >= 0).sum(1))
    assert matched > 0


@pytest.mark.parametrize('variant', range(32))
def test_every_combination_of_optional_arrays(variant):
    """With and without valid (1), truth_valid (2), trans (4), group (8) and flags (16), at K != G and three frames."""
    for gate, mp, D in ((INF, 1, 2), (30.0, 1, 3), (0.0, 21, 2)):
        c = make_case(50 + variant, 3, 3, 4, 21, D, variant)
        c['gate'], c['min_points'] = gate, mp
        assert_equal(run(c), reference(c), (variant, gate, mp))


@pytest.mark.parametrize('K,G', [(4, 4), (8, 8), (5, 8), (8, 3)])
def test_exact_ties_show_the_tie_order(K, G):
    """Integer-grid points with n = 1: many pairs of equal cost, identical truths and identical predictions."""
    g = np.random.default_rng(K * 9 + G)
    for D in (2, 3):
        pred = g.integers(0, 3, (16, K, 2, 1, D)).astype(np.float32)
        truth = g.integers(0, 3, (16, G, 2, 1, D)).astype(np.float32)
        truth[1] = truth[1, :1]                # identical truths
        pred[2] = pred[2, :1]                  # identical predictions
        truth[3], pred[3] = 1, 1               # everything identical: every cost 0
        pred[4, :min(K, G)] = truth[4, :min(K, G)]
        c = dict(pred=pred, truth=truth, flags=None, valid=None, truth_valid=None, trans=None, group=None, gate=INF, min_points=1)
        want = reference(c)
        assert_equal(run(c), want, ('ties', D))
        assert (want['counts'][:, :, 0] == min(K, G)).all() and (want['cost'][3][want['match'][3] >= 0] == 0).all()
        if K == G == 4:      # every cost equal: what the recurrence does with it (tests/test_match_host.py says why)
            assert want['match'][3, :, 0].tolist() == [3, 2, 1, 0]
        c['gate'] = 1.0                         # cost <= gate: exactly 1 is allowed, sqrt(2) is not
        assert_equal(run(c), reference(c), ('ties gated', D))


def test_nothing_to_match():
    c = make_case(7, 3, 4, 5, 21, 2, 3)
    c['flags'] = np.zeros((3, 4, 2), np.float32)      # no flagged prediction
    got, want = run(c), reference(c)
    assert_equal(got, want, 'no flag')
    assert (want['match'] == -1).all() and (want['counts'][:, :, :2] == 0).all() and (want['cost'] == -1).all()
    assert np.array_equal(want['counts'][:, :, 2], (c['truth_valid'] != 0).sum(1))
    c = make_case(8, 3, 4, 5, 21, 3, 2)
    c['truth_valid'][:] = 0                            # no valid truth
    got, want = run(c), reference(c)
    assert_equal(got, want, 'no truth')
    assert (want['pred_of'] == -1).all() and (want['group'] == -1).all() and (want['counts'][:, :, 2] == 0).all()
    assert np.array_equal(want['counts'][:, :, 1], R.finite_gt_half(c['flags']).sum(1))
    c = make_case(9, 3, 2, 2, 5, 2, 0)
    c['pred'][:] = np.nan                              # no finite point
    assert_equal(run(c), reference(c), 'nan')
    assert (reference(c)['match'] == -1).all()


def test_strided_flags_are_read_in_place():
    """slots[..., ACRMI_SLOT_FLAG] goes in as it is: a view with a stride of 176 floats."""
    L, ops = pkg('_lib'), pkg('ops')
    c = make_case(11, 3, 4, 3, 21, 2, 0)
    slots = torch.randn(3, 4, 2, L.SLOT, device='cuda')
    slots[..., L.SLOT_FLAG] = cuda(c['flags'])
    view = slots[..., L.SLOT_FLAG]
    assert ops._match_flags(view, 3, 4, view.device)[1] == L.SLOT and ops._match_flags(view, 3, 4, view.device)[0] is view
    got = ops.match_hands(cuda(c['pred']), cuda(c['truth']), flags=view, gate=c['gate'])
    assert_equal(got, reference(c), 'strided')
    odd = slots.permute(1, 0, 2, 3)[..., L.SLOT_FLAG]      # not a constant stride for [B,K,2]: copied
    assert ops._match_flags(odd, 4, 3, odd.device)[1] == 1


def test_a_frame_alone_equals_the_frame_in_a_batch_and_calls_repeat():
    c = make_case(21, 5, 5, 8, 21, 3, 15)
    whole, again = run(c), run(c)
    for k in KEYS:
        assert torch.equal(whole[k].view(torch.int32), again[k].view(torch.int32)), k
    for b in (0, 2, 4):
        one = {k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        got = run(one)
        for k in KEYS:
            assert torch.equal(got[k].view(torch.int32), whole[k][b:b + 1].view(torch.int32)), (b, k)


# ---- the gather ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W', [3, 63, 176, 2334])
def test_gather_equals_the_rule(W):
    L, ops = pkg('_lib'), pkg('ops')
    g = np.random.default_rng(W)
    B, Ks, Kd = 3, 3, 5
    src = g.integers(0, 2 ** 32, B * Ks * 2 * W + 1, dtype=np.uint32).view(np.float32)      # any bits, NaN among them
    index = g.integers(-1, Ks + 1, (B, Kd, 2)).astype(np.int32)
    index[0, 0], index[0, 1], index[1, 0], index[2, Kd - 1] = (-1, Ks), (INT_MIN, INT_MAX), (0, Ks - 1), (Ks - 1, 0)
    dev = torch.from_numpy(src).cuda()
    for off in (0, 1):      # off = 1: the base pointer is 4 bytes off a 16-byte boundary - the dword path also at W % 4 == 0
        s = dev[off:off + B * Ks * 2 * W].view(B, Ks, 2, W)
        assert s.data_ptr() % 16 == 4 * off and s.is_contiguous()
        got = ops.match_gather(s, cuda(index))
        want = R.gather(src[off:off + B * Ks * 2 * W].reshape(B, Ks, 2, W), index)
        assert got.shape == (B, Kd, 2, W) and np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), (W, off)
    # an unaligned destination, through the library itself; the words around it stay as they were
    s = dev[:B * Ks * 2 * W]
    room = torch.full((B * Kd * 2 * W + 2,), 7.0, device='cuda')
    ix = cuda(index)
    import ctypes
    rc = L.lib().acrmi_match_gather(ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(ix.data_ptr()), B, Ks, Kd, W,
                                    ctypes.c_void_p(room.data_ptr() + 4), None)
    torch.cuda.synchronize()
    assert rc == 0 and room[0] == 7 and room[-1] == 7
    want = R.gather(src[:B * Ks * 2 * W].reshape(B, Ks, 2, W), index)
    assert np.array_equal(room[1:-1].cpu().numpy().view(np.int32), want.reshape(-1).view(np.int32))
    # a tail of more than one dimension, K = 1 on either side
    s5 = torch.randn(2, 1, 2, 21, 3, device='cuda')
    got = ops.match_gather(s5, torch.tensor([[[0, -1]], [[5, 0]]], dtype=torch.int32).cuda())
    assert got.shape == (2, 1, 2, 21, 3) and torch.equal(got[0, 0, 0], s5[0, 0, 0]) and not got[0, 0, 1].any() and not got[1, 0, 0].any()
    assert torch.equal(got[1, 0, 1], s5[1, 0, 1])


# ---- the board -----------------------------------------------------------------------------------------------------------
def test_board_2B_in_one_call_equals_two_calls_of_B():
    E, ops = pkg('engine'), pkg('ops')
    c = make_case(31, 8, 4, 5, 21, 2, 3)
    res = run(c)
    want = reference(c)
    one, two, raw = E.MatchBoard(0), E.MatchBoard(0), E.MatchBoard(0)
    one.add(res)
    two.add({k: v[:4] for k, v in res.items()})
    two.add({k: v[4:] for k, v in res.items()})
    assert torch.equal(one.words, two.words)
    words = R.accumulate(np.zeros(8, np.int64), want['counts'], want['cost'])
    assert np.array_equal(one.words.cpu().numpy(), words)
    one.add(res)      # continues from its own values
    assert np.array_equal(one.words.cpu().numpy(), R.accumulate(words, want['counts'], want['cost']))
    ops.match_accumulate(raw.words, res['counts'], res['cost'])
    assert torch.equal(raw.words, two.words)
    s = two.summary()
    tp, fp, fn = (int(want['counts'][:, :, k].sum()) for k in range(3))
    assert (s['all']['tp'], s['all']['fp'], s['all']['fn']) == (tp, fp, fn) and tp > 0
    assert np.isclose(s['all']['precision'], tp / (tp + fp)) and np.isclose(s['all']['recall'], tp / (tp + fn))
    assert s['sides'][0]['tp'] + s['sides'][1]['tp'] == tp and s['all']['mean_cost'] > 0
    one.reset()
    assert not one.words.any()
    # costs of arbitrary bits: only those >= 0 are added (NaN and negative values are not)
    cost = torch.tensor([[[1.5, -1.0], [float('nan'), 2.0]], [[-0.0, 0.25], [3.0, float('-inf')]]]).cuda()
    counts = torch.tensor([[[1, 2, 3], [4, 5, 6]], [[10, 20, 30], [-1, 0, 1]]], dtype=torch.int32).cuda()
    ops.match_accumulate(one.words, counts, cost)
    assert np.array_equal(one.words.cpu().numpy(), R.accumulate(np.zeros(8, np.int64), counts.cpu().numpy(), cost.cpu().numpy()))
    a = one.arrays()
    assert a['tp'].tolist() == [11, 3] and a['cost_sum'].tolist() == [4.5, 2.25]


# ---- the engine ----------------------------------------------------------------------------------------------------------
def truth_of(out, K, G, seed, ct):
    """Ground truth of G hands per side for the K decoded ones of `out`: truth g = order[g] < K is decoded hand order[g] moved by
    a little noise, the others lie elsewhere; joints in the camera frame (joints + cam_trans), 'kp2d' in the pixels of pj2d_org."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    B = out['slots'].shape[0]
    lead = (B, K, 2)
    rnd = lambda *shape: torch.randn(shape, device='cuda', generator=g)
    j = out['joints'].view(lead + (21, 3)) + ct.view(lead + (1, 3))
    v = out['verts'].view(lead + (778, 3)) + ct.view(lead + (1, 3))
    k2 = out['pj2d_org'].view(lead + (21, 2))
    order = [(gi * 2 + 1) % G for gi in range(G)] if G > 2 else list(range(G))
    gt = {'joints': torch.empty(B, G, 2, 21, 3, device='cuda'), 'verts': torch.empty(B, G, 2, 778, 3, device='cuda'),
          'kp2d': torch.empty(B, G, 2, 21, 2, device='cuda')}
    for gi, src in enumerate(order):
        if src < K:
            gt['joints'][:, gi] = j[:, src] * 1.02 + 0.003 * rnd(B, 2, 21, 3)
            gt['verts'][:, gi] = v[:, src] * 1.02 + 0.003 * rnd(B, 2, 778, 3)
            gt['kp2d'][:, gi] = k2[:, src] + 2.0 * rnd(B, 2, 21, 2)
        else:
            gt['joints'][:, gi] = 0.3 + 0.05 * rnd(B, 2, 21, 3)
            gt['verts'][:, gi] = 0.3 + 0.05 * rnd(B, 2, 778, 3)
            gt['kp2d'][:, gi] = 900 + 20.0 * rnd(B, 2, 21, 2)
    valid = torch.rand(B, G, 2, 21, device='cuda', generator=g) > 0.2
    valid[..., 9] = True
    gt['joint_valid'] = valid
    gt['valid'] = torch.ones(B, G, 2, dtype=torch.uint8, device='cuda')
    gt['valid'][0, G - 1, 1] = 0
    return gt


def by_operators(ops, L, out, gt, on, K, ct, gate=INF, min_points=1):
    """The operators on the tensors Engine.match reads -> (the match result, the gathered rows)."""
    B = out['slots'].shape[0]
    lead = (B, K, 2)
    slots = out['slots'].view(lead + (L.SLOT,))
    res = ops.match_hands(out[on].view(lead + (21, -1)), gt['joints' if on == 'joints' else 'kp2d'], flags=slots[..., L.SLOT_FLAG],
                          valid=gt.get('joint_valid'), truth_valid=gt.get('valid'), trans=ct.view(lead + (3,)) if on == 'joints' else None,
                          group=gt.get('group'), gate=gate, min_points=min_points)
    rows = {k: ops.match_gather(t.contiguous().view(lead + tuple(t.shape[len(out['slots'].shape) - 1:])), res['pred_of'])
            for k, t in (('slots', out['slots']), ('joints', out['joints']), ('verts', out['verts']), ('cam_trans', ct),
                         ('pj2d', out['pj2d']), ('pj2d_org', out['pj2d_org']))}
    return res, rows


def assert_match(got, res, rows, what=''):
    for k in KEYS:
        assert torch.equal(got[k].view(torch.int32), res[k].view(torch.int32)), (what, k)
    assert set(got['out']) == set(rows), (what, set(got['out']))
    for k in rows:
        assert got['out'][k].shape == rows[k].shape and torch.equal(got['out'][k].view(torch.int32), rows[k].view(torch.int32)), (what, k)


def whole(B):
    """The offsets rows of B frames that are the 512 x 512 network input itself: pj2d_org is then in its pixels."""
    return torch.tensor([[512., 512, 0, 0, 0, 0, 0, 0, 0, 0]]).repeat(B, 1)


FLAGS2 = {2: [[[1., 1], [1, 0]], [[0, 1], [1, 1]]], 3: [[[1., 1], [1, 0]], [[0, 1], [1, 1]], [[1, 1], [1, 1]]]}


@pytest.mark.parametrize('B', [2, 3])
def test_engine_match_then_score_equals_the_operators(eng, frames3, B):
    ops, E, L = pkg('ops'), pkg('engine'), pkg('_lib')
    K, G = 2, 3
    out = eng.forward(frames3[:B], offsets=whole(B), project=True, max_hand=K)
    out['slots'][:, :, :, L.SLOT_FLAG] = torch.tensor(FLAGS2[B]).cuda()
    ct = placed(B, K)
    gt = truth_of(out, K, G, 40 + B, ct)
    for on, gate in (('joints', INF), ('pj2d_org', 50.0), ('joints', 0.05)):
        mboard, sboard, want_m, want_s = E.MatchBoard(0), E.ScoreBoard(0), E.MatchBoard(0), E.ScoreBoard(0)
        got = eng.match(out, gt, on=on, gate=gate, max_hand=K, cam_trans=ct, board=mboard)
        res, rows = by_operators(ops, L, out, gt, on, K, ct, gate=gate)
        assert_match(got, res, rows, (B, on))
        assert got['match'].shape == (B, K, 2) and got['out']['verts'].shape == (B, G, 2, 778, 3)
        want_m.add(res)
        assert torch.equal(mboard.words, want_m.words)
        assert got['gt'] is not gt and got['gt']['group'] is got['group'] and got['gt']['joints'] is gt['joints'] and 'group' not in gt
        # truth-ordered rows go into Engine.score unchanged
        sc = eng.score(got['out'], got['gt'], board=sboard, max_hand=G, cam_trans=got['out']['cam_trans'])
        rj, rv, grp, flags = by_operator(ops, rows, dict(gt, group=res['group']), G, rows['cam_trans'], group=res['group'])
        for name, want in (('joints', rj), ('verts', rv)):
            for k in ('e_ra', 'e_pa', 'row_f', 'row_i'):
                assert torch.equal(sc[name][k].view(torch.int32), want[k].view(torch.int32)), (B, on, name, k)
        assert torch.equal(sc['pair_err'].view(torch.int32), rj['pair_err'].view(torch.int32))
        want_s.add(0, rj, group=grp, flags=flags)
        want_s.add(1, rv, group=grp, flags=flags)
        assert torch.equal(sboard.words, want_s.words)
        # an unmatched valid truth is the ScoreBoard's "missed"; a truth that does not exist is not looked at
        s, m = sboard.summary(), mboard.summary()
        counts = got['counts'].cpu().numpy()
        assert [s['groups'][k]['missed'] for k in range(2)] == counts[:, :, 2].sum(0).tolist() == [m['sides'][k]['fn'] for k in range(2)]
        assert [s['groups'][k]['scored'] for k in range(2)] == counts[:, :, 0].sum(0).tolist()
        assert s['all']['scored'] + s['all']['missed'] == int((gt['valid'] != 0).sum()) and m['all']['tp'] >= 2
        if gate == INF:      # every pair is allowed: as many pairs as there are flagged hands or valid truths
            fl, tv = np.array(FLAGS2[B]) > 0.5, gt['valid'].cpu().numpy() != 0
            assert np.array_equal(counts[:, :, 0], np.minimum(fl.sum(1), tv.sum(1)))
    # without an optional key, K = 1 rows as [B,2,...], and what is refused
    one = eng.forward(frames3[:B], offsets=whole(B), project=True)
    gt1 = {'kp2d': gt['kp2d'][:, :1].contiguous()}
    got = eng.match(one, gt1, on='pj2d_org')
    res = ops.match_hands(one['pj2d_org'].view(B, 1, 2, 21, 2), gt1['kp2d'], flags=one['slots'].view(B, 1, 2, L.SLOT)[..., L.SLOT_FLAG])
    for k in KEYS:
        assert torch.equal(got[k].view(torch.int32), res[k].view(torch.int32)), k
    assert got['out']['slots'].shape == (B, 1, 2, L.SLOT) and 'cam_trans' not in got['out']
    for bad in (dict(on='verts'), dict(max_hand=2), dict(gate=-1.0), dict(min_points=22), dict(board=E.ScoreBoard(0))):
        with pytest.raises(ValueError):
            eng.match(one, gt1, **dict(dict(on='pj2d_org'), **bad))
    with pytest.raises(ValueError):
        eng.match(one, gt1, on='joints')      # no gt['joints']
    with pytest.raises(ValueError):
        eng.match(one, {'kp2d': gt['kp2d'][:1]}, on='pj2d_org')      # another batch size


def test_three_calls_queue_without_a_host_visit(eng, frames3):
    E, L = pkg('engine'), pkg('_lib')
    K, G = 2, 3
    out = eng.forward(frames3[:2], offsets=whole(2), project=True, max_hand=K)
    out['slots'][:, :, :, L.SLOT_FLAG] = torch.tensor(FLAGS2[2]).cuda()
    ct = placed(2, K)
    gt = truth_of(out, K, G, 50, ct)
    gt['joint_valid'] = gt['joint_valid'].to(torch.uint8)      # (what the library reads: nothing is converted)
    one, sone = E.MatchBoard(0), E.ScoreBoard(0)
    want = eng.match(out, gt, on='joints', max_hand=K, cam_trans=ct, board=one)
    eng.score(want['out'], want['gt'], board=sone, max_hand=G, cam_trans=want['out']['cam_trans'])
    board, sboard = E.MatchBoard(0), E.ScoreBoard(0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        res = []
        for _ in range(3):
            res.append(eng.match(out, gt, on='joints', max_hand=K, cam_trans=ct, board=board))
            eng.score(res[-1]['out'], res[-1]['gt'], board=sboard, max_hand=G, cam_trans=res[-1]['out']['cam_trans'])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for r in res:
        for k in KEYS:
            assert torch.equal(r[k].view(torch.int32), want[k].view(torch.int32)), k
    a, b = board.arrays(), one.arrays()
    assert all(np.array_equal(a[k], 3 * b[k]) for k in ('tp', 'fp', 'fn')) and a['tp'].sum() > 0
    assert np.array_equal(sboard.arrays()[0][0]['scored'], 3 * sone.arrays()[0][0]['scored'])


def test_pool_match_on_a_shared_board(eng, near_sd, mano_tables, frames3):
    E = pkg('engine')
    img = frames3[:2]
    K, G = 2, 3
    out = eng.forward(img, offsets=whole(2), project=True, max_hand=K)
    ct = placed(2, K)
    gt = truth_of(out, K, G, 60, ct)
    want_board, want_sboard = E.MatchBoard(0), E.ScoreBoard(0)
    want = []
    for k in range(4):
        want.append(eng.match(out, gt, on='joints' if k % 2 else 'pj2d_org', max_hand=K, cam_trans=ct, board=want_board))
        eng.score(want[-1]['out'], want[-1]['gt'], board=want_sboard, max_hand=G, cam_trans=want[-1]['out']['cam_trans'])
    pool = E.EnginePool(0, n=2)
    pool.load_state_dict(near_sd, max_batch=2)
    pool.load_mano(mano_tables)
    board, sboard = E.MatchBoard(0), E.ScoreBoard(0)      # shared by both contexts: updated in the order of the calls
    for k in range(4):
        t = pool.submit(img, offsets=whole(2), project=True, max_hand=K)
        got = pool.match(t, gt, on='joints' if k % 2 else 'pj2d_org', board=board, cam_trans=ct)
        pool.collect(t)
        for key in KEYS:
            assert torch.equal(got[key].view(torch.int32), want[k][key].view(torch.int32)), (k, key)
        for key in want[k]['out']:
            assert torch.equal(got['out'][key].view(torch.int32), want[k]['out'][key].view(torch.int32)), (k, key)
    assert torch.equal(board.words, want_board.words) and board.summary()['all']['tp'] > 0
    with pytest.raises(RuntimeError):
        pool.match(t, gt)
    pool.close()


def test_forward_batch_match_keys_and_boards(near_sd, mano_tables, frames3):
    ops, E, cfg, S, M, L = pkg('ops'), pkg('engine'), pkg('config'), pkg('score'), pkg('match'), pkg('_lib')
    acr = pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml']), state_dict=near_sd,
                              mano_tables=mano_tables, max_batch=2)
    img = frames3[:2]
    K, G = 2, 3
    e = acr.model.engine(2)
    out = e.forward(img, offsets=whole(2), project=True, max_hand=K)
    ct = ops.cam_trans(out['joints'].view(-1, 21, 3), out['pj2d'].view(-1, 21, 2), focal_length=acr.focal_length).view(2, K, 2, 3)
    gt = truth_of(out, K, G, 70, ct)
    plain = acr.forward_batch(img, ['a', 'b'], max_hand=K)
    new = set(S.SCORE_KEYS) | set(M.MATCH_KEYS)
    for how, on, gate in (('kp2d', 'pj2d_org', 40.0), ('joints', 'joints', INF)):
        sboard, mboard = E.ScoreBoard(0), E.MatchBoard(0)
        res = acr.forward_batch(img, ['a', 'b'], max_hand=K, gt=gt, match=how, match_gate=gate, board=sboard, match_board=mboard)
        again = acr.forward_batch(img, ['a', 'b'], max_hand=K)
        for k in plain:                                   # without match= the dicts are what they were
            assert len(res[k]) == len(plain[k]) == len(again[k])
            for h0, h1, h2 in zip(plain[k], res[k], again[k]):
                assert set(h1) == set(h0) | new and set(h2) == set(h0) and not new & set(h0)
                assert all(np.array_equal(h0[f], h1[f]) and np.array_equal(h0[f], h2[f]) for f in h0)
        want, rows = by_operators(ops, L, out, gt, on, K, ct, gate=gate)
        rj, rv, grp, flags = by_operator(ops, rows, dict(gt, group=want['group']), G, rows['cam_trans'], group=want['group'])
        want_s, want_m = E.ScoreBoard(0), E.MatchBoard(0)
        want_s.add(0, rj, group=grp, flags=flags)
        want_s.add(1, rv, group=grp, flags=flags)
        want_m.add(want)
        assert torch.equal(sboard.words, want_s.words) and torch.equal(mboard.words, want_m.words)
        mt, cost = want['match'].cpu().numpy(), want['cost'].cpu().numpy()
        fj, fv = rj['row_f'].cpu().numpy(), rv['row_f'].cpu().numpy()
        fl = out['slots'][..., L.SLOT_FLAG].cpu().numpy()
        seen = 0
        for b, key in enumerate('ab'):
            where = [(k, h) for h in (0, 1) for k in range(K) if fl[b, k, h] > 0.5]      # lefts in rank order, then rights
            assert len(where) == len(res[key])
            for (k, h), hand in zip(where, res[key]):
                assert hand['gt_index'] == mt[b, k, h] and hand['match_cost'] == cost[b, k, h]
                if mt[b, k, h] < 0:
                    assert all(np.isnan(hand[f]) for f in S.SCORE_KEYS)
                    continue
                row = (b * G + mt[b, k, h]) * 2 + h
                got4 = (hand['mpjpe'], hand['pa_mpjpe'], hand['mpvpe'], hand['pa_mpvpe'])
                want4 = tuple(np.float32(np.nan) if not v >= 0 else v for v in (fj[row, 0], fj[row, 1], fv[row, 0], fv[row, 1]))
                assert all(a == w or (np.isnan(a) and np.isnan(w)) for a, w in zip(got4, want4)), (key, k, h)
                seen += 1
        assert seen >= 2
    raw = acr.forward_raw_batch(torch.from_numpy(np.ascontiguousarray(img.cpu().numpy()[..., ::-1])).cuda(), ['a', 'b'], max_hand=K,
                                gt=gt, match='kp2d', match_board=mboard)
    assert all(new <= set(h) for k in raw for h in raw[k])
    s = mboard.summary()['all']
    assert s['tp'] + s['fn'] == 2 * int((gt['valid'] != 0).sum())
    for kw in (dict(match='kp2d'), dict(match='kp2d', gt={'joints': gt['joints']}), dict(match_board=mboard, gt=gt),
               dict(match='joints', gt=gt, match_gate=-1.0)):
        with pytest.raises(ValueError):
            acr.forward_batch(img, ['a', 'b'], max_hand=K, **kw)
