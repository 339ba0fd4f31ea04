"""Host-side checks of matching decoded hands to ground truth (acrmi_match_hands / acrmi_match_gather / acrmi_match_accumulate,
ops.match_hands, engine.MatchBoard, match= of ACR.forward_batch): the ABI surface and the argument checks
that need no device, the rule's numpy restatement (tests/match_ref.py) against exhaustive enumeration and against scipy's
assignment solver, the summary arithmetic on a hand-made board, the packaging of the match keys, and the plan's stand-alone
check program.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import match_ref as R
from conftest import ROOT, pkg

NEW = ('acrmi_match_board_bytes', 'acrmi_match_hands', 'acrmi_match_gather', 'acrmi_match_accumulate')
INF = float('inf')


def test_new_symbols_are_declared_exported_and_bound():
    L = pkg('_lib')
    lib = L.lib()
    header = open(os.path.join(ROOT, 'include', 'acrmi.h')).read()
    for name in NEW:
        assert name + '(' in header and name in L.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.acrmi_match_hands.argtypes) == 21 and len(lib.acrmi_match_gather.argtypes) == 8
    assert len(lib.acrmi_match_accumulate.argtypes) == 6
    assert lib.acrmi_match_board_bytes.restype is ctypes.c_size_t and lib.acrmi_match_board_bytes() == 64
    assert lib.acrmi_version() == L.VERSION == 303      # additive: the ABI version stays
    assert 'match.hip' in pkg('build').SOURCES
    # the rule stands in the header, in the plan and in the design document
    plan = open(os.path.join(ROOT, pkg().__name__, 'csrc', 'match_plan.h')).read()
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    for text in (header, plan, design):
        flat = ' '.join(text.replace('*', ' ').replace('//', ' ').replace('`', '').split())      # comment marks and mark-up aside
        assert 'strict improvement' in flat and 'bitmask of used truths' in flat and 'm ascending' in flat, text[:80]
    assert '## 24.' in design
    E, ops = pkg('engine'), pkg('ops')
    assert hasattr(E, 'MatchBoard') and hasattr(E.Engine, 'match') and hasattr(E.EnginePool, 'match')
    assert all(hasattr(ops, n) for n in ('match_hands', 'match_gather', 'match_accumulate'))
    assert all(hasattr(E.MatchBoard, n) for n in ('add', 'reset', 'summary'))


def test_bad_arguments_are_rejected_before_any_device_call():
    L = pkg('_lib')
    lib = L.lib()
    p = ctypes.c_void_p(256)      # never read: the checks come first
    good = dict(pred=p, truth=p, valid=None, tvalid=None, flags=p, stride=176, trans=None, group=None, B=2, K=2, G=3, n=21, D=2,
                gate=INF, min_points=1, match=p, pred_of=p, cost=p, counts=p, group_out=p, stream=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.acrmi_match_hands(*a.values()), lib.acrmi_last_error(None)

    for bad in (dict(pred=None), dict(truth=None), dict(match=None), dict(pred_of=None), dict(cost=None), dict(counts=None),
                dict(group_out=None), dict(B=-1), dict(K=0), dict(K=9), dict(G=0), dict(G=9), dict(n=0), dict(n=257), dict(D=1),
                dict(D=4), dict(gate=float('nan')), dict(gate=-1.0), dict(gate=-INF), dict(min_points=0), dict(min_points=22),
                dict(stride=0), dict(B=2 ** 31 - 1), dict(B=174763, K=8, G=1, n=256, D=3), dict(B=174763, K=1, G=8, n=256, D=3)):
        rc, msg = call(**bad)
        assert rc == L.E_INVAL and msg.startswith(b'acrmi_match_hands:'), (bad, rc, msg)
    # no frame: success, nothing is touched (also on a machine without a GPU)
    assert call(B=0)[0] == 0 and call(B=0, pred=None, truth=None, match=None, counts=None)[0] == 0
    assert call(B=0, K=9)[0] == L.E_INVAL and call(B=0, gate=-1.0)[0] == L.E_INVAL and call(B=0, min_points=0)[0] == L.E_INVAL
    if not torch.cuda.is_available():      # well-formed arguments reach the device: a loud failure, no host path
        assert call()[0] == L.E_HIP and call(gate=0.0, min_points=21, flags=None, stride=0)[0] == L.E_HIP

    gat = dict(src=p, index=p, B=2, Ks=2, Kd=3, W=176, dst=p, stream=None)

    def call2(**kw):
        a = dict(gat)
        a.update(kw)
        return lib.acrmi_match_gather(*a.values()), lib.acrmi_last_error(None)

    for bad in (dict(src=None), dict(index=None), dict(dst=None), dict(B=-1), dict(Ks=0), dict(Ks=9), dict(Kd=0), dict(Kd=9), dict(W=0),
                dict(W=-4), dict(src=ctypes.c_void_p(258)), dict(dst=ctypes.c_void_p(257)), dict(index=ctypes.c_void_p(259)),
                dict(B=2 ** 31 - 1), dict(B=2 ** 20, Ks=8, Kd=8, W=2334)):
        rc, msg = call2(**bad)
        assert rc == L.E_INVAL and msg.startswith(b'acrmi_match_gather:'), (bad, rc, msg)
    assert call2(B=0)[0] == 0 and call2(B=0, src=None, dst=None)[0] == 0 and call2(B=0, W=0)[0] == L.E_INVAL

    acc = dict(counts=p, cost=p, B=2, K=2, board=p, stream=None)

    def call3(**kw):
        a = dict(acc)
        a.update(kw)
        return lib.acrmi_match_accumulate(*a.values()), lib.acrmi_last_error(None)

    for bad in (dict(counts=None), dict(cost=None), dict(board=None), dict(board=ctypes.c_void_p(260)), dict(B=-1), dict(K=0), dict(K=9)):
        rc, msg = call3(**bad)
        assert rc == L.E_INVAL and msg.startswith(b'acrmi_match_accumulate:'), (bad, rc, msg)
    assert call3(B=0)[0] == 0 and call3(B=0, counts=None, board=None)[0] == 0 and call3(B=0, K=9)[0] == L.E_INVAL
    # the operators refuse host tensors and malformed arguments before they look at the device
    ops = pkg('ops')
    with pytest.raises(L.AcrmiError):
        ops.match_hands(torch.zeros(1, 2, 2, 21, 2), torch.zeros(1, 3, 2, 21, 2))
    with pytest.raises(L.AcrmiError):
        ops.match_gather(torch.zeros(1, 2, 2, 5), torch.zeros(1, 3, 2, dtype=torch.int32))
    for gate, mp in ((-1, 1), (float('nan'), 1), (1.0, 0), (1.0, 22), (1.0, 1.5)):
        with pytest.raises(ValueError):
            ops.check_match_params(gate, mp, 21)
    assert ops.check_match_params(INF, 21, 21) == (INF, 21) and ops.check_match_params(0, 1, 1) == (0.0, 1)


def _random_problem(g, K, G, density, hi=10):
    cost = g.integers(0, hi, (K, G)).astype(np.float64)
    allow = g.random((K, G)) < density
    return cost, allow


def _check_matching(match, cost, allow):
    """`match` is a one-to-one matching of allowed pairs -> (pairs, cost sum)."""
    used, total = set(), 0.0
    for i, t in enumerate(match):
        if t >= 0:
            assert allow[i, t] and t not in used and t < cost.shape[1], (match, allow)
            used.add(int(t))
            total += cost[i, t]
    return len(used), total


def test_rule_equals_exhaustive_enumeration():
    """The recurrence (match_ref.solve) on integer costs, K, G <= 5: count and cost equal exhaustive enumeration exactly."""
    g = np.random.default_rng(24)
    problems = []
    for K in range(1, 6):
        for G in range(1, 6):
            for density in (0.0, 0.3, 0.6, 0.9, 1.0):
                for hi in (3, 10):
                    problems.append((K, G) + _random_problem(g, K, G, density, hi))
    for K, G, cost, allow in problems:
        match, pairs, total = R.solve(cost[None], allow[None])
        want = R.brute_force(cost, allow)
        got = _check_matching(match[0], cost, allow)
        assert got == want and (int(pairs[0]), float(total[0])) == want, (K, G, cost, allow, match)
    assert len(problems) == 250


def test_rule_tie_order():
    same = np.full((3, 3), 2.0)
    on = np.ones((3, 3), bool)
    assert R.solve(same[None, :1], on[None, :1])[0].tolist() == [[0]]                  # identical truths: the lowest
    assert R.solve(same[None, :, :1], on[None, :, :1])[0].tolist() == [[0, -1, -1]]    # identical predictions: the first
    assert R.solve(same[None, :2, :2], on[None, :2, :2])[0].tolist() == [[1, 0]]
    assert R.solve(same[None], on[None])[0].tolist() == [[2, 1, 0]]
    cost = np.array([[0.0, 5.0], [5.0, 2.0]])
    allow = np.array([[1, 1], [1, 0]], bool)
    assert R.solve(cost[None], allow[None])[0].tolist() == [[1, 0]]                    # more pairs beat a smaller sum
    assert R.solve(cost[None], np.zeros((1, 2, 2), bool))[0].tolist() == [[-1, -1]]


@pytest.mark.parametrize('K,G', [(8, 8), (8, 5), (3, 8)])
def test_rule_equals_scipy_assignment(K, G):
    """Against scipy.optimize.linear_sum_assignment on the padded (K+G)^2 matrix: unmatched = big, forbidden = 3 * big."""
    lsa = pytest.importorskip('scipy.optimize').linear_sum_assignment
    g = np.random.default_rng(K * 10 + G)
    big = 1000.0
    for trial in range(40):
        cost = g.integers(0, 50, (K, G)).astype(np.float64)
        allow = g.random((K, G)) < (1.0, 0.7, 0.4, 0.15)[trial % 4]
        n = K + G
        M = np.zeros((n, n))
        M[:K, :G] = np.where(allow, cost, 3 * big)
        M[:K, G:] = big            # prediction i stays unmatched
        M[K:, :G] = big            # truth g stays unmatched
        rows, cols = lsa(M)
        pairs = [(i, j) for i, j in zip(rows, cols) if i < K and j < G]
        assert all(allow[i, j] for i, j in pairs)
        want = (len(pairs), float(sum(cost[i, j] for i, j in pairs)))
        match, cnt, total = R.solve(cost[None], allow[None])
        assert _check_matching(match[0], cost, allow) == want and (int(cnt[0]), float(total[0])) == want, (trial, want)


def test_restatement_outputs_on_a_small_scene():
    """Two predictions, three truths on a line: who is matched to whom, the inverse, the costs, the counts and the groups."""
    truth = np.zeros((1, 3, 2, 2, 2), np.float32)
    truth[0, :, :, :, 0] = np.array([0.0, 10.0, 20.0], np.float32)[:, None, None]
    pred = np.zeros((1, 2, 2, 2, 2), np.float32)
    pred[0, :, :, :, 0] = np.array([21.0, 1.0], np.float32)[:, None, None]
    res = R.match_hands(pred, truth)
    assert res['match'][0].tolist() == [[2, 2], [0, 0]] and res['pred_of'][0].tolist() == [[1, 1], [-1, -1], [0, 0]]
    assert res['cost'][0].tolist() == [[1.0, 1.0], [1.0, 1.0]] and res['counts'][0].tolist() == [[2, 0, 1], [2, 0, 1]]
    assert res['group'][0].tolist() == [[0, 1]] * 3
    flags = np.array([[[1.0, 0.4], [np.nan, 1.0]]], np.float32)
    tv = np.array([[[1, 1], [1, 0], [0, 7]]], np.uint8)
    res = R.match_hands(pred, truth, flags=flags, truth_valid=tv, gate=5.0, group=np.full((1, 3, 2), 4, np.int32))
    # left: prediction 0 alone is flagged, truth 2 is not valid: 21 -> 10 costs 11 > gate: nothing; right: prediction 1 -> truth 0
    assert res['match'][0].tolist() == [[-1, -1], [-1, 0]] and res['counts'][0].tolist() == [[0, 1, 2], [1, 0, 1]]
    assert res['group'][0].tolist() == [[4, 4], [4, -1], [-1, 4]] and res['cost'][0].tolist() == [[-1, -1], [-1, 1.0]]
    valid = np.ones((1, 3, 2, 2), np.uint8)
    valid[0, 0, 1, 1] = 0
    assert R.match_hands(pred, truth, valid=valid, min_points=2)['match'][0].tolist() == [[2, 2], [0, 1]]
    assert R.gather(pred, np.array([[[1, -1], [2, 0], [-2 ** 31, 2 ** 31 - 1]]]))[0, :, :, 0, 0].tolist() == [[1, 0], [0, 21], [0, 0]]
    words = R.accumulate(np.zeros(8, np.int64), res['counts'], res['cost'])
    assert words[:3].tolist() == [0, 1, 2] and words[4:7].tolist() == [1, 0, 1] and words.view(np.float64)[[3, 7]].tolist() == [0.0, 1.0]


def test_summary_arithmetic_on_a_hand_made_board():
    M = pkg('match')
    words = np.zeros(8, np.int64)
    words[0:3] = (6, 2, 3)
    words[4:7] = (0, 0, 5)
    words.view(np.float64)[3] = 0.3
    a = M.board_arrays(words)
    assert a['tp'].tolist() == [6, 0] and a['fp'].tolist() == [2, 0] and a['fn'].tolist() == [3, 5] and a['cost_sum'].tolist() == [0.3, 0.0]
    s = M.summarize(a)
    left, right, al = s['sides'][0], s['sides'][1], s['all']
    assert np.isclose(left['precision'], 6 / 8) and np.isclose(left['recall'], 6 / 9) and np.isclose(left['f1'], 12 / 17)
    assert np.isclose(left['mean_cost'], 0.05) and (left['tp'], left['fp'], left['fn']) == (6, 2, 3)
    assert np.isnan(right['precision']) and right['recall'] == 0 and right['f1'] == 0 and np.isnan(right['mean_cost'])
    assert np.isclose(al['precision'], 6 / 8) and np.isclose(al['recall'], 6 / 14) and np.isclose(al['f1'], 12 / 22) and np.isclose(al['mean_cost'], 0.05)
    empty = M.summarize(M.board_arrays(np.zeros(8, np.int64)))['all']
    assert all(np.isnan(empty[k]) for k in ('precision', 'recall', 'f1', 'mean_cost')) and empty['tp'] == 0
    with pytest.raises(ValueError):
        M.board_arrays(words[:-1])


def test_match_keys_of_the_hand_dicts_and_value_errors():
    """match= adds 'gt_index' and 'match_cost' to every hand dict, and only then; the score keys come from the matched truth."""
    from importlib import import_module
    main = import_module(pkg().__name__ + '.acr.main')
    g = np.random.default_rng(0)
    B, K, G = 2, 2, 3
    out = {'slots': g.normal(size=(B, K, 2, 176)).astype(np.float32), 'verts': np.zeros((B, K, 2, 778, 3), np.float32),
           'joints': np.zeros((B, K, 2, 21, 3), np.float32), 'pj2d': np.zeros((B, K, 2, 21, 2), np.float32),
           'pj2d_org': np.zeros((B, K, 2, 21, 2), np.float32), 'cam_trans': np.zeros((B, K, 2, 3), np.float32)}
    out['slots'][..., 0] = np.array([[[1, 1], [1, 0]], [[0, 1], [0, 0]]], np.float32)
    plain = main.results_from_out(out, ['a', 'b'])
    keys = set(plain['a'][0])
    new = set(pkg('match').MATCH_KEYS) | set(pkg('score').SCORE_KEYS)
    assert not keys & new and pkg('match').MATCH_KEYS == ('gt_index', 'match_cost')
    match = np.array([[[2, 0], [-1, -1]], [[-1, 1], [-1, -1]]], np.int32)
    cost = np.where(match >= 0, 1.5, -1).astype(np.float32)
    rows = np.full((B * G * 2, 4), -1, np.float32)      # truth order: row (b*G + g)*2 + h
    rows[:, 0] = np.arange(B * G * 2) * 0.001 + 0.001
    rows[:, 1] = rows[:, 0] / 2
    out['match'] = {'match': match, 'cost': cost, 'G': G}
    out['score'] = {'joints': rows, 'verts': None}
    res = main.results_from_out(out, ['a', 'b'])
    a = res['a']      # lefts of rank 0, 1, then the right of rank 0
    assert all(set(h) == keys | new for h in a + res['b'])
    assert [int(h['gt_index']) for h in a] == [2, -1, 0] and [float(h['match_cost']) for h in a] == [1.5, -1.0, 1.5]
    assert np.isclose(a[0]['mpjpe'], 0.005) and np.isclose(a[0]['pa_mpjpe'], 0.0025)      # row (0*3 + 2)*2 + 0 = 4
    assert np.isnan(a[1]['mpjpe']) and np.isnan(a[1]['pa_mpjpe']) and np.isclose(a[2]['mpjpe'], 0.002)      # row 1
    assert int(res['b'][0]['gt_index']) == 1 and np.isclose(res['b'][0]['mpjpe'], 0.010)      # row (1*3 + 1)*2 + 1 = 9
    assert a[0]['gt_index'].dtype == np.int32 and a[0]['match_cost'].dtype == np.float32
    gt = {'joints': 1}
    board = type('B', (), {'words': 1})()
    for bad in (dict(match='kp2d', gt=None), dict(match='joints', gt=None), dict(match='kp2d', gt=gt), dict(match='verts', gt=gt),
                dict(match=None, gt=gt, match_board=board), dict(match='joints', gt=gt, match_gate=-1.0),
                dict(match='joints', gt=gt, match_gate=float('nan')), dict(match='joints', gt=gt, match_board=object()),
                dict(match='joints', gt=gt, show_items=['error'])):
        with pytest.raises(ValueError):
            main._check_match(bad['match'], bad['gt'], bad.get('match_gate', INF), bad.get('match_board'), bad.get('show_items'))
    main._check_match(None, None, INF, None)
    main._check_match('joints', gt, 0.0, board)
    main._check_match('kp2d', {'joints': 1, 'kp2d': 1}, INF, None, ['mesh'])


def test_forward_batch_refuses_match_before_anything_runs():
    """match without gt, or match='kp2d' without gt['kp2d'], is a ValueError raised before the model is touched."""
    from importlib import import_module
    main = import_module(pkg().__name__ + '.acr.main')

    class Untouched(object):
        hands_per_side = 1

        def __getattr__(self, name):
            raise AssertionError('the model was touched: ' + name)

    for kw in (dict(match='kp2d'), dict(match='joints'), dict(match='kp2d', gt={'joints': torch.zeros(1, 1, 2, 21, 3)}),
               dict(match_board=object())):
        with pytest.raises(ValueError):
            main.ACR.forward_batch(Untouched(), None, ['a'], **kw)
        with pytest.raises(ValueError):
            main.ACR.forward_raw_batch(Untouched(), None, ['a'], **kw)


def test_plan_stand_alone_program(tmp_path):
    """tools/match_check.cpp: csrc/match_plan.h as a program of its own.  The plain build must pass; the build with the address
    and undefined-behaviour sanitizers must pass as well where the host compiler can make one that starts - which of the two
    ran is printed."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        assert os.path.exists(hipcc), 'no C++ compiler'
        cmd = [hipcc, '-x', 'c++']
    else:
        cmd = [cxx]
    src = os.path.join(ROOT, 'tools', 'match_check.cpp')
    cmd += ['-std=c++17', '-O1', '-g', '-ffp-contract=off', src, '-o']
    plain = str(tmp_path / 'match_check')
    subprocess.run(cmd + [plain], check=True, capture_output=True)
    run = subprocess.run([plain], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    ran = None
    for label, extra in (('static', san + ['-static-libasan', '-static-libubsan']), ('shared', san)):
        exe = str(tmp_path / ('match_check_' + label))
        if subprocess.run(cmd + [exe] + extra, capture_output=True).returncode != 0:
            continue
        run = subprocess.run([exe], capture_output=True, text=True)
        if 'does not come first in initial library list' in run.stderr:
            continue
        ran = label
        assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
        break
    print('sanitizer variant that ran: %s' % ran)
