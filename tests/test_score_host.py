"""Host-side checks of scoring against ground truth (acrmi_pose_errors / acrmi_score_accumulate / acrmi_score_hands,
ops.pose_errors, engine.ScoreBoard, gt= of ACR.forward_batch): the ABI surface and the argument checks
that need no device, the board's sizes and layout, the rule's numpy restatement (tests/score_ref.py) against an independent
LAPACK form, the summary arithmetic on a hand-made board, the packaging of the four score keys, and the plan's stand-alone
check program.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import score_cases as cases
import score_ref as R
from conftest import ROOT, pkg

NEW = ('acrmi_score_board_bytes', 'acrmi_score_pair_bytes', 'acrmi_pose_errors', 'acrmi_score_accumulate', 'acrmi_score_hands')


def test_new_symbols_are_declared_exported_and_bound():
    L = pkg('_lib')
    lib = L.lib()
    header = open(os.path.join(ROOT, 'include', 'acrmi.h')).read()
    for name in NEW:
        assert name + '(' in header and name in L.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.acrmi_pose_errors.argtypes) == 19 and len(lib.acrmi_score_accumulate.argtypes) == 13
    assert len(lib.acrmi_score_hands.argtypes) == 25
    assert lib.acrmi_score_board_bytes.restype is ctypes.c_size_t and lib.acrmi_score_pair_bytes.restype is ctypes.c_size_t
    assert lib.acrmi_version() == L.VERSION == 303      # additive: the ABI version stays
    assert 'score.hip' in pkg('build').SOURCES
    # the rule stands in the header, in the plan and in the design document
    plan = open(os.path.join(ROOT, pkg().__name__, 'csrc', 'score_plan.h')).read()
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    for text in (header, plan, design):
        assert 'exactly 6 sweeps' in text and 'Horn' in text and 'sign(0) = +1' in text, text[:80]
    assert '## 21.' in design
    assert all(hasattr(pkg('engine'), n) for n in ('ScoreBoard',)) and hasattr(pkg('engine').Engine, 'score')
    assert hasattr(pkg('engine').EnginePool, 'score') and hasattr(pkg('ops'), 'pose_errors')


def test_board_sizes_and_layout():
    lib, S = pkg('_lib').lib(), pkg('score')
    for n, g, b in ((0, 2, 100), (4001, 2, 100), (21, 0, 100), (21, 17, 100), (21, 2, 0), (21, 2, 4097), (-1, -1, -1)):
        assert lib.acrmi_score_board_bytes(n, g, b) == 0
    assert lib.acrmi_score_pair_bytes(0) == 0 and lib.acrmi_score_pair_bytes(17) == 0
    assert lib.acrmi_score_board_bytes(21, 2, 100) == 2 * (4 * 21 + 101 + 2) * 8
    assert lib.acrmi_score_board_bytes(4000, 16, 4096) == 16 * (16000 + 4097 + 2) * 8
    assert lib.acrmi_score_pair_bytes(2) == 64 and lib.acrmi_score_pair_bytes(16) == 4096
    for sets, g, b in (((21, 778), 2, 100), ((5,), 1, 1), ((1, 2, 3), 16, 7)):
        offs, pair_at, total = S.board_layout(sets, g, b)
        assert offs[0] == 0 and total * 8 == sum(lib.acrmi_score_board_bytes(n, g, b) for n in sets) + lib.acrmi_score_pair_bytes(g)
        assert all(o1 - o0 == S.group_words(n, b) * g for o0, o1, n in zip(offs, offs[1:] + [pair_at], sets))
    for bad in (dict(sets=()), dict(sets=(0,)), dict(sets=(4001,)), dict(n_groups=0), dict(n_groups=17), dict(n_bins=0),
                dict(n_bins=4097), dict(bin_width=0), dict(bin_width=float('nan')), dict(bin_width=float('inf')), dict(bin_width=-1)):
        with pytest.raises(ValueError):
            S.check_board_params(**dict(dict(sets=(21, 778), n_groups=2, n_bins=100, bin_width=0.0005), **bad))
    assert (S.N_BINS, S.BIN_WIDTH) == (100, 0.0005)


def test_bad_arguments_are_rejected_before_any_device_call():
    L = pkg('_lib')
    lib = L.lib()
    p = ctypes.c_void_p(256)      # never read: the checks come first
    good = dict(pred=p, gt=p, valid=None, N=2, n=21, root=9, oP=None, oG=None, trans=None, group=None, G=2, flags=None, e_ra=p,
                e_pa=p, row_f=p, row_i=p, xform=None, pair=None, stream=None)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.acrmi_pose_errors(*a.values()), lib.acrmi_last_error(None)

    for bad in (dict(pred=None), dict(gt=None), dict(e_ra=None), dict(e_pa=None), dict(row_f=None), dict(row_i=None), dict(n=0),
                dict(n=4001), dict(N=-1), dict(G=0), dict(G=17), dict(root=-2), dict(root=21), dict(oP=p), dict(oG=p, root=-1),
                dict(N=2 ** 31 - 1), dict(N=178957, n=4000, root=0)):
        rc, msg = call(**bad)
        assert rc == L.E_INVAL and msg.startswith(b'acrmi_pose_errors:'), (bad, rc, msg)
    # no row: success, nothing is touched (also on a machine without a GPU)
    assert call(N=0)[0] == 0 and call(N=0, pred=None, gt=None, e_ra=None, row_i=None)[0] == 0
    assert call(N=0, n=4001)[0] == L.E_INVAL and call(N=0, G=17)[0] == L.E_INVAL
    if not torch.cuda.is_available():      # well-formed arguments reach the device: a loud failure, no host path
        assert call(n=4000, root=-1)[0] == L.E_HIP

    acc = dict(e_ra=p, e_pa=p, N=2, n=21, group=None, G=2, flags=None, pair=None, bins=100, width=0.0005, board=p, pboard=None,
               stream=None)

    def call2(**kw):
        a = dict(acc)
        a.update(kw)
        return lib.acrmi_score_accumulate(*a.values()), lib.acrmi_last_error(None)

    for bad in (dict(e_ra=None), dict(e_pa=None), dict(board=None), dict(board=ctypes.c_void_p(260)), dict(pboard=ctypes.c_void_p(257)),
                dict(n=0), dict(n=4001), dict(N=-1), dict(G=0), dict(G=17), dict(bins=0), dict(bins=4097), dict(width=0.0),
                dict(width=float('nan')), dict(width=float('inf')), dict(width=-0.001)):
        rc, msg = call2(**bad)
        assert rc == L.E_INVAL and msg.startswith(b'acrmi_score_accumulate:'), (bad, rc, msg)
    assert call2(N=0)[0] == 0 and call2(N=0, e_ra=None, board=None)[0] == 0 and call2(N=0, width=0.0)[0] == L.E_INVAL
    # the context form
    args = [None, p, p, p, None, p, None, None, None, 2, 1, 2, 100, 0.0005, None, p, p, p, p, None, None, None, None, p, None]
    assert lib.acrmi_score_hands(*args) == L.E_INVAL and lib.acrmi_last_error(None).startswith(b'acrmi_score_hands:')
    # the operator refuses host tensors and malformed arguments before it looks at the device
    ops = pkg('ops')
    with pytest.raises(L.AcrmiError):
        ops.pose_errors(torch.zeros(2, 5, 3), torch.zeros(2, 5, 3))


def test_rule_agrees_with_the_lapack_form():
    """tests/score_ref.py (the rule: Horn's quaternion, six Jacobi sweeps, float64) against the SVD form of score_cases on
    float32-representable point sets of every kind.  The largest difference stays <= 1e-8 m; it is printed, and DESIGN.md
    section 21 records it."""
    worst, worst_kind, rows = 0.0, None, 0
    for n in (3, 4, 21, 778):
        for noise in (0.0, 0.001, 0.02, 0.1):
            P, G, kinds = cases.make_rows(1000 + n, 12 if n < 778 else 6, n, noise=noise)
            for p, g, kind in zip(P, G, kinds):
                res = R.row_errors(p, g)
                if res['row_i'][1] == 0:
                    continue
                # the float64 errors of the rule: recompute them from its own arithmetic, before the rounding to float32
                exact = _rule_errors_f64(p, g)
                ref = cases.umeyama_errors(p, g)
                d = float(np.abs(exact - ref).max())
                if d > worst:
                    worst, worst_kind = d, (n, kind, noise)
                rows += 1
                assert abs(float(res['row_f'][1]) - ref.mean()) <= 1e-8 + 6e-8 * ref.mean(), (n, kind)
    print('largest |rule - LAPACK| over %d point sets: %.3g m at %s' % (rows, worst, worst_kind))
    assert rows > 100 and worst <= 1e-8, (worst, worst_kind)


def _rule_errors_f64(p, g):
    """The rule's e_pa of one row in float64, all points counted (the arithmetic of score_ref.row_errors, not rounded)."""
    n = p.shape[0]
    T = R.threads(n)
    Pd, Gd = p.astype(np.float64), g.astype(np.float64)
    m = R.tree_sum(np.concatenate([Pd, Gd], 1), T)
    muP, muG = m[0:3] / float(n), m[3:6] / float(n)
    pc, gc = Pd - muP, Gd - muG
    prod = np.stack([pc[:, a] * gc[:, b] for a in range(3) for b in range(3)] +
                    [(pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1]) + pc[:, 2] * pc[:, 2]], 1)
    r = R.tree_sum(prod, T)
    q, lam = R.horn(r[:9].reshape(3, 3))
    return R.norm3(((lam / r[9]) * R.rot(R.quat_matrix(q), pc) + muG) - Gd)


def test_rule_edge_rows():
    """What has no error: fewer than three counted points, coincident points, an invalid root, bad origins; -1 is 'not counted'."""
    g = np.random.default_rng(3)
    P, G = g.normal(0, 0.05, (21, 3)).astype(np.float32), g.normal(0, 0.05, (21, 3)).astype(np.float32)
    res = R.row_errors(P, G, root=9)
    assert res['row_i'].tolist() == [21, 21] and res['e_ra'][9] == 0 and (res['e_pa'] >= 0).all()
    assert np.float32(R.row_errors(P, G, root=9)['row_f'][0]) == res['row_f'][0]
    valid = np.ones(21, np.uint8)
    valid[9] = 0
    res = R.row_errors(P, G, valid=valid, root=9)      # the root does not count: no e_ra at all, e_pa over the other 20
    assert res['row_i'].tolist() == [0, 20] and (res['e_ra'] == -1).all() and res['e_pa'][9] == -1 and res['row_f'][0] == -1
    valid[:] = 0
    valid[:2] = 1
    res = R.row_errors(P, G, valid=valid)              # two points: root-aligned on zero origins, no Procrustes
    assert res['row_i'].tolist() == [2, 0] and res['row_f'][2] == -1 and (res['xform'] == [0, 0, 0, 0, -1, 0, 0, 0]).all()
    same = np.repeat(P[:1], 21, 0)
    assert R.row_errors(same, G)['row_i'].tolist() == [21, 0]      # vP = 0
    bad = P.copy()
    bad[4, 1] = np.nan
    bad[5, 0] = np.inf
    res = R.row_errors(bad, G, root=9, trans=np.array([0.1, 0.2, 0.3], np.float32))
    assert res['row_i'].tolist() == [19, 19] and res['e_ra'][4] == res['e_ra'][5] == res['e_pa'][4] == -1
    assert res['row_f'][3] == np.float32(R.norm3((P[9].astype(np.float64) + np.array([0.1, 0.2, 0.3], np.float32)) - G[9]))
    assert R.row_errors(P, G, oP=np.array([0, np.inf, 0], np.float32), oG=np.zeros(3, np.float32))['row_i'].tolist() == [0, 21]
    big = (P * np.float32(3e19 / 0.05)).astype(np.float32)      # 3e19 coordinates are finite: counted, and nothing overflows
    res = R.row_errors(big, G)
    assert res['row_i'].tolist() == [21, 21] and np.isfinite(res['e_ra']).all() and np.isfinite(res['e_pa']).all()
    # an identity fit: scale 1, the unit quaternion, zero translation and zero error up to rounding
    res = R.row_errors(P, P.copy())
    assert abs(res['row_f'][2] - 1) < 1e-6 and abs(abs(res['xform'][0]) - 1) < 1e-6 and res['e_pa'].max() < 1e-9
    # rows: the states and the pair term
    assert [R.row_state(gp, 2, fl) for gp, fl in ((0, None), (1, 0.6), (1, 0.5), (0, np.nan), (2, 1.0), (-1, 1.0), (-2 ** 31, 1.0))] == \
        [2, 2, 1, 1, 0, 0, 0]
    pred, gt = np.stack([P, P + 1]), np.stack([G, G])
    trans = np.array([[0, 0, 0], [0.5, 0, 0]], np.float32)
    out = R.pose_errors(pred, gt, root=9, trans=trans, n_groups=2, group=np.array([0, 1]))
    assert out['pair_err'].shape == (1,) and abs(out['pair_err'][0] - np.sqrt(1.5 ** 2 + 2)) < 1e-6
    assert (R.pose_errors(pred, gt, root=9, trans=trans, n_groups=2, group=np.array([0, 2]))['pair_err'] == -1).all()


def test_summary_arithmetic_on_a_hand_made_board():
    S = pkg('score')
    sets, G, bins, width = (3, 2), 2, 4, 0.01
    offs, pair_at, total = S.board_layout(sets, G, bins)
    words = np.zeros(total, np.int64)
    f = words.view(np.float64)
    gw = S.group_words(3, bins)
    # joints, group 0: per-joint sums 0.03, 0.06, 0 over counts 3, 2, 0; Procrustes sums 0.01, 0.01, 0.02 over 1, 1, 2
    f[0:3], f[3:6] = (0.03, 0.06, 0.0), (0.01, 0.01, 0.02)
    words[6:9], words[9:12] = (3, 2, 0), (1, 1, 2)
    words[12:17] = (2, 1, 0, 1, 1)          # errors in bins 0, 0, 1, 3 and one beyond the range
    words[17:19] = (3, 1)                    # rows scored, missed
    # joints, group 1: one joint, one error in bin 2
    f[gw + 1], words[gw + 7], words[gw + 12 + 2], words[gw + 17] = 0.025, 1, 1, 1
    # vertices, group 0
    v = offs[1]
    f[v:v + 2], words[v + 4:v + 6] = (0.02, 0.04), (2, 2)
    # pairs: (0, 1) twice with sum 0.3, (1, 0) once with 0.5
    f[pair_at + 2], words[pair_at + 3], f[pair_at + 4], words[pair_at + 5] = 0.3, 2, 0.5, 1
    arrays, pairs = S.board_arrays(words, sets, G, bins)
    assert arrays[0]['sum_ra'][0].tolist() == [0.03, 0.06, 0.0] and arrays[0]['hist'][0].tolist() == [2, 1, 0, 1, 1]
    assert arrays[0]['scored'].tolist() == [3, 1] and pairs['pair_cnt'].tolist() == [[0, 2], [1, 0]]
    s = S.summarize(arrays, pairs, ('joints', 'verts'), width)
    g0, g1, al = s['groups'][0], s['groups'][1], s['all']
    assert np.isclose(g0['mpjpe'], 0.09 / 5) and np.isclose(g0['pa_mpjpe'], 0.04 / 4) and np.isclose(g0['mpvpe'], 0.06 / 4)
    assert np.isnan(g0['pa_mpvpe']) and np.isnan(g1['mpvpe'])
    assert np.allclose(g0['joints']['per_point_ra'][:2], [0.01, 0.03]) and np.isnan(g0['joints']['per_point_ra'][2])
    assert np.allclose(g0['joints']['per_point_pa'], [0.01, 0.01, 0.01])
    assert np.allclose(s['thresholds'], [0, 0.01, 0.02, 0.03, 0.04])
    assert np.allclose(g0['joints']['pck'], [0, 2 / 5, 3 / 5, 3 / 5, 4 / 5])
    # the trapezoid rule over the four bins, divided by the range
    assert np.isclose(g0['joints']['auc'], ((0 + .4) / 2 + (.4 + .6) / 2 + (.6 + .6) / 2 + (.6 + .8) / 2) / 4)
    assert np.allclose(g1['joints']['pck'], [0, 0, 0, 1, 1]) and np.isclose(g1['mpjpe'], 0.025)
    assert np.isclose(al['mpjpe'], (0.09 + 0.025) / 6) and np.allclose(al['joints']['pck'], [0, 2 / 6, 3 / 6, 4 / 6, 5 / 6])
    assert (g0['scored'], g0['missed'], al['scored'], al['missed']) == (3, 1, 4, 1)
    assert np.isclose(g0['mrrpe'], 0.15) and np.isclose(g1['mrrpe'], 0.5) and np.isclose(al['mrrpe'], 0.8 / 3) and al['n_pairs'] == 3
    assert np.isnan(s['mrrpe_pairs'][0, 0]) and np.isclose(s['mrrpe_pairs'][0, 1], 0.15)
    empty = S.summarize(*S.board_arrays(np.zeros(total, np.int64), sets, G, bins), ('joints', 'verts'), width)
    assert np.isnan(empty['all']['mpjpe']) and np.isnan(empty['all']['joints']['auc']) and empty['all']['scored'] == 0
    with pytest.raises(ValueError):
        S.board_arrays(words[:-1], sets, G, bins)


def test_score_keys_of_the_hand_dicts():
    """gt= adds 'mpjpe', 'pa_mpjpe', 'mpvpe', 'pa_mpvpe' to every hand dict, and only then; nan for a hand without truth."""
    from importlib import import_module
    main = import_module(pkg().__name__ + '.acr.main')
    g = np.random.default_rng(0)
    B, K = 2, 2
    out = {'slots': g.normal(size=(B, K, 2, 176)).astype(np.float32), 'verts': np.zeros((B, K, 2, 778, 3), np.float32),
           'joints': np.zeros((B, K, 2, 21, 3), np.float32), 'pj2d': np.zeros((B, K, 2, 21, 2), np.float32),
           'pj2d_org': np.zeros((B, K, 2, 21, 2), np.float32), 'cam_trans': np.zeros((B, K, 2, 3), np.float32)}
    out['slots'][..., 0] = np.array([[[1, 1], [1, 0]], [[0, 1], [0, 0]]], np.float32)
    plain = main.results_from_out(out, ['a', 'b'])
    keys = set(plain['a'][0])
    assert not keys & set(pkg('score').SCORE_KEYS)
    rows = np.full((B * K * 2, 4), -1, np.float32)
    rows[:, 0] = np.arange(8) * 0.001 + 0.001      # row (b*K + k)*2 + h
    rows[:, 1] = rows[:, 0] / 2
    rows[1] = -1                                    # (frame a, rank 0, right): no truth
    out['score'] = {'joints': rows, 'verts': None}
    res = main.results_from_out(out, ['a', 'b'])
    a = res['a']      # lefts of rank 0, 1, then the right of rank 0
    assert all(set(h) == keys | set(pkg('score').SCORE_KEYS) for h in a + res['b'])
    assert np.allclose([h['mpjpe'] for h in a[:2]], [0.001, 0.003]) and np.allclose([h['pa_mpjpe'] for h in a[:2]], [0.0005, 0.0015])
    assert np.isnan(a[2]['mpjpe']) and np.isnan(a[2]['pa_mpjpe']) and all(np.isnan(h['mpvpe']) and np.isnan(h['pa_mpvpe']) for h in a)
    assert np.isclose(res['b'][0]['mpjpe'], 0.006) and a[0]['mpjpe'].dtype == np.float32
    out['score']['verts'] = rows * 2
    assert np.isclose(main.results_from_out(out, ['a', 'b'])['a'][1]['mpvpe'], 0.006)
    for bad in (dict(gt=[1]), dict(gt={'verts': 1}), dict(gt=None, board=object()), dict(gt={'joints': 1}, board=object())):
        with pytest.raises(ValueError):
            main._check_score(bad.get('gt'), bad.get('board'))
    main._check_score(None, None)


def test_plan_stand_alone_program(tmp_path):
    """tools/score_check.cpp: csrc/score_plan.h against a plain restatement as a program of its own.  The plain build must
    pass; the build with the address and undefined-behaviour sanitizers must pass as well where the host compiler can make
    one that starts - which of the two ran is printed."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        assert os.path.exists(hipcc), 'no C++ compiler'
        cmd = [hipcc, '-x', 'c++']
    else:
        cmd = [cxx]
    src = os.path.join(ROOT, 'tools', 'score_check.cpp')
    cmd += ['-std=c++17', '-O1', '-g', '-ffp-contract=off', src, '-o']
    plain = str(tmp_path / 'score_check')
    subprocess.run(cmd + [plain], check=True, capture_output=True)
    run = subprocess.run([plain], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    ran = None
    for label, extra in (('static', san + ['-static-libasan', '-static-libubsan']), ('shared', san)):
        exe = str(tmp_path / ('score_check_' + label))
        if subprocess.run(cmd + [exe] + extra, capture_output=True).returncode != 0:
            continue
        run = subprocess.run([exe], capture_output=True, text=True)
        if 'does not come first in initial library list' in run.stderr:
            continue
        ran = label
        assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
        break
    print('sanitizer variant that ran: %s' % ran)
