"""Scoring against ground truth on the GPU (csrc/score.hip) against the numpy restatement
(tests/score_ref.py) FOR EQUALITY: e_ra, e_pa, row_f, row_i, xform, the pair terms and the board, bit for bit - the one thing
not compared is the payload of a NaN.  Every e_pa is also within 1e-7 m of the LAPACK form (tests/score_cases.py): the fp32
rounding of an output below 0.5 m (3e-8) plus the largest difference between the rule and LAPACK (5.5e-9) plus margin.
Then the engine level: Engine.score, EnginePool.score and forward_batch(gt=, board=) against the operator on the same tensors."""
import numpy as np
import pytest
import torch

import score_cases as cases
import score_ref as R
from conftest import pkg
from contact_cases import eng, frames3, near_sd, placed      # (fixtures)

pytestmark = pytest.mark.gpu

FLOAT_KEYS = ('e_ra', 'e_pa', 'row_f', 'xform', 'pair_err')
INT_MIN = -2 ** 31


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def ulps(a, b):
    """The largest distance in float32 steps between two arrays of finite values of one sign pattern (for the messages)."""
    ia, ib = a.astype(np.float32).view(np.int32).astype(np.int64), b.astype(np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max()) if a.size else 0


def assert_equal(got, want, what=''):
    assert np.array_equal(got['row_i'], want['row_i']), (what, 'row_i', np.argwhere(got['row_i'] != want['row_i'])[:4])
    for k in FLOAT_KEYS:
        if k in got:
            print('%s %s: largest difference %d ulp' % (what, k, ulps(got[k], want[k])))
            assert same_bits(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:4], ulps(got[k], want[k]))


def host(res):
    return {k: v.cpu().numpy() for k, v in res.items() if k in FLOAT_KEYS + ('row_i',)}


def cuda(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def make_case(seed, N, n, G, full):
    """The inputs of one operator call as host arrays.  full = False: the points alone; 'root', 'origin' or 'zero' (where the
    origins come from): valid bytes, trans, groups (INT_MIN, -1 and G among them), flags of arbitrary bytes, NaN / inf / 3e19
    coordinates, a row without a valid point, a row with an invalid root."""
    g = np.random.default_rng(seed)
    P, G_, kinds = cases.make_rows(seed, N, n)
    c = dict(pred=P, gt=G_, valid=None, root=-1, origin=None, group=None, flags=None, trans=None, n_groups=G)
    if not full:
        return c
    c['root'] = int(g.integers(0, n)) if full == 'root' else -1
    if full == 'origin':
        c['origin'] = (g.normal(0, 0.05, (N, 3)).astype(np.float32), g.normal(0, 0.05, (N, 3)).astype(np.float32))
    valid = g.choice(np.array([0, 1, 1, 1, 7, 255], np.uint8), (N, n))
    c['trans'] = g.normal(0, 0.3, (N, 3)).astype(np.float32)
    c['group'] = g.integers(0, G, N).astype(np.int32)
    flags = np.ones(N, np.float32)
    if N >= 3:
        P[0, g.integers(0, n), 1] = np.nan
        G_[1, g.integers(0, n), 2] = np.inf
        P[2 % N, g.integers(0, n), 0] = -np.inf
        flags[1] = 0.6
    if N >= 16:
        P[3] = (P[3] * np.float32(3e19 / 0.05)).astype(np.float32)      # finite: counted
        valid[4] = 0                                                     # a row without a valid point
        valid[5, max(c['root'], 0)] = 0                                  # a row with an invalid root
        valid[6] = 1
        P[6, max(c['root'], 0)] = np.nan                                 # a root that is not finite
        c['group'][7:11] = (INT_MIN, -1, G, 2 ** 31 - 1)
        c['trans'][11, 1] = np.nan
        if c['origin'] is not None:
            c['origin'][0][12, 2] = np.inf
        raw = g.integers(0, 256, 4 * N, dtype=np.uint8).view(np.float32)      # flags of arbitrary bytes
        flags[16:] = raw[16:]
        flags[13:16] = (0.5, np.nan, 0.0)
        special = np.array([0x7fc00000, 0x3f000000, 0x7f800000, 0xff800000, 0x3f000001, 0x00000001, 0x3f800000, 0xbf800000],
                           np.uint32).view(np.float32)      # NaN, 0.5, inf, -inf, just above 0.5, a denormal, 1, -1
        m = max(0, min(N, 28) - 20)
        flags[20:20 + m] = special[:m]
    c['valid'], c['flags'] = valid, flags
    return c


def run(c, **kw):
    ops = pkg('ops')
    res = ops.pose_errors(cuda(c['pred']), cuda(c['gt']), valid=cuda(c['valid']), root=c['root'],
                          origin=None if c['origin'] is None else tuple(cuda(o) for o in c['origin']), group=cuda(c['group']),
                          flags=cuda(c['flags']), trans=cuda(c['trans']), n_groups=c['n_groups'], xform=True, pairs=True, **kw)
    return res


def reference(c):
    return R.pose_errors(c['pred'], c['gt'], valid=c['valid'], root=c['root'], origin=c['origin'], group=c['group'],
                         flags=c['flags'], trans=c['trans'], n_groups=c['n_groups'])


def check_lapack(c, got):
    """Every e_pa within 1e-7 m of the SVD form over the points the kernel counted (errors below 0.5 m only)."""
    worst = 0.0
    for r in range(c['pred'].shape[0]):
        on = got['e_pa'][r] >= 0
        if not on.any() or np.abs(c['pred'][r][on]).max() > 10:
            continue
        ref = cases.umeyama_errors(c['pred'][r], c['gt'][r], on)
        assert ref[on].max() < 0.5
        worst = max(worst, float(np.abs(got['e_pa'][r][on].astype(np.float64) - ref[on]).max()))
    assert worst <= 1e-7, worst
    return worst


SHAPES = [(n, N) for n in (1, 2, 3, 21, 63, 64, 65, 257, 778) for N in (1, 3)] + [(21, 130), (64, 130), (65, 130), (778, 130),
                                                                                    (4000, 2)]


@pytest.mark.parametrize('n,N', SHAPES)
def test_operator_equals_the_rule(n, N):
    G = {1: 1, 2: 2, 3: 2, 130: 16}[N]
    for full in ((False, 'root', 'origin', 'zero') if N > 1 else (False,)):
        c = make_case(n * 1000 + N, N, n, G, full)
        got = host(run(c))
        want = reference(c)
        assert_equal(got, want, (n, N, full))
        worst = check_lapack(c, got)
        print('n %d N %d full %s: largest |e_pa - LAPACK| %.3g m' % (n, N, full, worst))
        if N == 130 and full:      # the cases are not trivial: every kind of row is there
            assert (got['row_i'][:, 1] > 0).sum() > 20
            assert (got['row_i'][7:11] == 0).all() and (got['e_ra'][7:11] == -1).all() and (got['row_f'][7:11] == -1).all()
            assert got['row_i'][4].tolist() == [0, 0] and got['row_f'][11, 3] == -1
            if full == 'root':      # an invalid root, a root that is not finite: no e_ra in the row
                assert got['row_i'][5, 0] == 0 and got['row_i'][6, 0] == 0
            if full == 'origin':    # an origin that is not finite
                assert got['row_i'][12, 0] == 0
            assert np.isfinite(got['e_ra'][3][got['e_ra'][3] >= 0]).all()


def test_a_row_alone_equals_the_row_in_a_batch_and_calls_repeat():
    for n in (21, 257):
        c = make_case(77 + n, 24, n, 2, 'root' if n == 21 else 'origin')
        whole, again = host(run(c)), host(run(c))
        for k in FLOAT_KEYS + ('row_i',):
            assert same_bits(whole[k], again[k]) if k != 'row_i' else np.array_equal(whole[k], again[k]), k
        for r in (0, 1, 5, 17, 23):
            one = dict(c, pred=c['pred'][r:r + 1], gt=c['gt'][r:r + 1], valid=c['valid'][r:r + 1], group=c['group'][r:r + 1],
                       flags=c['flags'][r:r + 1], trans=c['trans'][r:r + 1],
                       origin=None if c['origin'] is None else tuple(o[r:r + 1] for o in c['origin']))
            alone = host(run(one))
            for k in ('e_ra', 'e_pa', 'row_f', 'xform'):
                assert same_bits(alone[k][0], whole[k][r]), (n, r, k)
            assert np.array_equal(alone['row_i'][0], whole['row_i'][r]) and alone['pair_err'].shape == (0,)


def board_host(board):
    sets, pairs = board.arrays()
    return [dict(s, **pairs) for s in sets]


def assert_board(got, want, what=''):
    for k, v in want.items():
        same = same_bits64(got[k], v) if v.dtype == np.float64 else np.array_equal(got[k], v)
        assert same, (what, k, np.argwhere(got[k] != v)[:4])


def same_bits64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize('n,G,bins,width,mode', [(21, 2, 100, 0.0005, 'root'), (21, 1, 1, 0.01, 'zero'), (65, 16, 100, 0.0005, 'origin'),
                                                  (778, 2, 100, 0.0005, 'origin'), (257, 16, 1, 0.5, 'root')])
def test_board_is_the_sequential_sum_of_the_outputs(n, G, bins, width, mode):
    """The board equals the fp64 sum, in row order, of the kernel's own fp32 outputs; 2B rows in one call equal two calls of B
    rows; reset() clears it."""
    E = pkg('engine')
    N = 48
    c = make_case(500 + n + G, N, n, G, mode)
    res = run(c)
    got = host(res)
    board = E.ScoreBoard(0, sets=(n,), names=('points',), n_groups=G, n_bins=bins, bin_width=width)
    want = R.new_board(n, G, bins)
    for _ in range(2):      # the second call continues from the first
        board.add(0, res, group=cuda(c['group']), flags=cuda(c['flags']))
        R.board_add(want, got['e_ra'], got['e_pa'], got['pair_err'], c['group'], c['flags'], G, bins, width)
        assert_board(board_host(board)[0], want, (n, G, bins))
    assert want['hist'].sum() == 2 * (got['e_ra'] >= 0).sum() and want['scored'].sum() + want['missed'].sum() <= 2 * N
    assert want['missed'].sum() > 0 and want['pair_cnt'].sum() > 0 and (want['hist'][:, -1].sum() > 0 or bins > 1)
    # two halves
    halves = E.ScoreBoard(0, sets=(n,), names=('points',), n_groups=G, n_bins=bins, bin_width=width)
    for lo in (0, N // 2):
        part = {k: c[k][lo:lo + N // 2] for k in ('pred', 'gt', 'valid', 'group', 'flags', 'trans')}
        part['origin'] = None if c['origin'] is None else tuple(o[lo:lo + N // 2] for o in c['origin'])
        r = run(dict(c, **part))
        halves.add(0, r, group=cuda(part['group']), flags=cuda(part['flags']))
    once = E.ScoreBoard(0, sets=(n,), names=('points',), n_groups=G, n_bins=bins, bin_width=width)
    once.add(0, res, group=cuda(c['group']), flags=cuda(c['flags']))
    assert torch.equal(halves.words, once.words)
    s = once.summary()
    assert s['all']['scored'] == int(want['scored'].sum()) // 2 and len(s['groups']) == G and 'points' in s['all']
    once.reset()
    assert not once.words.any()


def as_rows(out, K):
    """The tensors Engine.score reads as the rows of the operator."""
    L = pkg('_lib')
    N = out['slots'].shape[0] * K * 2
    return (out['joints'].reshape(N, 21, 3), out['verts'].reshape(N, 778, 3), out['slots'].reshape(N, L.SLOT)[:, L.SLOT_FLAG].contiguous(), N)


def truth_for(eng, out, K, seed):
    """Ground truth for the hands of `out`: the meshes and joints of perturbed MANO parameters would do; here the prediction
    itself, moved by a few millimetres of noise, with some joints marked invalid (never the root) and a few rows without truth."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    lead = tuple(out['slots'].shape[:-1])
    gt = {'joints': out['joints'] * 1.05 + 0.004 * torch.randn(out['joints'].shape, device='cuda', generator=g),
          'verts': out['verts'] * 1.05 + 0.004 * torch.randn(out['verts'].shape, device='cuda', generator=g)}
    valid = torch.rand(lead + (21,), device='cuda', generator=g) > 0.2
    valid[..., 9] = True
    gt['joint_valid'] = valid
    return gt


def by_operator(ops, out, gt, K, ct, n_groups=2, group=None, root=9):
    joints, verts, flags, N = as_rows(out, K)
    grp = torch.arange(N, dtype=torch.int32, device='cuda') % 2 if group is None else group.reshape(N).to(torch.int32)
    gj = gt['joints'].reshape(N, 21, 3)
    trans = None if ct is None else ct.reshape(N, 3)
    jv = None if gt.get('joint_valid') is None else gt['joint_valid'].reshape(N, 21)
    rj = ops.pose_errors(joints, gj, valid=jv, root=root, group=grp, flags=flags, trans=trans, n_groups=n_groups, pairs=True)
    rv = None
    if gt.get('verts') is not None:
        rv = ops.pose_errors(verts, gt['verts'].reshape(N, 778, 3), origin=(joints[:, root].contiguous(), gj[:, root].contiguous()),
                             group=grp, flags=flags, trans=trans, n_groups=n_groups)
    return rj, rv, grp, flags


def assert_score(got, rj, rv, what=''):
    for name, want in (('joints', rj), ('verts', rv)):
        if want is None:
            assert got[name] is None
            continue
        for k in ('e_ra', 'e_pa', 'row_f', 'row_i'):
            assert torch.equal(got[name][k].view(torch.int32), want[k].view(torch.int32)), (what, name, k)
    assert torch.equal(got['pair_err'].view(torch.int32), rj['pair_err'].view(torch.int32)), what


def test_engine_score_matches_the_operator(eng, frames3):
    ops, E = pkg('ops'), pkg('engine')
    for B in (2, 3):
        out = eng.forward(frames3[:B], project=True)
        gt = truth_for(eng, out, 1, B)
        own = ops.cam_trans(out['joints'].view(-1, 21, 3), out['pj2d'].view(-1, 21, 2), focal_length=1265.0).view(B, 2, 3)
        board, want = E.ScoreBoard(0), E.ScoreBoard(0)
        got = eng.score(out, gt, board=board)              # the network's own camera, computed by the call
        rj, rv, grp, flags = by_operator(ops, out, gt, 1, own)
        assert_score(got, rj, rv, (B, 'own'))
        want.add(0, rj, group=grp, flags=flags)
        want.add(1, rv, group=grp, flags=flags)
        assert torch.equal(board.words, want.words)
        assert (got['joints']['n_pa'] > 0).sum() >= 4 and (got['pair_err'] >= 0).sum() >= 2      # (both hands of two frames are detected)
        ct = placed(B)[:, 0]
        got = eng.score(out, {'joints': gt['joints']}, cam_trans=ct)      # no vertex truth, no validity, no board
        rj, rv, _, _ = by_operator(ops, out, {'joints': gt['joints']}, 1, ct)
        assert_score(got, rj, None, (B, 'placed'))
    s = board.summary()
    assert s['all']['scored'] + s['all']['missed'] == 6 and 0 < s['all']['mpjpe'] < 0.5 and 0 < s['all']['pa_mpvpe'] < 0.02
    assert s['all']['n_pairs'] == int((got['pair_err'] >= 0).sum()) and s['groups'][0]['scored'] + s['groups'][1]['scored'] == s['all']['scored']
    # groups from the caller (one of them out of range: the row is not looked at), an invalid root joint, no root alignment
    group = torch.tensor([[0, 2], [1, 3], [INT_MIN, 0]], dtype=torch.int32).cuda()
    gt2 = dict(gt, group=group)
    gt2['joint_valid'] = gt['joint_valid'].clone()
    gt2['joint_valid'][0, 1, 9] = False
    got = eng.score(out, gt2, cam_trans=ct, n_groups=3)
    rj, rv, _, _ = by_operator(ops, out, gt2, 1, ct, n_groups=3, group=group)
    assert_score({'joints': got['joints'], 'verts': None, 'pair_err': got['pair_err']}, rj, None, 'groups')
    keep = torch.ones(6, dtype=torch.bool)
    keep[1] = False      # the vertices of the hand whose root joint is invalid have no e_ra (the operator knows no origin validity)
    for k in ('e_ra', 'e_pa', 'row_f', 'row_i'):
        assert torch.equal(got['verts'][k][keep].view(torch.int32), rv[k][keep].view(torch.int32)), k
    assert (got['verts']['e_ra'][1] == -1).all() and got['verts']['n_ra'][1] == 0 and got['joints']['n_ra'][1] == 0
    assert got['joints']['n_ra'][3] == 0 and got['joints']['n_ra'][4] == 0      # groups 3 and INT_MIN
    eng.set_center_idx(-1)
    try:
        got = eng.score(out, gt, cam_trans=ct)
    finally:
        eng.set_center_idx(9)
    rj = ops.pose_errors(*as_rows(out, 1)[:1], gt['joints'].reshape(6, 21, 3), valid=gt['joint_valid'].reshape(6, 21), root=-1,
                         group=torch.arange(6, dtype=torch.int32).cuda() % 2, flags=as_rows(out, 1)[2], trans=ct.reshape(6, 3),
                         n_groups=2, pairs=True)
    assert torch.equal(got['joints']['e_ra'].view(torch.int32), rj['e_ra'].view(torch.int32))
    with pytest.raises(ValueError):
        eng.score(out, {'verts': gt['verts']})
    with pytest.raises(ValueError):
        eng.score(out, gt, max_hand=2)
    with pytest.raises(ValueError):
        eng.score(out, gt, board=E.ScoreBoard(0, sets=(21,), names=('joints',)))


def test_engine_score_max_hand_2(eng, frames3):
    ops, E, L = pkg('ops'), pkg('engine'), pkg('_lib')
    B, K = 2, 2
    out = eng.forward(frames3[:B], project=True, max_hand=K)
    out['slots'][:, :, :, L.SLOT_FLAG] = torch.tensor([[[1., 1], [1, 0]], [[0, 1], [1, 1]]]).cuda()
    gt = truth_for(eng, out, K, 5)
    ct = placed(B, K)
    board, want = E.ScoreBoard(0), E.ScoreBoard(0)
    got = eng.score(out, gt, board=board, max_hand=K, cam_trans=ct)
    rj, rv, grp, flags = by_operator(ops, out, gt, K, ct)
    assert got['joints']['e_ra'].shape == (B * K * 2, 21) and got['pair_err'].shape == (B * K,)
    assert_score(got, rj, rv, 'K=2')
    pe = got['pair_err'].cpu().numpy()      # pairs are (left rank k, right rank k), both flagged
    assert pe[0] >= 0 and pe[1] == -1 and pe[2] == -1
    want.add(0, rj, group=grp, flags=flags)
    want.add(1, rv, group=grp, flags=flags)
    assert torch.equal(board.words, want.words)
    s = board.summary()
    assert (s['all']['scored'], s['all']['missed'], s['all']['n_pairs']) == (6, 2, int((pe >= 0).sum()))


def test_three_calls_queue_without_a_host_visit(eng, frames3):
    E = pkg('engine')
    out = eng.forward(frames3[:2], project=True)
    gt = truth_for(eng, out, 1, 9)
    ct = placed(2)[:, 0]
    one = E.ScoreBoard(0)
    want = eng.score(out, gt, board=one, cam_trans=ct)
    board = E.ScoreBoard(0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        res = [eng.score(out, gt, board=board, cam_trans=ct), eng.score(out, gt, board=board), eng.score(out, gt, board=board, cam_trans=ct)]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert_score(res[0], want['joints'], want['verts'])
    assert_score(res[2], want['joints'], want['verts'])
    a, b = board.arrays()[0][0], one.arrays()[0][0]
    assert np.array_equal(a['cnt_ra'], 3 * b['cnt_ra']) and np.array_equal(a['scored'], 3 * b['scored'])


def test_pool_score_on_the_tickets_stream(eng, near_sd, mano_tables, frames3):
    E = pkg('engine')
    img = frames3[:2]
    out = eng.forward(img, project=True)
    gt = truth_for(eng, out, 1, 11)
    ct = placed(2)[:, 0]
    want_board = E.ScoreBoard(0)
    want = [eng.score(out, gt, board=want_board), eng.score(out, gt, board=want_board, cam_trans=ct)]
    for k in range(2):
        eng.score(out, gt, board=want_board, cam_trans=ct if k % 2 else None)
    pool = E.EnginePool(0, n=2)
    pool.load_state_dict(near_sd, max_batch=2)
    pool.load_mano(mano_tables)
    board = E.ScoreBoard(0)      # shared by both contexts: updated in the order of the calls
    for k in range(4):
        t = pool.submit(img, project=True)
        got = pool.score(t, gt, board=board, cam_trans=ct if k % 2 else None)
        pool.collect(t)
        assert_score(got, want[k % 2]['joints'], want[k % 2]['verts'], k)
    assert torch.equal(board.words, want_board.words)
    with pytest.raises(RuntimeError):
        pool.score(t, gt)
    pool.close()


def test_forward_batch_score_keys_and_board(near_sd, mano_tables, frames3):
    ops, E, cfg, S = pkg('ops'), pkg('engine'), pkg('config'), pkg('score')
    acr = pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml']), state_dict=near_sd,
                              mano_tables=mano_tables, max_batch=2)
    img = frames3[:2]
    e = acr.model.engine(2)
    e.set_point_heads(True)      # (as forward_batch runs it: the towers at the decoded centres)
    try:
        out = e.forward(img, offsets=torch.tensor([[512., 512, 0, 0, 0, 0, 0, 0, 0, 0]]).repeat(2, 1), project=True)
    finally:
        e.set_point_heads(False)
    gt = truth_for(e, out, 1, 13)
    gt['group'] = torch.tensor([[0, 1], [0, 5]], dtype=torch.int32).cuda()      # the last hand has no truth
    plain = acr.forward_batch(img, ['a', 'b'])
    board = E.ScoreBoard(0)
    res = acr.forward_batch(img, ['a', 'b'], gt=gt, board=board)
    again = acr.forward_batch(img, ['a', 'b'])
    new = set(S.SCORE_KEYS)
    for k in plain:                                       # without gt= the dicts are what they were
        assert len(res[k]) == len(plain[k]) == len(again[k]) == 2
        for h0, h1, h2 in zip(plain[k], res[k], again[k]):
            assert set(h1) == set(h0) | new and set(h2) == set(h0) and not new & set(h0)
            assert all(np.array_equal(h0[f], h1[f]) and np.array_equal(h0[f], h2[f]) for f in h0)
    ct = ops.cam_trans(out['joints'].view(-1, 21, 3), out['pj2d'].view(-1, 21, 2), focal_length=acr.focal_length).view(2, 2, 3)
    rj, rv, grp, flags = by_operator(ops, out, gt, 1, ct, group=gt['group'])
    fj, fv = rj['row_f'].cpu().numpy(), rv['row_f'].cpu().numpy()
    for b, k in enumerate('ab'):
        for h, hand in enumerate(res[k]):
            row = 2 * b + h
            if (b, h) == (1, 1):
                assert all(np.isnan(hand[f]) for f in new)
                continue
            assert (hand['mpjpe'], hand['pa_mpjpe'], hand['mpvpe'], hand['pa_mpvpe']) == (fj[row, 0], fj[row, 1], fv[row, 0], fv[row, 1])
            assert 0 < hand['pa_mpjpe'] < hand['mpjpe'] < 0.5
    want = E.ScoreBoard(0)
    want.add(0, rj, group=grp, flags=flags)
    want.add(1, rv, group=grp, flags=flags)
    assert torch.equal(board.words, want.words)
    raw = acr.forward_raw_batch(torch.from_numpy(np.ascontiguousarray(img.cpu().numpy()[..., ::-1])).cuda(), ['a', 'b'], gt=gt, board=board)
    s = board.summary()['all']
    assert all(new <= set(h) for k in raw for h in raw[k]) and s['scored'] + s['missed'] == 6 and s['scored'] >= 3
    with pytest.raises(ValueError):
        acr.forward_batch(img, ['a', 'b'], board=board)
    with pytest.raises(ValueError):
        acr.forward_batch(img, ['a', 'b'], gt={'verts': gt['verts']})
