"""The fused MANO fitter on the GPU: Engine.mano_fit (acrmi_mano_fit, csrc/mano_fit.hip) against the float64 loop of
tests/mano_fit_ref.py - its gradient, short trajectories, the fits of DESIGN.md section 26 -, the carried state, determinism
and row isolation, ManoLayer.fit, and the calls that must not wait.  `pytest -m gpu`.

THE BARS.  A gradient row (pose, betas, trans, cam apart) is measured as max|g - g64| / max|g64| and held to the bar of
tests/test_gpu_mano_grad.py: 8 x the error of the reference ManoLayer's own float32 gradients (tests/golden/mano_grad.npz).  A
trajectory is held to 8 x the distance of the float32 loop from the float64 loop on the same problem, computed here."""
import numpy as np
import pytest
import torch

import mano_fit_ref as fref
import mano_grad_ref as ref
from conftest import golden, pkg

pytestmark = pytest.mark.gpu

POOL = 67
SIDES = ('left', 'right')
CENTERS = (None, 9, 0, 12)
KINDS = ('joints', 'kp2d', 'verts', 'lam_pose', 'lam_beta')
ROWS = (('pose', 0, 48), ('betas', 48, 58), ('trans', 58, 61), ('cam', 61, 64))
ALL = ('root', 'pose', 'betas', 'trans', 'cam')


@pytest.fixture(scope='module')
def eng(mano_tables):
    e = pkg('engine').Engine(0)
    e.load_mano(mano_tables)
    return e


@pytest.fixture(scope='module')
def bar(mano_tables):
    y, _ = ref.yardstick(mano_tables, golden('mano_grad.npz'))
    print('yardstick %.3g, bar %.3g' % (y, 8 * y))
    assert y < 1e-5
    return 8 * y


class Pool(object):
    """67 seeded hands, left and right mixed, with non-trivial states and targets; row 0 has a zero pose, row 1 a root rotation
    beyond 3 rad, row 2 large betas.  The float64 gradients are computed once per (center_idx, kind) and never written to."""

    def __init__(self, tables):
        rng = np.random.RandomState(11)
        f = lambda a: a.astype(np.float32)
        self.tables = tables
        self.init = {'poses': f(rng.randn(POOL, 48) * 0.3), 'betas': f(rng.randn(POOL, 10) * 0.5),
                     'trans': f(rng.randn(POOL, 3) * 0.05),
                     'cam': f(np.stack([rng.uniform(4, 8, POOL), rng.uniform(-0.3, 0.3, POOL), rng.uniform(-0.3, 0.3, POOL)], 1))}
        self.init['poses'][0] = 0
        self.init['poses'][1, :3] = np.array([2.0, -2.5, 1.5], np.float32)
        self.init['betas'][2] = f(rng.randn(10) * 3.0)
        self.side = (rng.rand(POOL) < 0.5).astype(np.int32)
        self.side[:3] = (0, 1, 0)
        self.t = {'joints': f(rng.randn(POOL, 21, 3) * 0.1), 'kp2d': f(rng.randn(POOL, 21, 2) * 0.5),
                  'verts': f(rng.randn(POOL, 778, 3) * 0.1), 'w_joints': f(rng.uniform(0.2, 1.0, (POOL, 21))),
                  'w_kp2d': f(rng.uniform(0.2, 1.0, (POOL, 21))), 'w_verts': f(rng.uniform(0.2, 1.0, POOL) / 100),
                  'prior': f(rng.randn(POOL, 58) * 0.2)}
        self.d_init = {k: torch.from_numpy(v).cuda() for k, v in self.init.items()}
        self.d_side = torch.from_numpy(self.side).cuda()
        self.d = {k: torch.from_numpy(v).cuda() for k, v in self.t.items()}
        self._g64 = {}

    @staticmethod
    def kwargs(kind, t, rows=slice(None)):
        """The arguments (of Engine.mano_fit and of fref.Fit alike) that make `kind` the only source of a gradient."""
        if kind in ('joints', 'kp2d', 'verts'):
            return {kind: t[kind][rows], 'w_' + kind: t['w_' + kind][rows]}
        return {'prior': t['prior'][rows], kind: 0.37}

    def g64(self, center_idx, kind):
        key = (center_idx, kind)
        if key not in self._g64:
            g = np.zeros((POOL, 64))
            for s, name in enumerate(SIDES):
                rows = np.nonzero(self.side == s)[0]
                fit = fref.Fit(self.tables[name], name, len(rows), center_idx, init={k: v[rows] for k, v in self.init.items()},
                               **self.kwargs(kind, self.t, rows))
                g[rows] = fit.gradient()[1]
            self._g64[key] = g
        return self._g64[key]


@pytest.fixture(scope='module')
def pool(mano_tables):
    return Pool(mano_tables)


def _fit(eng, pool, H, center_idx, rows=None, **kw):
    rows = slice(0, H) if rows is None else rows
    return eng.mano_fit(pool.d_side[rows], init={k: v[rows] for k, v in pool.d_init.items()}, center_idx=center_idx, **kw)


def _row_errors(g, g64):
    """ref.row_errors; a row whose true gradient is all zero must be exactly zero."""
    zero = np.abs(g64).max(1) == 0
    assert not g[zero].any()
    e = np.zeros(len(g))
    if (~zero).any():
        e[~zero] = ref.row_errors(g[~zero], g64[~zero])
    return e


@pytest.mark.parametrize('center_idx', CENTERS)
@pytest.mark.parametrize('H', (1, 2, 3, POOL))
def test_gradient_against_float64(eng, pool, bar, H, center_idx):
    """steps = 1 with the gradient asked for: every cotangent source alone, on the sparse and on the dense path, every row of
    the pose, betas, trans and cam groups within 8 x the yardstick of the float64 statement's gradient."""
    for kind in KINDS:
        g64 = pool.g64(center_idx, kind)[:H]
        for dense in ((True,) if kind == 'verts' else (False, True)):
            out = _fit(eng, pool, H, center_idx, steps=1, grad=True, free=ALL, dense=dense, **Pool.kwargs(kind, pool.d, slice(0, H)))
            g = out['grad'].cpu().numpy()
            assert np.isfinite(g).all()
            for name, lo, hi in ROWS:
                e = _row_errors(g[:, lo:hi], g64[:, lo:hi])
                print('H %d center %s %s %s %s: worst %.3g (row %d), bar %.3g'
                      % (H, center_idx, kind, 'dense' if dense else 'sparse', name, e.max(), e.argmax(), bar))
                assert e.max() <= bar


class Problem3D(object):
    """test_it_fits' problem: 8 right hands, RandomState(3), center_idx None, from zeros, w3 = 1/21, lr 0.02; the float64 and
    float32 loops at 1, 2, 7, 20 and 300 steps, computed once."""
    MARKS = (1, 2, 7, 20)

    def __init__(self, tables):
        poses, betas = fref.problem_3d()
        self.joints = fref.targets_of(tables['right'], 'right', poses, betas, None)[1]
        self.at = {}
        for dtype in (torch.float64, torch.float32):
            fit, done = fref.Fit(tables['right'], 'right', 8, None, joints=self.joints, dtype=dtype), 0
            for m in self.MARKS:
                fit.run(m - done)
                done = m
                self.at[(dtype, m)] = fit.params()
            if dtype == torch.float64:
                fit.run(300 - done)
                self.first, self.last = fit.first, fit.last


@pytest.fixture(scope='module')
def problem3d(mano_tables):
    return Problem3D(mano_tables)


def _dist(a, b):
    return np.abs(a[:, :48] - b[:, :48]).max(), np.abs(a[:, 48:58] - b[:, 48:58]).max()


@pytest.mark.parametrize('dense', (False, True))
def test_short_trajectories(eng, problem3d, dense):
    """After 1, 2, 7 and 20 steps from zeros the parameters are within 8 x (the distance of the float32 loop from the float64
    loop) of the float64 loop's, pose and betas apart."""
    side = torch.ones(8, dtype=torch.int32, device='cuda')
    y = torch.from_numpy(problem3d.joints).cuda()
    for m in Problem3D.MARKS:
        out = eng.mano_fit(side, joints=y, steps=m, center_idx=None, lr=0.02, dense=dense)
        got = torch.cat([out['poses'], out['betas']], 1).double().cpu().numpy()
        p64, p32 = problem3d.at[(torch.float64, m)], problem3d.at[(torch.float32, m)]
        yard, mine = _dist(p32, p64), _dist(got, p64)
        print('%s, %d steps: float32 loop %.3g / %.3g, kernel %.3g / %.3g (pose / betas)'
              % ('dense' if dense else 'sparse', m, yard[0], yard[1], mine[0], mine[1]))
        assert mine[0] <= 8 * yard[0] and mine[1] <= 8 * yard[1]


@pytest.mark.parametrize('dense', (False, True))
def test_it_fits_3d(eng, problem3d, dense):
    """One call of 300 steps on test_it_fits' problem: the loss of every hand falls at least 100-fold."""
    side = torch.ones(8, dtype=torch.int32, device='cuda')
    y = torch.from_numpy(problem3d.joints).cuda()
    out = eng.mano_fit(side, joints=y, steps=300, center_idx=None, lr=0.02, dense=dense)
    loss = out['loss'].double().cpu().numpy()
    # the loss at the returned parameters, through the forward kernel
    joints = eng.mano(out['poses'], out['betas'], side, center_idx=None)[1]
    final = ((joints - y) ** 2).sum(-1).mean(-1).double().cpu().numpy()
    print('%s: first %s' % ('dense' if dense else 'sparse', ' '.join('%.3g' % v for v in loss[:, 0])))
    print('fold (last evaluated step) %s' % ' '.join('%.0f' % v for v in loss[:, 0] / loss[:, 1]))
    print('fold (returned parameters) %s' % ' '.join('%.0f' % v for v in loss[:, 0] / final))
    print('relative difference of the last loss from the float64 loop %s'
          % ' '.join('%.2g' % v for v in np.abs(loss[:, 1] - problem3d.last) / problem3d.last))
    assert np.allclose(loss[:, 0], problem3d.first, rtol=1e-4)
    assert (loss[:, 1] * 100 <= loss[:, 0]).all() and (final * 100 <= loss[:, 0]).all()


def test_it_fits_2d(eng):
    """8 left hands against the pj2d of Engine.mano(cam=) at center_idx 9, from zero pose and betas with cam = (5, 0, 0): root,
    pose, betas and cam free, lam_pose = lam_beta = 1e-3: the loss of every hand falls at least 10-fold in 300 steps."""
    poses, betas, cam = fref.problem_2d()
    side = torch.zeros(8, dtype=torch.int32, device='cuda')
    pj = eng.mano(torch.from_numpy(poses).cuda(), torch.from_numpy(betas).cuda(), side, center_idx=9,
                  cam=torch.from_numpy(cam).cuda())[3]['pj2d']
    init = {'cam': torch.tensor([5.0, 0.0, 0.0], device='cuda').repeat(8, 1)}
    out = eng.mano_fit(side, kp2d=pj, init=init, free=('root', 'pose', 'betas', 'cam'), lam_pose=1e-3, lam_beta=1e-3, lr=0.02,
                       steps=300, center_idx=9)
    loss = out['loss'].double().cpu().numpy()
    print('2-D: fold %s' % ' '.join('%.0f' % v for v in loss[:, 0] / loss[:, 1]))
    assert (loss[:, 1] * 10 <= loss[:, 0]).all()
    assert not out['trans'].any()      # a frozen group that no term moves
    assert (out['cam'] != init['cam']).any()


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('dense', (False, True))
@pytest.mark.parametrize('split', ((1, 1), (7, 13), (0, 5)))
def test_state_carries_the_fit(eng, pool, split, dense):
    """One call of a + b steps equals a call of a steps followed by a call of b steps through `state`, bit for bit."""
    a, b = split
    H = 5
    kw = dict(center_idx=9, free=ALL, lr={'root': 0.02, 'pose': 0.02, 'betas': 0.01, 'trans': 0.005, 'cam': 0.03}, lam_pose=1e-3,
              lam_beta=1e-3, grad=True, dense=dense, joints=pool.d['joints'][:H], kp2d=pool.d['kp2d'][:H], prior=pool.d['prior'][:H])
    if dense:
        kw['verts'] = pool.d['verts'][:H]
    whole = _fit(eng, pool, H, steps=a + b, **kw)
    first = _fit(eng, pool, H, steps=a, **kw)
    kept = first['state'].clone()
    second = eng.mano_fit(pool.d_side[:H], state=first['state'], steps=b, **kw)
    assert torch.equal(first['state'], kept)      # the caller's state is not written to
    _same(whole, second)
    assert float(second['state'][0, 192]) == a + b


def test_deterministic_and_rows_isolated(eng, pool):
    kw = dict(steps=6, free=ALL, grad=True, lam_pose=1e-3, joints=pool.d['joints'], kp2d=pool.d['kp2d'], w_joints=pool.d['w_joints'])
    for center_idx, dense in ((9, False), (12, False), (None, True)):
        a = _fit(eng, pool, POOL, center_idx, dense=dense, **kw)
        b = _fit(eng, pool, POOL, center_idx, dense=dense, **kw)
        _same(a, b)
        for r in (0, 1, 40, POOL - 1):      # a row alone
            one = _fit(eng, pool, 1, center_idx, rows=slice(r, r + 1), dense=dense,
                       **{k: (v[r:r + 1] if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
            for k in a:
                assert torch.equal(one[k][0], a[k][r]), k
        # a NaN target under a non-zero weight stays in its row
        bad = pool.d['joints'].clone()
        bad[5, 3, 1] = float('nan')
        c = _fit(eng, pool, POOL, center_idx, dense=dense, **dict(kw, joints=bad))
        keep = [r for r in range(POOL) if r != 5]
        assert torch.isnan(c['poses'][5]).any()
        for k in a:
            assert torch.equal(c[k][keep], a[k][keep]), k
        # under a zero weight it changes nothing
        w = pool.d['w_joints'].clone()
        w[5, 3] = 0
        _same(_fit(eng, pool, POOL, center_idx, dense=dense, **dict(kw, w_joints=w)),
              _fit(eng, pool, POOL, center_idx, dense=dense, **dict(kw, joints=bad, w_joints=w)))


def test_what_must_not_move(eng, pool):
    H = 7
    # all weights zero and no regulariser: the parameters keep their bytes
    z = torch.zeros(H, 21, device='cuda')
    out = _fit(eng, pool, H, 9, steps=5, free=ALL, joints=pool.d['joints'][:H], w_joints=z, kp2d=pool.d['kp2d'][:H], w_kp2d=z)
    for k in ('poses', 'betas', 'trans', 'cam'):
        assert torch.equal(out[k], pool.d_init[k][:H]), k
    assert not out['loss'].any()
    # a frozen group keeps parameters, m and v while the others move
    moved = _fit(eng, pool, H, 9, steps=3, free=ALL, joints=pool.d['joints'][:H])
    cont = eng.mano_fit(pool.d_side[:H], state=moved['state'], steps=4, center_idx=9, free=('root', 'betas', 'trans'),
                        joints=pool.d['joints'][:H])
    s0, s1 = moved['state'], cont['state']
    for base in (0, 64, 128):      # parameters, m, v
        assert torch.equal(s1[:, base + 3:base + 48], s0[:, base + 3:base + 48])          # pose: frozen
        assert torch.equal(s1[:, base + 61:base + 64], s0[:, base + 61:base + 64])        # cam: frozen
        assert (s1[:, base:base + 3] != s0[:, base:base + 3]).any() and (s1[:, base + 48:base + 58] != s0[:, base + 48:base + 58]).any()
    # steps = 0 returns the state's parameters and touches nothing else
    still = eng.mano_fit(pool.d_side[:H], state=moved['state'], steps=0, center_idx=9, joints=pool.d['joints'][:H], grad=True)
    assert torch.equal(still['state'], moved['state']) and not still['grad'].any()
    for k in ('poses', 'betas', 'trans', 'cam', 'loss'):
        assert torch.equal(still[k], moved[k]), k
    # no hands
    none = _fit(eng, pool, 0, 9, steps=3, joints=pool.d['joints'][:0], grad=True)
    assert [tuple(none[k].shape) for k in ('poses', 'betas', 'trans', 'cam', 'loss', 'state', 'grad')] == \
        [(0, 48), (0, 10), (0, 3), (0, 3), (0, 2), (0, pkg('_lib').FIT_STATE), (0, 64)]


def test_manolayer_fit(eng, mano_tables, problem3d):
    """ManoLayer.fit is Engine.mano_fit at the layer's side and center_idx."""
    layer = pkg('mano.manolayer').ManoLayer(tables=mano_tables['right'], center_idx=None, side='right', use_pca=False,
                                            flat_hand_mean=False)
    y = torch.from_numpy(problem3d.joints).cuda()
    pose, betas, trans, cam, loss = layer.fit(joints=y, steps=20, lr=0.02)
    want = eng.mano_fit(torch.ones(8, dtype=torch.int32, device='cuda'), joints=y, steps=20, center_idx=None, lr=0.02)
    assert torch.equal(pose, want['poses']) and torch.equal(betas, want['betas']) and torch.equal(loss, want['loss'])
    assert not trans.any() and torch.equal(cam, want['cam'])


def test_nothing_waits(eng, pool):
    H = 4
    kw = dict(steps=3, joints=pool.d['joints'][:H], kp2d=pool.d['kp2d'][:H], free=ALL, lam_pose=1e-3, prior=pool.d['prior'][:H])
    warm = _fit(eng, pool, H, 9, **kw)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = _fit(eng, pool, H, 9, **kw)
        again = eng.mano_fit(pool.d_side[:H], state=out['state'], center_idx=9, **kw)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    _same(out, warm)
    assert torch.isfinite(again['poses']).all()


def test_estate_before_tables():
    E, L = pkg('engine'), pkg('_lib')
    fresh = E.Engine(0)
    with pytest.raises(L.AcrmiError, match='not loaded') as err:
        fresh.mano_fit(torch.zeros(2, dtype=torch.int32, device='cuda'), joints=torch.zeros(2, 21, 3, device='cuda'), steps=1)
    assert not isinstance(err.value, ValueError)


# ---- refinement: Engine.refine, EnginePool.refine, forward_batch(refine=) ---------------------------------------------------

WHOLE = [[512., 512, 0, 0, 0, 0, 0, 0, 0, 0]]


@pytest.fixture(scope='module')
def net(synth_sd, mano_tables):
    e = pkg('engine').Engine(0)
    e.load_state_dict(synth_sd, max_batch=2)
    e.load_mano(mano_tables)
    return e


def _forward_with_flags(net, frames2, flags=((1., 1.), (1., 0.))):
    L = pkg('_lib')
    out = net.forward(torch.from_numpy(frames2).cuda(), offsets=torch.tensor(WHOLE).repeat(2, 1), project=True)
    out['slots'][:, :, L.SLOT_FLAG] = torch.tensor(flags).cuda()
    return out


def _displaced(pj2d, seed=2):
    g = torch.Generator().manual_seed(seed)
    return pj2d + (0.05 * torch.randn(pj2d.shape, generator=g)).to(pj2d.device)


def test_engine_refine(net, frames2):
    """kp2d = the forward's own pj2d displaced by a seeded offset: fit_loss falls for every flagged hand, unflagged hands keep
    their slot bytes, and the returned dict goes through render and score unchanged in shape and dtype."""
    L, E = pkg('_lib'), pkg('engine')
    out = _forward_with_flags(net, frames2)
    kp = _displaced(out['pj2d'])
    ref_ = net.refine(out, kp2d=kp, steps=40, offsets=torch.tensor(WHOLE).repeat(2, 1))
    assert set(ref_) == set(out) | {'fit_loss'}
    for k in out:
        assert ref_[k].shape == out[k].shape and ref_[k].dtype == out[k].dtype, k
    on = (out['slots'][:, :, L.SLOT_FLAG] > 0.5).cpu().numpy()
    loss = ref_['fit_loss'].cpu().numpy()
    print('fit_loss first %s last %s' % (loss[..., 0].ravel(), loss[..., 1].ravel()))
    assert loss.shape == (2, 2, 2) and (loss[on][:, 1] < loss[on][:, 0]).all() and (loss[on][:, 0] > 0).all()
    assert not loss[~on].any()
    for k in out:
        assert torch.equal(ref_[k][1, 1], out[k][1, 1]), k      # the unflagged hand: every byte
    moved = ref_['slots'][:, :, L.SLOT_POSES:L.SLOT_POSES + 48] != out['slots'][:, :, L.SLOT_POSES:L.SLOT_POSES + 48]
    assert moved[0, 0].any() and moved[0, 1].any() and moved[1, 0].any()
    # what was not fitted is what it was
    other = [i for i in range(L.SLOT) if not (L.SLOT_CAM <= i < L.SLOT_CAM + 3 or L.SLOT_POSES <= i < L.SLOT_BETAS + 10)]
    assert torch.equal(ref_['slots'][..., other], out['slots'][..., other])
    # the refined pj2d is closer to the key points than the forward's, and is mano's on the refined slots
    d0 = ((out['pj2d'] - kp) ** 2).sum(-1).mean(-1).cpu().numpy()
    d1 = ((ref_['pj2d'] - kp) ** 2).sum(-1).mean(-1).cpu().numpy()
    assert (d1[on] < d0[on]).all()
    rows = ref_['slots'].reshape(4, L.SLOT)
    side = torch.tensor([0, 1, 0, 1], dtype=torch.int32, device='cuda')
    v, j, _, ex = net.mano(rows[:, L.SLOT_POSES:L.SLOT_POSES + 48], rows[:, L.SLOT_BETAS:L.SLOT_BETAS + 10], side,
                           center_idx=net.center_idx, cam=rows[:, L.SLOT_CAM:L.SLOT_CAM + 3])
    sel = torch.from_numpy(on.reshape(-1)).cuda()
    assert torch.equal(ref_['verts'].reshape(4, 778, 3)[sel], v[sel]) and torch.equal(ref_['pj2d'].reshape(4, 21, 2)[sel], ex['pj2d'][sel])
    img = torch.from_numpy(frames2).cuda()
    a, b = net.render(out, img), net.render(ref_, img)
    assert a.shape == b.shape and a.dtype == b.dtype
    gt = {'joints': out['joints'].clone(), 'verts': out['verts'].clone()}
    sa, sb = net.score(out, gt), net.score(ref_, gt)
    assert sorted(sa) == sorted(sb)
    for k in ('joints', 'verts'):
        assert sorted(sa[k]) == sorted(sb[k])
        for f in sa[k]:
            if isinstance(sa[k][f], torch.Tensor):
                assert sa[k][f].shape == sb[k][f].shape and sa[k][f].dtype == sb[k][f].dtype
    with pytest.raises(ValueError):
        net.refine(out)
    with pytest.raises(ValueError):
        net.refine(out, kp2d=kp[:1])
    with pytest.raises(ValueError):
        net.refine(out, kp2d=kp, max_hand=2)


def test_refine_queues_without_a_host_visit(net, frames2):
    out = _forward_with_flags(net, frames2)
    kp = _displaced(out['pj2d'])
    want = net.refine(out, kp2d=kp, steps=5)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = net.refine(out, kp2d=kp, steps=5)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    _same(got, want)


def test_pool_refine(net, synth_sd, mano_tables, frames2):
    E, L = pkg('engine'), pkg('_lib')
    img = torch.from_numpy(frames2).cuda()
    out = net.forward(img, project=True)
    kp = _displaced(out['pj2d'])
    want = net.refine(out, kp2d=kp, steps=10)
    pool = E.EnginePool(0, n=2)
    pool.load_state_dict(synth_sd, max_batch=2)
    pool.load_mano(mano_tables)
    for _ in range(2):
        t = pool.submit(img, project=True)
        got = pool.refine(t, kp2d=kp, steps=10)
        pool.collect(t)
        _same(got, want)
    with pytest.raises(RuntimeError):
        pool.refine(t, kp2d=kp)
    pool.close()


def test_forward_batch_refine(synth_sd, mano_tables, frames2):
    """forward_batch(refine=) equals forward_batch followed by Engine.refine on the same tensors; without refine= the hand
    dicts are what they were, byte for byte."""
    cfg, L = pkg('config'), pkg('_lib')
    main = pkg('acr.main')
    acr = main.ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml']), state_dict=synth_sd, mano_tables=mano_tables,
                   max_batch=2)
    img = torch.from_numpy(frames2).cuda()
    off = torch.tensor(WHOLE).repeat(2, 1)
    e = acr.model.engine(2)
    e.set_point_heads(True)      # (as forward_batch runs it: the towers at the decoded centres)
    try:
        out = e.forward(img, offsets=off, project=True)
    finally:
        e.set_point_heads(False)
    kp = _displaced(out['pj2d'])
    plain = acr.forward_batch(img, ['a', 'b'])
    res = acr.forward_batch(img, ['a', 'b'], refine=dict(kp2d=kp, steps=20))
    again = acr.forward_batch(img, ['a', 'b'])
    want = e.refine(out, kp2d=kp, steps=20, offsets=off)
    want['cam_trans'] = pkg('ops').cam_trans(want['joints'].view(-1, 21, 3), want['pj2d'].view(-1, 21, 2),
                                             focal_length=acr.focal_length).view(2, 2, 3)
    want = main.results_from_out(want, ['a', 'b'])
    n = 0
    for k in plain:
        assert len(res[k]) == len(plain[k]) == len(again[k]) == len(want[k])
        for h0, h1, h2, hw in zip(plain[k], res[k], again[k], want[k]):
            n += 1
            assert set(h1) == set(h0) | {'fit_loss'} == set(hw) and set(h2) == set(h0)
            assert all(np.array_equal(h0[f], h2[f]) for f in h0)
            assert all(np.array_equal(h1[f], hw[f]) for f in hw)
            assert h1['fit_loss'].shape == (2,) and h1['fit_loss'][1] < h1['fit_loss'][0]
            assert not np.array_equal(h1['poses'], h0['poses'])
    assert n > 0
    # key points in pixels of the original frames: the inverse of pj2d_org's formula (whole-frame offsets: (pj + 1) * 256)
    org = acr.forward_batch(img, ['a', 'b'], refine=dict(kp2d_org=(kp + 1) * 256, steps=20))
    for k in res:
        for h1, h3 in zip(res[k], org[k]):
            assert np.allclose(h1['poses'].astype(np.float32), h3['poses'].astype(np.float32), atol=2e-3)
    with pytest.raises(ValueError):
        acr.forward_batch(img, ['a', 'b'], refine=dict(kp2d=kp, step=3))
    with pytest.raises(ValueError):
        acr.forward_batch(img, ['a', 'b'], refine=dict(kp2d=kp, kp2d_org=kp))
