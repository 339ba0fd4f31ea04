"""The MANO backward on the GPU: acrmi_mano_backward (csrc/mano_grad.hip) against the float64 statement
(tests/mano_grad_ref.py), its determinism and row isolation, ManoLayer under torch autograd, the paths that must not change,
and a fit.  `pytest -m gpu`.

THE BAR.  The error of a gradient row is max|g - g64| / max|g64|, pose and betas apart.  The yardstick is the largest such
error of the reference ManoLayer's own float32 gradients (tests/golden/mano_grad.npz) over all fixture rows, 7.7e-7; the
kernel and ManoLayer must stay within 8 x the yardstick on every row (same float32 arithmetic, other summation orders)."""
import warnings

import numpy as np
import pytest
import torch

import mano_grad_cases as cases
import mano_grad_ref as ref
from conftest import golden, pkg

pytestmark = pytest.mark.gpu

POOL = 67
SIDES = ('left', 'right')
CENTERS = (None, 9, 0, 12)
KINDS = ('g_verts', 'g_joints', 'g_center')


@pytest.fixture(scope='module')
def eng(mano_tables):
    e = pkg('engine').Engine(0)
    e.load_mano(mano_tables)
    return e


@pytest.fixture(scope='module')
def bar(mano_tables):
    y, g64 = ref.yardstick(mano_tables, golden('mano_grad.npz'))
    print('yardstick %.3g, bar %.3g' % (y, 8 * y))
    assert y < 1e-5
    return 8 * y, g64


class Pool(object):
    """67 seeded hands, left and right mixed, in [H,176] slot rows (poses at 6..53, betas at 54..63); row 0 has a zero pose,
    row 1 a root rotation beyond 3 rad, row 2 large betas.  The float64 gradients are computed once per (center_idx,
    cotangent) and never written to again."""

    def __init__(self, tables):
        L = pkg('_lib')
        rng = np.random.RandomState(7)
        self.poses = (rng.randn(POOL, 48) * 0.3).astype(np.float32)
        self.betas = (rng.randn(POOL, 10) * 0.5).astype(np.float32)
        self.poses[0] = 0
        self.poses[1, :3] = np.array([2.0, -2.5, 1.5], np.float32)      # 3.5 rad
        self.betas[2] = (rng.randn(10) * 3.0).astype(np.float32)
        self.side = (rng.rand(POOL) < 0.5).astype(np.int32)
        self.side[:3] = (0, 1, 0)
        self.cot = {'g_verts': rng.randn(POOL, 778, 3).astype(np.float32), 'g_joints': rng.randn(POOL, 21, 3).astype(np.float32),
                    'g_center': rng.randn(POOL, 1, 3).astype(np.float32)}
        slots = rng.randn(POOL, L.SLOT).astype(np.float32)
        slots[:, L.SLOT_POSES:L.SLOT_POSES + 48] = self.poses
        slots[:, L.SLOT_BETAS:L.SLOT_BETAS + 10] = self.betas
        self.slots = torch.from_numpy(slots).cuda()
        self.d_poses = self.slots[:, L.SLOT_POSES:L.SLOT_POSES + 48]      # views: pose_stride = beta_stride = 176
        self.d_betas = self.slots[:, L.SLOT_BETAS:L.SLOT_BETAS + 10]
        self.d_side = torch.from_numpy(self.side).cuda()
        self.d_cot = {k: torch.from_numpy(v).cuda() for k, v in self.cot.items()}
        self.T = {s: ref.as_tables(tables[s]) for s in SIDES}
        self._g64 = {}

    def g64(self, center_idx, kind):
        key = (center_idx, kind)
        if key not in self._g64:
            gp, gb = np.zeros((POOL, 48)), np.zeros((POOL, 10))
            for s, name in enumerate(SIDES):
                rows = np.nonzero(self.side == s)[0]
                p = torch.tensor(self.poses[rows], dtype=torch.float64, requires_grad=True)
                b = torch.tensor(self.betas[rows], dtype=torch.float64, requires_grad=True)
                out = dict(zip(KINDS, ref.mano(self.T[name], name, p, b, center_idx)))
                if out[kind] is not None:
                    (out[kind] * torch.tensor(self.cot[kind][rows], dtype=torch.float64)).sum().backward()
                    gp[rows], gb[rows] = p.grad.numpy(), b.grad.numpy()
            self._g64[key] = (gp, gb)
        return self._g64[key]


@pytest.fixture(scope='module')
def pool(mano_tables):
    return Pool(mano_tables)


def _run(eng, pool, H, center_idx, **cot):
    gp, gb = eng.mano_backward(pool.d_poses[:H], pool.d_betas[:H], pool.d_side[:H], center_idx,
                               **{k: (v if v is None else v[:H]) for k, v in cot.items()})
    return gp, gb


def _row_errors(g, g64):
    """ref.row_errors; a row whose true gradient is all zero (the wrist as root joint does not depend on the pose, so g_center
    alone leaves the pose without a gradient) has no relative error: the kernel's row must then be exactly zero."""
    zero = np.abs(g64).max(1) == 0
    assert not g[zero].any()
    e = np.zeros(len(g))
    e[~zero] = ref.row_errors(g[~zero], g64[~zero])
    return e


@pytest.mark.parametrize('center_idx', CENTERS)
@pytest.mark.parametrize('H', (1, 2, 3, POOL))
def test_kernel_against_float64(eng, pool, bar, H, center_idx):
    """Engine.mano_backward on slot rows read in place, every cotangent alone, within 8 x the yardstick of float64 per row."""
    tol, _ = bar
    assert pool.d_poses.stride(0) == 176 and not pool.d_poses.is_contiguous()
    for kind in KINDS:
        gp, gb = _run(eng, pool, H, center_idx, **{kind: pool.d_cot[kind]})
        gp64, gb64 = pool.g64(center_idx, kind)
        if kind == 'g_center' and center_idx is None:      # center is a constant then
            assert not gp.any() and not gb.any()
            continue
        ep = _row_errors(gp.cpu().numpy(), gp64[:H])
        eb = _row_errors(gb.cpu().numpy(), gb64[:H])
        print('H %d center %s %s: worst pose %.3g (row %d) betas %.3g (row %d), bar %.3g'
              % (H, center_idx, kind, ep.max(), ep.argmax(), eb.max(), eb.argmax(), tol))
        assert ep.max() <= tol and eb.max() <= tol


def test_deterministic_and_rows_isolated(eng, pool):
    for center_idx in (9, 12, None):
        a = _run(eng, pool, POOL, center_idx, g_verts=pool.d_cot['g_verts'], g_joints=pool.d_cot['g_joints'])
        b = _run(eng, pool, POOL, center_idx, g_verts=pool.d_cot['g_verts'], g_joints=pool.d_cot['g_joints'])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for r in (0, 1, 40, POOL - 1):      # a row alone
            one = eng.mano_backward(pool.d_poses[r:r + 1], pool.d_betas[r:r + 1], pool.d_side[r:r + 1], center_idx,
                                    g_verts=pool.d_cot['g_verts'][r:r + 1], g_joints=pool.d_cot['g_joints'][r:r + 1])
            assert torch.equal(one[0][0], a[0][r]) and torch.equal(one[1][0], a[1][r])
        bad = pool.d_cot['g_verts'].clone()
        bad[5, 100, 1] = float('nan')
        c = _run(eng, pool, POOL, center_idx, g_verts=bad, g_joints=pool.d_cot['g_joints'])
        keep = [r for r in range(POOL) if r != 5]
        assert torch.isnan(c[0][5]).any()
        assert torch.equal(c[0][keep], a[0][keep]) and torch.equal(c[1][keep], a[1][keep])
    gp, gb = _run(eng, pool, POOL, 9)
    assert gp.shape == (POOL, 48) and gb.shape == (POOL, 10) and not gp.any() and not gb.any()
    gp, gb = eng.mano_backward(pool.d_poses[:0], pool.d_betas[:0], pool.d_side[:0], 9, g_verts=pool.d_cot['g_verts'][:0])
    assert gp.shape == (0, 48) and gb.shape == (0, 10)


def _layer(tables, name):
    side = cases.CASES[name][0]
    return pkg('mano.manolayer').ManoLayer(tables=tables[side], **cases.layer_kwargs(name))


def _layer_backward(tables, name):
    """A case of the fixture through ManoLayer and torch autograd -> (layer, leaves, outputs, the cotangents on the device)."""
    opt = cases.CASES[name][4]
    x = cases.inputs(name)
    layer = _layer(tables, name)
    leaf = lambda a: None if a is None else torch.from_numpy(a).cuda().requires_grad_()
    coeffs, betas, trans = leaf(x['coeffs']), leaf(x['betas']), leaf(x['trans'])
    kw = {}
    if trans is not None:
        kw['th_trans'] = trans
    if opt.get('root_palm'):
        kw['root_palm'] = torch.Tensor([1])
    if opt.get('share_betas'):
        kw['share_betas'] = torch.Tensor([1])
    verts, joints, center = layer(coeffs, betas, **kw)
    cot = {k: None if x[k] is None else torch.from_numpy(x[k]).cuda() for k in ('c_verts', 'c_joints')}
    loss = 0
    if cot['c_verts'] is not None:
        loss = loss + (verts * cot['c_verts']).sum()
    if cot['c_joints'] is not None:
        loss = loss + (joints * cot['c_joints']).sum()
    return layer, (coeffs, betas, trans), (verts, joints, center), cot, loss


@pytest.mark.parametrize('name', list(cases.CASES))
def test_manolayer_autograd(mano_tables, bar, name):
    """verts carry a graph, and backward() fills the gradients of pose (48 values or PCA coordinates), betas and th_trans
    within the bar of the float64 counterpart of the reference's own gradients."""
    tol, g64 = bar
    layer, (coeffs, betas, trans), (verts, joints, center), cot, loss = _layer_backward(mano_tables, name)
    assert verts.requires_grad and joints.requires_grad
    loss.backward()
    got = {'g_pose': coeffs.grad, 'g_betas': betas.grad}
    if trans is not None:
        got['g_trans'] = trans.grad
    for k, g in got.items():
        e = ref.row_errors(g.cpu().numpy(), g64[name][k])
        print('%s %s: worst %.3g (row %d), bar %.3g' % (name, k, e.max(), e.argmax(), tol))
        assert e.max() <= tol
    with pytest.raises(RuntimeError):      # the graph is gone: a second backward raises torch's error
        loss.backward()


def test_manolayer_gradients_are_the_engines(mano_tables):
    """On the plain path ManoLayer's gradients are Engine.mano_backward's on the same tensors, bit for bit."""
    for name in ('right_c9', 'left_c12'):
        layer, (coeffs, betas, _), _, cot, loss = _layer_backward(mano_tables, name)
        loss.backward()
        side = torch.full((cases.N,), 0 if cases.CASES[name][0] == 'left' else 1, dtype=torch.int32, device='cuda')
        gp, gb = layer._engine.mano_backward(coeffs.detach(), betas.detach(), side, cases.CASES[name][1],
                                             g_verts=cot['c_verts'], g_joints=cot['c_joints'])
        assert torch.equal(coeffs.grad, gp) and torch.equal(betas.grad, gb)


def test_double_backward_raises(mano_tables):
    layer, (coeffs, betas, _), (verts, _, _), _, _ = _layer_backward(mano_tables, 'right_c9')
    g, = torch.autograd.grad(verts.sum(), coeffs, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_paths_without_gradient_are_unchanged(mano_tables):
    x = cases.inputs('right_c9')
    layer = _layer(mano_tables, 'right_c9')
    coeffs, betas = torch.from_numpy(x['coeffs']), torch.from_numpy(x['betas'])
    side = torch.ones(cases.N, dtype=torch.int32)
    out = layer(coeffs, betas)
    want = layer._engine.mano(coeffs, betas, side, center_idx=9)[:3]
    with torch.no_grad():
        quiet = layer(coeffs.clone().requires_grad_(), betas.clone().requires_grad_())
    for o, q, w in zip(out, quiet, want):
        assert not o.requires_grad and not q.requires_grad
        assert torch.equal(o, w) and torch.equal(q, w)
    # rotmat: the projection onto SO(3) runs on the host - a warning, the values of the call without requires_grad
    rot = pkg('mano.manolayer').ManoLayer(tables=mano_tables['right'], center_idx=9, side='right', use_pca=False,
                                          joint_rot_mode='rotmat')
    from oracle import mano as omano
    mats = omano.batch_rodrigues(torch.from_numpy(x['coeffs']).reshape(-1, 3)).view(cases.N, 16, 3, 3)
    plain = rot(mats, betas)
    with pytest.warns(UserWarning, match='no gradient'):
        warned = rot(mats.clone().requires_grad_(), betas)
    with warnings.catch_warnings():
        warnings.simplefilter('error')      # once per layer
        rot(mats.clone().requires_grad_(), betas)
    for p, w in zip(plain, warned):
        assert torch.equal(p, w) and not w.requires_grad


def test_no_host_waits(mano_tables):
    layer = _layer(mano_tables, 'right_c9')
    x = cases.inputs('right_c9')
    coeffs = torch.from_numpy(x['coeffs']).cuda().requires_grad_()
    betas = torch.from_numpy(x['betas']).cuda().requires_grad_()
    (layer(coeffs, betas)[0].sum()).backward()      # tables and buffers go up here
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        verts, joints, center = layer(coeffs, betas)
        (verts.sum() + (joints * joints).sum() + center.sum()).backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert torch.isfinite(coeffs.grad).all() and torch.isfinite(betas.grad).all()


def test_it_fits(mano_tables):
    """Adam on pose and betas against the unaligned joints of 8 seeded right hands, from zeros: the mean squared joint distance
    falls at least 100-fold in 300 steps (the float64 and float32 statements fall about 1600-fold on this loop)."""
    layer = pkg('mano.manolayer').ManoLayer(tables=mano_tables['right'], center_idx=None, side='right', use_pca=False,
                                            flat_hand_mean=False)
    rng = np.random.RandomState(3)
    with torch.no_grad():
        target = layer(torch.from_numpy((rng.randn(8, 48) * 0.3).astype(np.float32)),
                       torch.from_numpy((rng.randn(8, 10) * 0.5).astype(np.float32)))[1]
    pose = torch.zeros(8, 48, device='cuda', requires_grad=True)
    betas = torch.zeros(8, 10, device='cuda', requires_grad=True)
    opt = torch.optim.Adam([pose, betas], lr=0.02)
    first = last = None
    for step in range(300):
        opt.zero_grad()
        loss = ((layer(pose, betas)[1] - target) ** 2).sum(-1).mean()
        loss.backward()
        opt.step()
        first = loss.detach() if first is None else first
    with torch.no_grad():
        last = ((layer(pose, betas)[1] - target) ** 2).sum(-1).mean()
    first, last = float(first), float(last)
    print('fit: loss %.3g -> %.3g (%.0f-fold)' % (first, last, first / last))
    assert last * 100 <= first


def test_estate_before_tables():
    E, L = pkg('engine'), pkg('_lib')
    fresh = E.Engine(0)
    z = lambda *s: torch.zeros(*s, device='cuda')
    with pytest.raises(L.AcrmiError, match='not loaded') as err:
        fresh.mano_backward(z(2, 48), z(2, 10), torch.zeros(2, dtype=torch.int32, device='cuda'), 9, g_verts=z(2, 778, 3))
    assert not isinstance(err.value, ValueError)
