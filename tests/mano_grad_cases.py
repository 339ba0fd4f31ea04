"""The seeded cases of the MANO gradient tests: inputs and cotangents are made from seeds here, so that the fixture
(tests/golden/mano_grad.npz, the reference ManoLayer's float32 gradients) holds gradients only.

A case is one ManoLayer configuration on N = 5 hands; the scalar that is differentiated is
    sum(verts * c_verts) + sum(joints * c_joints)
with the cotangents c_* of the case's kind ('verts', 'joints' or 'both').  Row 0 has an all-zero pose, row 1 a root rotation
of 3 to 5 rad, row 2 large betas."""
import numpy as np

N = 5
# name -> (side, center_idx, cotangent kind, seed, options)
CASES = {}
for _s, _side in enumerate(('left', 'right')):
    for _c, (_cidx, _kind) in enumerate(((None, 'both'), (9, 'verts'), (0, 'joints'), (12, 'both'))):
        CASES['%s_c%s' % (_side, 'none' if _cidx is None else _cidx)] = (_side, _cidx, _kind, 100 + 10 * _s + _c, {})
CASES['right_pca'] = ('right', 9, 'both', 131, {'use_pca': True, 'ncomps': 6, 'flat_hand_mean': True})
CASES['left_trans'] = ('left', 9, 'both', 132, {'trans': True})
CASES['right_palm'] = ('right', 9, 'both', 133, {'root_palm': True})
CASES['left_share'] = ('left', 0, 'joints', 134, {'share_betas': True})
BASE = [k for k, v in CASES.items() if not v[4]]


def inputs(name):
    """-> dict of float32 arrays: coeffs [N,48] (or [N,9] PCA coordinates), betas [N,10], trans [N,3] or None,
    c_verts [N,778,3] or None, c_joints [N,21,3] or None."""
    side, cidx, kind, seed, opt = CASES[name]
    rng = np.random.RandomState(seed)
    ncoef = 3 + opt['ncomps'] if opt.get('use_pca') else 48
    coeffs = (rng.randn(N, ncoef) * (1.0 if opt.get('use_pca') else 0.3)).astype(np.float32)
    betas = (rng.randn(N, 10) * 0.5).astype(np.float32)
    coeffs[0] = 0
    axis = rng.randn(3)
    coeffs[1, :3] = (axis / np.linalg.norm(axis) * rng.uniform(3.0, 5.0)).astype(np.float32)
    betas[2] = (rng.randn(10) * 3.0).astype(np.float32)
    out = {'coeffs': coeffs, 'betas': betas, 'trans': None, 'c_verts': None, 'c_joints': None}
    if opt.get('trans'):
        out['trans'] = (rng.randn(N, 3) * 0.2).astype(np.float32)
    if kind in ('verts', 'both'):
        out['c_verts'] = rng.randn(N, 778, 3).astype(np.float32)
    if kind in ('joints', 'both'):
        out['c_joints'] = rng.randn(N, 21, 3).astype(np.float32)
    return out


def layer_kwargs(name):
    """The ManoLayer constructor arguments of a case (the reference's and this package's take the same)."""
    side, cidx, kind, seed, opt = CASES[name]
    return dict(center_idx=cidx, side=side, use_pca=bool(opt.get('use_pca')), ncomps=opt.get('ncomps', 6),
                flat_hand_mean=bool(opt.get('flat_hand_mean')))
