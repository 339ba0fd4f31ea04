"""A differentiable restatement of MANO in torch ops (test infrastructure): float64 by default, the yardstick the HIP backward
(acrmi_mano_backward) and the reference's own float32 gradients are measured against.  Plain autograd carries the gradient;
nothing here is hand-differentiated.  `layer` adds what ManoLayer.forward puts around the kernel: the PCA map, share_betas,
th_trans, the palm root and the root alignment.

Forward pinned against oracle.mano.mano_forward (tests/test_mano_grad_host.py)."""
import numpy as np
import torch

PARENTS = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14]
REORDER = [0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20]
TIPS = {'left': [745, 317, 445, 556, 673], 'right': [745, 317, 444, 556, 673]}
TABLE_KEYS = ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'weights', 'hands_mean')


def as_tables(tables, dtype=torch.float64, device='cpu'):
    return {k: torch.as_tensor(np.asarray(tables[k]), dtype=dtype, device=device) for k in TABLE_KEYS}


def rodrigues(aa):
    """[M,3] axis-angle -> [M,3,3]: the quaternion route with the 1e-8 inside the norm, as the model is defined."""
    angle = torch.sqrt(((aa + 1e-8) ** 2).sum(1, keepdim=True))
    half = angle * 0.5
    q = torch.cat([torch.cos(half), torch.sin(half) * (aa / angle)], 1)
    q = q / torch.sqrt((q * q).sum(1, keepdim=True))
    w, x, y, z = q.unbind(1)
    rows = [w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z,
            2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x,
            2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z]
    return torch.stack(rows, 1).view(-1, 3, 3)


def mano(T, side, poses, betas, center_idx=9, palm=False):
    """T: as_tables(...) of one side; poses [N,48] (hands_mean is added to the 45 finger values), betas [N,10], tensors of T's
    dtype -> (verts [N,778,3], joints [N,21,3], center [N,1,3] or None).  palm: joint 0 is the mean of vertices 95 and 22."""
    N = poses.shape[0]
    full = torch.cat([poses[:, :3], poses[:, 3:48] + T['hands_mean'].view(1, 45)], 1)
    R = rodrigues(full.reshape(-1, 3)).view(N, 16, 3, 3)
    eye = torch.eye(3, dtype=R.dtype, device=R.device)
    pose_map = (R[:, 1:] - eye).reshape(N, 135)
    v_shaped = torch.einsum('vdk,nk->nvd', T['shapedirs'], betas) + T['v_template']
    J = torch.einsum('jv,nvd->njd', T['J_regressor'], v_shaped)
    v_posed = v_shaped + torch.einsum('vdk,nk->nvd', T['posedirs'], pose_map)
    G = [None] * 16
    bottom = torch.zeros(N, 1, 4, dtype=R.dtype, device=R.device)
    bottom[:, 0, 3] = 1
    for j in range(16):
        p = PARENTS[j]
        t = J[:, j] if p < 0 else J[:, j] - J[:, p]
        M = torch.cat([torch.cat([R[:, j], t.unsqueeze(2)], 2), bottom], 1)
        G[j] = M if p < 0 else G[p] @ M
    G = torch.stack(G, 1)                                            # [N,16,4,4]
    A = G[:, :, :3, :].clone()
    A[:, :, :, 3] = G[:, :, :3, 3] - torch.einsum('njrc,njc->njr', G[:, :, :3, :3], J)
    Tv = torch.einsum('vj,njrc->nvrc', T['weights'], A)              # [N,778,3,4]
    verts = torch.einsum('nvrc,nvc->nvr', Tv[..., :3], v_posed) + Tv[..., 3]
    chain = G[:, :, :3, 3]
    if palm:
        chain = torch.cat([((verts[:, 95] + verts[:, 22]) / 2).unsqueeze(1), chain[:, 1:]], 1)
    joints = torch.cat([chain, verts[:, TIPS[side]]], 1)[:, REORDER]
    if center_idx is None:
        return verts, joints, None
    center = joints[:, center_idx].unsqueeze(1)
    return verts - center, joints - center, center


def layer(T, side, coeffs, betas, center_idx=9, comps=None, trans=None, palm=False, share_betas=False, flat_hand_mean=False):
    """ManoLayer.forward around `mano`: coeffs [N,48], or [N,3+ncomps] PCA coordinates with comps [ncomps,45]; trans [N,3] (non-zero)
    replaces the root alignment."""
    if flat_hand_mean:
        T = dict(T, hands_mean=torch.zeros_like(T['hands_mean']))
    if comps is not None:
        coeffs = torch.cat([coeffs[:, :3], coeffs[:, 3:3 + comps.shape[0]] @ comps], 1)
    if share_betas:
        betas = betas.mean(0, keepdim=True).expand(betas.shape[0], 10)
    verts, joints, center = mano(T, side, coeffs, betas, None if trans is not None else center_idx, palm=palm)
    if trans is not None:
        t = trans.unsqueeze(1)
        return verts + t, joints + t, t
    return verts, joints, center


def case_gradients(tables, name, dtype=torch.float64):
    """The gradients of one case of tests/mano_grad_cases.py by autograd through `layer`: {'g_pose', 'g_betas'[, 'g_trans']}."""
    import mano_grad_cases as cases
    side, cidx, kind, seed, opt = cases.CASES[name]
    T = as_tables(tables[side], dtype)
    x = cases.inputs(name)
    leaf = lambda a: None if a is None else torch.tensor(a, dtype=dtype, requires_grad=True)
    coeffs, betas, trans = leaf(x['coeffs']), leaf(x['betas']), leaf(x['trans'])
    comps = torch.as_tensor(tables[side]['hands_components'][:opt['ncomps']], dtype=dtype) if opt.get('use_pca') else None
    verts, joints, _ = layer(T, side, coeffs, betas, cidx, comps=comps, trans=trans, palm=bool(opt.get('root_palm')),
                             share_betas=bool(opt.get('share_betas')), flat_hand_mean=bool(opt.get('flat_hand_mean')))
    loss = 0
    if x['c_verts'] is not None:
        loss = loss + (verts * torch.as_tensor(x['c_verts'], dtype=dtype)).sum()
    if x['c_joints'] is not None:
        loss = loss + (joints * torch.as_tensor(x['c_joints'], dtype=dtype)).sum()
    loss.backward()
    out = {'g_pose': coeffs.grad.numpy(), 'g_betas': betas.grad.numpy()}
    if trans is not None:
        out['g_trans'] = trans.grad.numpy()
    return out


_YARDSTICK = {}


def yardstick(tables, fixture):
    """The largest error of the reference's own float32 gradients (the fixture) against float64, over every fixture row,
    pose and betas taken separately; computed once.  -> (yardstick, {case: {'g_pose': g64, ...}})."""
    if not _YARDSTICK:
        import mano_grad_cases as cases
        worst, g64 = 0.0, {}
        for name in cases.CASES:
            g64[name] = case_gradients(tables, name)
            for k in ('g_pose', 'g_betas'):
                worst = max(worst, float(row_errors(fixture[name + '_' + k], g64[name][k]).max()))
        _YARDSTICK.update(worst=worst, g64=g64)
    return _YARDSTICK['worst'], _YARDSTICK['g64']


def row_errors(g, g64):
    """The error measure of a gradient: per row, max|g - g64| / max|g64| ([N,K] arrays -> [N])."""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    return np.abs(g - g64).max(1) / np.abs(g64).max(1)
