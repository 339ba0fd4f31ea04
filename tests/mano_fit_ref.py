"""The fused MANO fitter (acrmi_mano_fit) restated as a torch loop (test infrastructure): the loss of
csrc/mano_fit_plan.h written in torch ops over tests/mano_grad_ref.py's `mano`, per-hand losses summed, and torch.optim.Adam
with one parameter group per learning-rate group.  float64 by default - what the kernel is measured against -, float32 for the
yardstick of the trajectory tests.  Nothing here is hand-differentiated."""
import numpy as np
import torch

import mano_grad_ref as ref

GROUPS = ('root', 'pose', 'betas', 'trans', 'cam')


def _t(a, dtype):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype)


def losses(T, side, p, center_idx, joints=None, kp2d=None, verts=None, w_joints=None, w_kp2d=None, w_verts=None, prior=None,
           lam_pose=0., lam_beta=0.):
    """p: {'root' [N,3], 'pose' [N,45], 'betas' [N,10], 'trans' [N,3], 'cam' [N,3]} of one side -> the loss per hand [N].
    A weight that is exactly 0 removes its point, target and all (a NaN target there changes nothing)."""
    dtype = p['root'].dtype
    N = p['root'].shape[0]
    v, j, _ = ref.mano(T, side, torch.cat([p['root'], p['pose']], 1), p['betas'], center_idx)
    loss = torch.zeros(N, dtype=dtype)
    if joints is not None:
        w = torch.full((N, 21), 1.0 / 21, dtype=dtype) if w_joints is None else w_joints
        d = torch.where((w != 0).unsqueeze(2), j + p['trans'].unsqueeze(1) - torch.nan_to_num(joints), torch.zeros((), dtype=dtype))
        d = torch.where((w != 0).unsqueeze(2) & torch.isnan(joints), torch.full((), float('nan'), dtype=dtype), d)
        loss = loss + (w * (d ** 2).sum(2)).sum(1)
    if kp2d is not None:
        w = torch.full((N, 21), 1.0 / 21, dtype=dtype) if w_kp2d is None else w_kp2d
        pj = j[:, :, :2] * p['cam'][:, 0].view(N, 1, 1) + p['cam'][:, 1:].unsqueeze(1)
        d = torch.where((w != 0).unsqueeze(2), pj - torch.nan_to_num(kp2d), torch.zeros((), dtype=dtype))
        d = torch.where((w != 0).unsqueeze(2) & torch.isnan(kp2d), torch.full((), float('nan'), dtype=dtype), d)
        loss = loss + (w * (d ** 2).sum(2)).sum(1)
    if verts is not None:
        w = torch.full((N,), 1.0 / 778, dtype=dtype) if w_verts is None else w_verts
        loss = loss + w * ((v + p['trans'].unsqueeze(1) - verts) ** 2).sum((1, 2))
    if lam_pose:
        loss = loss + lam_pose * ((p['pose'] - (0 if prior is None else prior[:, 3:48])) ** 2).sum(1)
    if lam_beta:
        loss = loss + lam_beta * ((p['betas'] - (0 if prior is None else prior[:, 48:58])) ** 2).sum(1)
    return loss


class Fit(object):
    """One side's hands under torch.optim.Adam.  tables: one side's MANO tables; init: {'poses','betas','trans','cam'} arrays
    (zeros and cam = (1, 0, 0) where absent); free / lr as Engine.mano_fit; targets as numpy arrays or None."""

    def __init__(self, tables, side, N, center_idx, init=None, free=('root', 'pose', 'betas'), lr=0.02, dtype=torch.float64,
                 **targets):
        self.T = ref.as_tables(tables, dtype)
        self.side, self.center_idx, self.dtype = side, center_idx, dtype
        init = init or {}
        poses = np.asarray(init.get('poses', np.zeros((N, 48))), np.float64)
        cam = np.asarray(init.get('cam', np.tile([1.0, 0.0, 0.0], (N, 1))), np.float64)
        start = {'root': poses[:, :3], 'pose': poses[:, 3:], 'betas': init.get('betas', np.zeros((N, 10))),
                 'trans': init.get('trans', np.zeros((N, 3))), 'cam': cam}
        self.p = {k: torch.tensor(np.asarray(v, np.float64), dtype=dtype, requires_grad=True) for k, v in start.items()}
        rate = lambda g: float(lr[g]) if isinstance(lr, dict) else float(lr)
        self.free = [g for g in GROUPS if g in free and rate(g) != 0]
        self.opt = torch.optim.Adam([{'params': [self.p[g]], 'lr': rate(g)} for g in self.free]) if self.free else None
        self.kw = {k: (_t(v, dtype) if k not in ('lam_pose', 'lam_beta') else v) for k, v in targets.items()}
        self.first = self.last = None

    def loss(self):
        return losses(self.T, self.side, self.p, self.center_idx, **self.kw)

    def gradient(self):
        """-> (the loss per hand [N], the gradient [N,64] in the kernel's parameter order)."""
        for t in self.p.values():
            t.grad = None
        l = self.loss()
        l.sum().backward()
        g = [torch.zeros_like(self.p[k]) if self.p[k].grad is None else self.p[k].grad for k in GROUPS]
        return l.detach().numpy(), torch.cat(g, 1).numpy()

    def run(self, steps):
        for _ in range(steps):
            if self.opt is not None:
                self.opt.zero_grad()
            l = self.loss()
            l.sum().backward()
            if self.opt is not None:
                self.opt.step()
            self.last = l.detach().numpy().copy()
            if self.first is None:
                self.first = self.last
        return self

    def params(self):
        """[N,64] in the kernel's order: pose [48] | betas [10] | trans [3] | cam [3]."""
        return torch.cat([self.p[k].detach() for k in GROUPS], 1).numpy().astype(np.float64)


def problem_3d(seed=3, n=8):
    """test_it_fits' problem: seeded poses randn * 0.3 and betas randn * 0.5 (float32), drawn in this order."""
    rng = np.random.RandomState(seed)
    return (rng.randn(n, 48) * 0.3).astype(np.float32), (rng.randn(n, 10) * 0.5).astype(np.float32)


def problem_2d(seed=5, n=8):
    """-> poses, betas, cam of the 2-D problem: poses randn * 0.3, betas randn * 0.5, s ~ U(4, 8), tx, ty ~ U(-0.3, 0.3)."""
    rng = np.random.RandomState(seed)
    poses = (rng.randn(n, 48) * 0.3).astype(np.float32)
    betas = (rng.randn(n, 10) * 0.5).astype(np.float32)
    s = rng.uniform(4, 8, n)
    tx = rng.uniform(-0.3, 0.3, n)
    ty = rng.uniform(-0.3, 0.3, n)
    return poses, betas, np.stack([s, tx, ty], 1).astype(np.float32)


def targets_of(tables, side, poses, betas, center_idx, cam=None, dtype=torch.float64):
    """(verts, joints[, pj2d]) of the float64 statement as float32 arrays: what a fit is asked to reach."""
    with torch.no_grad():
        v, j, _ = ref.mano(ref.as_tables(tables, dtype), side, torch.tensor(poses, dtype=dtype), torch.tensor(betas, dtype=dtype),
                           center_idx)
    out = [v.numpy().astype(np.float32), j.numpy().astype(np.float32)]
    if cam is not None:
        c = np.asarray(cam, np.float64)
        out.append((j.numpy()[:, :, :2] * c[:, None, None, 0] + c[:, None, 1:]).astype(np.float32))
    return out
