"""ManoLayer: the reference's constructor/forward signature (mano/manolayer.py:13-22,104-110,273-276)
over the fused HIP MANO kernel.  Buffers (th_faces, th_v_template, ...) are host tensors for callers
such as the visualiser (acr/visualization.py:80,120); the arithmetic runs in libacrmi.so.
"""
import io
import os
import pickle
import warnings

import numpy as np
import torch

_SHARED = {}       # device index -> Engine used for MANO-only calls


def shared_engine(device=0):
    from ..engine import Engine
    if device not in _SHARED:
        _SHARED[device] = Engine(device)
    return _SHARED[device]


class _Stub(object):
    """Stands in for chumpy classes when unpickling MANO_*.pkl without chumpy installed."""

    def __init__(self, *a, **k):
        pass

    def __setstate__(self, state):
        self.__dict__.update(state if isinstance(state, dict) else {'state': state})

    @property
    def r(self):
        for key in ('x', 'a'):
            if key in self.__dict__:
                return np.asarray(self.__dict__[key])
        raise AttributeError('cannot recover array from chumpy stub')


class _Unpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if module.startswith('chumpy'):
            return _Stub
        return super().find_class(module, name)


def _arr(v):
    if isinstance(v, _Stub):
        v = v.r
    if hasattr(v, 'toarray'):
        v = v.toarray()
    return np.asarray(v)


def load_mano_pkl(path):
    """mano/manolayer.py:350-394 (ready_arguments) without chumpy: returns the float32 tables."""
    if not os.path.exists(path):
        raise FileNotFoundError('%s not found: the MANO model files are licence gated (reference README.md:36); '
                                'pass tables= for synthetic tables' % path)
    with open(path, 'rb') as f:
        dd = _Unpickler(io.BytesIO(f.read()), encoding='latin1').load()
    return {'v_template': _arr(dd['v_template']).astype(np.float32),
            'shapedirs': _arr(dd['shapedirs']).astype(np.float32),
            'posedirs': _arr(dd['posedirs']).astype(np.float32),
            'J_regressor': _arr(dd['J_regressor']).astype(np.float32),
            'weights': _arr(dd['weights']).astype(np.float32),
            'hands_mean': _arr(dd['hands_mean']).astype(np.float32),
            'hands_components': _arr(dd['hands_components']).astype(np.float32),
            'faces': _arr(dd['f']).astype(np.int64),
            'kintree_table': _arr(dd['kintree_table']).astype(np.int64)}


def batch_rotprojs(rotmats):
    """mano/manolayer.py:436-453: every 3x3 matrix of [N,J,3,3] -> the nearest rotation U V^T (CPU SVD, like the reference),
    the last COLUMN negated when the result is a reflection."""
    m = rotmats.detach().float().cpu()
    out = torch.empty_like(m)
    for b in range(m.shape[0]):
        for r in range(m.shape[1]):
            U, S, V = torch.svd(m[b, r])
            rot = torch.matmul(U, V.transpose(0, 1))
            if rot.det() < 0:
                rot[:, 2] = -1 * rot[:, 2]
            out[b, r] = rot
    return out


class ManoLayer(object):
    _warned_rotmat = False      # a layer in rotmat mode warns once that it carries no gradient

    def __init__(self, center_idx=None, flat_hand_mean=True, ncomps=6, side='right', mano_root='model_data/mano/',
                 use_pca=True, root_rot_mode='axisang', joint_rot_mode='axisang', robust_rot=False, tables=None,
                 device=0):
        if root_rot_mode != 'axisang':
            # (the reference itself cannot run this mode: mano/manolayer.py:148-150 calls a module `rot6d` it never imports)
            raise ValueError("root_rot_mode=%r: only 'axisang' is implemented" % (root_rot_mode,))
        if not use_pca and joint_rot_mode not in ('axisang', 'rotmat'):
            raise ValueError("joint_rot_mode=%r: 'axisang' or 'rotmat'" % (joint_rot_mode,))
        if side not in ('left', 'right'):
            raise ValueError('side must be "left" or "right"')
        if use_pca and not 0 < ncomps <= 45:
            raise ValueError('ncomps must be 1..45')
        # use_pca: the pose coefficients are PCA coordinates, th_selected_comps = the first ncomps rows of hands_components
        # (mano/manolayer.py:47-50,89-93,124-129); ACR's own wrapper uses use_pca=False (acr/mano_wrapper.py:17-35)
        self.center_idx, self.side, self.use_pca, self.ncomps = center_idx, side, bool(use_pca), (ncomps if use_pca else 45)
        self.flat_hand_mean, self.rot, self.robust_rot = flat_hand_mean, 3, robust_rot
        self.root_rot_mode, self.joint_rot_mode = root_rot_mode, joint_rot_mode
        if tables is None:
            self.mano_path = os.path.join(mano_root, 'MANO_RIGHT.pkl' if side == 'right' else 'MANO_LEFT.pkl')
            tables = load_mano_pkl(self.mano_path)
        t = {k: np.asarray(v) for k, v in tables.items()}
        self.th_betas = torch.zeros(1, 10)
        self.th_shapedirs = torch.from_numpy(t['shapedirs'].astype(np.float32).copy())
        self.th_posedirs = torch.from_numpy(t['posedirs'].astype(np.float32).copy())
        self.th_v_template = torch.from_numpy(t['v_template'].astype(np.float32).copy()).unsqueeze(0)
        self.th_J_regressor = torch.from_numpy(t['J_regressor'].astype(np.float32).copy())
        self.th_weights = torch.from_numpy(t['weights'].astype(np.float32).copy())
        self.th_faces = torch.from_numpy(t['faces'].astype(np.int64).copy())
        hm = np.zeros(45, np.float32) if flat_hand_mean else t['hands_mean'].astype(np.float32)
        self.th_hands_mean = torch.from_numpy(hm.copy()).unsqueeze(0)
        if 'hands_components' in t:
            self.th_comps = torch.from_numpy(t['hands_components'].astype(np.float32).copy())
            self.th_selected_comps = self.th_comps[:self.ncomps].clone()
        elif use_pca:
            raise ValueError('use_pca=True needs the hands_components table')
        kt = t.get('kintree_table')
        self.kintree_parents = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14] if kt is None else list(kt[0].tolist())
        self._device = device
        self._engine = None
        self._dirty = True

    # the reference is an nn.Module; keep the calls user code makes on it
    def cuda(self, device=None):
        if device is not None:
            self._device = device if isinstance(device, int) else torch.device(device).index or 0
        return self

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def sync(self, engine=None):
        """(Re-)upload this side's tables; call after editing a th_* buffer (acr/mano_wrapper.py:35)."""
        eng = engine or shared_engine(self._device)
        eng.load_mano_side(self.side, self.tables())
        self._engine = eng
        self._dirty = False
        self._dev = {}

    def _on_device(self, name):
        """A th_* buffer on the engine's device for the gradient path (uploaded once per sync)."""
        if name not in self._dev:
            self._dev[name] = getattr(self, name).to(self._engine.device, torch.float32)
        return self._dev[name]

    def _forward_grad(self, th_pose_coeffs, th_betas, th_trans, root_palm, share_betas):
        """forward when an input asks for a gradient: the same function as torch ops on the device around the engine's
        differentiable MANO node (Engine.mano_autograd), so that autograd carries the PCA map, share_betas, th_trans, the palm
        root and its late alignment by itself."""
        eng = self._engine
        dev = eng.device
        N = th_pose_coeffs.shape[0]
        c = th_pose_coeffs.to(dev, torch.float32)
        if self.use_pca:
            pose = torch.cat([c[:, :3], c[:, 3:3 + self.ncomps].mm(self._on_device('th_selected_comps'))], 1)
        else:
            pose = c[:, :48]
        if th_betas is None or th_betas.numel() == 1:
            betas = self._on_device('th_betas').expand(N, 10)
        else:
            betas = th_betas.to(dev, torch.float32)
            if bool(share_betas):
                betas = betas.mean(0, keepdim=True).expand(N, 10)
        use_trans = not (th_trans is None or bool(torch.norm(th_trans.detach().float()) == 0))
        palm = bool(root_palm)
        side = torch.full((N,), 0 if self.side == 'left' else 1, dtype=torch.int32, device=dev)
        # as in forward: the palm root and th_trans take the kernel's outputs unaligned
        verts, joints, center = eng.mano_autograd(pose, betas, side, None if (palm or use_trans) else self.center_idx)
        if palm:
            joints = torch.cat([((verts[:, 95] + verts[:, 22]) / 2).unsqueeze(1), joints[:, 1:]], 1)
        if use_trans:
            t = th_trans.to(dev, torch.float32).unsqueeze(1)
            return verts + t, joints + t, t
        if self.center_idx is None:
            return verts, joints, None
        if palm:
            center = joints[:, self.center_idx].unsqueeze(1)
            return verts - center, joints - center, center
        return verts, joints, center

    def tables(self):
        return {'v_template': self.th_v_template[0].numpy(), 'shapedirs': self.th_shapedirs.numpy(),
                'posedirs': self.th_posedirs.numpy(), 'J_regressor': self.th_J_regressor.numpy(),
                'weights': self.th_weights.numpy(), 'hands_mean': self.th_hands_mean[0].numpy(),
                'faces': self.th_faces.numpy()}

    def forward(self, th_pose_coeffs, th_betas=torch.zeros(1), th_trans=torch.zeros(1), root_palm=torch.Tensor([0]),
                share_betas=torch.Tensor([0])):
        """-> (verts [N,778,3], joints [N,21,3], center_joint [N,1,3]) in metres (mano/manolayer.py:269-276)."""
        rotmat = not self.use_pca and self.joint_rot_mode == 'rotmat'
        wants_grad = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                                     for t in (th_pose_coeffs, th_betas, th_trans))
        if wants_grad and not rotmat:
            if th_pose_coeffs.dim() != 2 or th_pose_coeffs.shape[1] < 3 + self.ncomps:
                raise ValueError('th_pose_coeffs must be [N,%d], got %s' % (3 + self.ncomps, tuple(th_pose_coeffs.shape)))
            if not (th_betas is None or th_betas.numel() == 1) and tuple(th_betas.shape) != (th_pose_coeffs.shape[0], 10):
                raise ValueError('th_betas must be [N,10], got %s' % (tuple(th_betas.shape),))
        if self._dirty or self._engine is None:
            self.sync(self._engine)
        eng = self._engine
        N = th_pose_coeffs.shape[0]
        if wants_grad:
            # gradients reach th_pose_coeffs (48 values or 3 + ncomps PCA coordinates), th_betas and th_trans
            if not rotmat:
                return self._forward_grad(th_pose_coeffs, th_betas, th_trans, root_palm, share_betas)
            if not self._warned_rotmat:
                self._warned_rotmat = True
                warnings.warn("ManoLayer(joint_rot_mode='rotmat') carries no gradient: the rotations are projected onto SO(3) "
                              "on the host; the outputs do not require grad")
        if rotmat:
            # mano/manolayer.py:151-162: [N,16,3,3] matrices, projected onto SO(3) one by one with a CPU SVD exactly as the
            # reference's batch_rotprojs does (:436-453, U V^T with the last column flipped when det < 0); the kernel takes the
            # rotations as they are (acrmi_mano_rotmat)
            if th_pose_coeffs.dim() != 4 or tuple(th_pose_coeffs.shape[1:]) != (16, 3, 3):
                raise ValueError('joint_rot_mode="rotmat": th_pose_coeffs must be [N,16,3,3], got %s' % (tuple(th_pose_coeffs.shape),))
            th_pose_coeffs = batch_rotprojs(th_pose_coeffs.detach().float().cpu())
        if self.use_pca:      # PCA coordinates -> the 45 axis-angle values (the kernel adds th_hands_mean, :132-135)
            c = th_pose_coeffs.detach().float().cpu()
            th_pose_coeffs = torch.cat([c[:, :3], c[:, 3:3 + self.ncomps].mm(self.th_selected_comps)], 1)
        if th_betas is None or th_betas.numel() == 1:
            th_betas = self.th_betas.expand(N, 10)
        elif bool(share_betas):
            th_betas = th_betas.mean(0, keepdim=True).expand(N, 10)
        use_trans = not (th_trans is None or bool(torch.norm(th_trans.float()) == 0))
        side = torch.full((N,), 0 if self.side == 'left' else 1, dtype=torch.int32)
        if bool(root_palm):
            # mano/manolayer.py:249-251: the wrist joint is replaced by the palm = mean of vertices 95 and 22 BEFORE the
            # root alignment, so the kernel runs unaligned and the alignment (:258-266) happens here
            verts, joints, _, _ = eng.mano(th_pose_coeffs, th_betas.contiguous(), side, center_idx=None, rotmat=rotmat)
            joints = joints.clone()
            joints[:, 0] = (verts[:, 95] + verts[:, 22]) / 2
            if use_trans:
                t = th_trans.to(verts.device).float().unsqueeze(1)
                return verts + t, joints + t, t
            if self.center_idx is None:
                return verts, joints, None
            center = joints[:, self.center_idx].unsqueeze(1).clone()
            return verts - center, joints - center, center
        cidx = None if use_trans else self.center_idx
        verts, joints, center, _ = eng.mano(th_pose_coeffs, th_betas.contiguous(), side, center_idx=cidx, rotmat=rotmat)
        if use_trans:
            t = th_trans.to(verts.device).float().unsqueeze(1)
            return verts + t, joints + t, t
        if self.center_idx is None:
            return verts, joints, None
        return verts, joints, center

    __call__ = forward

    def fit(self, joints=None, kp2d=None, verts=None, steps=100, th_pose_coeffs=None, th_betas=None, th_trans=None, cam=None,
            free=('root', 'pose', 'betas'), **kw):
        """Fits this layer's hand to joints [N,21,3], kp2d [N,21,2] and / or verts [N,778,3] with `steps` Adam iterations in one
        launch (Engine.mano_fit; its other arguments - weights, prior, lam_pose, lam_beta, lr, state, dense - pass through
        **kw), starting from th_pose_coeffs [N,48] / th_betas / th_trans / cam where given (zeros, cam = (1, 0, 0) otherwise).
        The function fitted is this layer's forward at its center_idx, with th_trans ADDED to the root-aligned outputs.
        Axis-angle layers only.  -> (th_pose_coeffs [N,48], th_betas [N,10], th_trans [N,3], cam [N,3], loss [N,2])."""
        if self.use_pca or self.joint_rot_mode != 'axisang':
            raise ValueError("ManoLayer.fit fits the 48 axis-angle values: not with use_pca=True or joint_rot_mode='rotmat'")
        given = [t for t in (joints, kp2d, verts) if t is not None]
        if not given:
            raise ValueError('ManoLayer.fit needs joints, kp2d or verts')
        if self._dirty or self._engine is None:
            self.sync(self._engine)
        eng = self._engine
        N = given[0].shape[0]
        side = torch.full((N,), 0 if self.side == 'left' else 1, dtype=torch.int32, device=eng.device)
        init = {k: t for k, t in (('poses', th_pose_coeffs), ('betas', th_betas), ('trans', th_trans), ('cam', cam)) if t is not None}
        if 'state' in kw and kw['state'] is not None:
            init = None
        out = eng.mano_fit(side, joints=joints, kp2d=kp2d, verts=verts, init=init or None, steps=steps,
                           center_idx=self.center_idx, free=free, **kw)
        self.fit_state = out['state']
        return out['poses'], out['betas'], out['trans'], out['cam'], out['loss']
