"""The MANO kernel (csrc/mano.hip) at every slice count, at fingertip roots and in its fused launch.

A hand is split over `slices` workgroups by vertex range (csrc/mano_plan.h), and `slices` follows from the number of hands
in the call: 8 up to 32 hands, then 7, 6, 5, 4, 3, 2 and - from 256 hands on, or with a fingertip as root joint - 1.  The
other MANO tests all call with 1-16 hands, which is 8 slices.  Here the slice count is reached the only way production
reaches it, by the number of hands (cases.MANO_SLICE_HANDS; tests/test_mano_plan_host.py proves the list gives all eight),
and the kernel is held to what its comment claims:
  * every output element is written - the outputs start as NaN, where Engine.mano hands the kernel torch.empty;
  * a hand's results do not depend on the slice count - every row is bit-equal to the same hand run alone (8 slices, the
    form the goldens of tests/test_gpu_kernels.py pin);
  * and they are right: within the 2e-6 m of test_mano_matches_reference_golden of oracle.mano, the projections within the
    tolerances of test_mano_mixed_sides_projection_and_empty.
The hands are cases.mano_pool: left and right mixed in one call (different tables; the middle fingertip is vertex 445 on
the left, 444 on the right), a zero hand and a large pose in every 16.  `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import cases
from conftest import golden, pkg
from oracle import mano as omano
from test_gpu_hardening import _report
from test_gpu_kernels import engine  # noqa: F401  (the module fixture: left shapedirs x-flipped, eng._flipped_tables)

pytestmark = pytest.mark.gpu

POOL = max(cases.MANO_SLICE_HANDS)
SIDES = ('left', 'right')
VERT_TOL = 2e-6          # metres: test_mano_matches_reference_golden
TIP_ROOTS = (4, 8, 12, 16, 20)
TIP_JOINTS = (4, 8, 12, 16, 20)      # joint 4 k + 4 is fingertip k (oracle.mano.JOINT_REORDER)


class Pool(object):
    """cases.mano_pool on the host and on the device, the kernel's answers for every hand run alone and the oracle's,
    each computed once per mode and never written to again."""

    def __init__(self, eng):
        self.eng = eng
        self.poses, self.betas, self.side = cases.mano_pool(POOL)
        self.cam, self.offsets = cases.mano_pool_proj(POOL)
        self.rot = cases.mano_pool_rotmats(POOL)
        assert set(self.side[:2].tolist()) == {0, 1}      # from two hands on a call mixes the sides
        self.dev = {k: torch.from_numpy(getattr(self, k)).cuda() for k in ('poses', 'betas', 'side', 'cam', 'offsets', 'rot')}
        self._alone, self._oracle = {}, {}

    def run(self, rows, center_idx, rotmat=False):
        """acrmi_mano / acrmi_mano_rotmat as Engine.mano calls them - same arguments, same stream - on the pool rows
        [rows.start, rows.stop), but into outputs that hold NaN: an element no slice writes stays NaN."""
        eng, d = self.eng, self.dev
        E, L = pkg('engine'), pkg('_lib')
        H = rows.stop - rows.start
        nan = lambda *shape: torch.full((H,) + shape, float('nan'), dtype=torch.float32, device='cuda')
        out = {'verts': nan(778, 3), 'joints': nan(21, 3), 'center': nan(1, 3)}
        betas, side = d['betas'][rows].contiguous(), d['side'][rows].contiguous()
        ci = -1 if center_idx is None else int(center_idx)
        if rotmat:
            rot = d['rot'][rows].contiguous()
            L.check(eng.L.acrmi_mano_rotmat(eng.ctx, E._ptr(rot), E._ptr(betas), 10, E._ptr(side), H, ci, E._ptr(out['verts']),
                                            E._ptr(out['joints']), E._ptr(out['center']), E._stream(eng.device)), eng.ctx)
        else:
            out.update(verts_camed=nan(778, 3), pj2d=nan(21, 2), pj2d_org=nan(21, 2))
            poses, cam, offsets = d['poses'][rows].contiguous(), d['cam'][rows].contiguous(), d['offsets'][rows].contiguous()
            L.check(eng.L.acrmi_mano(eng.ctx, E._ptr(poses), 48, E._ptr(betas), 10, E._ptr(side), H, ci, E._ptr(out['verts']),
                                     E._ptr(out['joints']), E._ptr(out['center']), E._ptr(cam), 3, E._ptr(offsets),
                                     E._ptr(out['verts_camed']), E._ptr(out['pj2d']), E._ptr(out['pj2d_org']),
                                     E._stream(eng.device)), eng.ctx)
        torch.cuda.synchronize()
        return out

    def alone(self, n, center_idx, rotmat=False):
        """Rows 0..n-1, each from a call of ONE hand (8 slices; a fingertip root: 1), stacked."""
        key = (center_idx, rotmat, self.eng.mano_fp16)
        have = self._alone.setdefault(key, {'n': 0, 'rows': []})
        for r in range(have['n'], n):
            have['rows'].append(self.run(slice(r, r + 1), center_idx, rotmat))
        have['n'] = max(have['n'], n)
        return {k: torch.cat([row[k] for row in have['rows'][:n]]) for k in have['rows'][0]}

    def oracle(self, center_idx):
        """oracle.mano.mano_forward per side on the whole pool + oracle.mano.project -> numpy arrays [POOL, ...]."""
        if center_idx not in self._oracle:
            v, j, c = np.zeros((POOL, 778, 3), np.float32), np.zeros((POOL, 21, 3), np.float32), np.zeros((POOL, 1, 3), np.float32)
            for sid, name in enumerate(SIDES):
                m = self.side == sid
                ov, oj, oc = omano.mano_forward(self.eng._flipped_tables[name], name, self.poses[m], self.betas[m], center_idx=center_idx)
                v[m], j[m] = ov, oj
                if oc is not None:
                    c[m] = oc            # (center_idx None: the kernel reports a zero center)
            vc, pj, org = omano.project(v, j, self.cam, self.offsets)
            self._oracle[center_idx] = {'verts': v, 'joints': j, 'center': c, 'verts_camed': vc, 'pj2d': pj, 'pj2d_org': org}
        return self._oracle[center_idx]


@pytest.fixture(scope='module')
def pool(engine):  # noqa: F811
    return Pool(engine)


def _written_and_equal_alone(out, alone, what):
    for k, t in out.items():
        assert bool(torch.isfinite(t).all()), '%s: %d elements of %s were never written' % (what, int((~torch.isfinite(t)).sum()), k)
    for k, t in out.items():
        if not torch.equal(t, alone[k]):
            bad = (t != alone[k]).reshape(t.shape[0], -1)
            rows = bad.any(1).nonzero().flatten().tolist()
            where = bad[rows[0]].nonzero().flatten().tolist()
            raise AssertionError('%s: %s of rows %s differs from the same hand run alone (row %d: elements %s..%s, max |d| %.3g)' % (
                what, k, rows[:8], rows[0], where[0], where[-1], float((t - alone[k]).abs().max())))


def _worst_vs_oracle(out, ora, H, keys=('verts', 'joints', 'center')):
    return {k: float(np.abs(out[k].cpu().numpy() - ora[k][:H]).max()) for k in keys}


@pytest.mark.parametrize('center_idx', [9, 0, None], ids=lambda c: 'root_%s' % c)
@pytest.mark.parametrize('H', cases.MANO_SLICE_HANDS)
def test_every_slice_count(pool, H, center_idx):
    """8, 8, 8, 7, 7, 6, 5, 4, 3, 2, 1 and 1 workgroups per hand (H = 300: more workgroups than CUs too), projection and
    offsets on.  The ragged last slices (106 of 112 vertices, 128 of 130, 154 of 156, 258 of 260), the slices longer than the
    256-thread workgroup (260, 389, 778) and the fingertips next to a slice border (673 is the second vertex of slice 6
    of 7) are all in here."""
    what = 'H=%d center_idx=%s' % (H, center_idx)
    out = pool.run(slice(0, H), center_idx)
    _written_and_equal_alone(out, pool.alone(H, center_idx), what)          # (a), (b)
    ora = pool.oracle(center_idx)
    worst = _worst_vs_oracle(out, ora, H)
    _report('mano_slices_H%03d_root_%s' % (H, center_idx), {'hands': H, 'max_abs_err_m_vs_oracle': worst})
    print(what, worst)
    assert max(worst.values()) < VERT_TOL, (what, worst)                    # (c)
    np.testing.assert_allclose(out['verts_camed'].cpu().numpy(), ora['verts_camed'][:H], 1e-5, 2e-6)      # (d)
    np.testing.assert_allclose(out['pj2d'].cpu().numpy(), ora['pj2d'][:H], 1e-5, 2e-6)
    np.testing.assert_allclose(out['pj2d_org'].cpu().numpy(), ora['pj2d_org'][:H], 1e-5, 2e-3)


@pytest.mark.parametrize('H', [2, 36, 129])
@pytest.mark.parametrize('center_idx', TIP_ROOTS, ids=lambda c: 'root_%d' % c)
def test_fingertip_roots(pool, center_idx, H):
    """A root joint that is a skinned vertex: launch_mano then runs one workgroup per hand whatever the number of hands
    (only the slice that skinned the vertex knows the center)."""
    what = 'H=%d center_idx=%d' % (H, center_idx)
    out = pool.run(slice(0, H), center_idx)
    _written_and_equal_alone(out, pool.alone(H, center_idx), what)
    worst = _worst_vs_oracle(out, pool.oracle(center_idx), H)
    _report('mano_tip_root_H%03d_root_%d' % (H, center_idx), {'hands': H, 'max_abs_err_m_vs_oracle': worst})
    assert max(worst.values()) < VERT_TOL, (what, worst)
    # the root joint, and the vertex that is this side's tip, sit at the origin exactly
    k = TIP_JOINTS.index(center_idx)
    tip = torch.tensor([omano.TIPS[SIDES[s]][k] for s in pool.side[:H]], device='cuda')
    assert bool((out['joints'][:, center_idx] == 0).all())
    assert bool((out['verts'][torch.arange(H, device='cuda'), tip] == 0).all())
    # the center is the tip before alignment
    free = pool.run(slice(0, H), None)
    assert float((out['center'][:, 0] - free['joints'][:, center_idx]).abs().max()) < VERT_TOL
    assert float((out['center'][:, 0] - free['verts'][torch.arange(H, device='cuda'), tip]).abs().max()) < VERT_TOL
    assert float((out['verts'] + out['center'] - free['verts']).abs().max()) < VERT_TOL


@pytest.fixture(scope='module')
def lone_layers(mano_tables):
    """The tables as a lone ManoLayer holds them (left shapedirs NOT flipped: that is MANOWrapper's doing)."""
    eng = pkg('engine').Engine(0)
    eng.load_mano(mano_tables)
    yield eng
    eng.close()


@pytest.mark.parametrize('name', list(cases.MANO_TIP_CASES))
def test_fingertip_roots_match_the_reference_vectors(lone_layers, name):
    """The rows of tests/golden/mano_tips.npz: the REAL reference's ManoLayer at center_idx 4, 8, 12, 16, 20 on either side
    (tests/golden/make_golden_mano_tips.py)."""
    g = golden('mano_tips.npz')
    side, center_idx, n, seed = cases.MANO_TIP_CASES[name]
    poses, betas = cases.mano_tip_inputs(name)
    v, j, c, _ = lone_layers.mano(torch.from_numpy(poses), torch.from_numpy(betas), torch.full((n,), SIDES.index(side)),
                                  center_idx=center_idx)
    torch.cuda.synchronize()
    for got, key in ((v, '_verts'), (j, '_joints'), (c, '_center')):
        assert np.abs(got.cpu().numpy() - g[name + key]).max() < VERT_TOL, (name, key)
    assert bool((j[:, center_idx] == 0).all())


@pytest.mark.parametrize('H', [36, 85, 129])
@pytest.mark.parametrize('mode', ['fp16_tables', 'rotmat'])
def test_other_modes_do_not_depend_on_the_slice_count(pool, mode, H):
    """The kernel's other instantiation (ACRMI_OPT_MANO_FP16: f16 tables, fp32 arithmetic) and its other input form
    (joint_rot_mode='rotmat') at 7, 3 and 1 slices: all written, bit-equal to the hand alone.  The f16 tables have not been
    measured beyond 16 hands: their distance from the fp32-table oracle is reported and held to the path's stated budget
    of 1e-4 m only."""
    eng = pool.eng
    what = '%s H=%d' % (mode, H)
    try:
        eng.set_mano_fp16(mode == 'fp16_tables')
        out = pool.run(slice(0, H), 9, rotmat=mode == 'rotmat')
        _written_and_equal_alone(out, pool.alone(H, 9, rotmat=mode == 'rotmat'), what)
        if mode == 'fp16_tables':
            worst = _worst_vs_oracle(out, pool.oracle(9), H)
            _report('mano_slices_fp16_tables_H%03d' % H, {'hands': H, 'max_abs_err_m_vs_fp32_oracle': worst})
            print(what, worst)
            assert max(worst.values()) < 1e-4, (what, worst)
    finally:
        eng.set_mano_fp16(False)


def test_fused_forward_launch_equals_the_stand_alone_kernel(synth_sd, mano_tables):
    """acrmi_forward launches the kernel its own way - side from row parity (side == nullptr), poses / betas / cam at slot
    strides, one offsets row per FRAME (off_div = 2): 18 frames are 36 rows and 7 slices.  The same poses, betas and cams
    through acrmi_mano (explicit sides, dense rows, one offsets row per hand) give the same bits."""
    L, synth = pkg('_lib'), pkg('synth')
    B = 18
    t = {k: dict(v) for k, v in mano_tables.items()}
    t['left']['shapedirs'] = t['left']['shapedirs'].copy()
    t['left']['shapedirs'][:, 0, :] *= -1
    eng = pkg('engine').Engine(0)
    try:
        eng.load_state_dict(synth_sd, max_batch=B)
        eng.load_mano(t)
        frames = torch.from_numpy(synth.make_frames(B, seed=0)).cuda()
        offsets = torch.from_numpy(cases.mano_pool_proj(B)[1]).cuda()

        def both(n, center_idx):
            out = eng.forward(frames[:n].contiguous(), offsets=offsets[:n], project=True)
            torch.cuda.synchronize()
            slots = out['slots'].reshape(2 * n, L.SLOT)
            poses = slots[:, L.SLOT_POSES:L.SLOT_POSES + 48]
            betas = slots[:, L.SLOT_BETAS:L.SLOT_BETAS + 10]
            cam = slots[:, L.SLOT_CAM:L.SLOT_CAM + 3]
            assert bool(torch.isfinite(slots[:, L.SLOT_CAM:L.SLOT_BETAS + 10]).all())
            v, j, _, extra = eng.mano(poses, betas, torch.arange(2 * n) & 1, center_idx=center_idx, cam=cam,
                                      offsets=offsets[:n].repeat_interleave(2, 0))
            torch.cuda.synchronize()
            alone = dict(extra, verts=v, joints=j)
            for k in ('verts', 'joints', 'verts_camed', 'pj2d', 'pj2d_org'):
                fused = out[k].reshape(alone[k].shape)
                assert bool(torch.isfinite(fused).all()), k
                assert torch.equal(fused, alone[k]), (n, center_idx, k, float((fused - alone[k]).abs().max()))
            return out

        out = both(B, 9)
        assert float(out['verts'][:, 0].sub(out['verts'][:, 1]).abs().max()) > 1e-3        # the two hands of a frame differ
        eng.set_center_idx(16)
        out = both(2, 16)
        assert bool((out['joints'][:, :, 16] == 0).all())
    finally:
        eng.close()
