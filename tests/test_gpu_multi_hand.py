"""GPU tests of the top-K decode: the kernel against the numpy rule of tests/multi_ref.py bit for bit,
K = 1 against the existing decode in every byte, the rotations against the existing kernel and the oracle, hostile maps, the
fused call against its parts, and the views and result dicts of the acr layer."""
import numpy as np
import pytest
import torch

import multi_ref as mr
from conftest import pkg
from oracle import decode as odec

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 8)
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _special_centres():
    """Three frames of (left, right) maps a top-K selection can get wrong."""
    cl = np.zeros((3, 1, 64, 64), np.float32)
    cr = np.zeros((3, 1, 64, 64), np.float32)
    # frame 0, left: two exactly equal peaks in different waves' pixels (lower index first), a third one, and a fourth
    # equal to the third; right: a two-pixel plateau (both survive the NMS: two candidates) beside a single peak
    cl[0, 0, 40, 17] = cl[0, 0, 3, 50] = 0.8
    cl[0, 0, 20, 20] = cl[0, 0, 60, 2] = 0.6
    cr[0, 0, 30, 30] = cr[0, 0, 30, 31] = 0.7
    cr[0, 0, 10, 50] = 0.9
    # frame 1: peaks in the corners and on the borders, where the NMS window is clipped; neighbours inside one window
    for i, (y, x) in enumerate([(0, 0), (0, 63), (63, 0), (63, 63), (0, 31), (31, 63), (63, 30), (32, 0), (33, 33)]):
        cl[1, 0, y, x] = 0.95 - 0.05 * i
    cr[1, 0, 0, 1], cr[1, 0, 1, 0], cr[1, 0, 63, 62], cr[1, 0, 2, 2] = 0.5, 0.6, 0.7, 0.55      # (0,1) and (2,2) lose to (1,0)
    # frame 2, left: all pixels equal and above the threshold (4096 candidates that tie: the first K indices); right: all
    # negative (every loser is -0.0, the maxima are negative: the candidates are signed zeros)
    cl[2] = 0.5
    cr[2] = -mr.rng(7).uniform(0.1, 1.0, (1, 64, 64)).astype(np.float32)
    return cl, cr


def _batches():
    """name -> (head maps NCHW, center_cs, params_cs, prior_cs)."""
    if 'batches' not in _cache:
        a_l, a_r = mr.topk_case_maps('uniform_a')[0], mr.topk_case_maps('planted_c')[0]
        b_l, b_r = mr.topk_case_maps('planted_b')[0], mr.topk_case_maps('planted_a')[0]
        c_l, c_r = _special_centres()
        _cache['batches'] = {'golden_a': (mr.head_maps(a_l, a_r, 31), 4, 112, 108),
                             'golden_b': (mr.head_maps(b_l, b_r, 32), 2, 112, 106),      # center_cs = 2
                             'special': (mr.head_maps(c_l, c_r, 33), 1, 109, 112)}
    return _cache['batches']


def _device_maps(name):
    if ('dev', name) not in _cache:
        ops = pkg('ops')
        maps, ccs, pcs, qcs = _batches()[name]
        cs = {'center_map': ccs, 'params_maps': pcs, 'prior_maps': qcs}
        _cache['dev', name] = {k: ops.to_nhwc(torch.from_numpy(v), cs=cs[k[2:]]) for k, v in maps.items()}
    return _cache['dev', name]


def _ref(name, K):
    if ('ref', name, K) not in _cache:
        _cache['ref', name, K] = mr.decode_multi(_batches()[name][0], K)
    return _cache['ref', name, K]


def _multi(name, K, thresh=mr.CONF_THRESH):
    m = _device_maps(name)
    s = pkg('ops').decode_maps_multi(m['l_center_map'], m['r_center_map'], m['l_params_maps'], m['r_params_maps'],
                                     m['l_prior_maps'], m['r_prior_maps'], K, conf_thresh=thresh)
    torch.cuda.synchronize()
    return s


def test_the_cases_hold_what_they_are_for():
    """More and fewer survivors than K, exact ties, a plateau, border peaks - in the reference rule, before any kernel runs."""
    r = _ref('special', 8)
    assert r['flat_ind'][0, :4, 0].tolist() == [3 * 64 + 50, 40 * 64 + 17, 20 * 64 + 20, 60 * 64 + 2]      # ties: lower index first
    assert r['flat_ind'][0, :3, 1].tolist() == [10 * 64 + 50, 30 * 64 + 30, 30 * 64 + 31] and r['flag'][0, :, 1].sum() == 3
    assert r['flat_ind'][1, :4, 0].tolist() == [0, 63, 63 * 64, 63 * 64 + 63] and r['flag'][1, :, 0].all()
    assert r['flat_ind'][2, :, 0].tolist() == list(range(8)) and not r['flag'][2, :, 1].any()
    assert np.signbit(r['score'][2, :, 1]).all() and (r['score'][2, :, 1] == 0).all()
    counts = [int(r2['flag'][b, :, h].sum()) for r2 in (_ref('golden_a', 3), _ref('golden_b', 3)) for b in range(3) for h in (0, 1)]
    assert 0 in counts and 3 in counts and {1, 2} & set(counts)
    assert (r['partner'] >= 0).any() and ((r['partner'] < 0) & r['flag']).any()


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('name', ['golden_a', 'golden_b', 'special'])
def test_decode_maps_multi_equals_the_rule_bit_for_bit(name, K):
    L = pkg('_lib')
    got = _multi(name, K).cpu().numpy()
    want = _ref(name, K)
    B = want['flag'].shape[0]
    assert got.shape == (B, K, 2, L.SLOT)
    np.testing.assert_array_equal(got[..., L.SLOT_FLAG], want['flag'].astype(np.float32))
    np.testing.assert_array_equal(got[..., L.SLOT_FLATIND], want['flat_ind'].astype(np.float32))
    np.testing.assert_array_equal(_bits(got[..., L.SLOT_SCORE]), _bits(want['score']))
    np.testing.assert_array_equal(_bits(got[..., L.SLOT_PARAMS:L.SLOT_PARAMS + 109]), _bits(want['params_pred']))
    np.testing.assert_array_equal(_bits(got[..., L.SLOT_CAM:L.SLOT_CAM + 3]), _bits(want['params_pred'][..., :3]))
    np.testing.assert_array_equal(_bits(got[..., L.SLOT_BETAS:L.SLOT_BETAS + 10]), _bits(want['params_pred'][..., 99:]))
    assert (got[..., 173:176] == 0).all()


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('name', ['golden_a', 'special'])
def test_poses_are_the_existing_kernels_rotations(name, K):
    """POSES of every slot == what the existing decode writes for a one-pair frame whose placeholder (all-zero centre maps:
    pixel 0, no prior) samples that slot's PARAMS - bit for bit - and the oracle's rot6d_to_aa within the tolerance
    tests/test_gpu_kernels.py uses."""
    L, ops = pkg('_lib'), pkg('ops')
    slots = _multi(name, K)
    n = slots.shape[0] * K
    rows = slots.reshape(n, 2, L.SLOT)
    zc = torch.zeros(n, 64, 64, 1, device='cuda')
    zp = torch.zeros(n, 64, 64, 106, device='cuda')
    par = [torch.zeros(n, 64, 64, 109, device='cuda') for _ in (0, 1)]
    for h in (0, 1):
        par[h][:, 0, 0, :] = rows[:, h, L.SLOT_PARAMS:L.SLOT_PARAMS + 109]
    single = ops.decode_maps(zc, zc, par[0], par[1], zp, zp)
    torch.cuda.synchronize()
    assert not (single[:, :, L.SLOT_FLAG] > 0.5).any()
    got = rows[:, :, L.SLOT_POSES:L.SLOT_POSES + 48].cpu().numpy()
    np.testing.assert_array_equal(_bits(got), _bits(single[:, :, L.SLOT_POSES:L.SLOT_POSES + 48].cpu().numpy()))
    x6 = rows[:, :, L.SLOT_PARAMS + 3:L.SLOT_PARAMS + 99].reshape(2 * n, 96).cpu()
    np.testing.assert_allclose(got.reshape(2 * n, 48), odec.rot6d_to_aa(x6).numpy(), rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize('name', ['golden_a', 'golden_b', 'special'])
def test_k1_is_the_existing_decode_in_every_byte(name):
    m = _device_maps(name)
    one = pkg('ops').decode_maps(m['l_center_map'], m['r_center_map'], m['l_params_maps'], m['r_params_maps'],
                                 m['l_prior_maps'], m['r_prior_maps'])
    multi = _multi(name, 1)
    torch.cuda.synchronize()
    assert tuple(multi.shape) == (one.shape[0], 1, 2, pkg('_lib').SLOT)
    assert torch.equal(multi[:, 0].contiguous().view(torch.int32), one.view(torch.int32))


@pytest.mark.parametrize('K', (1, 8))
def test_hostile_maps_stay_inside_the_maps(K):
    """All-NaN, all-equal, +inf, -inf and mixed maps: the call returns and every FLATIND is a pixel.  Nothing else is asked."""
    L, ops = pkg('_lib'), pkg('ops')
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    g = mr.rng(9)
    mixed = g.uniform(-1, 1, (64, 64)).astype(np.float32)
    mixed[g.integers(0, 64, 200), g.integers(0, 64, 200)] = nan
    mixed[g.integers(0, 64, 50), g.integers(0, 64, 50)] = inf
    mixed[g.integers(0, 64, 50), g.integers(0, 64, 50)] = -inf
    full = lambda v: np.full((64, 64), v, np.float32)
    cl = np.stack([full(nan), full(0.5), full(inf)])[:, None]
    cr = np.stack([full(-inf), mixed, full(nan)])[:, None]
    m = {k: ops.to_nhwc(torch.from_numpy(v)) for k, v in mr.head_maps(cl, cr, 34).items()}
    slots = ops.decode_maps_multi(m['l_center_map'], m['r_center_map'], m['l_params_maps'], m['r_params_maps'],
                                  m['l_prior_maps'], m['r_prior_maps'], K)
    torch.cuda.synchronize()
    flat = slots[..., L.SLOT_FLATIND].cpu().numpy()
    assert flat.shape == (3, K, 2) and ((flat >= 0) & (flat < 4096)).all() and (flat == np.floor(flat)).all()


# ---- the fused call -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def engine2(synth_sd, mano_tables, frames2):
    eng = pkg('engine').Engine(0)
    eng.load_state_dict(synth_sd, max_batch=2)
    eng.load_mano(mano_tables)
    img = torch.from_numpy(frames2).cuda()
    offsets = torch.tensor([[512., 512, 0, 0, 0, 0, 0, 0, 0, 0], [640., 512, 64, 64, 0, 0, 0, 0, 0, 0]])
    yield eng, img, offsets
    eng.close()


def _survivors(center_maps):
    """[B,2,64,64] -> per map (b, h) the NMS'd values, descending."""
    return {(b, h): np.sort(mr.nms_det(center_maps[b, h]).reshape(-1))[::-1] for b in range(center_maps.shape[0]) for h in (0, 1)}


def test_forward_with_one_hand_per_side_is_forward_with_dense_heads(engine2):
    eng, img, offsets = engine2
    eng.set_point_heads(False)
    want = eng.forward(img, offsets=offsets, project=True)
    eng.set_point_heads(True)      # forward_multi runs the dense heads whatever the option says
    try:
        got = {k: torch.empty_like(v) for k, v in want.items()}
        off_dev = offsets.cuda()
        pkg('_lib').check(eng.L.acrmi_forward_multi(eng.ctx, img.data_ptr(), 2, 1, off_dev.data_ptr(),
                                                    *[got[k].data_ptr() for k in ('slots', 'verts', 'joints', 'verts_camed',
                                                                                  'pj2d', 'pj2d_org')], None), eng.ctx)
    finally:
        eng.set_point_heads(False)
    same = eng.forward(img, offsets=offsets, project=True, max_hand=1)
    torch.cuda.synchronize()
    assert sorted(want) == sorted(same) == ['joints', 'pj2d', 'pj2d_org', 'slots', 'verts', 'verts_camed']
    for k in want:
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k
        assert torch.equal(same[k].view(torch.int32), want[k].view(torch.int32)), k


def test_forward_with_three_hands_per_side_equals_its_parts(engine2):
    eng, img, offsets = engine2
    L, ops = pkg('_lib'), pkg('ops')
    K = 3
    eng.backbone_heads(img)
    sv = _survivors(eng.center_maps(2).cpu().numpy())
    # a threshold under the 4th value of one map (more than K survivors) and not under the 3rd of another (fewer than K)
    many = max(sv, key=lambda m: sv[m][3])
    few = min(sv, key=lambda m: sv[m][2])
    assert many != few and sv[few][2] < sv[many][3], 'the maps of the synthetic checkpoint do not separate'
    thresh = float(np.float32((float(sv[few][2]) + float(sv[many][3])) / 2))
    old = eng.conf_thresh
    eng.set_conf_thresh(thresh)
    try:
        out = eng.forward(img, offsets=offsets, project=True, max_hand=K)
        hl = eng.program['heads']
        bufs = [eng.buffer(b[si], 2).float().contiguous() for b in (hl.center_buf, hl.params_buf, hl.prior_buf) for si in (0, 1)]
        want = ops.decode_maps_multi(*bufs, K, conf_thresh=thresh)
        assert torch.equal(eng.decode(2, max_hand=K).view(torch.int32), want.view(torch.int32))
    finally:
        eng.set_conf_thresh(old)
    torch.cuda.synchronize()
    assert tuple(out['slots'].shape) == (2, K, 2, L.SLOT) and tuple(out['verts'].shape) == (2, K, 2, 778, 3)
    assert torch.equal(out['slots'].view(torch.int32), want.view(torch.int32))
    flags = (out['slots'][..., L.SLOT_FLAG] > 0.5).cpu().numpy()
    assert flags[many[0], :, many[1]].all() and int((sv[many] > np.float32(thresh)).sum()) > K      # more survivors than ranks
    assert flags[few[0], :, few[1]].sum() < K and not flags[few[0], K - 1, few[1]]
    # one MANO call on the same 2 * K * B rows
    rows = out['slots'].reshape(-1, L.SLOT)
    side = torch.arange(rows.shape[0]) & 1
    v, j, _, extra = eng.mano(rows[:, L.SLOT_POSES:L.SLOT_POSES + 48], rows[:, L.SLOT_BETAS:L.SLOT_BETAS + 10], side,
                              center_idx=eng.center_idx, cam=rows[:, L.SLOT_CAM:L.SLOT_CAM + 3],
                              offsets=offsets.repeat_interleave(2 * K, 0))
    torch.cuda.synchronize()
    for k, w in (('verts', v), ('joints', j), ('verts_camed', extra['verts_camed']), ('pj2d', extra['pj2d']),
                 ('pj2d_org', extra['pj2d_org'])):
        assert torch.equal(out[k].reshape(w.shape).view(torch.int32), w.view(torch.int32)), k
    assert not torch.equal(out['pj2d_org'][0], out['pj2d_org'][1])


def test_what_knows_one_hand_per_side_is_refused(engine2):
    eng, img, offsets = engine2
    L = pkg('_lib')
    table = pkg('engine').StreamTable(0, 4)
    try:
        with pytest.raises(ValueError, match='streams='):
            eng.forward(img, offsets=offsets, project=True, max_hand=2, streams=[0, 1], table=table)
    finally:
        table.close()
    eng.set_batch_semantics('reference')
    try:
        with pytest.raises(ValueError, match='ACRMI_OPT_BATCH_PRIOR'):
            eng.forward(img, max_hand=2)
        eng.forward(img, max_hand=1)      # one hand per side: every option keeps its meaning
    finally:
        eng.set_batch_semantics('frame')
    eng.set_temporal(True)
    try:
        with pytest.raises(ValueError, match='ACRMI_OPT_TEMPORAL'):
            eng.forward(img, max_hand=2)
    finally:
        eng.set_temporal(False)
    for K in (0, 9):
        with pytest.raises(ValueError):
            eng.forward(img, max_hand=K)
        with pytest.raises(ValueError):
            eng.decode(2, max_hand=K)
        p = img.data_ptr()
        assert eng.L.acrmi_forward_multi(eng.ctx, p, 2, K, None, p, p, p, None, None, None, None) == L.E_INVAL
        assert eng.L.acrmi_decode_multi(eng.ctx, 2, K, p, None) == L.E_INVAL
    with pytest.raises(ValueError, match='prior_gate'):
        eng.decode(2, prior_gate=torch.zeros(2, dtype=torch.int32), max_hand=2)
    torch.cuda.synchronize()


# ---- the acr layer ------------------------------------------------------------------------------------------------------------
def test_acr_layer_results_and_views_with_two_hands_per_side(mano_tables):
    cfg, ops, L = pkg('config'), pkg('ops'), pkg('_lib')
    K, B = 2, 3
    acr = pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml', '--renderer', 'hip']),
                              state_dict=pkg('synth').make_state_dict(seed=10), mano_tables=mano_tables, max_batch=B)
    seeded = pkg('synth').make_frames(2, seed=0)
    # (the checkpoint answers a black frame with clearly higher centre maps than the seeded ones: room for a threshold between)
    frames = torch.from_numpy(np.stack([seeded[0], np.zeros_like(seeded[0]), seeded[1]])).cuda()
    paths = ['a', 'b', 'c']
    eng = acr.model.engine(B)
    eng.backbone_heads(frames)
    sv = _survivors(eng.center_maps(B).cpu().numpy())
    # a threshold that leaves one frame without any hand and gives another one two hands of a side
    top = [max(float(sv[b, 0][0]), float(sv[b, 1][0])) for b in range(B)]
    empty = int(np.argmin(top))
    second = {m: float(v[1]) for m, v in sv.items() if m[0] != empty}
    two = max(second, key=second.get)
    assert top[empty] < second[two], 'the maps of the synthetic checkpoint do not separate'
    thresh = float(np.float32((top[empty] + second[two]) / 2))
    eng.set_conf_thresh(thresh)
    res, views = acr.forward_batch(frames, paths, max_hand=K, render=frames, show_items=('mesh', 'pj2d', 'org_img'))
    plain = acr.forward_batch(frames, paths, max_hand=K)
    # the engine's call and the stand-alone operators on the same rows
    offsets = torch.tensor([[512., 512, 0, 0, 0, 0, 0, 0, 0, 0]]).repeat(B, 1)
    out = eng.forward(frames, offsets=offsets, project=True, max_hand=K)
    focal = float(acr.focal_length)
    n = B * K
    cam_trans = ops.cam_trans(out['joints'].view(-1, 21, 3), out['pj2d'].view(-1, 21, 2), focal_length=focal)
    flags = (out['slots'][..., L.SLOT_FLAG] > 0.5).cpu()      # [B,K,2]
    assert not flags[empty].any() and flags[two[0], :, two[1]].all()
    frame_of = torch.arange(B)[:, None, None].expand(B, K, 2)
    hand_frame = torch.where(flags, frame_of, torch.full((B, K, 2), -1)).reshape(-1)
    mesh = ops.render_meshes(out['verts'].view(2 * n, 778, 3), (mano_tables['left']['faces'], mano_tables['right']['faces']),
                             frames, mesh_frame=hand_frame, trans=cam_trans, colors=torch.tensor(ops.HAND_COLORS_RGB).repeat(n, 1),
                             focal_length=focal, mesh_view=ops.view_from_offsets(offsets).repeat_interleave(2 * K, 0),
                             topo_index=torch.tensor([0, 1]).repeat(n))
    skel = ops.draw_skeletons(out['pj2d_org'].reshape(-1, 21, 2), frames, hand_frame=hand_frame.to(torch.int32))
    torch.cuda.synchronize()
    assert sorted(views) == ['mesh', 'org_img', 'pj2d']
    assert torch.equal(views['mesh'], mesh) and torch.equal(views['pj2d'], skel) and views['org_img'] is frames
    assert torch.equal(views['mesh'][empty], frames[empty]) and torch.equal(views['pj2d'][empty], frames[empty])
    assert not torch.equal(views['pj2d'][two[0]], frames[two[0]])
    # the dicts: the fp16 casts of the slots and MANO outputs, the flagged lefts by rank, then the flagged rights by rank
    assert res[paths[empty]] == {} and plain[paths[empty]] == {}
    slots = out['slots'].cpu().numpy()
    host = {k: out[k].cpu().numpy() for k in ('verts', 'joints', 'pj2d', 'pj2d_org')}
    ct = cam_trans.view(B, K, 2, 3).cpu().numpy()
    for b, path in enumerate(paths):
        order = [(k, h) for h in (0, 1) for k in range(K) if flags[b, k, h]]
        assert len(res[path]) == len(order) == len(plain[path])
        for hand, again, (k, h) in zip(res[path], plain[path], order):
            assert int(hand['hand_type']) == h
            s = slots[b, k, h]
            np.testing.assert_array_equal(hand['poses'], s[L.SLOT_POSES:L.SLOT_POSES + 48].astype(np.float16))
            np.testing.assert_array_equal(hand['betas'], s[L.SLOT_BETAS:L.SLOT_BETAS + 10].astype(np.float16))
            np.testing.assert_array_equal(hand['cam'], s[L.SLOT_CAM:L.SLOT_CAM + 3].astype(np.float16))
            np.testing.assert_array_equal(hand['cam_trans'], ct[b, k, h].astype(np.float16))
            for key, src in (('verts', 'verts'), ('j3d', 'joints'), ('pj2d', 'pj2d'), ('pj2d_org', 'pj2d_org')):
                np.testing.assert_array_equal(hand[key], host[src][b, k, h].astype(np.float16))
            assert all(np.array_equal(hand[f], again[f]) for f in hand)
    assert len(res[paths[two[0]]]) >= 2 and [int(h['hand_type']) for h in res[paths[two[0]]]].count(two[1]) == 2
    # the default is the config's key; what cannot run with more than one hand of a side says so
    assert acr.hands_per_side == 1
    one = acr.forward_batch(frames, paths, point_heads=False)
    assert all(len(one[p]) <= 2 for p in paths)
    with pytest.raises(ValueError, match='batch_semantics'):
        acr.forward_batch(frames, paths, max_hand=K, batch_semantics='reference')
    with pytest.raises(ValueError, match='streams='):
        acr.forward_batch(frames, paths, max_hand=K, streams=[0, 1, 2])
    with pytest.raises(ValueError, match='boxes='):
        acr.forward_raw_batch(frames, paths, boxes=np.array([[0, 0, 64, 64]] * 3, np.int32), max_hand=K)


def test_acr_forward_reads_hands_per_side_from_the_config(mano_tables):
    """acr(frame, path) with hands_per_side = 2 in the config is forward_raw_batch(max_hand=2) of that frame, views included;
    forward_batch's default is the config's key."""
    cfg = pkg('config')
    a = cfg.parse_args(['--configs_yml', '/nonexistent.yml', '--renderer', 'hip', '--hands_per_side', '2'])
    acr = pkg('acr.main').ACR(args_set=a, state_dict=pkg('synth').make_state_dict(seed=10), mano_tables=mano_tables, max_batch=1)
    acr.show_items = ['mesh', 'pj2d', 'centermap', 'org_img']
    frame = np.random.default_rng(5).integers(0, 256, (96, 160, 3)).astype(np.uint8)
    dev = torch.from_numpy(frame)[None].cuda()
    res = acr(frame, 'p')
    want, views = acr.forward_raw_batch(dev, ['p'], render=True, show_items=acr.show_items, max_hand=2)
    by_default = acr.forward_raw_batch(dev, ['p'])
    assert len(res['p']) > 2, 'more hands than one pair holds: the synthetic checkpoint flags every rank at the default threshold'
    for got in (res, by_default):
        assert len(got['p']) == len(want['p'])
        for h1, h2 in zip(got['p'], want['p']):
            assert sorted(h1) == sorted(h2) and all(np.array_equal(h1[f], h2[f]) for f in h1)
    kinds = [int(h['hand_type']) for h in res['p']]
    assert kinds == sorted(kinds)      # lefts, then rights
    r = acr.rendering
    assert sorted(r) == ['centermap', 'mesh_rendering_orgimgs', 'org_img', 'pj2d']
    assert np.array_equal(r['mesh_rendering_orgimgs'][0], views['mesh'][0].cpu().numpy())
    assert np.array_equal(r['pj2d'][0], views['pj2d'][0].cpu().numpy()) and np.array_equal(r['org_img'][0], frame)
    assert np.array_equal(r['centermap'][0][0], views['centermap'][0, 0].cpu().numpy())
    assert np.array_equal(r['centermap'][0][1], views['centermap'][1, 0].cpu().numpy())
    assert not np.array_equal(r['mesh_rendering_orgimgs'][0], frame) and r['mesh_rendering_orgimgs'][0].shape == frame.shape
    one = acr.forward_raw_batch(dev, ['p'], max_hand=1)
    assert len(one['p']) <= 2


def test_views_over_a_list_of_frames_with_two_hands_per_side_are_those_of_each_frame_alone(mano_tables):
    """forward_raw_batch(max_hand=2, render=True, show_items=...) on a LIST of frames of two sizes (A, B, A: one draw call per
    size, the regions of the other size's frames switched off): every view of frame i equals, byte for byte, the view the same
    call gives for frame i alone as a one-frame tensor - a frame's results do not depend on the batch it is in."""
    cfg = pkg('config')
    acr = pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml', '--renderer', 'hip']),
                              state_dict=pkg('synth').make_state_dict(seed=10), mano_tables=mano_tables, max_batch=3)
    g = np.random.default_rng(5)
    sizes = [(96, 128), (64, 112), (96, 128)]
    frames = [torch.from_numpy(g.integers(0, 256, (h, w, 3)).astype(np.uint8)).cuda() for h, w in sizes]
    paths, items = ['a', 'b', 'c'], ('mesh', 'pj2d', 'centermap', 'org_img')
    res, views = acr.forward_raw_batch(frames, paths, max_hand=2, render=True, show_items=items)
    assert sorted(views) == sorted(items) and all(isinstance(views[name], list) and len(views[name]) == 3 for name in items)
    for i, (frame, path) in enumerate(zip(frames, paths)):
        alone_res, alone = acr.forward_raw_batch(frame[None], [path], max_hand=2, render=True, show_items=items)
        torch.cuda.synchronize()
        assert len(res[path]) > 2 and len(alone_res[path]) == len(res[path]), 'the synthetic checkpoint flags every rank'
        for name in items:
            got, want = views[name][i], alone[name][:, 0] if name == 'centermap' else alone[name][0]
            assert tuple(got.shape) == ((2,) if name == 'centermap' else ()) + tuple(frame.shape), (name, i)
            assert torch.equal(got, want), (name, i)
        assert torch.equal(views['org_img'][i], frame)
        for name, view in (('mesh', views['mesh'][i]), ('pj2d', views['pj2d'][i]), ('centermap', views['centermap'][i][0])):
            assert not torch.equal(view, frame), (name, i)      # something was drawn
