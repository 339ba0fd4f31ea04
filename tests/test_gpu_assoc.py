"""GPU: tracks - which hand of a frame is which hand of the frame before when several hands of a side are decoded
(engine.TrackTable, acrmi_associate / acrmi_forward_tracks).  Order and ids against the numpy rule
(tests/assoc_ref.py) exactly; the smoothing of a track against the existing single-stream Engine.smooth on that track's rows
alone, bit for bit.  `pytest -m gpu`."""
import ctypes

import numpy as np
import pytest
import torch

import assoc_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu

COEFF = 3.0
KS = (1, 2, 3, 8)


def bits(t):
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().cpu().view(torch.int32)


def trim(frames, K):
    """What a decode with max_hand = K leaves of frames written for more hands: the first K ranks of each side."""
    return [tuple(list(side)[:K] for side in f) for f in frames]


@pytest.fixture(scope='module')
def eng():
    e = pkg('engine').Engine(0)
    e.set_temporal(False, smooth_coeff=COEFF)
    yield e
    e.close()


def associate(eng, slots, ids, table, smooth):
    """-> (rows, track_ids, perm) on the host; slots (numpy [B,K,2,176]) is not changed."""
    d = torch.from_numpy(np.ascontiguousarray(slots)).cuda()
    tids, perm = eng.associate(d, ids, table, smooth=smooth)
    torch.cuda.synchronize()
    return d.cpu().numpy(), tids.cpu().numpy(), perm.cpu().numpy()


def walk_slots(frames, K, seed):
    """make_slots with poses / betas of a random walk along the frames (so that filtering moves them visibly)."""
    s = R.make_slots(frames, K, seed)
    g = np.random.default_rng(100 + seed)
    s[..., R.POSES:R.POSES + 48] = np.cumsum(g.normal(0, 0.12, s.shape[:3] + (48,)), 0).astype(np.float32)
    s[..., R.BETAS:R.BETAS + 10] = np.cumsum(g.normal(0, 0.05, s.shape[:3] + (10,)), 0).astype(np.float32)
    return s


@pytest.fixture(scope='module')
def long_batch():
    """Per K: the 259 frames over three interleaved streams with -1 frames among them, their slots, and the rule's answer."""
    out = {}
    for K in KS:
        frames, ids = R.interleaved(K)
        slots = walk_slots(frames, K, seed=K)
        out[K] = (slots, ids) + R.run(slots, ids, K, 8, 5)[:4]
    return out


# ---- 1: order and ids are the rule's, exactly ------------------------------------------------------------------------------
@pytest.mark.parametrize('K', KS)
def test_scenarios_equal_the_rule(eng, K):
    E = pkg('engine')
    for name, (_, gate, max_miss, frames) in sorted(R.scenarios().items()):
        frames = trim(frames, K)
        slots = R.make_slots(frames, K, seed=5)
        ids = np.zeros(len(frames), np.int32)
        want_rows, want_ids, want_perm = R.run(slots, ids, K, gate, max_miss)[:3]
        table = E.TrackTable(0, 1, K, gate=gate, max_miss=max_miss)
        rows, tids, perm = associate(eng, slots, ids, table, smooth=False)
        table.close()
        assert tids.tolist() == want_ids.tolist(), name
        assert perm.tolist() == want_perm.tolist(), name
        assert torch.equal(bits(rows), bits(want_rows)), name      # whole rows moved, NaN payloads included


@pytest.mark.parametrize('K', KS)
def test_259_frames_of_three_interleaved_streams(eng, long_batch, K):
    """More frames than one launch takes (256), several frames of one stream per call, frames of no stream among them."""
    slots, ids, want_rows, want_ids, want_perm, _ = long_batch[K]
    assert len(ids) == 259 and (ids == -1).any() and min((ids == s).sum() for s in (0, 2, 5)) > 20
    assert (ids[256:] >= 0).any()      # the second launch has work
    table = pkg('engine').TrackTable(0, 6, K)
    rows, tids, perm = associate(eng, slots, ids, table, smooth=False)
    table.close()
    assert np.array_equal(tids, want_ids) and np.array_equal(perm, want_perm)
    assert torch.equal(bits(rows), bits(want_rows))
    assert torch.equal(bits(rows[ids == -1]), bits(slots[ids == -1]))       # left exactly as decoded
    if K > 1:
        assert (perm != np.arange(K)[None, :, None]).any()                   # ranks did swap
    # every output row is an input row of its (frame, side), byte for byte
    src = np.take_along_axis(slots, perm[..., None].astype(np.int64), 1)
    assert torch.equal(bits(rows), bits(src))


# ---- 2: one slot per side, any distance, no expiry = the per-stream smoothing ------------------------------------------------
def test_one_slot_is_the_stream_table_smoothing(eng):
    E = pkg('engine')
    g = np.random.default_rng(7)
    n = 40
    ids = g.choice(np.array([0, 1, 3, -1]), size=n).astype(np.int32)
    frames = [tuple([(int(g.integers(0, 64)), int(g.integers(0, 64)))] if g.random() < 0.75 else [] for _ in (0, 1)) for _ in range(n)]
    slots = walk_slots(frames, 1, seed=11)
    assert 0 < (slots[..., R.FLAG] > 0.5).sum() < 2 * n
    streams = E.StreamTable(0, 4)
    want = torch.from_numpy(slots[:, 0].copy()).cuda()
    eng.smooth(want, streams=ids, table=streams)
    tracks = E.TrackTable(0, 4, 1, gate=128, max_miss=-1)
    rows, tids, perm = associate(eng, slots, ids, tracks, smooth=True)
    # a second call: the state both tables carry
    want2 = torch.from_numpy(slots[:, 0].copy()).cuda()
    eng.smooth(want2, streams=ids, table=streams)
    rows2, tids2, _ = associate(eng, slots, ids, tracks, smooth=True)
    torch.cuda.synchronize()
    streams.close()
    tracks.close()
    assert torch.equal(bits(rows[:, 0]), bits(want)) and torch.equal(bits(rows2[:, 0]), bits(want2))
    assert not torch.equal(bits(rows), bits(slots)) and not torch.equal(bits(rows), bits(rows2))      # it did filter
    flagged = slots[..., R.FLAG] > 0.5
    assert ((tids == 0) == (flagged & (ids >= 0)[:, None, None])).all() and ((tids == -1) | (tids == 0)).all()
    assert np.array_equal(tids, tids2) and (perm == 0).all()


# ---- 3: every track is smoothed as if it were alone -----------------------------------------------------------------------
def three_hand_sequence():
    """One stream, K = 3, max_miss = 2.  Left: A, B, C wander and swap ranks every frame; A is away in frames 4-5 (within
    max_miss: it returns with its id); B leaves after frame 6 for good and expires; D appears in frame 10 far from all and is
    born into B's slot, whose filter state is stale.  Right: one steady hand."""
    g = np.random.default_rng(21)
    pos = {'A': (10, 10), 'B': (30, 30), 'C': (52, 50), 'D': (30, 55)}
    frames = []
    for t in range(13):
        for k in pos:
            pos[k] = (pos[k][0] + int(g.integers(-1, 2)), pos[k][1] + int(g.integers(-1, 2)))
        seen = [k for k in 'ABCD' if not (k == 'A' and t in (4, 5)) and not (k == 'B' and t > 6) and not (k == 'D' and t < 10)]
        order = [seen[(i + t) % len(seen)] for i in range(len(seen))]
        frames.append(([pos[k] for k in order], [(40, 20)]))
    return frames


def test_each_track_gets_what_it_would_get_alone(eng):
    E = pkg('engine')
    K, gate, max_miss = 3, 8, 2
    frames = three_hand_sequence()
    slots = walk_slots(frames, K, seed=31)
    ids = np.zeros(len(frames), np.int32)
    _, want_ids, want_perm, born, _ = R.run(slots, ids, K, gate, max_miss)
    left = want_ids[:, :, 0]
    assert (want_perm[:, :, 0] != np.arange(K)).any()                                         # rank swaps
    assert (left[3] == 0).any() and not (left[4:6] == 0).any() and (left[6] == 0).any()       # A: a gap, the same id after it
    assert left.max() == 3 and born[10, :, 0].sum() == 1                                      # D is a new track ...
    reborn_slot = int(np.argmax(born[10, :, 0]))
    assert (left[:7, reborn_slot] == 1).all()                                                 # ... in the slot that was B's
    table = E.TrackTable(0, 1, K, gate=gate, max_miss=max_miss)
    rows, tids, perm = associate(eng, slots, ids, table, smooth=True)
    table.close()
    assert np.array_equal(tids, want_ids) and np.array_equal(perm, want_perm)
    checked = 0
    for h in (0, 1):
        for tid in range(int(want_ids[:, :, h].max()) + 1):
            where = [(b, k) for b in range(len(frames)) for k in range(K) if want_ids[b, k, h] == tid]
            seq = np.zeros((len(where), 2, R.SLOT), np.float32)            # the other side: an unflagged placeholder
            for i, (b, k) in enumerate(where):
                seq[i, h] = slots[b, want_perm[b, k, h], h]
            d = torch.from_numpy(seq).cuda()
            eng.smooth_reset()
            eng.smooth(d)
            torch.cuda.synchronize()
            alone = d.cpu()
            for i, (b, k) in enumerate(where):
                assert torch.equal(bits(rows[b, k, h]), bits(alone[i, h])), (h, tid, b, k)
                checked += 1
            if len(where) > 1:
                assert not torch.equal(bits(alone[1:, h]), bits(seq[1:, h]))      # later samples are filtered
    assert checked == int((want_ids >= 0).sum())
    # the reborn track's first sample passes through: finger poses and betas are the input's bits
    b, k = 10, reborn_slot
    src = slots[b, want_perm[b, k, 0], 0]
    assert torch.equal(bits(rows[b, k, 0, R.POSES + 3:R.POSES + 48]), bits(src[R.POSES + 3:R.POSES + 48]))
    assert torch.equal(bits(rows[b, k, 0, R.BETAS:R.BETAS + 10]), bits(src[R.BETAS:R.BETAS + 10]))
    # rows without a detection are moved, not edited
    none = want_ids < 0
    moved = np.take_along_axis(slots, want_perm[..., None].astype(np.int64), 1)
    assert torch.equal(bits(rows[none]), bits(moved[none]))


# ---- 4: state persists across calls; reset ----------------------------------------------------------------------------------
def test_two_calls_are_one_call_and_reset_restarts_a_stream(eng, long_batch):
    E = pkg('engine')
    K = 2
    slots, ids = long_batch[K][:2]
    one = E.TrackTable(0, 6, K)
    rows, tids, perm = associate(eng, slots, ids, one, smooth=True)
    two = E.TrackTable(0, 6, K)
    cut = 101
    first = associate(eng, slots[:cut], ids[:cut], two, smooth=True)
    second = associate(eng, slots[cut:], ids[cut:], two, smooth=True)
    assert torch.equal(bits(np.concatenate([first[0], second[0]])), bits(rows))
    assert np.array_equal(np.concatenate([first[1], second[1]]), tids) and np.array_equal(np.concatenate([first[2], second[2]]), perm)
    assert not torch.equal(bits(rows), bits(long_batch[K][2]))       # (smoothing did change the rows)
    # both tables are in the same state; `two` loses stream 2, then both see the same frames again
    two.reset([2])
    tail, tail_ids = slots[:60], ids[:60]
    a = associate(eng, tail, tail_ids, one, smooth=True)
    b = associate(eng, tail, tail_ids, two, smooth=True)
    others = tail_ids != 2
    assert (tail_ids == 2).any() and (tail_ids == 0).any()
    assert torch.equal(bits(a[0][others]), bits(b[0][others]))
    assert np.array_equal(a[1][others], b[1][others]) and np.array_equal(a[2][others], b[2][others])
    fresh = R.run(tail, np.where(tail_ids == 2, 2, -1), K, 8, 5)
    assert np.array_equal(b[1][~others], fresh[1][~others]) and np.array_equal(b[2][~others], fresh[2][~others])
    first_birth = np.argmax((fresh[1][:, :, 0] >= 0).any(1) & ~others)
    assert 0 in b[1][first_birth, :, 0]                              # the ids of stream 2 started at 0 again
    assert not (np.array_equal(a[1][~others], b[1][~others]) and torch.equal(bits(a[0][~others]), bits(b[0][~others])))
    two.reset()
    c = associate(eng, tail, tail_ids, two, smooth=False)
    fresh = R.run(tail, tail_ids, K, 8, 5)
    assert np.array_equal(c[1], fresh[1]) and torch.equal(bits(c[0]), bits(fresh[0]))
    one.close()
    two.close()


# ---- 5: garbage ----------------------------------------------------------------------------------------------------------------
def test_garbage_slots_stay_inside_and_do_not_reach_other_streams(eng):
    E = pkg('engine')
    K = 3
    frames, _ = R.interleaved(K, n=40, seed=9)
    clean = walk_slots(frames, K, seed=41)
    g = np.random.default_rng(43)
    n = 2 * len(frames)
    slots = np.empty((n, K, 2, R.SLOT), np.float32)
    ids = np.empty(n, np.int32)
    slots[0::2], ids[0::2] = clean, 0
    odd = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, -1.0, 4096.0, 1e30, 0.5, 65536.0 * 65536.0, -0.0, 4095.0, 1.0], np.float32)
    slots[1::2] = odd[g.integers(0, len(odd), slots[1::2].shape)]
    ids[1::2] = 1
    table = E.TrackTable(0, 2, K)
    rows, tids, perm = associate(eng, slots, ids, table, smooth=True)
    table.close()
    assert (np.sort(perm, 1) == np.arange(K)[None, :, None]).all()       # permutations of 0..K-1, garbage frames too
    want = R.run(slots, ids, K, 8, 5)
    assert np.array_equal(tids, want[1]) and np.array_equal(perm, want[2])
    table = E.TrackTable(0, 2, K)
    alone = associate(eng, clean, np.zeros(len(frames), np.int32), table, smooth=True)
    table.close()
    assert torch.equal(bits(rows[0::2]), bits(alone[0])) and np.array_equal(tids[0::2], alone[1]) and np.array_equal(perm[0::2], alone[2])


# ---- 6 - 8: the fused call -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def engine4(synth_sd, mano_tables, frames2):
    e = pkg('engine').Engine(0)
    e.load_state_dict(synth_sd, max_batch=4)
    e.load_mano(mano_tables)
    e.set_temporal(False, smooth_coeff=COEFF)
    img = torch.from_numpy(np.stack([frames2[0], frames2[1], frames2[1], frames2[0]])).cuda()
    offsets = torch.tensor([[512., 512, 0, 0, 0, 0, 0, 0, 0, 0], [640., 512, 64, 64, 0, 0, 0, 0, 0, 0]]).repeat(2, 1)
    yield e, img, offsets
    e.close()


def _survivors(center_maps):
    import multi_ref as mr
    return {(b, h): np.sort(mr.nms_det(center_maps[b, h]).reshape(-1))[::-1] for b in range(center_maps.shape[0]) for h in (0, 1)}


def test_forward_with_tracks_equals_its_parts(engine4):
    eng, img, offsets = engine4
    E, L, ops = pkg('engine'), pkg('_lib'), pkg('ops')
    K, B = 3, 4
    tracks = [0, 1, 0, -1]
    eng.backbone_heads(img)
    sv = _survivors(eng.center_maps(B).cpu().numpy())
    # a threshold under the 4th value of one map (more than K survivors) and not under the 3rd of another (fewer than K)
    many = max(sv, key=lambda m: sv[m][3])
    few = min(sv, key=lambda m: sv[m][2])
    assert many != few and sv[few][2] < sv[many][3], 'the maps of the synthetic checkpoint do not separate'
    thresh = float(np.float32((float(sv[few][2]) + float(sv[many][3])) / 2))
    old = eng.conf_thresh
    eng.set_conf_thresh(thresh)
    fused_table, parts_table = E.TrackTable(0, 2, K, gate=128), E.TrackTable(0, 2, K, gate=128)
    try:
        for call in range(2):      # the second call continues the tracks of the first
            out = eng.forward(img, offsets=offsets, project=True, max_hand=K, tracks=tracks, track_table=fused_table)
            hl = eng.program['heads']
            bufs = [eng.buffer(b[si], B).float().contiguous() for b in (hl.center_buf, hl.params_buf, hl.prior_buf) for si in (0, 1)]
            want = ops.decode_maps_multi(*bufs, K, conf_thresh=thresh)
            decoded = want.clone()
            want_ids, want_perm = eng.associate(want, tracks, parts_table)
            rows = want.reshape(-1, L.SLOT)
            side = torch.arange(rows.shape[0]) & 1
            v, j, _, extra = eng.mano(rows[:, L.SLOT_POSES:L.SLOT_POSES + 48], rows[:, L.SLOT_BETAS:L.SLOT_BETAS + 10], side,
                                      center_idx=eng.center_idx, cam=rows[:, L.SLOT_CAM:L.SLOT_CAM + 3],
                                      offsets=offsets.repeat_interleave(2 * K, 0))
            torch.cuda.synchronize()
            assert sorted(out) == ['joints', 'pj2d', 'pj2d_org', 'slots', 'track_ids', 'verts', 'verts_camed']
            assert out['track_ids'].dtype == torch.int32 and tuple(out['track_ids'].shape) == (B, K, 2)
            assert torch.equal(out['track_ids'], want_ids)
            assert torch.equal(bits(out['slots']), bits(want))
            for k, w in (('verts', v), ('joints', j), ('verts_camed', extra['verts_camed']), ('pj2d', extra['pj2d']),
                         ('pj2d_org', extra['pj2d_org'])):
                assert torch.equal(bits(out[k].reshape(w.shape)), bits(w)), (call, k)
            flags = (decoded[..., L.SLOT_FLAG] > 0.5).cpu().numpy()
            assert flags[many[0], :, many[1]].all() and flags[few[0], :, few[1]].sum() < K
            ids = out['track_ids'].cpu().numpy()
            assert (ids[3] == -1).all() and torch.equal(bits(out['slots'][3]), bits(decoded[3]))      # the frame of no stream
            assert ((ids[:3] >= 0) == (out['slots'][:3, ..., L.SLOT_FLAG] > 0.5).cpu().numpy()).all()
        # smooth=False: order and ids only - every row of the result is a decoded row of its (frame, side)
        fused_table.reset()
        out = eng.forward(img, offsets=offsets, project=True, max_hand=K, tracks=tracks, track_table=fused_table, smooth=False)
        parts_table.reset()
        ids2, perm2 = eng.associate(decoded.clone(), tracks, parts_table, smooth=False)
        torch.cuda.synchronize()
        assert torch.equal(out['track_ids'], ids2)
        moved = np.take_along_axis(decoded.cpu().numpy(), perm2.cpu().numpy()[..., None].astype(np.int64), 1)
        assert torch.equal(bits(out['slots']), bits(moved))
    finally:
        eng.set_conf_thresh(old)
        fused_table.close()
        parts_table.close()


def test_forward_without_tracks_is_unchanged(engine4):
    eng, img, offsets = engine4
    for K in (1, 2):
        want = eng.forward(img, offsets=offsets, project=True, max_hand=K) if K > 1 else None
        shape = (4, K, 2)
        got = {'slots': torch.empty(shape + (176,)), 'verts': torch.empty(shape + (778, 3)), 'joints': torch.empty(shape + (21, 3)),
               'verts_camed': torch.empty(shape + (778, 3)), 'pj2d': torch.empty(shape + (21, 2)), 'pj2d_org': torch.empty(shape + (21, 2))}
        got = {k: v.cuda() for k, v in got.items()}
        off_dev = offsets.cuda()
        pkg('_lib').check(eng.L.acrmi_forward_multi(eng.ctx, img.data_ptr(), 4, K, off_dev.data_ptr(),
                                                    *[got[k].data_ptr() for k in ('slots', 'verts', 'joints', 'verts_camed', 'pj2d',
                                                                                  'pj2d_org')], None), eng.ctx)
        if K == 1:
            eng.set_point_heads(False)
            want = {k: v.unsqueeze(1) for k, v in eng.forward(img, offsets=offsets, project=True).items()}
        torch.cuda.synchronize()
        assert sorted(want) == sorted(got) and 'track_ids' not in want
        for k in want:
            assert torch.equal(bits(got[k]), bits(want[k])), (K, k)


def test_queued_calls_do_not_wait_for_the_device(engine4):
    eng, img, offsets = engine4
    E = pkg('engine')
    K = 2
    table = E.TrackTable(0, 4, K)
    off_dev = offsets.cuda()
    warm = eng.forward(img, offsets=off_dev, project=True, max_hand=K, tracks=[0, 1, 2, 3], track_table=table)
    loose = warm['slots'].clone()
    torch.cuda.synchronize()
    table.reset()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            warm['slots'].sum().item()      # the mode is honoured by this build
        outs = [eng.forward(img, offsets=off_dev, project=True, max_hand=K, tracks=[0, 1, 0, -1], track_table=table) for _ in range(3)]
        again = [eng.associate(loose, np.array([3, 3, -1, 2], np.int32), table, smooth=True) for _ in range(3)]
        table.reset([3])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert all(tuple(o['track_ids'].shape) == (4, K, 2) for o in outs) and len(again) == 3
    table.close()


# ---- 9: a pool of two contexts shares one table ------------------------------------------------------------------------------
def test_pool_contexts_share_one_track_table(synth_sd, mano_tables, frames2):
    E = pkg('engine')
    K = 2
    batches = [torch.from_numpy(frames2 if k % 2 == 0 else frames2[::-1].copy()).cuda() for k in range(6)]
    pool = E.EnginePool(0, n=2)
    pool.load_state_dict(synth_sd, max_batch=2)
    pool.load_mano(mano_tables)
    pool.configure(lambda e: e.set_temporal(False, smooth_coeff=COEFF))
    with pytest.raises(ValueError):
        pool.submit(batches[0], max_hand=K, tracks=[0, 1])      # no table yet
    assert pool.track_table(2, K, gate=128) is pool.track_table(2, K, gate=128)
    with pytest.raises(ValueError):
        pool.track_table(2, K, gate=8)
    got, tickets = [], []
    for img in batches:
        if len(tickets) == 2:
            got.append({k: v.clone() for k, v in pool.collect(tickets.pop(0)).items()})
        tickets.append(pool.submit(img, max_hand=K, tracks=[0, 1]))
    while tickets:
        got.append({k: v.clone() for k, v in pool.collect(tickets.pop(0)).items()})
    torch.cuda.synchronize()
    one = E.Engine(0)
    one.load_state_dict(synth_sd, max_batch=2)
    one.load_mano(mano_tables)
    one.set_temporal(False, smooth_coeff=COEFF)
    table = E.TrackTable(0, 2, K, gate=128)
    for k, img in enumerate(batches):
        want = one.forward(img, max_hand=K, tracks=[0, 1], track_table=table)
        for key in ('slots', 'verts', 'joints', 'track_ids'):
            assert torch.equal(bits(got[k][key]), bits(want[key])), (k, key)
    plain = one.forward(batches[5], max_hand=K)
    assert not torch.equal(bits(plain['slots']), bits(got[5]['slots']))      # (the sixth batch was reordered or filtered)
    table.close()
    one.close()
    pool.close()


# ---- 10: the acr layer -------------------------------------------------------------------------------------------------------
def test_acr_forward_batch_keeps_track_ids_while_ranks_change(mano_tables):
    cfg, L = pkg('config'), pkg('_lib')
    K, B = 2, 2
    acr = pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml', '--renderer', 'hip']),
                              state_dict=pkg('synth').make_state_dict(seed=10), mano_tables=mano_tables, max_batch=B)
    pool = np.concatenate([pkg('synth').make_frames(5, seed=0), np.zeros((1, 512, 512, 3), np.uint8)])
    eng = acr.model.engine(B)
    # a threshold under the second value of every map: two hands of each side in every frame
    maps = []
    for i in range(0, len(pool), B):
        eng.backbone_heads(torch.from_numpy(pool[i:i + B]).cuda())
        maps.append(eng.center_maps(B).cpu().numpy())
    sv = _survivors(np.concatenate(maps))
    eng.set_conf_thresh(float(min(v[1] for v in sv.values())) - 1.0)
    offsets = torch.tensor([[512., 512, 0, 0, 0, 0, 0, 0, 0, 0]]).repeat(B, 1)
    dec = np.concatenate([eng.forward(torch.from_numpy(pool[i:i + B]).cuda(), offsets=offsets, project=True, max_hand=K)['slots'].cpu().numpy()
                          for i in range(0, len(pool), B)])
    assert (dec[..., L.SLOT_FLAG] > 0.5).all()
    # two frames between which the nearest-centre pairing crosses the ranks of some side: the planted hand
    pick = None
    for a in range(len(pool)):
        for b in range(len(pool)):
            if a == b or pick is not None:
                continue
            perm = R.run(dec[[a, b]], np.zeros(2, np.int32), K, 128, 5)[2]
            for h in (0, 1):
                if perm[1, :, h].tolist() == [1, 0]:
                    pick = (a, b, h)
    assert pick is not None, 'no pair of synthetic frames swaps ranks'
    a, b, h = pick
    still = [i for i in range(len(pool)) if i not in (a, b)][0]
    calls = [np.stack([pool[a], pool[still]]), np.stack([pool[b], pool[still]])]
    # the un-tracked decode of the two calls as they will be made (no claim that a frame's bits survive a move in the batch)
    dec = np.concatenate([eng.forward(torch.from_numpy(f).cuda(), offsets=offsets, project=True, max_hand=K)['slots'].cpu().numpy()
                          for f in calls])
    want = R.run(dec, np.array([0, 1, 0, 1], np.int32), K, 128, 5)
    for c, frames in enumerate(calls):
        res = acr.forward_batch(torch.from_numpy(frames).cuda(), ['x', 'y'], max_hand=K, tracks=[0, 1], max_streams=2, track_gate=128)
        for f, path in enumerate(('x', 'y')):
            rows, ids = want[0][2 * c + f], want[1][2 * c + f]
            order = [(k, s) for s in (0, 1) for k in range(K)]      # every hand is flagged: lefts in slot order, then rights
            assert len(res[path]) == len(order)
            for hand, (k, s) in zip(res[path], order):
                assert int(hand['hand_type']) == s and int(hand['track_id']) == int(ids[k, s]) and hand['track_id'].dtype == np.int32
                np.testing.assert_array_equal(hand['poses'], rows[k, s, L.SLOT_POSES:L.SLOT_POSES + 48].astype(np.float16))
                np.testing.assert_array_equal(hand['betas'], rows[k, s, L.SLOT_BETAS:L.SLOT_BETAS + 10].astype(np.float16))
    # the planted hand: rank 1 in the second call, still in slot 0 with the id it had as rank 0 of the first
    assert want[2][0, :, h].tolist() == [0, 1] and want[2][2, :, h].tolist() == [1, 0]
    assert want[1][0, :, h].tolist() == want[1][2, :, h].tolist() == [0, 1]
    assert want[1][1].tolist() == want[1][3].tolist()              # the stream that saw one frame twice
    assert acr.track_table is not None and acr.track_table.max_hand == K
    with pytest.raises(ValueError, match='streams='):
        acr.forward_batch(torch.from_numpy(calls[0]).cuda(), ['x', 'y'], max_hand=K, tracks=[0, 1], streams=[0, 1])
    with pytest.raises(ValueError, match='boxes='):
        acr.forward_raw_batch(torch.from_numpy(calls[0]).cuda(), ['x', 'y'], boxes=np.array([[0, 0, 64, 64]] * 2, np.int32), tracks=[0, 1])
    with pytest.raises(ValueError):
        acr.forward_batch(torch.from_numpy(calls[0]).cuda(), ['x', 'y'], max_hand=K, tracks=[0, 2])      # the table holds 2 streams
    with pytest.raises(ValueError):
        acr.forward_batch(torch.from_numpy(calls[0]).cuda(), ['x', 'y'], max_hand=1, tracks=[0, 1])      # a table of another K
    acr.reset_tracks([0])
    acr.reset_tracks()
    acr.close_tracks()
    assert acr.track_table is None
    one = acr.forward_batch(torch.from_numpy(calls[0]).cuda(), ['x', 'y'], max_hand=1, tracks=[0, 1], max_streams=2)
    assert all(int(hd['track_id']) == 0 for p in ('x', 'y') for hd in one[p])
    acr.close_tracks()


# ---- 11: what is refused ------------------------------------------------------------------------------------------------------
def test_what_is_refused(engine4):
    eng, img, offsets = engine4
    E, L = pkg('engine'), pkg('_lib')
    K = 2
    table = E.TrackTable(0, 4, K)
    streams = E.StreamTable(0, 4)
    other = E.TrackTable(0, 4, 3)
    ok = [0, 1, 2, 3]
    try:
        for kw in (dict(tracks=ok, track_table=table, streams=ok, table=streams), dict(tracks=ok), dict(track_table=table),
                   dict(tracks=[0, 1, 2, 4], track_table=table), dict(tracks=[0, 1, 2, -2], track_table=table),
                   dict(tracks=[0, 1, 2], track_table=table), dict(tracks=ok, track_table=other),
                   dict(tracks=ok, track_table=streams)):
            with pytest.raises(ValueError):
                eng.forward(img, max_hand=K, **kw)
        with pytest.raises(ValueError, match='streams='):      # as tests/test_gpu_multi_hand.py pins it
            eng.forward(img, max_hand=K, streams=ok, table=streams)
        slots = torch.zeros(4, K, 2, L.SLOT).cuda()
        for tracks, tbl in (([0, 1, 2, 4], table), ([0, 1, 2, -2], table), ([0, 1, 2], table), (ok, other)):
            with pytest.raises(ValueError):
                eng.associate(slots, tracks, tbl)
        # the ABI says the same before anything is launched
        ids = np.array(ok, np.int32)
        bad = np.array([0, 1, 2, 4], np.int32)
        out = torch.full((4, K, 2), 77, dtype=torch.int32).cuda()
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        call = lambda t, k, i: eng.L.acrmi_associate(eng.ctx, t.handle, slots.data_ptr(), 4, k, p(i), 1, out.data_ptr(), None, None)
        assert call(table, K, bad) == L.E_INVAL and b'ids[3]' in eng.L.acrmi_last_error(eng.ctx)
        assert call(other, K, ids) == L.E_INVAL and call(table, 3, ids) == L.E_INVAL and call(table, 9, ids) == L.E_INVAL
        assert eng.L.acrmi_associate(eng.ctx, None, slots.data_ptr(), 4, K, p(ids), 1, out.data_ptr(), None, None) == L.E_INVAL
        assert eng.L.acrmi_associate(eng.ctx, table.handle, slots.data_ptr(), 4, K, None, 1, out.data_ptr(), None, None) == L.E_INVAL
        assert eng.L.acrmi_tracks_reset(table.handle, p(bad), 4, None) == L.E_INVAL
        eng.set_batch_semantics('reference')
        try:
            with pytest.raises(ValueError, match='ACRMI_OPT_BATCH_PRIOR'):
                eng.forward(img, max_hand=K, tracks=ok, track_table=table)
        finally:
            eng.set_batch_semantics('frame')
        torch.cuda.synchronize()
        assert (out == 77).all()                               # nothing was launched
        with pytest.raises(ValueError):
            table.reset([4])
        table.close()
        with pytest.raises(ValueError):
            eng.associate(slots, ok, table)                    # closed
        with pytest.raises(ValueError):
            table.reset()
    finally:
        table.close()
        streams.close()
        other.close()
