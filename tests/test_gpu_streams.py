"""GPU: One-Euro smoothing with per-stream state (engine.StreamTable, acrmi_smooth_streams / acrmi_forward_streams) - every
video stream of a mixed batch gets exactly what the single-stream path (Engine.smooth, pinned to the reference's 14-frame
sequence) gives that stream alone.  `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import cases
from conftest import golden, pkg

pytestmark = pytest.mark.gpu

SEEDS = (41, 42, 43)       # 41 = the sequence smooth_seq.npz records
COEFF = 4.0                # its smooth_coeff


def _L():
    return pkg('_lib')


def make_slots(n_frames, seed):
    """Host slots [T,2,176] of cases.smooth_inputs: flags, poses and betas in their fields, noise in every other field."""
    L = _L()
    poses, betas, flags = cases.smooth_inputs(n_frames, seed)
    slots = torch.from_numpy(np.random.default_rng(1000 + seed).normal(0, 1, (n_frames, 2, L.SLOT)).astype(np.float32))
    slots[:, :, L.SLOT_FLAG] = torch.from_numpy(flags.astype(np.float32))
    slots[:, :, L.SLOT_POSES:L.SLOT_POSES + 48] = torch.from_numpy(poses)
    slots[:, :, L.SLOT_BETAS:L.SLOT_BETAS + 10] = torch.from_numpy(betas)
    return slots


def oracle_stream(slots, coeff):
    """oracle/smooth.py over one stream's host slots [T,2,176] -> (poses [T,2,48], betas [T,2,10]); a hand without flag keeps
    its input and leaves its filters alone (acr/main.py:78-80)."""
    from oracle import smooth as osm
    L = _L()
    s = slots.numpy()
    poses = s[:, :, L.SLOT_POSES:L.SLOT_POSES + 48].copy()
    betas = s[:, :, L.SLOT_BETAS:L.SLOT_BETAS + 10].copy()
    filt = {0: osm.new_filters(coeff), 1: osm.new_filters(coeff)}
    for t in range(s.shape[0]):
        for h in range(2):
            if s[t, h, L.SLOT_FLAG] > 0.5:
                poses[t, h], betas[t, h] = osm.smooth_results(filt[h], poses[t, h], betas[t, h])
    return poses, betas


def untouched_mask():
    L = _L()
    m = torch.ones(L.SLOT, dtype=torch.bool)
    m[L.SLOT_POSES:L.SLOT_BETAS + 10] = False
    return m


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope='module')
def eng():
    e = pkg('engine').Engine(0)
    e.set_temporal(False, smooth_coeff=COEFF)
    yield e
    e.close()


def alone(eng, slots):
    """The single-stream path on one stream's frames: a new sequence, all frames in one call."""
    d = slots.clone().cuda()
    eng.smooth_reset()
    eng.smooth(d)
    return d


@pytest.fixture(scope='module')
def ref(eng):
    """Per seed: the input slots, what Engine.smooth gives the stream alone, and the oracle's poses / betas.  Read only."""
    out = {}
    for seed in SEEDS:
        slots = make_slots(14, seed)
        out[seed] = {'in': slots, 'alone': alone(eng, slots), 'oracle': oracle_stream(slots, COEFF)}
    return out


def deal(order, per_batch):
    """order: the stream (0..2) of each of the 42 frames in arrival order -> [(stream, t)] cut into batches."""
    seen = [0, 0, 0]
    seq = []
    for s in order:
        seq.append((s, seen[s]))
        seen[s] += 1
    assert seen == [14, 14, 14]
    return [seq[i:i + per_batch] for i in range(0, len(seq), per_batch)]


def interleaved_order():
    """[0,1,0,2,1,0,...]: the pattern repeated, a stream that has dealt its 14 frames is skipped."""
    left, order, k = [14, 14, 14], [], 0
    while sum(left):
        s = (0, 1, 0, 2, 1, 0)[k % 6]
        k += 1
        if left[s]:
            left[s] -= 1
            order.append(s)
    return order


@pytest.mark.parametrize('name', ['round_robin', 'interleaved', 'one_call'])
def test_interleaved_streams_equal_each_stream_alone(eng, ref, name):
    """Three sequences dealt into batches - one frame of each per batch; several frames of one stream in a batch; all 42
    frames in one call - come out as Engine.smooth gives each stream alone (bit for bit), within 1e-5 of oracle/smooth.py
    and (seed 41) of the reference's own recording; no field outside poses / betas is written."""
    L = _L()
    batches = {'round_robin': deal([0, 1, 2] * 14, 3), 'interleaved': deal(interleaved_order(), 5),
               'one_call': deal(interleaved_order(), 42)}[name]
    rows = (2, 0, 3)                                  # table row of stream 0..2
    table = pkg('engine').StreamTable(0, 4)
    got = [torch.zeros(14, 2, L.SLOT) for _ in SEEDS]
    for batch in batches:
        d = torch.stack([ref[SEEDS[s]]['in'][t] for s, t in batch]).cuda()
        eng.smooth(d, streams=[rows[s] for s, _ in batch], table=table)
        for i, (s, t) in enumerate(batch):
            got[s][t] = d[i].cpu()
    table.close()
    keep = untouched_mask()
    g = golden('smooth_seq.npz')
    assert float(g['smooth_coeff']) == COEFF
    for s, seed in enumerate(SEEDS):
        r = ref[seed]
        assert torch.equal(got[s], r['alone'].cpu()), seed
        a = got[s].numpy()
        dp = np.abs(a[:, :, L.SLOT_POSES:L.SLOT_POSES + 48] - r['oracle'][0]).max()
        db = np.abs(a[:, :, L.SLOT_BETAS:L.SLOT_BETAS + 10] - r['oracle'][1]).max()
        print('%s seed %d: |poses - oracle| %.2e, |betas - oracle| %.2e' % (name, seed, dp, db))
        assert dp < 1e-5 and db < 1e-5, seed
        if seed == 41:
            assert np.abs(a[:, :, L.SLOT_POSES:L.SLOT_POSES + 48] - g['poses']).max() < 1e-5
            assert np.abs(a[:, :, L.SLOT_BETAS:L.SLOT_BETAS + 10] - g['betas']).max() < 1e-5
        assert torch.equal(bits(got[s][:, :, keep]), bits(r['in'][:, :, keep])), seed
        assert not torch.equal(got[s], r['in'])       # (something was filtered)


def test_skipped_frames_leave_slots_and_state_alone(eng, ref):
    """A frame with id -1, a frame whose flags are NaN (an 'fp16x3' range error poisons slots with NaN) and a frame whose
    flags are 0 come back bit-unchanged and leave the stream's state as it was: the stream's next frame gets what it would
    have got without them."""
    L = _L()
    r = ref[42]
    junk = make_slots(14, 77)[:3].clone()
    junk[0, :, L.SLOT_FLAG] = 1.0                    # would be filtered if its id were not -1
    junk[1] = float('nan')                           # flags NaN, everything else too
    junk[2, :, L.SLOT_FLAG] = 0.0
    table = pkg('engine').StreamTable(0, 3)
    first = torch.cat([r['in'][0:3], junk]).cuda()                      # t = 0, 1, 2, then the three
    eng.smooth(first, streams=[1, 1, 1, -1, 1, 1], table=table)
    second = torch.cat([junk, r['in'][3:6]]).cuda()[[0, 3, 1, 4, 2, 5]]    # interleaved with t = 3, 4, 5
    eng.smooth(second, streams=torch.tensor([-1, 1, 1, 1, 1, 1]), table=table)
    table.close()
    first, second = first.cpu(), second.cpu()
    assert torch.equal(bits(first[3:]), bits(junk))
    assert torch.equal(bits(second[[0, 2, 4]]), bits(junk))
    assert torch.equal(torch.cat([first[:3], second[[1, 3, 5]]]), r['alone'][:6].cpu())


def test_capacity_and_id_range(eng, ref):
    """Capacity 1; capacity 65536 with its first and last row; ids outside [-1, capacity) and capacities outside 1..65536 are
    ValueError (ACRMI_EINVAL) and nothing is launched."""
    E = pkg('engine')
    a, b = ref[41], ref[42]
    t1 = E.StreamTable(0, 1)
    d = a['in'].clone().cuda()
    eng.smooth(d, streams=np.zeros(14, np.int64), table=t1)
    assert torch.equal(d, a['alone'])
    for bad in (1, -2):
        before = d.clone()
        with pytest.raises(ValueError):
            eng.smooth(d, streams=[0] * 13 + [bad], table=t1)
        torch.cuda.synchronize()
        assert torch.equal(d, before)
    t1.close()
    big = E.StreamTable(0, 65536)
    d = torch.stack([a['in'], b['in']], 1).reshape(28, 2, -1).cuda()      # frames of the two streams alternate
    eng.smooth(d, streams=[0, 65535] * 14, table=big)
    assert torch.equal(d[0::2], a['alone']) and torch.equal(d[1::2], b['alone'])
    before = d.clone()
    with pytest.raises(ValueError):
        eng.smooth(d, streams=[0, 65536] * 14, table=big)
    torch.cuda.synchronize()
    assert torch.equal(d, before)
    big.close()
    for cap in (0, 65537, -1):
        with pytest.raises(ValueError):
            E.StreamTable(0, cap)


def test_null_table_ids_and_slots_with_a_live_context(eng, ref):
    """The C entry point itself (Python's checks are not in the way): a NULL table, NULL ids, NULL slots or B = 0 with a real
    context is ACRMI_EINVAL, nothing is launched and the context says which call refused."""
    import ctypes
    L = _L()
    lib = L.lib()
    table = pkg('engine').StreamTable(0, 2)
    d = ref[41]['in'][:1].clone().cuda()
    before = d.clone()
    ids = (ctypes.c_int32 * 1)(0)
    p = ctypes.c_void_p(d.data_ptr())
    for tbl, slots, idp, B in ((None, p, ids, 1), (table.handle, p, None, 1), (table.handle, None, ids, 1), (table.handle, p, ids, 0)):
        assert lib.acrmi_smooth_streams(eng.ctx, tbl, slots, B, idp, None) == L.E_INVAL
        assert b'acrmi_smooth_streams' in lib.acrmi_last_error(eng.ctx)
    assert lib.acrmi_forward_streams(eng.ctx, None, ids, p, 1, None, p, p, p, None, None, None, None) == L.E_INVAL
    assert lib.acrmi_forward_streams(eng.ctx, table.handle, None, p, 1, None, p, p, p, None, None, None, None) == L.E_INVAL
    torch.cuda.synchronize()
    assert torch.equal(d, before)
    table.close()


def test_more_frames_than_one_launch_carries(eng):
    """300 frames of two alternating streams in ONE call (256 frames per launch: both streams have frames on either side of the
    split, and their state crosses it) == the same frames as 300 calls of one frame."""
    E = pkg('engine')
    two = torch.stack([make_slots(150, 44), make_slots(150, 45)], 1).reshape(300, 2, -1)
    ids = [3, 1] * 150
    whole, single = two.clone().cuda(), two.clone().cuda()
    ta, tb = E.StreamTable(0, 4), E.StreamTable(0, 4)
    eng.smooth(whole, streams=ids, table=ta)
    for i in range(300):
        eng.smooth(single[i:i + 1], streams=ids[i:i + 1], table=tb)
    torch.cuda.synchronize()
    assert torch.equal(whole, single)
    assert not torch.equal(whole.cpu(), two)
    ta.close()
    tb.close()


def test_reset_of_listed_streams_and_of_all(eng, ref):
    """reset([1]): stream 1's next sample starts a new sequence while stream 0 continues; reset(): both start anew."""
    L = _L()
    a, b = ref[41], ref[42]
    table = pkg('engine').StreamTable(0, 2)

    def run(lo, hi):
        d = torch.stack([a['in'][lo:hi], b['in'][lo:hi]], 1).reshape(2 * (hi - lo), 2, -1).cuda()
        eng.smooth(d, streams=[0, 1] * (hi - lo), table=table)
        return d[0::2], d[1::2]

    run(0, 5)
    table.reset([1])
    g0, g1 = run(5, 10)
    assert torch.equal(g0, a['alone'][5:10])                       # stream 0 went on
    assert torch.equal(g1, alone(eng, b['in'][5:10]))              # stream 1 = a new sequence from frame 5
    fing = slice(L.SLOT_POSES + 3, L.SLOT_POSES + 48)
    assert torch.equal(g1[0, :, fing].cpu(), b['in'][5, :, fing])  # whose first sample passes through
    assert not torch.equal(g0[0, :, fing].cpu(), a['in'][5, :, fing])
    table.reset()
    g0, g1 = run(10, 14)
    assert torch.equal(g0, alone(eng, a['in'][10:14])) and torch.equal(g1, alone(eng, b['in'][10:14]))
    table.close()


# ---- the fused call ------------------------------------------------------------------------------------------------
FUSED_IDS = [0, 1, 0, 1]
FUSED_COEFF = 3.0


def fused_batch(frames2):
    return torch.from_numpy(np.stack([frames2[0], frames2[1], frames2[1], frames2[0]]))


@pytest.fixture(scope='module')
def fused(synth_sd, mano_tables, frames2):
    """One Engine on the synthetic checkpoint: the un-smoothed forward of the four frames, and three forward(..., streams=
    [0,1,0,1], table=) calls on them (stream 0 sees frames 0, 2 of each call, stream 1 frames 1, 3).  Host copies, read only."""
    E = pkg('engine')
    e = E.Engine(0)
    e.load_state_dict(synth_sd, max_batch=4)
    e.load_mano(mano_tables)
    e.set_temporal(False, smooth_coeff=FUSED_COEFF)
    img = fused_batch(frames2).cuda()
    raw = {k: v.cpu() for k, v in e.forward(img).items()}
    table = E.StreamTable(0, 2)
    calls = [{k: v.cpu() for k, v in e.forward(img, streams=FUSED_IDS, table=table).items()} for _ in range(3)]
    table.close()
    e.close()
    return {'raw': raw, 'calls': calls}


def fused_oracle(raw_slots, calls=3):
    """The oracle's filters per stream over the un-smoothed slots of `calls` calls -> [call][frame] (poses [2,48], betas [2,10])."""
    from oracle import smooth as osm
    L = _L()
    s = raw_slots.numpy()
    filt = {sid: {0: osm.new_filters(FUSED_COEFF), 1: osm.new_filters(FUSED_COEFF)} for sid in set(FUSED_IDS)}
    out = []
    for _ in range(calls):
        frames = []
        for i, sid in enumerate(FUSED_IDS):
            p = s[i, :, L.SLOT_POSES:L.SLOT_POSES + 48].copy()
            b = s[i, :, L.SLOT_BETAS:L.SLOT_BETAS + 10].copy()
            for h in range(2):
                if s[i, h, L.SLOT_FLAG] > 0.5:
                    p[h], b[h] = osm.smooth_results(filt[sid][h], p[h], b[h])
            frames.append((p, b))
        out.append(frames)
    return out


def test_fused_forward_smooths_per_stream(fused):
    """forward(..., streams=, table=): poses / betas within 2e-5 (the bound of test_temporal_optimization_through_acr_main) of
    the oracle's filters run per stream over the un-smoothed forward; a stream's first sample passes through, later ones are
    filtered."""
    L = _L()
    raw, calls = fused['raw'], fused['calls']
    assert (raw['slots'][:, :, L.SLOT_FLAG] > 0.5).any()
    want = fused_oracle(raw['slots'])
    for c, out in enumerate(calls):
        s = out['slots'].numpy()
        for i in range(4):
            dp = np.abs(s[i, :, L.SLOT_POSES:L.SLOT_POSES + 48] - want[c][i][0]).max()
            db = np.abs(s[i, :, L.SLOT_BETAS:L.SLOT_BETAS + 10] - want[c][i][1]).max()
            print('call %d frame %d: |poses - oracle| %.2e, |betas - oracle| %.2e' % (c, i, dp, db))
            assert dp < 2e-5 and db < 2e-5, (c, i)
            moved = float((out['verts'][i] - raw['verts'][i]).abs().max())
            if c == 0 and i < 2:
                assert moved <= 1e-6, (c, i)           # first sample of stream 0 / stream 1
            else:
                assert moved > 1e-5, (c, i)


def test_pool_contexts_share_one_table(synth_sd, mano_tables, frames2):
    """EnginePool(n=2) with one table: six two-frame batches with streams [0,1] land on the two contexts in turn, each on its
    own HIP stream; the table's event orders the updates, so the results equal one Engine's with its own table."""
    E = pkg('engine')
    batches = [torch.from_numpy(frames2 if k % 2 == 0 else frames2[::-1].copy()).cuda() for k in range(6)]
    pool = E.EnginePool(0, n=2)
    pool.load_state_dict(synth_sd, max_batch=2)
    pool.load_mano(mano_tables)
    pool.configure(lambda e: e.set_temporal(False, smooth_coeff=FUSED_COEFF))
    assert pool.stream_table(2) is pool.stream_table(2)
    got, tickets = [], []
    for img in batches:
        if len(tickets) == 2:
            got.append({k: v.clone() for k, v in pool.collect(tickets.pop(0)).items()})
        tickets.append(pool.submit(img, streams=[0, 1]))
    while tickets:
        got.append({k: v.clone() for k, v in pool.collect(tickets.pop(0)).items()})
    torch.cuda.synchronize()
    one = E.Engine(0)
    one.load_state_dict(synth_sd, max_batch=2)
    one.load_mano(mano_tables)
    one.set_temporal(False, smooth_coeff=FUSED_COEFF)
    table = E.StreamTable(0, 2)
    for k, img in enumerate(batches):
        want = one.forward(img, streams=[0, 1], table=table)
        for key in ('slots', 'verts', 'joints'):
            assert torch.equal(got[k][key], want[key]), (k, key)
    plain = one.forward(batches[5])
    assert not torch.equal(plain['slots'], got[5]['slots'])      # (the sixth batch was filtered)
    table.close()
    one.close()
    pool.close()


def test_acr_main_forward_batch_streams(fused, synth_sd, mano_tables, frames2):
    """acr.main.ACR.forward_batch(..., streams=) with -t gives the fused call's numbers (results are float16: compared at the
    2e-5 of the fused test plus half a float16 ulp); without -t it raises; without `streams` the results are those of an ACR
    that never saw `streams`."""
    L = _L()
    cfg = pkg('config')
    A = pkg('acr.main').ACR
    base = ['--configs_yml', '/nonexistent.yml']
    t_args = base + ['-t', '--smooth_coeff', str(FUSED_COEFF)]
    img, paths = fused_batch(frames2), ['a', 'b', 'c', 'd']
    acr = A(args_set=cfg.parse_args(t_args), state_dict=synth_sd, mano_tables=mano_tables, max_batch=4)
    for c in range(2):
        res = acr.forward_batch(img, paths, point_heads=False, streams=FUSED_IDS, max_streams=2)
        ref_slots = fused['calls'][c]['slots'].numpy()
        for i, p in enumerate(paths):
            hands = res[p] if res[p] else []
            assert [int(h['hand_type']) for h in hands] == [h for h in (0, 1) if ref_slots[i, h, L.SLOT_FLAG] > 0.5]
            for hand in hands:
                s = ref_slots[i, int(hand['hand_type'])]
                for key, want in (('poses', s[L.SLOT_POSES:L.SLOT_POSES + 48]), ('betas', s[L.SLOT_BETAS:L.SLOT_BETAS + 10])):
                    assert hand[key].dtype == np.float16
                    assert (np.abs(hand[key].astype(np.float32) - want) <= 2e-5 + np.abs(want) * 2.0 ** -11).all(), (c, p, key)
    with pytest.raises(ValueError):
        acr.forward_batch(img, paths, streams=FUSED_IDS, max_streams=3)      # the table exists with 2 streams
    # the table is the ACR object's, not the context's: a checkpoint reload builds a new context and the streams go on -
    # a third call gives what the fused call's third pass over the same frames gives
    old_engine = acr.model.engine(4)
    acr.model.load_state_dict(synth_sd)
    res = acr.forward_batch(img, paths, point_heads=False, streams=FUSED_IDS)
    assert acr.model.engine(4) is not old_engine
    first, third = fused['calls'][0]['slots'].numpy(), fused['calls'][2]['slots'].numpy()
    told_apart = False          # a stream that had started anew would give the first call again: the two must differ by more than the bound
    for i, p in enumerate(paths):
        for hand in res[p] or []:
            h = int(hand['hand_type'])
            for key, lo, n in (('poses', L.SLOT_POSES, 48), ('betas', L.SLOT_BETAS, 10)):
                want = third[i, h, lo:lo + n]
                tol = 2e-5 + np.abs(want) * 2.0 ** -11
                assert (np.abs(hand[key].astype(np.float32) - want) <= tol).all(), (p, key)
                told_apart |= bool((np.abs(first[i, h, lo:lo + n] - want) > 4 * tol).any())
    assert told_apart
    acr.reset_streams([0])
    acr.reset_streams()
    acr.close_streams()
    assert acr.stream_table is None
    # without `streams`: the batch is one video, exactly as before
    fresh = A(args_set=cfg.parse_args(t_args), state_dict=synth_sd, mano_tables=mano_tables, max_batch=4)
    mine, theirs = acr.forward_batch(img, paths), fresh.forward_batch(img, paths)
    for p in paths:
        assert len(mine[p]) == len(theirs[p])
        for x, y in zip(mine[p] or [], theirs[p] or []):
            for key in x:
                np.testing.assert_array_equal(x[key], y[key], err_msg='%s %s' % (p, key))
    plain = A(args_set=cfg.parse_args(base), state_dict=synth_sd, mano_tables=mano_tables, max_batch=4)
    with pytest.raises(ValueError):
        plain.forward_batch(img, paths, streams=FUSED_IDS)
