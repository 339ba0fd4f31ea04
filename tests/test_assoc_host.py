"""Host-side checks of the tracks (engine.TrackTable, acrmi_tracks_* / acrmi_associate / acrmi_forward_tracks /
acrmi_assoc_step): the rule of csrc/assoc_plan.h through acrmi_assoc_step against the numpy restatement
(tests/assoc_ref.py) on hand-made sequences, the ABI surface and the argument checks that need no device, the packaging of
'track_id', and the rule's stand-alone check program.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import assoc_ref as R
from conftest import ROOT, pkg

NEW = ('acrmi_tracks_create', 'acrmi_tracks_destroy', 'acrmi_tracks_reset', 'acrmi_associate', 'acrmi_forward_tracks',
       'acrmi_assoc_step')


def lib_run(frames, K, gate, max_miss):
    """One stream's frames through acrmi_assoc_step and through the numpy rule -> per side the list of (ids, perm) per frame
    (the library's; they have been compared with the rule's)."""
    ops = pkg('ops')
    slots = R.make_slots(frames, K)
    state = [np.zeros(41, np.int32), np.zeros(41, np.int32)]
    sides = [R.new_side(K), R.new_side(K)]
    got = ([], [])
    for b in range(len(frames)):
        for h in (0, 1):
            ids, perm, born = ops.assoc_step_host(slots[b, :, h], state[h], gate, max_miss)
            want = R.step(sides[h], slots[b, :, h], gate, max_miss)
            assert ids.tolist() == want[0].tolist() and perm.tolist() == want[1].tolist() and born.tolist() == want[2].tolist(), \
                (b, h, ids, perm, born, want)
            assert sorted(perm.tolist()) == list(range(K))
            # the state agrees too: next_id, and the live slots' fields
            assert state[h][0] == sides[h]['next_id']
            for k in range(K):
                t = sides[h]['slots'][k]
                assert bool(state[h][1 + k]) == (t is not None)
                if t is not None:
                    assert [int(state[h][1 + 8 * q + k]) for q in (1, 2, 3, 4)] == [t['miss'], t['id'], t['cy'], t['cx']]
            got[h].append((ids.tolist(), perm.tolist()))
    return got


@pytest.mark.parametrize('name', sorted(R.scenarios()))
def test_rule_agrees_with_numpy_on_the_scenarios(name):
    K, gate, max_miss, frames = R.scenarios()[name]
    for k in sorted({K, 3, 8} - set(range(K))):      # the same hands with more slots than the scenario needs, too
        lib_run(frames, k, gate, max_miss)


def test_rank_swap_keeps_ids_with_positions():
    K, gate, mm, frames = R.scenarios()['rank_swap']
    left, _ = lib_run(frames, K, gate, mm)
    assert [ids for ids, _ in left] == [[0, 1]] * 6
    assert [perm for _, perm in left] == [[0, 1], [1, 0]] * 3


def test_gate_is_inclusive():
    K, gate, mm, frames = R.scenarios()['gate_on']
    assert [ids for ids, _ in lib_run(frames, K, gate, mm)[0]] == [[0, -1]] * 3       # c == gate * gate, twice
    K, gate, mm, frames = R.scenarios()['gate_off']
    assert [ids for ids, _ in lib_run(frames, K, gate, mm)[0]] == [[0, -1], [-1, 1]]  # c == gate * gate + 1


def test_miss_budget():
    sc = R.scenarios()
    assert lib_run(*[sc['miss_within'][i] for i in (3, 0, 1, 2)])[0][-1] == ([0, 1], [1, 0])      # same id after max_miss frames
    assert lib_run(*[sc['miss_beyond'][i] for i in (3, 0, 1, 2)])[0][-1] == ([2, 1], [1, 0])      # a new one after one more
    assert lib_run(*[sc['miss_never'][i] for i in (3, 0, 1, 2)])[0][-1] == ([0, 1], [1, 0])       # -1: never expires


def test_eviction_ties_greedy_and_ordering():
    sc = R.scenarios()
    run = lambda name: lib_run(*[sc[name][i] for i in (3, 0, 1, 2)])
    assert run('eviction')[0][-1] == ([3, 2], [1, 0])          # the track unseen for longer goes first, then the other
    assert run('tie_tracks')[0][-1] == ([0, -1], [0, 1])       # two tracks, one detection: the lower slot
    assert run('tie_dets')[0][-1] == ([0, 1], [0, 1])          # one track, two detections: the lower rank
    # greedy: (track 1, rank 0) first, track 0 is left without a partner in its gate and is evicted by rank 1's birth; the optimal
    # assignment would have given ([0, 1, 2], [0, 1, 2])
    assert run('greedy')[0][-1] == ([3, 1, 2], [1, 0, 2])
    left, right = run('ordering')
    assert left[1] == ([-1, -1, 2], [1, 2, 0])                 # rows without a detection fill in rank order
    assert left[2] == ([3, 4, 2], [1, 2, 0])                   # births take the lowest free slot
    assert right[1] == ([0, -1, -1], [0, 1, 2]) and right[2] == ([0, 1, -1], [0, 1, 2])


def test_garbage_is_not_a_detection():
    ops = pkg('ops')
    nan, inf = float('nan'), float('inf')
    rows = np.array([[nan, 100], [1, nan], [1, -1], [1, 4096], [1, 1e30], [0.5, 7], [1, -inf], [1, inf]], np.float32)
    state = np.zeros(41, np.int32)
    ids, perm, born = ops.assoc_step_host(rows, state, 8, 5)
    assert ids.tolist() == [-1] * 8 and perm.tolist() == list(range(8)) and not born.any() and not state.any()
    left, right = lib_run(*[R.scenarios()['garbage'][i] for i in (3, 0, 1, 2)])
    assert [ids for ids, _ in left] == [[0, -1, -1], [0, -1, -1], [0, 1, -1]]      # (10,10) -> (10,11) -> (10,12); inf flag at (63,63)
    assert [ids for ids, _ in right][:2] == [[0, -1, -1], [0, -1, -1]]


def test_new_symbols_are_declared_exported_and_bound():
    L = pkg('_lib')
    lib = L.lib()
    header = open(os.path.join(ROOT, 'include', 'acrmi.h')).read()
    for name in NEW:
        assert name + '(' in header and name in L.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.acrmi_forward_tracks.argtypes) == len(lib.acrmi_forward_multi.argtypes) + 4
    assert len(lib.acrmi_associate.argtypes) == 10 and len(lib.acrmi_tracks_create.argtypes) == 6
    assert lib.acrmi_tracks_destroy.restype is None
    assert '#define ACRMI_ASSOC_STATE %d' % L.ASSOC_STATE in header
    assert lib.acrmi_version() == L.VERSION == 303      # additive: the ABI version stays


def test_bad_arguments_are_rejected_before_any_device_call():
    L = pkg('_lib')
    lib = L.lib()
    h = ctypes.c_void_p()
    assert lib.acrmi_tracks_create(None, 0, 4, 2, 8, 5) == L.E_INVAL
    # every parameter is checked before the device is looked at
    for cap, K, gate, mm in ((0, 2, 8, 5), (-1, 2, 8, 5), (4, 0, 8, 5), (4, 9, 8, 5), (4, 2, -1, 5), (4, 2, 129, 5), (4, 2, 8, -2),
                             (65537, 1, 8, 5), (32769, 2, 8, 5), (8193, 8, 8, 5), (1 << 30, 8, 8, 5)):
        assert lib.acrmi_tracks_create(ctypes.byref(h), 0, cap, K, gate, mm) == L.E_INVAL and not h.value, (cap, K, gate, mm)
    if not torch.cuda.is_available():                     # a loud failure, no host-side table
        for cap, K, gate, mm in ((4, 2, 8, 5), (65536, 1, 0, -1), (8192, 8, 128, 1 << 30)):
            assert lib.acrmi_tracks_create(ctypes.byref(h), 0, cap, K, gate, mm) == L.E_HIP and not h.value
        with pytest.raises(L.AcrmiError):
            pkg('engine').TrackTable(0, 4, 2)
    with pytest.raises(ValueError):
        pkg('engine').TrackTable(0, 4, 0)
    with pytest.raises(ValueError):
        pkg('engine').TrackTable(0, 4, 2, gate=129)
    lib.acrmi_tracks_destroy(None)                        # like free(NULL)
    ids = (ctypes.c_int32 * 2)(0, 1)
    p = ctypes.c_void_p(256)
    assert lib.acrmi_tracks_reset(None, None, 0, None) == L.E_INVAL
    assert lib.acrmi_tracks_reset(None, ids, 2, None) == L.E_INVAL
    for table, slots, idp, out in ((None, p, ids, p), (p, None, ids, p), (p, p, ids, None), (None, None, None, None)):
        assert lib.acrmi_associate(None, table, slots, 2, 2, idp, 1, out, None, None) == L.E_INVAL
    assert lib.acrmi_forward_tracks(None, None, None, 1, None, 2, 2, None, None, None, None, None, None, None, None, None) == L.E_INVAL
    st = np.zeros(41, np.int32)
    rows = np.zeros((2, 2), np.float32)
    out = np.zeros(8, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.acrmi_assoc_step(2, 8, 5, vp(rows), 2, vp(st), vp(out), vp(out), None) == 0
    for K, gate, mm in ((0, 8, 5), (9, 8, 5), (2, -1, 5), (2, 129, 5), (2, 8, -2)):
        assert lib.acrmi_assoc_step(K, gate, mm, vp(rows), 2, vp(st), vp(out), vp(out), None) == L.E_INVAL
    assert lib.acrmi_assoc_step(2, 8, 5, None, 2, vp(st), vp(out), vp(out), None) == L.E_INVAL
    assert lib.acrmi_assoc_step(2, 8, 5, vp(rows), 1, vp(st), vp(out), vp(out), None) == L.E_INVAL


class StubTable(object):
    """What the argument checks look at of a TrackTable."""
    def __init__(self, capacity=4, max_hand=2, handle=1):
        self.capacity, self.max_hand, self.handle = capacity, max_hand, handle


def test_tracks_arguments():
    E, ops = pkg('engine'), pkg('ops')
    tbl = StubTable()
    assert E.track_args(None, None, None, None, 2, 3) is None
    assert E.track_args([0, -1, 3], tbl, None, None, 2, 3).tolist() == [0, -1, 3]
    for bad in (dict(tracks=[0, 1, 2], track_table=None), dict(tracks=None, track_table=tbl),
                dict(tracks=[0, 1, 2], track_table=tbl, streams=[0, 1, 2]), dict(tracks=[0, 1, 2], track_table=tbl, table=object()),
                dict(tracks=[0, 1, 4], track_table=tbl), dict(tracks=[0, -2, 1], track_table=tbl), dict(tracks=[0, 1], track_table=tbl),
                dict(tracks=[0., 1., 2.], track_table=tbl), dict(tracks=[0, 1, 2], track_table=StubTable(max_hand=3)),
                dict(tracks=[0, 1, 2], track_table=StubTable(handle=None)), dict(tracks=[0, 1, 2], track_table=object())):
        kw = dict(tracks=None, track_table=None, streams=None, table=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            E.track_args(kw['tracks'], kw['track_table'], kw['streams'], kw['table'], 2, 3)
    # the stand-alone operator checks shapes, the table and the ids before it looks at the device
    good = torch.zeros(3, 2, 2, 176)
    for slots, tracks, table in ((torch.zeros(3, 2, 2, 175), [0, 1, 2], tbl), (torch.zeros(3, 9, 2, 176), [0, 1, 2], StubTable(max_hand=9)),
                                 (good.double(), [0, 1, 2], tbl), (good, [0, 1, 9], tbl), (good, [0, 1], tbl),
                                 (good, [0, 1, 2], StubTable(max_hand=1)), (torch.zeros(3, 2, 176), [0, 1, 2], tbl),
                                 (good[:, :, :, ::2], [0, 1, 2], tbl)):
        with pytest.raises(ValueError):
            ops.associate_hands(slots, tracks, table)


def test_track_id_is_packaged_into_the_hand_dicts():
    from importlib import import_module
    main = import_module(pkg().__name__ + '.acr.main')
    g = np.random.default_rng(0)
    B, K = 2, 2
    out = {'slots': g.normal(size=(B, K, 2, 176)).astype(np.float32), 'verts': np.zeros((B, K, 2, 778, 3), np.float32),
           'joints': np.zeros((B, K, 2, 21, 3), np.float32), 'pj2d': np.zeros((B, K, 2, 21, 2), np.float32),
           'pj2d_org': np.zeros((B, K, 2, 21, 2), np.float32), 'cam_trans': np.zeros((B, K, 2, 3), np.float32),
           'track_ids': np.array([[[4, 7], [-1, 2]], [[-1, -1], [5, -1]]], np.int32)}
    out['slots'][..., 0] = (out['track_ids'] >= 0).astype(np.float32)      # flagged where a track has a hand
    res = main.results_from_out(out, ['a', 'b'])
    # flagged lefts in slot order, then flagged rights in slot order
    assert [(int(h['hand_type']), int(h['track_id'])) for h in res['a']] == [(0, 4), (1, 7), (1, 2)]
    assert [(int(h['hand_type']), int(h['track_id'])) for h in res['b']] == [(0, 5)]
    assert all(h['track_id'].dtype == np.int32 for h in res['a'])
    del out['track_ids']                                                     # without tracks= nothing is added
    assert all('track_id' not in h for h in main.results_from_out(out, ['a', 'b'])['a'])


def test_rule_stand_alone_program(tmp_path):
    """tools/assoc_check.cpp: csrc/assoc_plan.h against a plain restatement as a program of its own.  The plain build must pass;
    the build with the address and undefined-behaviour sanitizers must pass as well where the host compiler can make one that
    starts - which of the two ran is printed."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        assert os.path.exists(hipcc), 'no C++ compiler'
        cmd = [hipcc, '-x', 'c++']
    else:
        cmd = [cxx]
    src = os.path.join(ROOT, 'tools', 'assoc_check.cpp')
    cmd += ['-std=c++17', '-O1', '-g', src, '-o']
    plain = str(tmp_path / 'assoc_check')
    subprocess.run(cmd + [plain], check=True, capture_output=True)
    run = subprocess.run([plain], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    ran = None
    for label, extra in (('static', san + ['-static-libasan', '-static-libubsan']), ('shared', san)):
        exe = str(tmp_path / ('assoc_check_' + label))
        if subprocess.run(cmd + [exe] + extra, capture_output=True).returncode != 0:
            continue
        run = subprocess.run([exe], capture_output=True, text=True)
        if 'does not come first in initial library list' in run.stderr:
            continue
        ran = label
        assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
        break
    print('sanitizer variant that ran: %s' % ran)
