"""csrc/mano_plan.h is the one statement of how the MANO kernel splits a hand over workgroups: launch_mano takes the slice count
from it, the kernel its vertex range.  The stand-alone program tools/mano_plan_check.cpp prints the plan - slice count for 1..600
hands and every root joint, vertex ranges for every slice count, fingertip vertices - and the rules the kernel relies on are
held against it here: every vertex and every fingertip belongs to exactly one slice.  tests/test_gpu_mano.py reaches the slice
counts by its number of hands alone (cases.MANO_SLICE_HANDS): that the list still reaches all of them is checked here too.
No GPU."""
import os
import shutil
import subprocess

import pytest

import cases
from conftest import ROOT

NV = 778
TIP_ROOTS = (4, 8, 12, 16, 20)


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    """The check program's lines, parsed: the compiler is found the way tests/test_conv_rules_host.py finds one."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        assert os.path.exists(hipcc), 'no C++ compiler'
        cmd = [hipcc, '-x', 'c++']
    else:
        cmd = [cxx]
    exe = str(tmp_path_factory.mktemp('mano_plan') / 'mano_plan_check')
    subprocess.run(cmd + ['-std=c++17', '-O1', os.path.join(ROOT, 'tools', 'mano_plan_check.cpp'), '-o', exe], check=True, capture_output=True)
    run = subprocess.run([exe], check=True, capture_output=True, text=True)
    p = {'nv': None, 'tips': {}, 'slices': {}, 'ranges': {}}
    for line in run.stdout.splitlines():
        kind, *v = line.split()
        v = [int(x) for x in v]
        if kind == 'NV':
            p['nv'], = v
        elif kind == 'T':
            p['tips'][(v[0], v[1])] = v[2]
        elif kind == 'S':
            p['slices'][(v[0], v[1])] = v[2]
        else:
            assert kind == 'R', line
            p['ranges'].setdefault(v[0], []).append(tuple(v[1:]))
    assert p['nv'] == NV and len(p['tips']) == 10 and len(p['slices']) == 600 * 22 and sorted(p['ranges']) == list(range(1, 9))
    return p


def test_ranges_partition_the_vertices(plan):
    for slices, rows in plan['ranges'].items():
        assert [r[0] for r in rows] == list(range(slices)), slices
        end = 0
        for _, v0, v1 in rows:
            assert v0 == end and v1 > v0, (slices, rows)        # in order, nothing skipped, nothing twice, none empty
            end = v1
        assert end == NV, (slices, rows)


def test_every_fingertip_has_one_owner(plan):
    from oracle import mano as omano
    assert [plan['tips'][(0, k)] for k in range(5)] == omano.TIPS['left']          # [left, right], as the kernel indexes them
    assert [plan['tips'][(1, k)] for k in range(5)] == omano.TIPS['right']
    for slices, rows in plan['ranges'].items():
        for tip in plan['tips'].values():
            assert sum(v0 <= tip < v1 for _, v0, v1 in rows) == 1, (slices, tip)


def test_slice_counts(plan):
    for (H, c), s in plan['slices'].items():
        assert 1 <= s <= 8, (H, c, s)
        assert H * s >= min(H, 256), (H, c, s)
        if c in TIP_ROOTS or H >= 256:
            assert s == 1, (H, c, s)                             # a fingertip root is known to the slice that skinned it only
        else:
            assert s == plan['slices'][(H, -1)], (H, c, s)       # no other root joint matters
    assert plan['slices'][(2, 9)] == 8 and plan['slices'][(128, 9)] == 2          # (the figures of the header's comment)


def test_the_gpu_tests_hand_counts_reach_every_slice_count(plan):
    """tests/test_gpu_mano.py forces nothing: it reaches a slice count by calling the kernel with that many hands.  If this
    fails the formula was retuned: choose new hand counts for cases.MANO_SLICE_HANDS, so that every count of 1..8 that the
    formula can still give is run on the GPU, and more than one hand at the ragged ones."""
    for c in (9, 0, -1):
        got = [plan['slices'][(H, c)] for H in cases.MANO_SLICE_HANDS]
        assert got == [8, 8, 8, 7, 7, 6, 5, 4, 3, 2, 1, 1], (c, got)
        assert set(got) == set(range(1, 9))
    reachable = {s for (H, c), s in plan['slices'].items()}
    assert reachable == set(range(1, 9))
    for H in (2, 36, 129):                                       # test_fingertip_roots: one slice whatever the hand count
        assert all(plan['slices'][(H, c)] == 1 for c in TIP_ROOTS)
    assert max(cases.MANO_SLICE_HANDS) <= 300
