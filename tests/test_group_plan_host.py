"""The executor's grouping rule (csrc/group_plan.h) on the lowered large-batch program, through the stand-alone check program
tools/group_plan_check.cpp: what it groups is held against the rule's own terms there (exit status) and, here, against an
independent search of the program's dependencies (tests/group_ref.py).  No GPU."""
import os
import shutil
import subprocess

import pytest

import group_ref
from conftest import ROOT, pkg


@pytest.fixture(scope='module')
def checker(tmp_path_factory):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        assert os.path.exists(hipcc), 'no C++ compiler'
        cmd = [hipcc, '-x', 'c++']
    else:
        cmd = [cxx]
    exe = str(tmp_path_factory.mktemp('group_plan') / 'group_plan_check')
    subprocess.run(cmd + ['-std=c++17', '-O1', os.path.join(ROOT, 'tools', 'group_plan_check.cpp'), '-o', exe], check=True, capture_output=True)
    return exe


def run_checker(exe, table, n_bufs, gmax=2):
    """table rows (index, key, reads, writes) -> (return code, groups as (leader, follower) in the rows' indices, order, verdict)"""
    idx = [row[0] for row in table]
    lines = ['%d %d %d' % (len(table), n_bufs, gmax)]
    for _i, key, R, W in table:
        lines.append(' '.join(str(v) for v in [key, len(R)] + list(R) + [len(W)] + list(W)))
    run = subprocess.run([exe], input='\n'.join(lines) + '\n', capture_output=True, text=True)
    out = run.stdout.splitlines()
    n = int(out[0].split()[1])
    groups = [tuple(idx[int(v)] for v in line.split()) for line in out[1:1 + n]]
    order = [idx[int(v)] for v in out[1 + n].split()]
    return run.returncode, groups, order, out[-1]


@pytest.fixture(scope='module')
def large_prog(synth_sd):
    return pkg('packer').lower(synth_sd, point_heads=True)      # what Engine.load_state_dict lowers for max_batch >= 16


@pytest.mark.parametrize('point', [False, True])
def test_groups_of_the_large_batch_program(checker, large_prog, point):
    prog = large_prog
    table = group_ref.program_table(prog, point)
    rc, groups, order, verdict = run_checker(checker, table, len(prog['bufs']) + 2)
    assert rc == 0 and verdict == 'ok', verdict
    anc = group_ref.ancestors(table)
    key = {row[0]: row[1] for row in table}
    names = [i['name'] for i in prog['op_info']]
    # no group contains a dependency edge (nor a path), none spans instantiations, no op is in two groups
    seen = set()
    for x, y in groups:
        assert key[x] and key[x] == key[y], (names[x], names[y])
        assert x not in anc[y] and y not in anc[x], (names[x], names[y])
        assert not ({x, y} & seen)
        seen |= {x, y}
    # the enqueue order is the program's ops, each once, every op behind everything it depends on
    assert sorted(order) == sorted(row[0] for row in table)
    pos = {j: k for k, j in enumerate(order)}
    for j in order:
        assert all(pos[d] < pos[j] for d in anc[j]), names[j]
    for x, y in groups:
        assert pos[y] == pos[x] + 1
    # every branch-1 / branch-2 pair of an HR module is a group: 32 in stage 3 and 24 in stage 4 of HRNet-W32
    want = group_ref.hr_pairs(prog, point)
    assert len(want) == 56
    got = {(names[x], names[y]) for x, y in groups}
    assert set(want) <= got, sorted(set(want) - got)[:4]


def test_small_cases(checker):
    # two independent ops of one instantiation with a third between them that the second does not read: a group, made adjacent
    t = [(0, 1, [0], [1]), (1, 0, [1], [2]), (2, 1, [3], [4])]
    rc, groups, order, verdict = run_checker(checker, t, 5)
    assert (rc, groups, order, verdict) == (0, [(0, 2)], [0, 2, 1], 'ok')
    # ... that the second DOES read (a path from the first): no group
    t = [(0, 1, [0], [1]), (1, 0, [1], [2]), (2, 1, [2], [4])]
    assert run_checker(checker, t, 5)[1] == []
    # a WAR hazard through a reused buffer id is an edge: the second op overwrites what the first reads
    t = [(0, 1, [0], [1]), (1, 1, [2], [0])]
    assert run_checker(checker, t, 3)[1] == []
    # different instantiations, and ops of none
    t = [(0, 1, [0], [1]), (1, 2, [2], [3]), (2, 0, [4], [5]), (3, 0, [6], [7])]
    assert run_checker(checker, t, 8)[1] == []
    # three candidates, groups of two: the third launches alone
    t = [(0, 1, [0], [1]), (1, 1, [2], [3]), (2, 1, [4], [5])]
    assert run_checker(checker, t, 6)[1] == [(0, 1)]
    # a partner beyond the look-ahead stays where it is
    far = [(0, 1, [0], [1])] + [(i, 0, [2], [3]) for i in range(1, 18)] + [(18, 1, [4], [5])]
    assert run_checker(checker, far, 6)[1] == []
