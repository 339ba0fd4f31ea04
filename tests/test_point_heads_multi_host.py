"""CPU-side checks of the point heads for several hands of each side: the rule of csrc/point_plan.h
through its stand-alone check program - plain, under the address and undefined-behaviour sanitizers, and as plain C++ through
hipcc - against the numpy restatement in tests/point_ref.py; the additive ABI; the argument checks that return before HIP is
touched; the new keyword of the acr layer.  None of it needs a GPU."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import multi_ref as M
import point_ref as P
from conftest import ROOT, pkg

KS = (1, 2, 3, 8)
SRC = os.path.join(ROOT, 'tools', 'point_plan_check.cpp')


def _frame(K, lefts, rights, thresh=M.CONF_THRESH):
    """Peaks [(y, x, height)] of the two sides -> (K, flag [K,2], flat [K,2], partner [K,2]) by multi_ref's rule."""
    maps = []
    for peaks in (lefts, rights):
        c = np.zeros((M.MAP, M.MAP), np.float32)
        for y, x, a in peaks:
            c[y, x] = a
        maps.append(c)
    flag, flat, partner, _ = P.plan_of_maps(maps[0], maps[1], K, thresh)
    return K, flag, flat, partner


def _frames():
    """The named cases at every K, and seeded frames."""
    named = {
        'all ranks unflagged': ([], []),
        'a flagged centre at pixel 0 next to placeholders': ([(0, 0, 0.9)], [(3, 3, 0.8)]),
        'pixel 0 flagged on both sides': ([(0, 0, 0.9), (9, 9, 0.5)], [(0, 0, 0.7)]),
        'shared partners': ([(20, 20, 0.9), (20, 23, 0.8), (26, 20, 0.7)], [(22, 30, 0.9)]),
        'no partner within 32 px': ([(2, 2, 0.9), (60, 60, 0.8)], [(2, 40, 0.9)]),
        'nobody within 32 px': ([(0, 0, 0.9)], [(63, 63, 0.9)]),
        'one side empty': ([], [(5, 5, 0.9), (40, 40, 0.8)]),
        'eight and eight': ([(4 + 7 * i, 5, 0.9 - 0.05 * i) for i in range(8)], [(4 + 7 * i, 50, 0.9 - 0.05 * i) for i in range(8)]),
        'nine peaks': ([(3 + 6 * i, 30, 0.95 - 0.05 * i) for i in range(9)], [(3 + 6 * i, 36, 0.5 + 0.05 * i) for i in range(9)]),
        'under the threshold': ([(10, 10, 0.35)], [(12, 12, 0.36)]),
    }
    frames = [(name, _frame(K, l, r)) for name, (l, r) in named.items() for K in KS]
    g = M.rng(20261019)
    for i in range(120):
        K = KS[i % len(KS)]
        sides = []
        for _ in (0, 1):
            n = int(g.integers(0, 11))
            pts = {(int(g.integers(0, 22)) * 3, int(g.integers(0, 22)) * 3) for _ in range(n)}      # >= 3 px apart: all survive the NMS
            sides.append([(y, x, float(np.float32(g.uniform(0.2, 1.0)))) for y, x in sorted(pts)])
        frames.append(('seeded %d' % i, _frame(K, sides[0], sides[1])))
    return frames


def _line(K, flat, partner):
    return '%d %s\n' % (K, ' '.join('%d %d %d %d' % (flat[k, 0], partner[k, 0], flat[k, 1], partner[k, 1]) for k in range(K)))


def _parse(line):
    w = line.split()
    out, i = {}, 0
    for key in ('own_l', 'own_r', 'prior_l', 'prior_r'):
        assert w[i] == key, line
        n = int(w[i + 1])
        out[key] = [int(v) for v in w[i + 2:i + 2 + n]]
        i += 2 + n
    for key in ('grid_l', 'grid_r'):
        assert w[i] == key, line
        j = i + 1
        while j < len(w) and not w[j].startswith('grid_'):
            j += 1
        out[key] = [int(v) for v in w[i + 1:j]]
        i = j
    assert i == len(w), line
    return out


def test_the_restatement_on_known_frames():
    K, flag, flat, partner = _frame(3, [(0, 0, 0.9)], [(3, 3, 0.8)])
    assert flag[:, 0].tolist() == [True, False, False] and flat[:, 0].tolist() == [0, 0, 0]
    plan = P.plan(flat, partner)
    assert plan['own'] == ([0], [3 * 64 + 3, 0])               # pixel 0 once on the left; the right's placeholders add it
    assert plan['prior'] == ([3 * 64 + 3], [0])
    K, flag, flat, partner = _frame(3, [(20, 20, 0.9), (20, 23, 0.8), (26, 20, 0.7)], [(22, 30, 0.9)])
    plan = P.plan(flat, partner)
    assert plan['prior'][0] == [22 * 64 + 30] and len(plan['own'][0]) == 3      # three hands share one partner
    assert plan['prior'][1] == [20 * 64 + 23] and plan['own'][1] == [22 * 64 + 30, 0]
    K, flag, flat, partner = _frame(2, [], [])
    assert P.plan(flat, partner) == {'own': ([0], [0]), 'prior': ([], [])}
    K, flag, flat, partner = _frame(2, [(2, 2, 0.9), (60, 60, 0.8)], [(2, 40, 0.9)])
    assert partner[:, 0].tolist() == [-1, -1] and P.plan(flat, partner)['prior'] == ([], [])      # 38 px and more


def _compiler():
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        assert os.path.exists(hipcc), 'no C++ compiler'
        return [hipcc, '-x', 'c++']
    return [cxx]


def _check_program(exe):
    frames = _frames()
    run = subprocess.run([exe], input=''.join(_line(K, flat, partner) for _, (K, _, flat, partner) in frames),
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    got = run.stdout.strip().split('\n')
    assert len(got) == len(frames)
    seen = set()
    for line, (name, (K, flag, flat, partner)) in zip(got, frames):
        want, have = P.plan(flat, partner), _parse(line)
        for s, c in enumerate('lr'):
            own, prior = want['own'][s], want['prior'][s]
            assert have['own_' + c] == own and have['prior_' + c] == prior, (name, K, line, want)
            assert 1 <= len(own) <= K and len(prior) <= K
            pad = lambda v: v + [-1] * (K - len(v))
            assert have['grid_' + c] == pad(own) + pad(own) + pad(prior), (name, K, line)      # params, cam, prior towers
            # what decode_multi_kernel reads is in the lists, and the lists hold nothing else
            assert set(own) == set(flat[:, s].tolist()) and set(prior) == set(p for p in partner[:, s].tolist() if p >= 0)
            if not flag[:, s].all() and (flag[:, s] & (flat[:, s] == 0)).any():
                seen.add('flagged pixel 0 with placeholders')
            if len(prior) < (partner[:, s] >= 0).sum():
                seen.add('shared partner')
            if flag[:, s].any() and not (partner[:, s] >= 0).any() and flag[:, 1 - s].any():
                seen.add('nobody within 32 px')
            if not flag[:, s].any():
                seen.add('nothing flagged')
            if len(own) == K == 8:
                seen.add('eight own pixels')
    assert seen == {'flagged pixel 0 with placeholders', 'shared partner', 'nobody within 32 px', 'nothing flagged', 'eight own pixels'}
    for bad in ('0\n', '9' + ' 0 -1 0 -1' * 9 + '\n', '2 0 -1 0 -1\n', '1 4096 -1 0 -1\n', '1 0 -2 0 -1\n', '1 0 4096 0 -1\n',
                '1 -1 -1 0 -1\n', '1 0 -1 0 x\n', '1.5 0 -1 0 -1\n'):
        assert subprocess.run([exe], input=bad, capture_output=True, text=True).returncode == 2, bad
    assert subprocess.run([exe, 'other'], input='', capture_output=True, text=True).returncode == 2


def test_point_plan_stand_alone_program(tmp_path):
    """tools/point_plan_check.cpp: csrc/point_plan.h as a program of its own (a host program with its own main), once as a
    plain build and once with the address and undefined-behaviour sanitizers.  How this compiler links a sanitized program that
    starts is found with an empty program first; nothing here skips."""
    base = _compiler() + ['-std=c++17', '-O1', '-g']
    plain = str(tmp_path / 'point_plan_check')
    built = subprocess.run(base + [SRC, '-o', plain], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    _check_program(plain)
    empty = tmp_path / 'empty.cpp'
    empty.write_text('int main() { return 0; }\n')
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    flags = None
    for extra in (san + ['-static-libasan', '-static-libubsan'], san):
        exe = str(tmp_path / 'empty')
        if subprocess.run(base + [str(empty), '-o', exe] + extra, capture_output=True).returncode == 0 and \
                subprocess.run([exe], capture_output=True).returncode == 0:
            flags = extra
            break
    assert flags is not None, 'this compiler makes no address/undefined sanitizer build that starts'
    checked = str(tmp_path / 'point_plan_check_san')
    built = subprocess.run(base + [SRC, '-o', checked] + flags, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    _check_program(checked)


def test_point_plan_header_compiles_as_plain_cxx_through_hipcc(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc)
    exe = str(tmp_path / 'by_hipcc')
    built = subprocess.run([hipcc, '-x', 'c++', '-std=c++17', '-O1', SRC, '-o', exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    _check_program(exe)


def test_the_kernels_use_the_header():
    csrc = os.path.join(ROOT, pkg().__name__, 'csrc')
    heads = open(os.path.join(csrc, 'heads.hip')).read()
    assert 'point_plan_side(' in heads and 'point_plan_entry(' in heads
    assert '#include "point_plan.h"' in open(os.path.join(csrc, 'kernels.h')).read()
    assert 'POINT_PLAN_INTS' in open(os.path.join(csrc, 'acrmi_program.hip')).read()      # the size of the picks workspace
    plan = open(os.path.join(csrc, 'point_plan.h')).read()
    assert 'hip' not in plan.split('#pragma once', 1)[1].lower()
    L = pkg('_lib')
    assert 'POINT_MAX_HAND = %d;' % L.MAX_HAND in plan and M.MAX_HAND == L.MAX_HAND


def test_abi_is_additive():
    L = pkg('_lib')
    lib = L.lib()
    header = open(os.path.join(ROOT, 'include', 'acrmi.h')).read()
    assert L.OPT_POINT_HEADS_MULTI == 10 and '#define ACRMI_OPT_POINT_HEADS_MULTI 10' in header
    assert 'acrmi_point_heads_multi' in L.EXPORTS and hasattr(lib, 'acrmi_point_heads_multi')
    fn = lib.acrmi_point_heads_multi
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 4
    assert 'int acrmi_point_heads_multi(acrmi_ctx* ctx, int B, int max_hand, void* stream);' in header
    assert lib.acrmi_version() == L.VERSION == 303 and '#define ACRMI_VERSION 303' in header


def test_bad_arguments_are_rejected_without_a_gpu():
    L = pkg('_lib')
    lib = L.lib()
    assert lib.acrmi_point_heads_multi(None, 1, 2, None) == L.E_INVAL
    assert b'acrmi_point_heads_multi' in lib.acrmi_last_error(None)
    assert lib.acrmi_set_option(None, L.OPT_POINT_HEADS_MULTI, 1) == L.E_INVAL


def test_python_layer_has_the_option_and_refuses_a_non_bool():
    E, main = pkg('engine'), pkg('acr.main')
    assert hasattr(E.Engine, 'set_point_heads_multi')
    assert inspect.signature(E.Engine.run_point_heads).parameters['max_hand'].default == 1
    for fn in (main.ACR.forward_batch, main.ACR.forward_raw_batch, main.ACR._fused_call):
        assert inspect.signature(fn).parameters['multi_point_heads'].default is False, fn
    frames = np.zeros((1, 512, 512, 3), np.uint8)
    for bad in (1, 0, None, 'yes', np.bool_(True)):
        # refused before the frames, the model or the engine are looked at
        with pytest.raises(ValueError, match='multi_point_heads must be True or False'):
            main.ACR._fused_call(None, frames, ['a'], point_heads=True, K=1, multi_point_heads=bad)
        with pytest.raises(ValueError, match='multi_point_heads must be True or False'):
            main.ACR._fused_call(None, frames, ['a'], K=2, multi_point_heads=bad)
        with pytest.raises(ValueError, match='multi_point_heads must be True or False'):
            main._forward_raw_batch(None, None, ['a'], multi_point_heads=bad)
    assert 'hands_per_side' in pkg('config').DEFAULTS and not any('point' in k for k in pkg('config').DEFAULTS)      # no new config key
