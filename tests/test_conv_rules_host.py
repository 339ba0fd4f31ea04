"""csrc/conv_rules.h is the one statement of which convolution kernel takes which layer.  packer.py keeps pure-Python copies
(lower() must work without the library): they are held against the header here, over a grid of shapes printed by the stand-alone
program tools/conv_rules_check.cpp.  The validators of the C ABI read the header directly: the refusals they owe it are checked
through the loaded library.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

TAKES = ('n_tiles', 'wino3', 'wino24b', 'wino24c', 'pp2', 'x3', 'x3p', 'x3s2', 'p1', 'dma')
GRID_POINTS = 2 * 2 * 9 * 7 * 9 * 9


@pytest.fixture(scope='module')
def grid(tmp_path_factory):
    """The check program's lines as dicts: the compiler is found the way tests/test_streams_host.py finds one."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        assert os.path.exists(hipcc), 'no C++ compiler'
        cmd = [hipcc, '-x', 'c++']
    else:
        cmd = [cxx]
    exe = str(tmp_path_factory.mktemp('conv_rules') / 'conv_rules_check')
    subprocess.run(cmd + ['-std=c++17', '-O1', os.path.join(ROOT, 'tools', 'conv_rules_check.cpp'), '-o', exe], check=True, capture_output=True)
    run = subprocess.run([exe], check=True, capture_output=True, text=True)
    points = []
    for line in run.stdout.splitlines():
        shape, takes, ok, floats = (tuple(int(v) for v in part.split()) for part in line.split('|'))
        p = dict(zip(('ks', 'stride', 'cin', 'cout', 'H', 'W'), shape))
        p.update(zip(TAKES, takes))
        p['ok'], p['floats'] = ok, floats
        pad = p['ks'] // 2
        p['ho'], p['wo'] = (p['H'] + 2 * pad - p['ks']) // p['stride'] + 1, (p['W'] + 2 * pad - p['ks']) // p['stride'] + 1
        p['even'] = p['H'] == 2 * p['ho'] and p['W'] == 2 * p['wo']
        points.append(p)
    assert len(points) == GRID_POINTS and all(len(p['ok']) == 8 and len(p['floats']) == 8 for p in points)
    return points


def test_packer_predicates_agree_with_the_header(grid):
    """n_tiles_for, split16_ok, polyphase2_ok, wino24b_width and conv_algo's algo-3 clause at every grid point - odd input sizes
    included: a stride-2 layer on an odd-sized input is taken by none of the stride-2 kernels of the four-wave frame."""
    packer = pkg('packer')
    assert packer.SPLIT16_STRIDE2 and packer.WINOGRAD and packer.WINOGRAD_2D and packer.WINOGRAD_LDS      # (the defaults)
    seen = {k: 0 for k in ('x3', 'x3p', 'x3s2', 'pp2', 'wino24b', 'wino3', 'odd_s2')}
    for p in grid:
        k, s, cin, cout, ho, wo = p['ks'], p['stride'], p['cin'], p['cout'], p['ho'], p['wo']
        assert packer.n_tiles_for(cout) == p['n_tiles'], p
        assert packer.split16_ok(k, s, cin, cout, ho, wo, even_input=p['even']) == bool(p['x3'] or p['x3p'] or p['x3s2']), p
        if k == 3 and s == 2:
            assert packer.polyphase2_ok(cin, cout, ho, wo, even_input=p['even']) == bool(p['pp2']), p
            seen['odd_s2'] += not p['even'] and packer.polyphase2_ok(cin, cout, ho, wo)
        if k == 3 and s == 1:
            assert packer.wino24b_width(cin, cout, ho, wo) == p['wino24b'], p
            assert (packer.conv_algo(k, s, cin, cout, 1, ho, wo) == 3) == bool(p['wino3']), p
        for name in ('x3', 'x3p', 'x3s2', 'pp2', 'wino24b', 'wino3'):
            seen[name] += bool(p[name])
    assert all(seen.values()), seen      # every kernel is taken somewhere on the grid, and the odd stride-2 inputs matter


def test_conv_algo_only_returns_what_the_header_accepts(grid):
    packer = pkg('packer')
    returned = set()
    for p in grid:
        for wino24 in (True, False):
            for split16 in (False, 'fp16', 'bf16'):
                algo = packer.conv_algo(p['ks'], p['stride'], p['cin'], p['cout'], 1, p['ho'], p['wo'], wino24=wino24, split16=split16,
                                        even_input=p['even'])
                assert p['ok'][algo], (p, wino24, split16, algo)
                returned.add(algo)
    assert returned == {0, 2, 3, 4, 5, 6, 7}      # (nothing lowers to algo 1 any more)


def test_packed_weight_sizes_are_conv_weight_floats(grid):
    packer = pkg('packer')
    floats = {}
    for p in grid:
        floats.setdefault((p['ks'], p['cin'], p['cout']), p['floats'])
    rng = np.random.default_rng(0)

    def size(algo, ks, cin, cout):
        w, b = rng.standard_normal((cout, cin, ks, ks)), np.zeros(cout)
        if algo == 3:
            return packer.pack_wino3(w, b)[0].size
        if algo >= 6:
            return packer.pack_conv_x3([(w, b)], packer.DT_BF16 if algo == 7 else packer.DT_F16)[0].size
        tr = {0: lambda t: t, 1: packer.winograd_weights, 2: packer.winograd2d_weights, 4: packer.winograd24_weights,
              5: packer.polyphase2_weights}[algo]
        return packer.pack_conv(tr(w), b)[0].size
    cases = {0: [(1, 34, 33), (3, 8, 16), (3, 96, 40), (1, 128, 128)], 1: [(3, 24, 32), (3, 64, 96)], 2: [(3, 34, 33), (3, 128, 64)],
             3: [(3, 8, 32), (3, 24, 32), (3, 32, 32)], 4: [(3, 34, 40), (3, 64, 64), (3, 32, 128)], 5: [(3, 16, 32), (3, 48, 96)],
             6: [(3, 32, 32), (1, 64, 96), (3, 128, 64)], 7: [(3, 32, 64), (1, 96, 32)]}
    for algo, shapes in cases.items():
        for (ks, cin, cout) in shapes:
            assert size(algo, ks, cin, cout) == floats[(ks, cin, cout)][algo], (algo, ks, cin, cout)


# (algo, ksize, stride, cin, cout, H, W, out_cs, out_coff, res_cs, res_coff, what the message names)
REFUSED = [
    (6, 3, 1, 32, 32, 8, 32, 36, 2, 0, 0, 'out_coff'),            # out_coff % 4
    (5, 3, 2, 32, 32, 16, 32, 32, 0, 36, 2, 'res_coff'),          # res_coff % 4
    (6, 3, 2, 32, 32, 15, 64, 32, 0, 0, 0, 'even input size'),    # odd input height
    (4, 3, 1, 32, 48, 8, 32, 48, 0, 0, 0, 'Cin = 32 with Cout % 32 == 0'),
]


@pytest.mark.parametrize('case', REFUSED, ids=lambda c: 'algo%d_%s' % (c[0], c[-1].split()[0]))
def test_acrmi_conv2d_refuses_up_front_with_the_rule(case):
    """Calls that pass the pointer and range checks but that no kernel takes are refused by the validator (ValueError with the
    rule's sentence), not inside a launcher: host addresses serve as pointers, a refused call never touches them."""
    L = pkg('_lib')
    algo, ks, stride, cin, cout, H, W, out_cs, out_coff, res_cs, res_coff, names = case
    ho, wo = (H + 2 * (ks // 2) - ks) // stride + 1, (W + 2 * (ks // 2) - ks) // stride + 1
    x = np.zeros((1, H, W, cin), np.float32)
    w = np.zeros(1 << 16, np.float32)
    b = np.zeros(128, np.float32)
    out = np.full((1, ho, wo, out_cs), 7.0, np.float32)
    res = np.zeros((1, ho, wo, res_cs), np.float32) if res_cs else None
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    rc = L.lib().acrmi_conv2d(ptr(x), 1, H, W, cin, 0, cin, ptr(w), ptr(b), 0, ptr(res), res_cs, res_coff, ptr(out), out_cs, out_coff,
                              cout, ks, stride, 0, 1, algo, None)
    assert rc == L.E_INVAL
    with pytest.raises(ValueError, match=re.escape(names)) as err:
        L.check(rc)
    assert 'acrmi_conv2d' in str(err.value) and (out == 7.0).all()
