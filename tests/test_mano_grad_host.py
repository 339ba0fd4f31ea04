"""The MANO gradient without a GPU: the float64 statement (tests/mano_grad_ref.py) against the oracle and against the
reference's own gradients (tests/golden/mano_grad.npz) - which yields the yardstick of the GPU tests' bar -, the export, the
argument rules that need no device, and csrc/mano_grad_plan.h as a stand-alone program."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mano_grad_cases as cases
import mano_grad_ref as ref
from conftest import ROOT, golden, pkg
from oracle import mano as omano


@pytest.mark.parametrize('name', cases.BASE)
def test_statement_forward_matches_oracle(mano_tables, name):
    """Within 2e-5 m, the bar tests/test_oracle_pinned.py holds oracle and reference to."""
    side, cidx, kind, seed, opt = cases.CASES[name]
    x = cases.inputs(name)
    with torch.no_grad():
        v, j, c = ref.mano(ref.as_tables(mano_tables[side]), side, torch.tensor(x['coeffs'], dtype=torch.float64),
                           torch.tensor(x['betas'], dtype=torch.float64), cidx)
    ov, oj, oc = omano.mano_forward(mano_tables[side], side, x['coeffs'], x['betas'], cidx)
    assert np.abs(v.numpy() - ov).max() < 2e-5 and np.abs(j.numpy() - oj).max() < 2e-5
    assert (c is None) == (oc is None) and (c is None or np.abs(c.numpy() - oc).max() < 2e-5)


def test_cases_hold_what_they_promise():
    assert {(v[0], v[1]) for v in cases.CASES.values() if not v[4]} == {(s, c) for s in ('left', 'right') for c in (None, 9, 0, 12)}
    assert {v[2] for v in cases.CASES.values()} == {'verts', 'joints', 'both'}
    for name in cases.CASES:
        x = cases.inputs(name)
        assert x['coeffs'].shape[0] == cases.N == 5 and not x['coeffs'][0].any()
        assert 3.0 <= np.linalg.norm(x['coeffs'][1, :3]) <= 5.0 and np.abs(x['betas'][2]).max() > 2.0
    assert (cases.inputs('left_trans')['trans'] != 0).all()


def test_yardstick_reference_gradients_against_float64(mano_tables):
    """The error of the reference's own float32 gradients against the float64 statement, max|g - g64| / max|g64| per row: the
    yardstick.  A wrong restatement shows as 1e-2 or more."""
    fx = golden('mano_grad.npz')
    y, g64 = ref.yardstick(mano_tables, fx)
    rows = 0
    for name in cases.CASES:
        for k in ('g_pose', 'g_betas', 'g_trans'):
            if name + '_' + k in fx.files:
                e = ref.row_errors(fx[name + '_' + k], g64[name][k])
                rows += k == 'g_pose' and len(e)
                print('%-12s %-8s %s' % (name, k, ' '.join('%.1e' % v for v in e)))
                assert e.max() < 1e-5
    assert sorted(fx.files) == sorted(n + '_' + k for n in cases.CASES for k in g64[n])      # gradients only
    print('yardstick %.3g over %d rows; the kernel bar is 8 x = %.3g' % (y, rows, 8 * y))
    assert y < 1e-5


def test_export_version_and_prototype():
    L = pkg('_lib')
    assert L.lib().acrmi_version() == L.VERSION == 303
    assert 'acrmi_mano_backward' in L.EXPORTS
    fn = L.lib().acrmi_mano_backward
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 14
    src = open(os.path.join(ROOT, 'include', 'acrmi.h')).read()
    proto = re.search(r'int acrmi_mano_backward\(([^;]*)\);', src)
    assert proto and len(proto.group(1).split(',')) == 14
    for arg in ('pose_stride', 'beta_stride', 'center_idx', 'g_verts', 'g_joints', 'g_center', 'g_poses', 'g_betas', 'stream'):
        assert arg in proto.group(1)
    # the C entry refuses bad arguments before it touches a device
    z = ctypes.c_void_p(0)
    assert fn(None, z, 48, z, 10, z, 1, 9, z, z, z, z, z, z) == L.E_INVAL


def test_argument_rules_without_a_device():
    check = pkg('engine').Engine.check_mano_backward
    p, b, s = torch.zeros(3, 48), torch.zeros(3, 10), torch.zeros(3, dtype=torch.int32)
    check(p, b, s, 9, None, None, None)
    check(torch.zeros(3, 176)[:, 6:54], b, s, None, torch.zeros(3, 778, 3), torch.zeros(3, 21, 3), torch.zeros(3, 1, 3))
    for bad in ((torch.zeros(3, 47), b, s, 9, None, None, None), (torch.zeros(48), b, s, 9, None, None, None),
                (p, torch.zeros(2, 10), s, 9, None, None, None), (p, torch.zeros(3, 9), s, 9, None, None, None),
                (p, b, s[:2], 9, None, None, None), (p, b, s, 21, None, None, None), (p, b, s, -1, None, None, None),
                (p, b, s, 9, torch.zeros(3, 778), None, None), (p, b, s, 9, None, torch.zeros(2, 21, 3), None),
                (p, b, s, 9, None, None, torch.zeros(3, 2))):
        with pytest.raises(ValueError):
            check(*bad)


def test_manolayer_gradient_arguments_without_a_device(mano_tables):
    M = pkg('mano.manolayer')
    layer = M.ManoLayer(tables=mano_tables['right'], use_pca=False, side='right')
    with pytest.raises(ValueError, match='th_pose_coeffs'):
        layer(torch.zeros(2, 40).requires_grad_())
    with pytest.raises(ValueError, match='th_betas'):
        layer(torch.zeros(2, 48).requires_grad_(), torch.zeros(3, 10))
    pca = M.ManoLayer(tables=mano_tables['left'], use_pca=True, ncomps=6, side='left')
    with pytest.raises(ValueError, match='th_pose_coeffs'):
        pca(torch.zeros(2, 8), torch.zeros(2, 10).requires_grad_())


def test_plan_stand_alone_program(tmp_path):
    """tools/mano_grad_check.cpp: every backward of csrc/mano_grad_plan.h against central differences of its forward, in double,
    as a program of its own.  The plain build must pass; the build with the address and undefined-behaviour sanitizers must
    pass as well where the host compiler can make one that starts - which of the two ran is printed."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        assert os.path.exists(hipcc), 'no C++ compiler'
        cmd = [hipcc, '-x', 'c++']
    else:
        cmd = [cxx]
    src = os.path.join(ROOT, 'tools', 'mano_grad_check.cpp')
    cmd += ['-std=c++17', '-O1', '-g', '-ffp-contract=off', src, '-o']
    plain = str(tmp_path / 'mano_grad_check')
    subprocess.run(cmd + [plain], check=True, capture_output=True)
    run = subprocess.run([plain], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    ran = None
    for label, extra in (('static', san + ['-static-libasan', '-static-libubsan']), ('shared', san)):
        exe = str(tmp_path / ('mano_grad_check_' + label))
        if subprocess.run(cmd + [exe] + extra, capture_output=True).returncode != 0:
            continue
        run = subprocess.run([exe], capture_output=True, text=True)
        if 'does not come first in initial library list' in run.stderr:
            continue
        ran = label
        assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
        break
    print('sanitizer variant that ran: %s' % ran)
