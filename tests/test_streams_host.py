"""Host-side checks of per-stream smoothing (engine.StreamTable, acrmi_streams_* / acrmi_smooth_streams /
acrmi_forward_streams): the ABI surface, the argument checks that need no device, the Python argument checks against a stub
table, and the launch planner (csrc/smooth_plan.h) through its stand-alone check program.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg

NEW = ('acrmi_streams_create', 'acrmi_streams_destroy', 'acrmi_streams_reset', 'acrmi_smooth_streams', 'acrmi_forward_streams')


def test_new_symbols_are_declared_exported_and_bound():
    L = pkg('_lib')
    lib = L.lib()
    header = open(os.path.join(ROOT, 'include', 'acrmi.h')).read()
    for name in NEW:
        assert name + '(' in header and name in L.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.acrmi_smooth_streams.argtypes) == 6
    assert len(lib.acrmi_forward_streams.argtypes) == len(lib.acrmi_forward.argtypes) + 2
    assert lib.acrmi_streams_destroy.restype is None
    assert lib.acrmi_version() == L.VERSION == 303      # additive: the ABI version stays


def test_bad_arguments_are_rejected_before_any_device_call():
    """Without a device only the NULL-context branch of acrmi_smooth_streams / acrmi_forward_streams can be reached (an error
    is stored in the context); NULL table / ids / slots with a live context: tests/test_gpu_streams.py."""
    L = pkg('_lib')
    lib = L.lib()
    p = ctypes.c_void_p(256)
    ids = (ctypes.c_int32 * 2)(0, 1)
    for table, slots, idp in ((None, p, ids), (p, None, ids), (p, p, None), (None, None, None)):
        assert lib.acrmi_smooth_streams(None, table, slots, 2, idp, None) == L.E_INVAL
    assert lib.acrmi_forward_streams(None, None, None, None, 2, None, None, None, None, None, None, None, None) == L.E_INVAL
    assert lib.acrmi_streams_reset(None, None, 0, None) == L.E_INVAL
    assert lib.acrmi_streams_reset(None, ids, 2, None) == L.E_INVAL
    lib.acrmi_streams_destroy(None)                       # like free(NULL)
    h = ctypes.c_void_p()
    assert lib.acrmi_streams_create(None, 0, 4) == L.E_INVAL
    for cap in (0, -1, 65537, 1 << 30):                   # the capacity is checked before the device is looked at
        assert lib.acrmi_streams_create(ctypes.byref(h), 0, cap) == L.E_INVAL and not h.value
        assert b'capacity' in lib.acrmi_last_error(None)
    if not torch.cuda.is_available():                     # a loud failure, no host-side table
        assert lib.acrmi_streams_create(ctypes.byref(h), 0, 4) == L.E_HIP and not h.value
        with pytest.raises(L.AcrmiError):
            pkg('engine').StreamTable(0, 4)
    with pytest.raises(ValueError):
        pkg('engine').StreamTable(0, 0)
    with pytest.raises(ValueError):
        pkg('engine').StreamTable(0, 65537)


class StubTable(object):
    """What the argument checks look at of a StreamTable."""
    def __init__(self, capacity=4, handle=1):
        self.capacity, self.handle = capacity, handle


def test_stream_ids_conversion():
    E = pkg('engine')
    for given in ([0, 1, -1], (0, 1, -1), np.array([0, 1, -1], np.int64), np.array([0, 1, 255], np.uint8)[:3],
                  torch.tensor([0, 1, -1]), torch.tensor([0, 1, -1], dtype=torch.int16), range(3)):
        a = E.stream_ids(given, 3)
        assert a.dtype == np.int32 and a.flags['C_CONTIGUOUS'] and a.shape == (3,)
        assert a.tolist()[:2] == [0, 1]
    assert E.stream_ids(np.arange(8)[::2], 4).tolist() == [0, 2, 4, 6]       # a strided view is packed
    for bad in ([0, 1], [0, 1, 2, 3], [[0, 1, 2]], 5, np.zeros((3, 1), np.int32), torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(ValueError):
            E.stream_ids(bad, 3)                             # wrong length / shape
    for bad in ([0.0, 1.0, 2.0], np.zeros(3, np.float32), torch.zeros(3), [True, False, True], ['0', '1', '2'],
                torch.zeros(3, dtype=torch.bool)):
        with pytest.raises(ValueError):
            E.stream_ids(bad, 3)                             # wrong dtype
    with pytest.raises(ValueError):
        E.stream_ids([0, 1, 2 ** 31], 3)                     # would wrap in 32 bits


def test_streams_and_table_go_together():
    E = pkg('engine')
    tbl = StubTable()
    assert E.stream_args(None, None, 3) is None
    assert E.stream_args([0, 1, 2], tbl, 3).tolist() == [0, 1, 2]
    with pytest.raises(ValueError):
        E.stream_args([0, 1, 2], None, 3)
    with pytest.raises(ValueError):
        E.stream_args(None, tbl, 3)
    with pytest.raises(ValueError):
        E.stream_args([0, 1, 2], StubTable(handle=None), 3)      # closed
    with pytest.raises(ValueError):
        E.stream_args([0, 1, 2], object(), 3)                    # not a table
    with pytest.raises(ValueError):
        E.stream_args([0, 1], tbl, 3)


def test_sharded_runner_says_what_is_missing():
    doc = pkg('parallel').ShardedRunner.forward_global.__doc__
    assert 'StreamTable' in doc and 'not built' in doc and 'not combined' in doc


def test_launch_planner_stand_alone_program(tmp_path):
    """tools/smooth_plan_check.cpp: csrc/smooth_plan.h (id validation, grouping by stream, splitting into launches) against a
    plain restatement, as a program of its own.  The plain build must pass; the build with the address and
    undefined-behaviour sanitizers must pass as well where the host compiler can make one that starts - which of the two
    ran is printed and asserted, never left open."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        assert os.path.exists(hipcc), 'no C++ compiler'
        cmd = [hipcc, '-x', 'c++']
    else:
        cmd = [cxx]
    src = os.path.join(ROOT, 'tools', 'smooth_plan_check.cpp')
    cmd += ['-std=c++17', '-O1', '-g', src, '-o']
    plain = str(tmp_path / 'smooth_plan_check')
    subprocess.run(cmd + [plain], check=True, capture_output=True)
    run = subprocess.run([plain], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
    # the runtimes linked into the program first: a shared sanitizer runtime only starts when it is first in the process's
    # library list
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    ran = None
    for label, extra in (('static', san + ['-static-libasan', '-static-libubsan']), ('shared', san)):
        exe = str(tmp_path / ('smooth_plan_check_' + label))
        if subprocess.run(cmd + [exe] + extra, capture_output=True).returncode != 0:
            continue
        run = subprocess.run([exe], capture_output=True, text=True)
        if 'does not come first in initial library list' in run.stderr:
            continue
        ran = label
        assert run.returncode == 0 and run.stdout.strip().endswith('ok'), run.stdout + run.stderr
        break
    print('sanitizer variant that ran: %s' % ran)
    if ran is None:
        pytest.skip('no address/undefined sanitizer build of the check program starts with this compiler; the plain build passed')
