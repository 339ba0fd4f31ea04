"""CPU-side checks of NV12 output (DESIGN.md "NV12 output"): the library's five rows against the literal copy and the formula
of tests/nv12_out_ref.py; the row refusals; every argument refusal of the C ABI and of the Python layer, all of which return
before HIP is touched; the additive ABI; the stand-alone check program of csrc/nv12_out_plan.h, plain and under the address and
undefined-behaviour sanitizers, against the numpy rule; and the compose identity in numpy, next to the plain conversion that
does NOT give the surface back.  None of it needs a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import nv12_out_ref as O
import nv12_ref as N
from conftest import ROOT, pkg

NEW_SYMBOLS = ('acrmi_nv12_out_matrix', 'acrmi_rgb_to_nv12', 'acrmi_nv12_compose')
NAMES = ('cv601', 'bt601', 'bt601-full', 'bt709', 'bt709-full')
CUSTOM_ROW = (250001, 500003, 99991, -150001, -300007, 450011, 440003, -380003, -70001, 9)


def test_the_five_rows_and_the_formula():
    ops, L = pkg('ops'), pkg('_lib')
    assert sorted(O.MATRICES) == sorted(N.MATRICES) == sorted(L.NV12_MATRICES)      # one set of names for both directions
    for name in NAMES:
        assert tuple(ops.nv12_out_matrix(name).tolist()) == O.MATRICES[name], name
        assert O.row_ok(O.MATRICES[name])
    for name in ('bt601', 'bt601-full', 'bt709', 'bt709-full'):
        assert O.formula_row(name) == O.MATRICES[name], name
    row = np.zeros(10, np.int32)
    for which in (-1, 5):
        assert L.lib().acrmi_nv12_out_matrix(which, row.ctypes.data_as(ctypes.c_void_p)) == L.E_INVAL
    assert L.lib().acrmi_nv12_out_matrix(0, None) == L.E_INVAL
    assert tuple(ops.nv12_out_matrix(CUSTOM_ROW).tolist()) == CUSTOM_ROW
    assert tuple(ops.nv12_out_matrix(torch.tensor(CUSTOM_ROW)).tolist()) == CUSTOM_ROW
    six, ten = ops._nv12_matrix_pair('bt709')
    assert tuple(six.tolist()) == N.MATRICES['bt709'] and tuple(ten.tolist()) == O.MATRICES['bt709']
    six, ten = ops._nv12_matrix_pair((N.MATRICES['cv601'], 'bt601-full'))
    assert tuple(six.tolist()) == N.MATRICES['cv601'] and tuple(ten.tolist()) == O.MATRICES['bt601-full']
    for bad in ('bt2020', (1, 2, 3), [1.0] * 10, np.zeros((2, 5), np.int32), [2 ** 31] + [0] * 9):
        with pytest.raises(ValueError):
            ops.nv12_out_matrix(bad)
    for bad in ((1, 2), CUSTOM_ROW, None, ('cv601',)):
        with pytest.raises(ValueError):
            ops._nv12_matrix_pair(bad)


def _surfaces(L, n=1, Hf=8, Wf=8, y=256, uv=512, y_pitch=None, uv_pitch=None):
    su = (L.NV12Surface * n)()
    for i in range(n):
        su[i].y_dev, su[i].uv_dev, su[i].H, su[i].W = y, uv, Hf, Wf
        su[i].y_pitch, su[i].uv_pitch = Wf if y_pitch is None else y_pitch, Wf if uv_pitch is None else uv_pitch
    return su


def _frames(L, n=1, Hf=8, Wf=8, y=1024, uv=2048, pitch=None):
    fr = (L.NV12Frame * n)()
    for i in range(n):
        fr[i].y_dev, fr[i].uv_dev, fr[i].H, fr[i].W = y, uv, Hf, Wf
        fr[i].y_pitch = fr[i].uv_pitch = Wf if pitch is None else pitch
    return fr


def _ptrs(n=1, value=4096):
    return (ctypes.c_void_p * n)(*([value] * n))


LUMA_LIMIT, CHROMA_LIMIT, REFUSED_ROWS, ACCEPTED_ROWS = O.LUMA_LIMIT, O.CHROMA_LIMIT, O.REFUSED_ROWS, O.ACCEPTED_ROWS


def test_overflow_and_y_off_refusals():
    L = pkg('_lib')
    lib = L.lib()
    for row, word in REFUSED_ROWS:
        assert not O.row_ok(row), row
        c = (ctypes.c_int32 * 10)(*row)
        assert lib.acrmi_rgb_to_nv12(_ptrs(), _surfaces(L), 1, c, 1, None) == L.E_INVAL, row
        msg = lib.acrmi_last_error(None)
        assert word.encode() in msg and b'acrmi_rgb_to_nv12' in msg, (row, msg)
        assert lib.acrmi_nv12_compose(_frames(L), _ptrs(), _surfaces(L), 1, None, c, 1, None) == L.E_INVAL, row
        assert word.encode() in lib.acrmi_last_error(None)
    for row in ACCEPTED_ROWS + [O.MATRICES[name] for name in NAMES] + [CUSTOM_ROW]:
        assert O.row_ok(row), row
    # the arithmetic of the limits, as the issue states them
    assert 255 * LUMA_LIMIT + (16 << 20) + 2 ** 19 >= 2 ** 31 > 255 * (LUMA_LIMIT - 1) + (16 << 20) + 2 ** 19
    assert 1020 * CHROMA_LIMIT + (128 << 22) + 2 ** 21 >= 2 ** 31 > 1020 * (CHROMA_LIMIT - 1) + (128 << 22) + 2 ** 21
    # the chroma sums of the full-range rows reach 0.75 of the range
    top = 1020 * sum(abs(v) for v in O.MATRICES['bt601-full'][3:6]) + (128 << 22) + 2 ** 21
    assert 0.74 < top / 2 ** 31 < 0.76


@pytest.mark.skipif(torch.cuda.is_available(), reason='a good call would run on the GPU: the accepted rows are checked where there is none')
def test_accepted_rows_reach_hip():
    """Without a GPU a call that passes every check fails in HIP, not in the checks: the accepted rows get that far."""
    L = pkg('_lib')
    lib = L.lib()
    for row in ACCEPTED_ROWS + [O.MATRICES[name] for name in NAMES]:
        c = (ctypes.c_int32 * 10)(*row)
        assert lib.acrmi_rgb_to_nv12(_ptrs(), _surfaces(L), 1, c, 1, None) == L.E_HIP, row


def test_bad_arguments_are_rejected_without_a_gpu():
    L = pkg('_lib')
    lib = L.lib()

    def plain(src=True, su=True, n=1, coef=None):
        return lib.acrmi_rgb_to_nv12(_ptrs() if src is True else src, _surfaces(L) if su is True else su, n, coef, 1, None)

    def compose(fr=True, drawn=True, su=True, n=1, coef6=None, coef10=None):
        return lib.acrmi_nv12_compose(_frames(L) if fr is True else fr, _ptrs() if drawn is True else drawn,
                                      _surfaces(L) if su is True else su, n, coef6, coef10, 1, None)

    assert plain(src=None) == plain(su=None) == plain(n=0) == plain(n=-1) == L.E_INVAL
    assert compose(fr=None) == compose(drawn=None) == compose(su=None) == compose(n=0) == L.E_INVAL
    assert plain(src=_ptrs(value=None)) == L.E_INVAL and b'null source' in lib.acrmi_last_error(None)
    assert compose(drawn=_ptrs(value=None)) == L.E_INVAL and b'null drawn' in lib.acrmi_last_error(None)
    for kw, word in ((dict(y=None), b'null plane'), (dict(uv=None), b'null plane'), (dict(Hf=0), b'even'), (dict(Hf=7), b'even'),
                     (dict(Wf=6, Hf=3), b'even'), (dict(Wf=9), b'even'), (dict(Wf=0), b'even'), (dict(Hf=-2), b'even'),
                     (dict(y_pitch=7), b'pitch'), (dict(uv_pitch=6), b'pitch')):
        assert plain(su=_surfaces(L, **kw)) == L.E_INVAL, kw
        assert word in lib.acrmi_last_error(None) and b'surface 0' in lib.acrmi_last_error(None), kw
        assert compose(su=_surfaces(L, **kw)) == L.E_INVAL, kw
    # the second surface of two
    su = _surfaces(L, 2)
    su[1].W = 5
    assert plain(src=_ptrs(2), su=su, n=2) == L.E_INVAL and b'surface 1' in lib.acrmi_last_error(None)
    # compose: the source frames as acrmi_nv12_to_rgb checks them, the sizes, both rows
    for kw in (dict(y=None), dict(uv=None), dict(Hf=6, Wf=7), dict(pitch=6)):
        assert compose(fr=_frames(L, **kw)) == L.E_INVAL, kw
        assert b'frame 0' in lib.acrmi_last_error(None)
    assert compose(su=_surfaces(L, Hf=10)) == L.E_INVAL
    assert b'output surface is 10 x 8' in lib.acrmi_last_error(None)
    assert compose(su=_surfaces(L, Wf=10)) == L.E_INVAL
    overflow6 = (ctypes.c_int32 * 6)(-(1 << 24), 0, 0, 0, 0, 16)
    assert compose(coef6=overflow6) == L.E_INVAL and b'overflow' in lib.acrmi_last_error(None)
    bad10 = (ctypes.c_int32 * 10)(*REFUSED_ROWS[2][0])
    assert compose(coef10=bad10) == L.E_INVAL and b'luma' in lib.acrmi_last_error(None)
    assert plain(coef=bad10) == L.E_INVAL


def test_abi_is_additive():
    L = pkg('_lib')
    src = open(os.path.join(ROOT, 'include', 'acrmi.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    lib = L.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, src), '%s is not declared' % name
        assert name in L.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is ctypes.c_int
    assert [len(getattr(lib, name).argtypes) for name in NEW_SYMBOLS] == [2, 6, 8]
    declared = sorted(set(re.findall(r'\b(acrmi_[a-z0-9_]+)\s*\(', src)))
    assert sorted(L.EXPORTS) == declared
    assert re.search(r'typedef struct acrmi_nv12_surface\s*\{', src)
    assert ctypes.sizeof(L.NV12Surface) == ctypes.sizeof(L.NV12Frame) == 32
    assert lib.acrmi_version() == L.VERSION == 303
    kernels = open(os.path.join(ROOT, pkg().__name__, 'csrc', 'kernels.h')).read()
    assert 'NV12 output kernel arguments must fit the 4 KB argument block' in kernels
    assert 'nv12_out.hip' in pkg('build').SOURCES


def test_python_layer_refuses_bad_arguments_without_a_gpu():
    ops = pkg('ops')
    u8 = torch.uint8
    frames = torch.zeros(2, 4, 6, 3, dtype=u8)
    for bad in (torch.zeros(2, 3, 6, 3, dtype=u8), [torch.zeros(4, 5, 3, dtype=u8)], torch.zeros(1, 0, 4, 3, dtype=u8)):
        with pytest.raises(ValueError, match='even'):
            ops.bgr_to_nv12(bad)
    with pytest.raises(ValueError, match='uint8'):
        ops.bgr_to_nv12(torch.zeros(2, 4, 6, 3))
    with pytest.raises(ValueError, match='unknown NV12 matrix'):
        ops.bgr_to_nv12(frames, matrix='bt2020')
    with pytest.raises(ValueError, match='ten int32'):
        ops.bgr_to_nv12(frames, matrix=(1, 2, 3, 4, 5, 6))
    with pytest.raises(ValueError, match='out='):
        ops.bgr_to_nv12(frames, out=torch.zeros(2, 9, 6, dtype=u8))
    with pytest.raises(ValueError, match='out='):
        ops.bgr_to_nv12(frames, out=[torch.zeros(6, 6, dtype=u8)])
    with pytest.raises(ValueError, match='dense'):
        ops.bgr_to_nv12(frames, out=torch.zeros(2, 6, 12, dtype=u8)[:, :, ::2])
    surfaces = torch.zeros(2, 6, 6, dtype=u8)
    with pytest.raises(ValueError, match='drawn frames are'):
        ops.nv12_compose(surfaces, torch.zeros(2, 4, 8, 3, dtype=u8))
    with pytest.raises(ValueError, match='drawn frames are'):
        ops.nv12_compose(surfaces, frames[:1])
    with pytest.raises(ValueError, match='name or a pair'):
        ops.nv12_compose(surfaces, frames, matrix=CUSTOM_ROW)
    with pytest.raises(ValueError, match='out='):
        ops.nv12_compose(surfaces, frames, out=torch.zeros(2, 6, 8, dtype=u8))
    with pytest.raises(ValueError, match='even'):
        ops.nv12_compose(torch.zeros(6, 5, dtype=u8), torch.zeros(1, 4, 5, 3, dtype=u8))
    # forward_raw_batch: the keyword is looked at before anything else is
    forward = pkg('acr.main').ACR.forward_raw_batch
    with pytest.raises(ValueError, match='render_format'):
        forward(None, frames, ['a', 'b'], render=True, render_format='i420')
    with pytest.raises(ValueError, match='needs render=True'):
        forward(None, frames, ['a', 'b'], render_format='nv12')
    with pytest.raises(ValueError, match='even'):
        forward(None, torch.zeros(2, 5, 6, 3, dtype=u8), ['a', 'b'], render=True, render_format='nv12')
    with pytest.raises(ValueError, match='even'):
        forward(None, [frames[0], torch.zeros(4, 7, 3, dtype=u8)], ['a', 'b'], render=True, render_format='nv12')
    with pytest.raises(ValueError, match='name or a pair'):
        forward(None, surfaces, ['a', 'b'], render=True, render_format='nv12', pixel_format='nv12', matrix=N.MATRICES['bt601'])


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_no_cpu_fallback():
    ops, L = pkg('ops'), pkg('_lib')
    with pytest.raises(L.AcrmiError):
        ops.bgr_to_nv12(torch.zeros(1, 4, 6, 3, dtype=torch.uint8))
    with pytest.raises(L.AcrmiError):
        ops.nv12_compose(torch.zeros(1, 6, 6, dtype=torch.uint8), torch.zeros(1, 4, 6, 3, dtype=torch.uint8))


# ---- the stand-alone check program ---------------------------------------------------------------------------------
def _compiler():
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        assert os.path.exists(hipcc), 'no C++ compiler'
        return [hipcc, '-x', 'c++']
    return [cxx]


def _seeded_blocks():
    """[(row, rgb [4,3])]: all-0, all-255 and the pure primaries (which hit the clamps of the full-range rows) for every named row
    and the custom one, then seeded random blocks."""
    g = np.random.default_rng(20261019)
    rows = [O.MATRICES[name] for name in NAMES] + [CUSTOM_ROW]
    fixed = [np.zeros((4, 3), np.uint8), np.full((4, 3), 255, np.uint8)]
    for c in range(3):
        p = np.zeros((4, 3), np.uint8)
        p[:, c] = 255
        fixed.append(p)
        fixed.append(255 - p)
    blocks = [(row, b) for row in rows for b in fixed]
    for i in range(600):
        blocks.append((rows[i % len(rows)], g.integers(0, 256, (4, 3), dtype=np.uint8)))
    return blocks


def _ref_block(row, rgb):
    y, uv = O.to_nv12(rgb.reshape(2, 2, 3), row, bgr=False)
    return tuple(int(v) for v in y.reshape(-1)) + tuple(int(v) for v in uv.reshape(-1))


def _seeded_compose_blocks():
    """[(row6 name, row10, drawn [4,3], shown [4,3], src y [4], U, V)]: the shown triples are the input rule's; the drawn ones
    are those with no, one, some or all pixels changed."""
    g = np.random.default_rng(20261020)
    cases = []
    for i in range(400):
        name = NAMES[i % 5]
        y = g.integers(0, 256, 4, dtype=np.uint8)
        U, V = (int(v) for v in g.integers(0, 256, 2))
        R, G, B = N.yuv_to_rgb(y, np.full(4, U), np.full(4, V), name)
        shown = np.stack([R, G, B], -1)
        drawn = shown.copy()
        kind = i % 4
        mask = [np.zeros(4, bool), np.eye(4, dtype=bool)[(i // 4) % 4], g.random(4) < 0.5, np.ones(4, bool)][kind]
        drawn[mask] = g.integers(0, 256, (int(mask.sum()), 3), dtype=np.uint8)
        cases.append((name, O.MATRICES[NAMES[(i // 5) % 5]], drawn, shown, y, U, V))
    return cases


def _ref_compose_block(name, row10, drawn, shown, y, U, V):
    out_y, out_uv = O.compose(y.reshape(2, 2), np.array([[U, V]], np.uint8), drawn.reshape(2, 2, 3), name, row10, bgr=False)
    return tuple(int(v) for v in out_y.reshape(-1)) + tuple(int(v) for v in out_uv.reshape(-1))


def _words(line):
    w = line.split()
    assert len(w) == 8 and w[0] == 'y' and w[5] == 'uv', line
    return tuple(int(v) for v in w[1:5] + w[6:8])


def _check_program(exe):
    blocks = _seeded_blocks()
    text = ''.join('%s %s\n' % (' '.join(str(c) for c in row), ' '.join(str(v) for v in rgb.reshape(-1))) for row, rgb in blocks)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().split('\n')
    assert len(lines) == len(blocks)
    clamped = set()
    for line, (row, rgb) in zip(lines, blocks):
        got = _words(line)
        assert got == _ref_block(row, rgb), (row, rgb.tolist(), got)
        clamped |= {v for v in got if v in (0, 255)}
    assert clamped == {0, 255}      # both clamps were met
    cases = _seeded_compose_blocks()
    text = ''.join('%s %s %s %s %d %d\n' % (' '.join(str(c) for c in row10), ' '.join(str(v) for v in drawn.reshape(-1)),
                                            ' '.join(str(v) for v in shown.reshape(-1)), ' '.join(str(v) for v in y), U, V)
                   for _, row10, drawn, shown, y, U, V in cases)
    run = subprocess.run([exe, 'compose'], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().split('\n')
    assert len(lines) == len(cases)
    kept = 0
    for line, case in zip(lines, cases):
        got = _words(line)
        assert got == _ref_compose_block(*case), (case, got)
        kept += got == tuple(int(v) for v in case[4]) + (case[5], case[6])
    assert kept >= 100      # the unchanged blocks keep their source bytes
    run = subprocess.run([exe, 'rows'], capture_output=True, text=True)
    assert run.returncode == 0
    assert [tuple(int(v) for v in line.split()[1:]) for line in run.stdout.strip().split('\n')] == [O.MATRICES[name] for name in NAMES]
    rows = [row for row, _ in REFUSED_ROWS] + ACCEPTED_ROWS
    run = subprocess.run([exe, 'check'], input=''.join(' '.join(str(c) for c in row) + '\n' for row in rows), capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    verdicts = run.stdout.strip().split('\n')
    assert [v == 'ok' for v in verdicts] == [O.row_ok(row) for row in rows]
    for (_, word), verdict in zip(REFUSED_ROWS, verdicts):
        assert verdict.startswith('refused') and word in verdict
    good = ' '.join(str(c) for c in O.MATRICES['cv601'])
    for bad in (good + ' 1 2 3\n', good + ' 0' * 11 + ' 256\n', good + ' 0' * 11 + ' -1\n', good + ' 0' * 11 + ' x\n',
                ' '.join(str(c) for c in REFUSED_ROWS[2][0]) + ' 0' * 12 + '\n'):
        assert subprocess.run([exe], input=bad, capture_output=True, text=True).returncode == 2, bad
    assert subprocess.run([exe, 'compose'], input=good + ' 0' * 12 + '\n', capture_output=True, text=True).returncode == 2
    assert subprocess.run([exe, 'check'], input='1 2 3\n', capture_output=True, text=True).returncode == 2
    assert subprocess.run([exe, 'other'], input='', capture_output=True, text=True).returncode == 2


def test_nv12_out_stand_alone_program(tmp_path):
    """tools/nv12_out_check.cpp: csrc/nv12_out_plan.h as a program of its own (a host program with its own main), once as a
    plain build and once with the address and undefined-behaviour sanitizers.  How this compiler links a sanitized program
    that starts is found with an empty program first; nothing here skips."""
    base = _compiler() + ['-std=c++17', '-O1', '-g', '-ffp-contract=off']
    src = os.path.join(ROOT, 'tools', 'nv12_out_check.cpp')
    plain = str(tmp_path / 'nv12_out_check')
    built = subprocess.run(base + [src, '-o', plain], capture_output=True, text=True)
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
    checked = str(tmp_path / 'nv12_out_check_san')
    built = subprocess.run(base + [src, '-o', checked] + flags, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    _check_program(checked)


def test_nv12_out_header_compiles_alone_with_hipcc(tmp_path):
    """As plain C++ the host / device macro of csrc/nv12_out_plan.h expands to nothing: hipcc -x c++ builds the same program."""
    src = os.path.join(ROOT, 'tools', 'nv12_out_check.cpp')
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc)
    exe = str(tmp_path / 'by_hipcc')
    built = subprocess.run([hipcc, '-x', 'c++', '-std=c++17', '-O1', src, '-o', exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    line = ' '.join(str(c) for c in O.MATRICES['bt709-full']) + ' 255 0 0 255 0 0 255 0 0 255 0 0\n'
    run = subprocess.run([exe], input=line, capture_output=True, text=True)
    assert run.stdout == 'y 54 54 54 54 uv 99 255\n'
    assert _ref_block(O.MATRICES['bt709-full'], np.array([[255, 0, 0]] * 4, np.uint8)) == (54, 54, 54, 54, 99, 255)


# ---- compose in numpy: the identity, and what tells it from a conversion ----------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_compose_is_the_identity_where_conversion_is_not(name):
    for H, W, seed in ((2, 2, 1), (6, 10, 2), (34, 70, 3)):
        y, uv = N.random_nv12(H, W, seed)
        bgr = N.nv12_to_bgr(y, uv, name)
        out_y, out_uv = O.compose(y, uv, bgr, name, name)
        assert np.array_equal(out_y, y) and np.array_equal(out_uv, uv)
        again_y, again_uv = O.to_nv12(bgr, name)
        if H * W >= 60:      # random bytes: out-of-gamut samples clamp, so the round trip loses them
            assert not np.array_equal(again_y, y) and not np.array_equal(again_uv, uv)
        # RGB order is the same rule on the other channel order
        out_y, out_uv = O.compose(y, uv, bgr[:, :, ::-1], name, name, bgr=False)
        assert np.array_equal(out_y, y) and np.array_equal(out_uv, uv)


def test_one_drawn_pixel_changes_one_luma_byte_and_one_chroma_pair():
    y, uv = N.random_nv12(8, 12, 5)
    drawn = N.nv12_to_bgr(y, uv)
    drawn[3, 7] ^= 255
    out_y, out_uv = O.compose(y, uv, drawn)
    dy, duv = out_y != y, (out_uv != uv).reshape(4, 6, 2).any(-1)
    assert dy.sum() <= 1 and not dy[np.arange(8) != 3][:, :].any() and not dy[:, np.arange(12) != 7].any()
    duv[1, 3] = False
    assert not duv.any()
    want_y, want_uv = O.to_nv12(drawn)
    assert out_y[3, 7] == want_y[3, 7] and np.array_equal(out_uv[1, 6:8], want_uv[1, 6:8])
