"""GPU tests of NV12 output (rgb_to_nv12_kernel and nv12_compose_kernel of csrc/nv12_out.hip; DESIGN.md "NV12 output") against
the numpy statement of the rule in tests/nv12_out_ref.py.  Everything is integer, so everything is compared byte for byte.
The wide path of the kernels takes frames whose width is a multiple of 8 and whose planes and pitches are 8-byte aligned; the
sizes below hold both kinds, and the alignment tests push the same picture through both paths."""
import numpy as np
import pytest
import torch

import nv12_out_ref as O
import nv12_ref as N
from conftest import pkg

pytestmark = pytest.mark.gpu

# the narrowest frame; widths below, at and above the wide path's step of 8 that are not its multiples (4x6, 6x10, 34x70: a
# ragged last block column against that step); multiples of it (16x24, 64x48)
SIZES = [(2, 2), (2, 4), (4, 6), (6, 10), (16, 24), (34, 70), (64, 48)]
NAMES = ('cv601', 'bt601', 'bt601-full', 'bt709', 'bt709-full')
CUSTOM_ROW = (250001, 500003, 99991, -150001, -300007, 450011, 440003, -380003, -70001, 9)
CUSTOM_ROW6 = (1200000, 2000003, -400001, -800003, 1600001, 7)
_cache = {}


def _picture(H, W, seed=None):
    """Seeded random bytes [H,W,3]: every primary and both clamps of the full-range rows occur at these sizes."""
    key = ('pic', H, W, seed)
    if key not in _cache:
        _cache[key] = np.random.default_rng(7000 * H + W if seed is None else seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    return _cache[key]


def _want(H, W, row, bgr, seed=None):
    """The numpy surface [H*3/2, W] of the seeded picture, computed once and shared."""
    key = ('nv12', H, W, row, bgr, seed)
    if key not in _cache:
        _cache[key] = O.surface(*O.to_nv12(_picture(H, W, seed), row, bgr))
    return _cache[key]


def _source(H, W, seed=None):
    key = ('src', H, W, seed)
    if key not in _cache:
        _cache[key] = N.random_nv12(H, W, 3000 * H + W if seed is None else seed)
    return _cache[key]


@pytest.mark.parametrize('matrix', NAMES + (CUSTOM_ROW,))
@pytest.mark.parametrize('bgr', (True, False))
def test_plain_conversion_equals_the_rule(matrix, bgr):
    ops = pkg('ops')
    frames = [torch.from_numpy(_picture(H, W)).cuda() for H, W in SIZES]
    got = ops.bgr_to_nv12(frames, matrix=matrix, bgr=bgr)      # mixed sizes in one call: a list in input order
    assert isinstance(got, list) and [tuple(g.shape) for g in got] == [(H * 3 // 2, W) for H, W in SIZES]
    for g, (H, W) in zip(got, SIZES):
        assert np.array_equal(g.cpu().numpy(), _want(H, W, matrix, bgr)), (H, W)
    one = ops.bgr_to_nv12(torch.stack([frames[4], frames[4]]), matrix=matrix, bgr=bgr)      # a tensor in, a tensor out
    assert tuple(one.shape) == (2, 24, 24) and torch.equal(one[0], got[4]) and torch.equal(one[1], got[4])


def test_extreme_bytes():
    """All-0, all-255, the primaries and their complements in 2x2 blocks, and single extreme pixels in blocks of the other
    extreme: the clamps of every row, on the wide path (W = 16) and on the byte path (W = 12)."""
    ops = pkg('ops')
    colours = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 255, 255), (255, 0, 255), (255, 255, 0)]
    for W in (16, 12):
        pic = np.zeros((8, W, 3), np.uint8)
        for i in range(4):
            for j in range(W // 2):
                pic[2 * i:2 * i + 2, 2 * j:2 * j + 2] = colours[(i * (W // 2) + j) % 8]
        pic[5, 3], pic[6, 9], pic[7, W - 1] = (255, 255, 255), (0, 0, 0), (0, 0, 255)
        dev = torch.from_numpy(pic).cuda()[None]
        hit = set()
        for name in NAMES:
            for bgr in (True, False):
                got = ops.bgr_to_nv12(dev, matrix=name, bgr=bgr)[0].cpu().numpy()
                assert np.array_equal(got, O.surface(*O.to_nv12(pic, name, bgr))), (W, name, bgr)
                hit |= {int(got.min()), int(got.max())}
        assert hit >= {0, 255}


def test_more_frames_than_one_launch_holds():
    ops = pkg('ops')
    g = np.random.default_rng(65)
    pics = g.integers(0, 256, (65, 4, 8, 3), dtype=np.uint8)
    got = ops.bgr_to_nv12(torch.from_numpy(pics).cuda()).cpu().numpy()
    assert got.shape == (65, 6, 8)
    for i in (0, 1, 57, 58, 63, 64):
        assert np.array_equal(got[i], O.surface(*O.to_nv12(pics[i]))), i
    assert len({got[i].tobytes() for i in range(65)}) == 65
    # compose splits at 58 frames: the identity and one drawn pixel a frame, in place
    src = np.stack([O.surface(*N.random_nv12(4, 8, 900 + i)) for i in range(65)])
    surf = torch.from_numpy(src).cuda()
    drawn = ops.nv12_to_bgr(surf)
    assert torch.equal(ops.nv12_compose(surf, drawn), surf)
    drawn[:, 1, 5] ^= 255
    host = drawn.cpu().numpy()
    out = ops.nv12_compose(surf, drawn, out=surf)
    assert out is surf
    for i in (0, 57, 58, 64):
        assert np.array_equal(surf[i].cpu().numpy(), O.surface(*O.compose(src[i][:4], src[i][4:], host[i]))), i



@pytest.mark.parametrize('row', O.ACCEPTED_ROWS)
def test_rows_next_to_the_limits_are_taken_and_follow_the_rule(row):
    """The nearest rows the host's check must take (one below the smallest magnitude each inequality refuses), through the C ABI
    on a real 2x2 surface and a 4x8 one (the wide path): accepted, and byte for byte the numpy rule, whose int32 range is
    asserted.  The refused neighbours raise before anything runs."""
    ops = pkg('ops')
    for H, W in ((2, 2), (4, 8)):
        pic = _picture(H, W)
        pic = np.where(np.arange(W)[None, :, None] % 2 == 0, pic, np.uint8(255)).astype(np.uint8)      # the largest sums occur
        got = ops.bgr_to_nv12(torch.from_numpy(pic).cuda()[None], matrix=row)[0].cpu().numpy()
        assert np.array_equal(got, O.surface(*O.to_nv12(pic, row))), (H, W)
    src = torch.from_numpy(O.surface(*_source(2, 2))).cuda()
    out = ops.nv12_compose([src], ops.nv12_to_bgr([src]), matrix=('cv601', row))
    assert torch.equal(out[0], src)
    for bad, word in O.REFUSED_ROWS:
        with pytest.raises(ValueError, match=word):
            ops.bgr_to_nv12(torch.from_numpy(_picture(2, 2)).cuda()[None], matrix=bad)


def _sentinel_surface(H, W, pitch, shift, fill):
    """A surface view [H*3/2, W] with row pitch `pitch` that starts `shift` bytes into the second row of a buffer full of
    `fill` -> (buffer, view)."""
    rows = H * 3 // 2
    buf = torch.full(((rows + 2) * pitch,), fill, dtype=torch.uint8, device='cuda')
    view = torch.as_strided(buf, (rows, W), (pitch, 1), pitch + shift)
    return buf, view


def _outside_is(buf, H, W, pitch, shift, fill):
    mask = torch.ones_like(buf, dtype=torch.bool)
    torch.as_strided(mask, (H * 3 // 2, W), (pitch, 1), pitch + shift)[:] = False
    return bool((buf[mask] == fill).all())


@pytest.mark.parametrize('H,W,pitch', [(16, 24, 32), (34, 70, 80), (64, 48, 64), (2, 2, 8)])
def test_pitch_alignment_and_both_paths(H, W, pitch):
    """Pitched output views with sentinel bytes between W and the pitch and in the rows around the surface: nothing outside
    the W bytes of a row is written.  The same picture aligned (the wide path where W allows it) and one byte off alignment
    (the byte path), inputs and outputs: the same bytes."""
    ops = pkg('ops')
    pic = _picture(H, W)
    want = torch.from_numpy(_want(H, W, 'bt709', True)).cuda()
    flat = torch.zeros(H * W * 3 + 16, dtype=torch.uint8, device='cuda')
    results = []
    for shift in (0, 1, 8):
        src = flat[shift:shift + H * W * 3].view(H, W, 3)
        src.copy_(torch.from_numpy(pic))
        assert src.data_ptr() % 8 == (shift % 8)
        buf, view = _sentinel_surface(H, W, pitch, shift, 0xA5)
        got = ops.bgr_to_nv12([src], matrix='bt709', out=[view])
        assert got[0] is view
        assert torch.equal(view, want), shift
        assert _outside_is(buf, H, W, pitch, shift, 0xA5), shift
        results.append(view.clone())
        # separate planes, each with its own pitch and alignment
        ybuf = torch.full((H + 2, pitch + 8), 0x5A, dtype=torch.uint8, device='cuda')
        uvbuf = torch.full((H // 2 + 2, pitch + 16), 0x5A, dtype=torch.uint8, device='cuda')
        y, uv = ybuf[1:H + 1, shift:shift + W], uvbuf[1:H // 2 + 1, shift:shift + W]
        ops.bgr_to_nv12([src], matrix='bt709', out=[(y, uv)])
        assert torch.equal(y, want[:H]) and torch.equal(uv, want[H:])
        y[:], uv[:] = 0x5A, 0x5A
        assert bool((ybuf == 0x5A).all()) and bool((uvbuf == 0x5A).all())
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[2])


@pytest.mark.parametrize('H,W', SIZES)
def test_compose_identity(H, W):
    """compose(S, nv12_to_bgr(S)) == S on random bytes, into a separate surface and in place, aligned and one byte off, for
    every named row and a custom pair, in both channel orders; the plain conversion of the same frame is NOT S."""
    ops = pkg('ops')
    y, uv = _source(H, W)
    src = O.surface(y, uv)
    surf = torch.from_numpy(src).cuda()
    for matrix in NAMES + ((CUSTOM_ROW6, CUSTOM_ROW),):
        six = matrix if isinstance(matrix, str) else matrix[0]
        for rgb in (False, True):
            drawn = ops.nv12_to_bgr([surf], six, rgb=rgb)
            assert np.array_equal(drawn[0].cpu().numpy(), N.nv12_to_bgr(y, uv, six)[:, :, ::-1 if rgb else 1])
            out = ops.nv12_compose([surf], drawn, matrix=matrix, bgr=not rgb)
            assert out.data_ptr() != surf.data_ptr() and tuple(out.shape) == (1, H * 3 // 2, W)
            assert torch.equal(out[0], surf), (matrix, rgb)
    drawn = ops.nv12_to_bgr([surf])
    if H * W >= 60:
        assert not torch.equal(ops.bgr_to_nv12(drawn)[0], surf)      # the conversion clamps and rounds twice
    # in place, on an aligned surface and on one sliced one byte off alignment from a larger buffer
    for shift in (0, 1):
        pitch = W + 8
        buf, view = _sentinel_surface(H, W, pitch, shift, 0x33)
        view.copy_(surf)
        got = ops.nv12_compose([view], drawn, out=[view])
        assert got[0] is view and torch.equal(view, surf)
        assert _outside_is(buf, H, W, pitch, shift, 0x33)


@pytest.mark.parametrize('H,W', SIZES)
@pytest.mark.parametrize('bgr', (True, False))
def test_compose_with_sparse_changes(H, W, bgr):
    ops = pkg('ops')
    y, uv = _source(H, W)
    surf = torch.from_numpy(O.surface(y, uv)).cuda()
    shown = N.nv12_to_bgr(y, uv, 'bt601')
    if not bgr:
        shown = shown[:, :, ::-1]
    drawn = np.ascontiguousarray(shown).copy()
    g = np.random.default_rng(H * 131 + W)
    changed = {(0, 0), (H - 1, W - 1), (H - 2, 0), (H - 1, 1)}      # the corners; two pixels of one block
    for _ in range(min(6, H * W // 8)):
        changed.add((int(g.integers(0, H)), int(g.integers(0, W))))
    for r, c in sorted(changed):
        drawn[r, c] = drawn[r, c] ^ np.uint8(1 << int(g.integers(0, 8)))      # differs for certain
    want_y, want_uv = O.compose(y, uv, drawn, 'bt601', 'bt601', bgr)
    dev = torch.from_numpy(drawn).cuda()[None]
    for shift in (0, 1):      # the wide path where W allows it, and the byte path
        buf, view = _sentinel_surface(H, W, W + 8, shift, 0)
        got = ops.nv12_compose([surf], dev, matrix='bt601', bgr=bgr, out=[view])[0].cpu().numpy()
        assert np.array_equal(got[:H], want_y) and np.array_equal(got[H:], want_uv), shift
    # every other Y byte and UV pair is the source's
    mask = np.zeros((H, W), bool)
    for r, c in changed:
        mask[r, c] = True
    assert np.array_equal(got[:H][~mask], y[~mask])
    blocks = mask[0::2, 0::2] | mask[0::2, 1::2] | mask[1::2, 0::2] | mask[1::2, 1::2]
    assert np.array_equal(got[H:].reshape(H // 2, W // 2, 2)[~blocks], uv.reshape(H // 2, W // 2, 2)[~blocks])
    new_y, _ = O.to_nv12(drawn, 'bt601', bgr)
    assert np.array_equal(got[:H][mask], new_y[mask])
    # in place gives the same surface
    inplace = surf.clone()
    ops.nv12_compose([inplace], dev, matrix='bt601', bgr=bgr, out=[inplace])
    assert np.array_equal(inplace.cpu().numpy(), got)


def test_mixed_sizes_and_layouts_compose():
    """Surfaces of different sizes in one call, as one tensor each and as (y, uv) tuples: a list in input order."""
    ops = pkg('ops')
    sizes = [(6, 10), (16, 24), (2, 2)]
    planes = [_source(H, W) for H, W in sizes]
    surfaces = [torch.from_numpy(O.surface(*planes[0])).cuda(),
                (torch.from_numpy(planes[1][0]).cuda(), torch.from_numpy(planes[1][1]).cuda().view(8, 12, 2)),
                torch.from_numpy(O.surface(*planes[2])).cuda()]
    drawn = ops.nv12_to_bgr(surfaces)
    drawn[1][5, 7] ^= 128
    host = [d.cpu().numpy() for d in drawn]
    got = ops.nv12_compose(surfaces, drawn)
    assert isinstance(got, list) and [tuple(g.shape) for g in got] == [(9, 10), (24, 24), (3, 2)]
    for g, (y, uv), d in zip(got, planes, host):
        assert np.array_equal(g.cpu().numpy(), O.surface(*O.compose(y, uv, d)))
    assert not np.array_equal(got[1].cpu().numpy(), O.surface(*planes[1]))


# ---- end to end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def near_sd():
    return pkg('synth').make_state_dict(seed=10)      # the checkpoint of tests/test_gpu_render.py: it detects both hands


def _same_results(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert len(a[k]) == len(b[k])
        for h1, h2 in zip(a[k], b[k]):
            assert sorted(h1) == sorted(h2) and all(np.array_equal(h1[f], h2[f]) for f in h1)


def test_end_to_end_views_as_nv12(near_sd, mano_tables):
    cfg, ops = pkg('config'), pkg('ops')
    acr = pkg('acr.main').ACR(args_set=cfg.parse_args(['--configs_yml', '/nonexistent.yml', '--renderer', 'hip']),
                              state_dict=near_sd, mano_tables=mano_tables, max_batch=3)
    nv12 = [torch.from_numpy(O.surface(*N.random_nv12(96, 160, s))).cuda() for s in (11, 12)]
    keep = [s.clone() for s in nv12]
    paths = ['a', 'b']
    items = ('mesh', 'pj2d', 'centermap', 'org_img')
    res_bgr, views_bgr = acr.forward_raw_batch(nv12, paths, pixel_format='nv12', render=True, show_items=items)
    res, views = acr.forward_raw_batch(nv12, paths, pixel_format='nv12', render=True, show_items=items, render_format='nv12')
    _same_results(res, res_bgr)
    assert sorted(views) == sorted(items)
    assert all(torch.equal(a, b) for a, b in zip(nv12, keep))      # the sources are not written
    assert views['org_img'] is nv12
    assert tuple(views_bgr['mesh'].shape) == (2, 96, 160, 3) and tuple(views['mesh'].shape) == (2, 144, 160)
    src = torch.stack(nv12)
    differs = 0
    for name in ('mesh', 'pj2d'):
        assert torch.equal(views[name], ops.nv12_compose(nv12, views_bgr[name])), name
        differs += _only_drawn_blocks_differ(views[name], src, views_bgr[name], views_bgr['org_img'])
    assert tuple(views_bgr['centermap'].shape) == (2, 2, 96, 160, 3) and tuple(views['centermap'].shape) == (2, 2, 144, 160)
    for side in (0, 1):
        assert torch.equal(views['centermap'][side], ops.nv12_compose(nv12, views_bgr['centermap'][side]))
        differs += _only_drawn_blocks_differ(views['centermap'][side], src, views_bgr['centermap'][side], views_bgr['org_img'])
    assert differs >= 1, 'nothing was drawn: the comparison shows nothing'
    # render=True alone: the meshes
    res2, mesh = acr.forward_raw_batch(nv12, paths, pixel_format='nv12', render=True, render_format='nv12')
    _same_results(res2, res_bgr)
    assert torch.equal(mesh, views['mesh'])
    # a list of frames of different sizes comes back as a list in input order
    mixed = [nv12[0], torch.from_numpy(O.surface(*N.random_nv12(64, 96, 13))).cuda(), nv12[1]]
    paths3 = ['a', 'b', 'c']
    _, mixed_bgr = acr.forward_raw_batch(mixed, paths3, pixel_format='nv12', render=True, show_items=('pj2d', 'centermap'))
    _, mixed_nv12 = acr.forward_raw_batch(mixed, paths3, pixel_format='nv12', render=True, show_items=('pj2d', 'centermap'),
                                          render_format='nv12')
    assert isinstance(mixed_nv12['pj2d'], list) and [tuple(v.shape) for v in mixed_nv12['pj2d']] == [(144, 160), (96, 96), (144, 160)]
    want = ops.nv12_compose(mixed, mixed_bgr['pj2d'])
    assert all(torch.equal(a, b) for a, b in zip(mixed_nv12['pj2d'], want))
    assert [tuple(v.shape) for v in mixed_nv12['centermap']] == [(2, 144, 160), (2, 96, 96), (2, 144, 160)]
    for side in (0, 1):
        want = ops.nv12_compose(mixed, [v[side] for v in mixed_bgr['centermap']])
        assert all(torch.equal(v[side], w) for v, w in zip(mixed_nv12['centermap'], want))
    # regions: the skeletons of all regions of a frame over that frame
    boxes, box_frame = [(20.5, 10.2, 120.7, 90.0), (-5, -5, 101, 61), (31, 7, 160, 96)], [1, 0, 1]
    kw = dict(boxes=boxes, box_frame=box_frame, pixel_format='nv12', render=True, show_items=('pj2d', 'org_img'))
    res_r_bgr, reg_bgr = acr.forward_raw_batch(nv12, paths3, **kw)
    res_r, reg = acr.forward_raw_batch(nv12, paths3, render_format='nv12', **kw)
    _same_results(res_r, res_r_bgr)
    assert reg['org_img'] is nv12 and torch.equal(reg['pj2d'], ops.nv12_compose(nv12, reg_bgr['pj2d']))
    assert not torch.equal(reg['pj2d'], src)
    with pytest.raises(ValueError, match='over regions is not implemented'):
        acr.forward_raw_batch(nv12, paths3, boxes=boxes, box_frame=box_frame, pixel_format='nv12', render=True, render_format='nv12')
    # BGR input: the views through the plain conversion
    bgr = ops.nv12_to_bgr(nv12)
    res_b, views_b = acr.forward_raw_batch(bgr, paths, render=True, show_items=items)
    res_n, views_n = acr.forward_raw_batch(bgr, paths, render=True, show_items=items, render_format='nv12')
    _same_results(res_b, res_bgr)
    _same_results(res_n, res_bgr)
    for name in ('mesh', 'pj2d', 'org_img'):
        assert torch.equal(views_n[name], ops.bgr_to_nv12(views_b[name])), name
    for side in (0, 1):
        assert torch.equal(views_n['centermap'][side], ops.bgr_to_nv12(views_b['centermap'][side]))
    with pytest.raises(ValueError, match='even'):
        acr.forward_raw_batch(bgr[:, :95].contiguous(), paths, render=True, render_format='nv12')
    # the calls without the keyword return what they return today: the BGR views of the NV12 call are those of the BGR call
    for name in ('mesh', 'pj2d', 'centermap', 'org_img'):
        assert torch.equal(views_b[name], views_bgr[name]), name
    res_d, drawn_default = acr.forward_raw_batch(nv12, paths, pixel_format='nv12', render=True, render_format='bgr')
    assert torch.equal(drawn_default, views_bgr['mesh'])
    _same_results(res_d, res_bgr)
    _same_results(acr.forward_raw_batch(nv12, paths, pixel_format='nv12'), res_bgr)


def _only_drawn_blocks_differ(view, src, drawn_bgr, org_bgr):
    """view, src [n,H*3/2,W]; the bytes of a view outside the blocks of its drawn pixels are the source's -> whether the view
    differs from its source at all."""
    n, rows, W = view.shape
    H = rows * 2 // 3
    changed = (drawn_bgr != org_bgr).any(-1)                                       # [n,H,W]
    blocks = changed.view(n, H // 2, 2, W // 2, 2).any(4).any(2)                     # [n,H/2,W/2]
    assert torch.equal(view[:, :H][~changed], src[:, :H][~changed])
    uv_v, uv_s = view[:, H:].reshape(n, H // 2, W // 2, 2), src[:, H:].reshape(n, H // 2, W // 2, 2)
    assert torch.equal(uv_v[~blocks], uv_s[~blocks])
    return int(not torch.equal(view, src))
