"""Host-side checks of the key-point skeleton and heat-map views (DESIGN.md "Key-point and heat-map views"): the constant
tables against what the reference yields, the numpy restatement (tests/overlay_ref.py) against PIL and against torch's
bilinear form, the colour table, and the argument checks of the new entry points.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import overlay_ref as R
from conftest import golden, pkg


def _dilate(m, r):
    o = np.zeros_like(m)
    H, W = m.shape
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            o[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] |= m[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
    return o


def test_tables_equal_the_recorded_reference_ones():
    """Parent list, colours and mapper recorded from the reference's load_skeleton / get_keypoint_rgb / Visualizer
    (tests/golden/make_golden_overlay.py) = the product's tables (Python and C) = the restatement's."""
    g = golden('overlay_pil.npz')
    ops = pkg('ops')
    for parents, mapper, colors in ((ops.SKELETON_PARENTS, ops.MANO2INTERHAND, ops.SKELETON_COLORS_RGB),
                                    (R.PARENTS, R.MAPPER, R.COLORS_RGB)):
        assert list(parents) == g['parents'].tolist()
        assert list(mapper) == g['mapper'].tolist()
        assert np.array_equal(np.array(colors, np.uint8), g['colors'])
    rgb, _ = ops.overlay_tables()
    bgr, _ = ops.overlay_tables(bgr=True)
    assert np.array_equal(rgb, g['colors']) and np.array_equal(bgr, g['colors'][:, ::-1])
    assert np.array_equal(R.default_colors(True), bgr)
    # the tree as the rule words it: five fingers of four joints, tip to base, each base on the wrist
    assert all(R.PARENTS[i] == (20 if i % 4 == 3 else i + 1) for i in range(20)) and R.PARENTS[20] == -1


def test_restatement_against_pil():
    """The restatement (not the kernel) next to PIL's own drawing of the recorded cases: a sanity bound, PIL builds its wide
    lines as polygons.  Measured on the eight committed cases (two hands on 128 x 128):
      mask difference / PIL's pixels   0.033 0.036 0.023 0.009 0.031 0.023 0.028 0.035   -> worst 0.0357, bound 0.0357 * 1.25
      colour difference / common       0.0051 0.0012 0.0007 0.0015 0.0025 0.0061 0.0047 0.0043 -> worst 0.0061, bound * 1.25
      pixels more than two pixels outside the other mask: 0 in every case, both ways    -> bound 0
    (on 300 random two-hand skeletons at 256 x 256 the same rule measured 11 % / 2.6 % on average, 20 % worst, 9 of 1.4 M
    pixels beyond two pixels: longer bones, where the polygon and the distance rule part more often)."""
    g = golden('overlay_pil.npz')
    worst_mask = worst_col = 0.0
    for c in range(len(g['kps'])):
        bg, pil = g['images'][c], g['drawn'][c]
        mine = R.draw_skeletons(g['kps'][c], bg[None], hand_frame=[0, 0])[0]
        # the window each primitive is evaluated on changes nothing
        assert np.array_equal(mine, R.draw_skeletons(g['kps'][c], bg[None], hand_frame=[0, 0], windowed=False)[0])
        mp, mm = (pil != bg).any(-1), (mine != bg).any(-1)
        both = mp & mm
        d_mask = (mp ^ mm).sum() / mp.sum()
        d_col = ((pil != mine).any(-1) & both).sum() / both.sum()
        far = int((mm & ~_dilate(mp, 2)).sum()), int((mp & ~_dilate(mm, 2)).sum())
        print('case %d: PIL %d px, restatement %d px, mask diff %.4f, colour diff %.4f, beyond two pixels %s'
              % (c, mp.sum(), mm.sum(), d_mask, d_col, far))
        worst_mask, worst_col = max(worst_mask, d_mask), max(worst_col, d_col)
        assert far == (0, 0)
        assert np.array_equal(mine[~mm], bg[~mm])
    assert worst_mask <= 0.0357 * 1.25 and worst_col <= 0.0061 * 1.25, (worst_mask, worst_col)


def test_restatement_drops_what_the_rule_drops():
    bg = np.full((1, 64, 64, 3), 7, np.uint8)
    kp = R.random_hands(1, 64, 64, seed=3)
    bad = kp.copy()
    bad[0, 5, 1] = np.nan
    assert np.array_equal(R.draw_skeletons(bad, bg), bg)                 # non-finite: the hand is not drawn
    bad[0, 5, 1] = np.inf
    assert np.array_equal(R.draw_skeletons(bad, bg), bg)
    farp = kp.copy()
    farp[0, 8] = (20000.0, 10.0)                                         # MANO joint 8 = skeleton joint 4 (index tip)
    prims = R.primitives(farp[0])
    assert len(prims) == 61 - 2 and all(p[-1] != 4 for p in prims)       # its bone and its disc; nothing else
    same = np.zeros((1, 21, 2), np.float32) + 30.5                       # coincident joints: discs only
    prims = R.primitives(same[0])
    assert len(prims) == 41 and all(p[0] == 'disc' for p in prims)
    drawn = R.draw_skeletons(same, bg)[0]
    assert int((drawn != 7).any(-1).sum()) == 37                         # the blob PIL's ellipse((k-3, k-3, k+3, k+3)) fills
    assert np.array_equal(R.draw_skeletons(kp, bg, hand_frame=[-1]), bg)
    assert len(R.primitives(kp[0])) == 61


@pytest.mark.parametrize('size', [(512, 512), (480, 640), (333, 517), (1080, 1920)])
def test_heatmap_restatement_against_torch(size):
    """The colour-table index of the fp32 rule next to torch's interpolate(mode='bilinear') + .mul(255).clamp(0, 255).byte()
    (make_heatmaps, acr/visualization.py:280-285) on Gaussian-peak maps: the index may differ on at most 1e-5 of the pixels,
    and by at most 1 (torch maps the pixel to the map in one multiplication, the rule in two: through the 512 canvas)."""
    H, W = size
    n = 8
    maps = R.gaussian_maps(n, 64, 64, seed=H + W, peaks=3)
    want = torch.nn.functional.interpolate(torch.from_numpy(maps)[None], size=(H, W), mode='bilinear')[0]
    want = want.mul(255).clamp(0, 255).byte().numpy()
    diff = 0
    for i in range(n):
        idx, inside = R.heatmap_index(maps[i], H, W)
        assert inside.all()
        d = np.abs(idx.astype(np.int32) - want[i].astype(np.int32))
        assert d.max() <= 1
        diff += int((d != 0).sum())
    print('%d x %d: index differs on %d of %d pixels' % (H, W, diff, n * H * W))
    assert diff <= 1e-5 * n * H * W


def test_lut_properties():
    ops = pkg('ops')
    _, lut = ops.overlay_tables()
    _, lut_bgr = ops.overlay_tables(bgr=True)
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert np.array_equal(lut, R.jet_lut()) and np.array_equal(lut, R.jet_lut_formula())      # integer form = stated formula
    assert np.array_equal(lut_bgr, lut[:, ::-1]) and np.array_equal(lut_bgr, R.jet_lut(bgr=True))
    # end points: dark blue -> dark red (1.5 - 1 = 0.5 -> 128)
    assert lut[0].tolist() == [0, 0, 128] and lut[255].tolist() == [128, 0, 0]
    r, g, b = (lut[:, c].astype(np.int32) for c in range(3))
    # monotone pieces: each channel rises to its plateau of 255 and falls again, centred on t = 3/4, 1/2, 1/4
    for ch, k in ((r, 3), (g, 2), (b, 1)):
        peak = 255 * k / 4.0
        up, down = np.arange(256) <= peak, np.arange(256) >= peak
        assert (np.diff(ch[up]) >= 0).all() and (np.diff(ch[down]) <= 0).all()
        assert ch.max() == 255 and set(np.abs(np.diff(ch)).tolist()) <= {0, 1, 2, 3, 4}
    assert (g[:32] == 0).all() and (r[:96] == 0).all() and (b[160:] == 0).all() and (b[-1], r[-1]) == (0, 128)
    assert lut[128].tolist() == [130, 255, 126]


def test_null_arguments_are_rejected_without_a_gpu():
    L = pkg('_lib')
    lib = L.lib()
    p = ctypes.c_void_p(256)
    assert lib.acrmi_draw_skeletons(None, None, 2, None, 0, 3, 3, None, None, 1, 8, 8, None) == L.E_INVAL
    assert lib.acrmi_draw_skeletons(p, p, 2, None, 0, 3, 3, p, None, 1, 8, 8, None) == L.E_INVAL
    assert lib.acrmi_draw_skeletons(p, p, 0, None, 0, 3, 3, p, p, 1, 8, 8, None) == L.E_INVAL          # no hands
    assert lib.acrmi_draw_skeletons(p, p, 2, None, 0, 0, 3, p, p, 1, 8, 8, None) == L.E_INVAL          # width 0
    assert lib.acrmi_draw_skeletons(p, p, 2, None, 0, 12, 3, p, p, 1, 8, 8, None) == L.E_INVAL         # width beyond the int64 bound
    assert lib.acrmi_draw_skeletons(p, p, 2, None, 0, 3, -1, p, p, 1, 8, 8, None) == L.E_INVAL
    assert lib.acrmi_draw_skeletons(p, p, 2, None, 0, 3, 3, p, p, 1, 8, 20000, None) == L.E_INVAL
    assert lib.acrmi_draw_heatmaps(None, None, 16, 1, 4, 4, None, 0.7, None, 0, None, None, None, 8, 8, None) == L.E_INVAL
    assert lib.acrmi_draw_heatmaps(p, p, 16, 1, 4, 4, None, 0.7, None, 0, p, p, None, 8, 8, None) == L.E_INVAL     # right map, no right output
    assert lib.acrmi_draw_heatmaps(p, None, 16, 1, 4, 4, None, 1.5, None, 0, p, p, None, 8, 8, None) == L.E_INVAL   # weight
    assert lib.acrmi_draw_heatmaps(p, None, 8, 1, 4, 4, None, 0.7, None, 0, p, p, None, 8, 8, None) == L.E_INVAL    # stride < h * w
    assert lib.acrmi_draw_heatmaps(p, None, 16, 1, 4, 4, None, 0.7, None, 0, p, p, None, 0, 8, None) == L.E_INVAL
    assert lib.acrmi_overlay(None, L.OVERLAY_SKELETON, p, p, 1, None, 0, p, p, None, 8, 8, None) == L.E_INVAL
    assert lib.acrmi_overlay(None, L.OVERLAY_CENTERMAP, None, None, 1, None, 0, None, None, None, 8, 8, None) == L.E_INVAL
    assert lib.acrmi_overlay_tables(0, None, None) == 0


def test_python_wrappers_check_their_arguments():
    ops, L = pkg('ops'), pkg('_lib')
    img = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    kps = torch.zeros(2, 21, 2)
    with pytest.raises(ValueError):
        ops.draw_skeletons(kps, img.float())                       # dtype
    with pytest.raises(ValueError):
        ops.draw_skeletons(kps, img[0])                            # shape
    with pytest.raises(ValueError):
        ops.draw_skeletons(kps[:, :20], img)
    with pytest.raises(ValueError):
        ops.draw_skeletons(kps.double(), img)
    with pytest.raises(ValueError):
        ops.draw_heatmaps(torch.zeros(1, 3, 8, 8), img)            # [N,2,h,w] or [N,h,w]
    with pytest.raises(ValueError):
        ops.draw_heatmaps(torch.zeros(2, 8, 8), img)               # one row per image
    with pytest.raises(ValueError):
        ops.draw_heatmaps(torch.zeros(1, 8, 8, dtype=torch.int32), img)
    with pytest.raises(ValueError):
        ops.draw_heatmaps(torch.zeros(1, 8, 8), img.float())
    # host tensors: there is no CPU path
    with pytest.raises(L.AcrmiError):
        ops.draw_skeletons(kps, img)
    with pytest.raises(L.AcrmiError):
        ops.draw_heatmaps(torch.zeros(1, 8, 8), img)
    # ACR: unknown view names are refused before anything runs
    main = pkg('acr.main')
    with pytest.raises(ValueError):
        main.check_show_items(['mesh', 'j3d'])
    assert main.check_show_items(None) is None and main.check_show_items(('pj2d', 'centermap')) == ['pj2d', 'centermap']
