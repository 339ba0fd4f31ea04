"""CPU-side checks of the shared paths under acr.main's batched entry points: the per-size helper that every list of frames
of different sizes goes through, the one fused call (the engine options in force at Engine.forward, its keywords, and the
options afterwards), the views assembler and the render-argument check.  Fakes stand for the engine and the drawing
operators: nothing here needs a GPU."""
import itertools
from types import SimpleNamespace

import pytest
import torch

from conftest import pkg

A, B_ = (4, 6, 3), (2, 8, 3)      # two frame sizes [H,W,3]
DEFAULTS = dict(point_heads=False, temporal=False, semantics='frame', point_heads_multi=False)


def _frames_aba():
    """Frames of sizes A, B_, A; frame i is filled with i + 1."""
    return [torch.full(shape, i + 1, dtype=torch.uint8) for i, shape in enumerate((A, B_, A))]


# ---- the per-size helper -------------------------------------------------------------------------------------------------

def test_per_size_passes_a_tensor_through():
    main = pkg('acr.main')
    frames, calls, result = torch.zeros((3,) + A, dtype=torch.uint8), [], object()

    def draw(imgs, idx, place):
        calls.append((imgs, idx, place))
        return result

    assert main._per_size(frames, draw, count=7) is result      # the count is the engine's to check for a tensor
    assert len(calls) == 1 and calls[0][0] is frames and calls[0][1] is None and calls[0][2] is None


def test_per_size_groups_a_list_by_size_and_restores_input_order():
    main = pkg('acr.main')
    frames, calls = _frames_aba(), []

    def draw(imgs, idx, place):
        calls.append((tuple(imgs.shape), list(idx), place.tolist()))
        return imgs + 10

    got = main._per_size(frames, draw, count=3)
    assert calls == [((2,) + A, [0, 2], [0, -1, 1]), ((1,) + B_, [1], [-1, 0, -1])]
    assert isinstance(got, list) and len(got) == 3
    for i, (g, f) in enumerate(zip(got, frames)):
        assert g.shape == f.shape and torch.equal(g, f + 10), i
    assert main._per_size(tuple(frames), draw)[1].shape == B_      # a tuple is a list, and no count is no check


def test_per_size_with_the_leading_pair_axis():
    main = pkg('acr.main')
    frames = _frames_aba()
    got = main._per_size(frames, lambda imgs, idx, place: torch.stack([imgs + 10, imgs + 20]), count=3, pair=True)
    assert len(got) == 3
    for i, (g, f) in enumerate(zip(got, frames)):
        assert g.shape == (2,) + tuple(f.shape) and torch.equal(g[0], f + 10) and torch.equal(g[1], f + 20), i


def test_per_size_refuses_a_list_of_another_length():
    main = pkg('acr.main')

    def draw(imgs, idx, place):
        raise AssertionError('nothing is drawn')

    with pytest.raises(ValueError, match='^one frame to draw into per input frame$'):
        main._per_size(_frames_aba(), draw, count=2)
    # the sites that have a count hand it over
    out = {'slots': torch.zeros(2, 2, 176)}
    for call in (lambda: main.ACR._render_batch(SimpleNamespace(focal_length=1.), None, out, _frames_aba(), None, True),
                 lambda: main.ACR._overlay_batch(None, None, out, _frames_aba(), 'centermap', None, True)):
        with pytest.raises(ValueError, match='^one frame to draw into per input frame$'):
            call()


def test_draw_over_frames_keeps_an_undrawn_hand_undrawn(monkeypatch):
    main, ops = pkg('acr.main'), pkg('ops')
    calls = []

    def draw_skeletons(kps, imgs, hand_frame=None, bgr=False):
        calls.append((kps, tuple(imgs.shape), hand_frame, bgr))
        return imgs + 10

    monkeypatch.setattr(ops, 'draw_skeletons', draw_skeletons)
    kps, hand_frame = torch.zeros(5, 21, 2), torch.tensor([0, -1, 2, 1, -1])
    frames = _frames_aba()
    got = main._draw_over_frames(kps, frames, hand_frame)
    assert [c[1] for c in calls] == [(2,) + A, (1,) + B_]
    assert all(c[0] is kps and c[3] is True and c[2].dtype == torch.int32 for c in calls)
    assert calls[0][2].tolist() == [0, -1, 1, -1, -1]      # frame 2 is frame 1 of its group; -1 does not become the last frame
    assert calls[1][2].tolist() == [-1, -1, -1, 0, -1]
    assert all(torch.equal(g, f + 10) for g, f in zip(got, frames))
    del calls[:]
    stacked = torch.zeros((3,) + A, dtype=torch.uint8)
    assert torch.equal(main._draw_over_frames(kps, stacked, hand_frame), stacked + 10)
    assert len(calls) == 1 and calls[0][2].dtype == torch.int32 and calls[0][2].tolist() == hand_frame.tolist()


# ---- the fused call ------------------------------------------------------------------------------------------------------

class Sentinel(Exception):
    pass


class FakeEngine(object):
    """Records the option setters; `forward` notes the options in force and its arguments, and raises Sentinel."""

    def __init__(self):
        self.opts, self.coeff, self.seen = dict(DEFAULTS), 'unset', None

    def set_point_heads(self, on):
        self.opts['point_heads'] = on

    def set_temporal(self, on, smooth_coeff=None):
        self.opts['temporal'] = on
        if smooth_coeff is not None:
            self.coeff = smooth_coeff

    def set_batch_semantics(self, mode):
        self.opts['semantics'] = mode

    def set_point_heads_multi(self, on):
        self.opts['point_heads_multi'] = on

    def forward(self, img, **kw):
        self.seen = (dict(self.opts), img, kw)
        raise Sentinel()


def _fake_self(temporal, parser_semantics='frame'):
    eng = FakeEngine()
    asked = []

    def tracks_for(K, max_streams, gate, max_miss):
        asked.append((K, max_streams, gate, max_miss))
        return 'the track table'

    fake = SimpleNamespace(model=SimpleNamespace(engine=lambda B: eng, _result_parser=SimpleNamespace(batch_semantics=parser_semantics)),
                           temporal_optimization=temporal, _args=SimpleNamespace(smooth_coeff=3.0), hands_per_side=1,
                           focal_length=1265., stream_table=None, track_table=None, _device=0,
                           _streams_for=lambda streams, max_streams, B: ('ids of %r' % (streams,), 'the stream table'),
                           _tracks_for=tracks_for)
    return fake, eng, asked


FRAMES = torch.zeros(2, 512, 512, 3, dtype=torch.uint8)
OFFSETS = torch.zeros(2, 10)


def _call(fake, **kw):
    with pytest.raises(Sentinel):
        pkg('acr.main').ACR._fused_call(fake, FRAMES, ['a', 'b'], offsets=OFFSETS, **kw)


@pytest.mark.parametrize('point_heads, temporal, streams, multi_point_heads, semantics',
                         [c for c in itertools.product((True, False), (True, False), (None, [0, 1]), (True, False),
                                                       (None, 'reference')) if c[1] or c[2] is None])
def test_fused_call_one_hand_per_side(point_heads, temporal, streams, multi_point_heads, semantics):
    fake, eng, _ = _fake_self(temporal)
    _call(fake, point_heads=point_heads, streams=streams, batch_semantics=semantics, multi_point_heads=multi_point_heads)
    opts, img, kw = eng.seen
    assert opts == dict(point_heads=point_heads, temporal=temporal and streams is None, semantics=semantics or 'frame',
                        point_heads_multi=False)
    ids, table = (None, None) if streams is None else ('ids of [0, 1]', 'the stream table')
    assert img is FRAMES and eng.coeff == 3.0 and set(kw) == {'offsets', 'project', 'streams', 'table'}
    assert kw['offsets'] is OFFSETS and kw['project'] is True and kw['streams'] == ids and kw['table'] == table
    assert eng.opts == DEFAULTS


def test_fused_call_takes_the_parsers_semantics_and_the_whole_frame_rows():
    main = pkg('acr.main')
    fake, eng, _ = _fake_self(False, parser_semantics='reference')
    with pytest.raises(Sentinel):
        main.ACR._fused_call(fake, FRAMES, ['a', 'b'])
    opts, _, kw = eng.seen
    assert opts == dict(point_heads=True, temporal=False, semantics='reference', point_heads_multi=False)
    whole = torch.tensor([[512., 512, 0, 0, 0, 0, 0, 0, 0, 0]]).repeat(2, 1)
    assert torch.equal(kw['offsets'], whole) and torch.equal(main._whole_frame_offsets(2), whole)
    assert eng.opts == DEFAULTS


@pytest.mark.parametrize('point_heads, multi_point_heads', list(itertools.product((True, False), (True, False))))
def test_fused_call_several_hands_per_side(point_heads, multi_point_heads):
    fake, eng, _ = _fake_self(False)
    _call(fake, point_heads=point_heads, K=2, multi_point_heads=multi_point_heads)
    opts, img, kw = eng.seen
    assert opts == dict(point_heads=False, temporal=False, semantics='frame', point_heads_multi=multi_point_heads)
    assert img is FRAMES and eng.coeff == 'unset' and set(kw) == {'offsets', 'project', 'max_hand'}
    assert kw['offsets'] is OFFSETS and kw['project'] is True and kw['max_hand'] == 2
    assert eng.opts == DEFAULTS


@pytest.mark.parametrize('K, point_heads, temporal, multi_point_heads',
                         list(itertools.product((1, 2), (True, False), (True, False), (True, False))))
def test_fused_call_with_tracks(K, point_heads, temporal, multi_point_heads):
    fake, eng, asked = _fake_self(temporal)
    tracks = [0, 1]
    _call(fake, point_heads=point_heads, K=K, tracks=tracks, max_streams=7, track_gate=5, track_max_miss=3,
          multi_point_heads=multi_point_heads)
    opts, img, kw = eng.seen
    # the dense heads also at K = 1, and ACRMI_OPT_TEMPORAL off: the tracks are smoothed through `smooth`
    assert opts == dict(point_heads=False, temporal=False, semantics='frame', point_heads_multi=multi_point_heads and K > 1)
    assert img is FRAMES and eng.coeff == 3.0 and asked == [(K, 7, 5, 3)]
    assert set(kw) == {'offsets', 'project', 'max_hand', 'tracks', 'track_table', 'smooth'}
    assert kw['offsets'] is OFFSETS and kw['project'] is True and kw['max_hand'] == K and kw['tracks'] is tracks
    assert kw['track_table'] == 'the track table' and kw['smooth'] is temporal
    assert eng.opts == DEFAULTS


def test_fused_call_refuses_before_the_engine_is_touched():
    main = pkg('acr.main')
    cases = [(dict(K=2, tracks=[0, 1], streams=[0, 1]), False, 'frame', 'not together with streams='),
             (dict(K=2, streams=[0, 1]), True, 'frame', 'streams= follows one hand of each side .* max_hand=2'),
             (dict(K=2), True, 'frame', 'temporal optimisation follows one hand of each side: not with max_hand=2'),
             (dict(K=2), False, 'reference', "batch_semantics='reference' .* not with max_hand=2"),
             (dict(K=1, tracks=[0, 1], batch_semantics='reference'), False, 'frame', 'not with max_hand=1'),
             (dict(K=9), False, 'frame', 'max_hand'),
             (dict(K=9, multi_point_heads=1), False, 'frame', 'max_hand')]
    for kw, temporal, parser, message in cases:
        fake, eng, asked = _fake_self(temporal, parser)
        fake.model.engine = None
        with pytest.raises(ValueError, match=message):
            main.ACR._fused_call(fake, FRAMES, ['a', 'b'], **kw)
        assert eng.seen is None and eng.opts == DEFAULTS and eng.coeff == 'unset' and not asked, kw


# ---- the views -----------------------------------------------------------------------------------------------------------

def test_views_assembler():
    main = pkg('acr.main')
    frames, asked = object(), []

    def draw(name):
        asked.append(name)
        return 'the %s view' % name

    assert main._views(None, frames, draw) == 'the mesh view' and asked == ['mesh']
    views = main._views(['pj2d', 'org_img', 'centermap'], frames, draw)
    assert list(views) == ['pj2d', 'org_img', 'centermap'] and asked == ['mesh', 'pj2d', 'centermap']
    assert views['org_img'] is frames and views['pj2d'] == 'the pj2d view' and views['centermap'] == 'the centermap view'
    assert main._views(['org_img'], frames, draw) == {'org_img': frames}


class FakeDrawer(object):
    """Engine's drawing calls: records them and returns the frames (two copies of them for 'centermap')."""

    def __init__(self):
        self.calls = []

    def render_regions(self, out, imgs, offsets, region_frame, focal_length=None, bgr=None):
        self.calls.append(('mesh', out, tuple(imgs.shape), offsets, region_frame, bgr))
        return imgs + 10

    def overlay_regions(self, out, imgs, what, offsets, region_frame, bgr=None):
        self.calls.append((what, out, tuple(imgs.shape), offsets, region_frame, bgr))
        return torch.stack([imgs + 10, imgs + 20]) if what == 'centermap' else imgs + 10

    def overlay(self, out, imgs, what, offsets=None, bgr=None):
        self.calls.append(('frame ' + what, out, tuple(imgs.shape), offsets, None, bgr))
        return torch.stack([imgs + 10, imgs + 20])


def test_views_of_several_hands_per_side_are_region_views():
    main = pkg('acr.main')
    B, K = 3, 2
    out = {'slots': torch.arange(B * K * 2 * 176.).view(B, K, 2, 176), 'verts': torch.zeros(B, K, 2, 778, 3),
           'pj2d_org': torch.zeros(B, K, 2, 21, 2), 'cam_trans': torch.zeros(B, K, 2, 3)}
    offsets = torch.arange(B * 10.).view(B, 10)
    me = SimpleNamespace(focal_length=1265., _overlay_batch=lambda *a: main.ACR._overlay_batch(None, *a))
    frames = torch.zeros((B,) + A, dtype=torch.uint8)
    for bgr in (True, False):
        eng = FakeDrawer()
        views = main._multi_views(me, eng, out, frames, offsets, bgr, ['mesh', 'pj2d', 'centermap', 'org_img'])
        assert list(views) == ['mesh', 'pj2d', 'centermap', 'org_img'] and views['org_img'] is frames
        assert [c[0] for c in eng.calls] == ['mesh', 'pj2d', 'frame centermap']
        for what, flat, shape, rows, region_frame, got_bgr in eng.calls[:2]:      # pair k of frame b = region b * K + k of frame b
            assert torch.equal(flat['slots'], out['slots'].flatten(0, 1)) and flat['verts'].shape == (B * K, 2, 778, 3)
            assert torch.equal(rows, offsets.repeat_interleave(K, 0)) and got_bgr is bgr
            assert region_frame.dtype == torch.int32 and region_frame.tolist() == [0, 0, 1, 1, 2, 2]
        _, sub, _, off, _, got_bgr = eng.calls[2]      # the centre maps: per frame, pair 0's slots standing for the frame
        assert torch.equal(sub['slots'], out['slots'][:, 0]) and off is offsets and got_bgr is bgr
    # a list of frames: per size, the regions of the other sizes' frames at -1; offsets None = the network input
    eng, frames = FakeDrawer(), _frames_aba()
    got = main._multi_views(me, eng, out, frames, None, False, None)
    assert [(c[0], c[2], c[4].tolist()) for c in eng.calls] == [('mesh', (2,) + A, [0, 0, -1, -1, 1, 1]),
                                                               ('mesh', (1,) + B_, [-1, -1, 0, 0, -1, -1])]
    assert torch.equal(eng.calls[0][3], main._whole_frame_offsets(B * K))
    assert isinstance(got, list) and all(torch.equal(g, f + 10) for g, f in zip(got, frames))
    with pytest.raises(ValueError, match='^one frame to draw into per input frame$'):
        main._multi_views(me, eng, out, frames[:2], None, False, ['org_img'])


def test_region_views_follow_box_frame():
    main = pkg('acr.main')
    out, offsets, frames = {'slots': torch.zeros(4, 2, 176)}, object(), _frames_aba()
    eng = FakeDrawer()
    views = main._region_views(SimpleNamespace(focal_length=1265.), eng, out, frames, offsets, [2, 0, 1, 2], ['centermap', 'org_img'])
    assert views['org_img'] is frames
    assert [(c[0], c[2], c[4].tolist(), c[5]) for c in eng.calls] == [('centermap', (2,) + A, [1, 0, -1, 1], True),
                                                                     ('centermap', (1,) + B_, [-1, -1, 0, -1], True)]
    assert all(c[1] is out and c[3] is offsets for c in eng.calls)
    for g, f in zip(views['centermap'], frames):
        assert g.shape == (2,) + tuple(f.shape) and torch.equal(g[0], f + 10) and torch.equal(g[1], f + 20)
    eng = FakeDrawer()
    stacked = torch.zeros((4,) + A, dtype=torch.uint8)
    assert torch.equal(main._region_views(SimpleNamespace(focal_length=1265.), eng, out, stacked, offsets, None, None), stacked + 10)
    assert [(c[0], c[4].tolist()) for c in eng.calls] == [('mesh', [0, 1, 2, 3])]


# ---- the render arguments ------------------------------------------------------------------------------------------------

def test_render_arguments_are_checked_in_one_order():
    main = pkg('acr.main')
    frames = torch.zeros((2,) + A, dtype=torch.uint8)
    check = main._check_render_args
    with pytest.raises(ValueError, match='show_items needs render=True'):
        check(frames, ['mesh'], False, 'i420', 'bgr', 'cv601')
    with pytest.raises(ValueError, match="render_format: 'i420' is not 'bgr' or 'nv12'"):
        check(frames, None, False, 'i420', 'bgr', 'cv601')
    with pytest.raises(ValueError, match="render_format='nv12' needs render=True"):
        check(torch.zeros(2, 5, 6, 3, dtype=torch.uint8), None, False, 'nv12', 'bgr', 'cv601')
    with pytest.raises(ValueError, match='even'):
        check(torch.zeros(2, 5, 6, 3, dtype=torch.uint8), None, True, 'nv12', 'bgr', 'cv601')
    matrix = object()
    assert check(frames, ['mesh'], True, 'bgr', 'bgr', matrix) == (None, matrix)
    to_nv12, row6 = check(frames, None, True, 'nv12', 'bgr', 'bt709')
    assert callable(to_nv12) and row6 == 'cv601'


def test_views_to_nv12_takes_a_view_or_a_dict_of_views():
    main = pkg('acr.main')
    to_nv12 = lambda name, view: (name, view)
    assert main._views_to_nv12(to_nv12, 'frames') == ('mesh', 'frames')
    assert main._views_to_nv12(to_nv12, {'pj2d': 1, 'centermap': 2}) == {'pj2d': ('pj2d', 1), 'centermap': ('centermap', 2)}
