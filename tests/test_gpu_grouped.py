"""Grouped launches (conv_frame.h ConvGroup): two independent convolutions of one kernel instantiation in one persistent launch
give, bit for bit, what their own launches give - at the kernel through ops.conv2d_group, and in the program, where the executor
forms the groups (csrc/group_plan.h).  `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import group_ref
from conftest import pkg

pytestmark = pytest.mark.gpu


def _problem(seed, cin, cout, H, W, B, residual=False, frame_bias=False, relu=True):
    g = torch.Generator().manual_seed(seed)
    p = {'x': torch.randn(B, H, W, cin, generator=g).cuda(),
         'weight': (torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9.0 * cin)).numpy(),
         'bias': torch.randn(cout, generator=g).numpy(), 'relu': relu}
    if residual:
        p['residual'] = torch.randn(B, H, W, cout, generator=g).cuda()
    if frame_bias:
        p['frame_bias'] = torch.randn(B, cout, generator=g).cuda()
    return p


def _alone(p):
    return pkg('ops').conv2d(p['x'], p['weight'], None if 'frame_bias' in p else p['bias'], relu=p['relu'], residual=p.get('residual'),
                             frame_bias=p.get('frame_bias'), algo='winograd24')


# 64 -> 64 @16x32 and 128 -> 128 @8x32 are the smallest maps the <2, 32> frame tiles exactly: 6 items each at B = 3, of two and
# of four chunks.  @64x64 at B = 20 is 320 items: more than there are workgroups, so a workgroup walks several, and some walk an
# item of each problem - the switch of all three cursors inside one workgroup, in either order.
SMALL_A = dict(cin=64, cout=64, H=16, W=32, B=3)
SMALL_B = dict(cin=128, cout=128, H=8, W=32, B=3)
LARGE = dict(cin=64, cout=64, H=64, W=64, B=20)
CASES = {
    'two chunk counts': (dict(SMALL_A), dict(SMALL_B)),
    'the other order': (dict(SMALL_B), dict(SMALL_A)),
    'residual first': (dict(SMALL_A, residual=True), dict(SMALL_B)),
    'residual second, no relu first': (dict(SMALL_A, relu=False), dict(SMALL_B, residual=True)),
    'per-frame bias': (dict(SMALL_A, frame_bias=True), dict(SMALL_B, residual=True)),
    'few items then many': (dict(SMALL_A, residual=True), dict(LARGE)),
    'many items then few': (dict(LARGE, residual=True), dict(SMALL_B, frame_bias=True)),
    'many then many, other width': (dict(LARGE), dict(cin=128, cout=128, H=32, W=32, B=33, residual=True)),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_group_of_two_is_bit_identical_to_two_launches(case):
    ops = pkg('ops')
    pa, pb = (_problem(11 + i, **kw) for i, kw in enumerate(CASES[case]))
    want = [_alone(pa), _alone(pb)]
    for rep in range(2):                       # (a second launch: nothing of the first one's state is left behind)
        got = ops.conv2d_group([pa, pb])
        torch.cuda.synchronize()
        for i in range(2):
            assert torch.equal(got[i], want[i]), (case, rep, i, (got[i] - want[i]).abs().max().item())


def test_group_of_one_is_the_plain_launch():
    p = _problem(5, residual=True, **SMALL_B)
    got = pkg('ops').conv2d_group([p])
    assert torch.equal(got[0], _alone(p))


def test_problems_of_two_instantiations_are_refused():
    L = pkg('_lib')
    one_chunk = _problem(7, cin=32, cout=64, H=16, W=32, B=2)      # Cin = 32: the single-chunk instantiation
    narrow = _problem(8, cin=64, cout=64, H=16, W=16, B=2)         # 16x16-pixel items
    for other in (one_chunk, narrow):
        with pytest.raises((ValueError, L.AcrmiError)):
            pkg('ops').conv2d_group([_problem(9, **SMALL_A), other])


def test_program_with_and_without_groups_is_bit_identical(synth_sd, mano_tables):
    """A max_batch = 16 engine with grouped launches and one without: every head map, the backbone map, slots, verts and joints
    are equal at B = 16, on one stream and on the lanes the library picks; the grouped one has formed the branch-1 / branch-2
    pairs of every HR module (counted from the op list), the other none."""
    L, engine = pkg('_lib'), pkg('engine')
    tables = {k: dict(v) for k, v in mano_tables.items()}
    x = torch.from_numpy(pkg('synth').make_frames(16, seed=3, structured=True)).cuda()

    def run(eng, lanes):
        eng.set_lanes(lanes)
        B = eng.backbone_heads(x)
        out = {k: v.clone() for k, v in eng.head_maps(B).items()}
        out['backbone'] = eng.buffer(eng.program['heads'].backbone_buf, B).clone()
        out.update({k: v.clone() for k, v in eng.forward(x).items()})
        return out

    engs = {}
    try:
        for on in (False, True):
            assert L.lib().acrmi_tune(5, int(on)) == 0
            engs[on] = engine.Engine(0)
            engs[on].load_state_dict(synth_sd, max_batch=16)
            engs[on].load_mano(tables)
    finally:
        L.lib().acrmi_tune(5, 1)
    want_groups = len(group_ref.hr_pairs(engs[True].program))
    assert want_groups > 0
    for lanes in (1, 0):
        for eng in engs.values():
            eng.set_lanes(lanes)
        assert L.lib().acrmi_program_groups(engs[False].ctx, 16) == 0
        assert L.lib().acrmi_program_groups(engs[True].ctx, 16) == want_groups
        a, b = run(engs[False], lanes), run(engs[True], lanes)
        assert set(a) == set(b) and {'slots', 'verts', 'joints', 'segms', 'backbone'} <= set(a)
        for k in a:
            assert torch.equal(a[k], b[k]), (lanes, k)
