"""What the grouped launches should be, from a lowered program alone (no library call): the buffers every op reads and writes,
which ops run on the kernel instantiation with a group form, and - by a search of its own, not csrc/group_plan.h's - which pairs
are independent.  Shared by tests/test_group_plan_host.py and tests/test_gpu_grouped.py."""
from conftest import pkg


def active(L, op, point=False):
    return op.kind != L.OP_COORDFILL and op.mode != (L.MODE_DENSE if point else L.MODE_POINT)


def op_rw(L, prog, op):
    """(reads, writes) of buffer ids; the two pseudo-buffers behind the real ones are the attention-pool and centre-pick
    workspaces (acrmi_program.hip op_rw)."""
    nb, h = len(prog['bufs']), prog['heads']
    R, W = [], []
    r = lambda i: R.append(i) if i >= 0 else None
    w = lambda i: W.append(i) if i >= 0 else None
    terms = [op.term_buf[t] for t in range(op.nterms)]
    k = op.kind
    if k in (L.OP_U8NORM, L.OP_STEM):
        w(op.out_buf)
    elif k == L.OP_CONV:
        r(op.in_buf), r(op.res_buf)
        if op.bias_per_frame:
            r(op.aux_buf)
        for t in terms:
            r(t)
        w(op.out_buf)
        if op.flags & L.CONV_DUAL:
            w(op.aux_buf)
    elif k == L.OP_FUSESUM:
        for t in terms:
            r(t)
        w(op.out_buf)
    elif k in (L.OP_BILINEAR2X, L.OP_MAXPOOL):
        r(op.in_buf), w(op.out_buf)
    elif k == L.OP_PAIR1X1:
        r(op.in_buf), r(op.res_buf), w(op.out_buf), w(op.aux_buf)
    elif k == L.OP_POW11:
        r(op.out_buf), w(op.out_buf)
    elif k == L.OP_ATTPOOL:
        r(op.in_buf), r(op.res_buf), w(op.out_buf), w(nb)
    elif k == L.OP_PAREBIAS:
        r(op.in_buf), w(op.out_buf)
    elif k == L.OP_POINTHEADS:
        r(op.in_buf), r(op.aux_buf), r(h.center_buf[0]), r(h.center_buf[1])
        w(op.res_buf), w(op.out_buf), w(h.prior_buf[op.flags & 1]), w(nb + 1)
    return R, W


def group_key(L, prog, op):
    """1 for a conv on conv_wino24b_kernel<2, 32> (the instantiation with a group form: F(2x4,3x3), fp32, 8x32-pixel items, two
    n-tiles per wave, more than one 32-channel chunk), else 0."""
    if op.kind != L.OP_CONV or (op.flags & 7) != 4 or op.ksize != 3 or op.stride != 1:
        return 0
    h, w, _cs, _p, dt = prog['bufs'][op.in_buf]
    if dt != L.DT_F32 or pkg('packer').wino24b_width(op.cin, op.cout, h, w) != 32:
        return 0
    return int(op.cin >= 64 and op.cout % 64 == 0)


def program_table(prog, point=False):
    """Per active op, in program order: (index, key, reads, writes)."""
    L = pkg('_lib')
    return [(i, group_key(L, prog, op)) + op_rw(L, prog, op) for i, op in enumerate(prog['ops']) if active(L, op, point)]


def ancestors(table):
    """op -> the set of ops it depends on, directly or not (RAW / WAR / WAW on buffer ids, program order)."""
    last_w, readers, anc = {}, {}, {}
    for i, _key, R, W in table:
        d = set()
        for b in R:
            d.add(last_w.get(b))
        for b in W:
            d.add(last_w.get(b))
            d.update(readers.get(b, ()))
        d.discard(None)
        d.discard(i)
        full = set(d)
        for j in d:
            full |= anc[j]
        anc[i] = full
        for b in R:
            readers.setdefault(b, []).append(i)
        for b in W:
            last_w[b] = i
            readers[b] = []
    return anc


def hr_pairs(prog, point=False):
    """The branch-1 / branch-2 convolutions of one HR module and one depth: (name of the branch-1 op, of the branch-2 op), both on
    the grouping instantiation.  The groups the executor is expected to form."""
    L = pkg('_lib')
    by_name = {info['name']: (i, op) for i, (op, info) in enumerate(zip(prog['ops'], prog['op_info'])) if active(L, op, point)}
    pairs = []
    for name, (_i, op) in by_name.items():
        if '.branches.1.' in name and group_key(L, prog, op):
            other = name.replace('.branches.1.', '.branches.2.')
            if other in by_name and group_key(L, prog, by_name[other][1]):
                pairs.append((name, other))
    return pairs
