"""ORACLE (test infrastructure, not product): CPU interpreter of a lowered op program (packer.lower).

What it is for: the 16-bit programs (the reference's autocast branch, acr/model.py:33-37, re-stated for gfx950 in
packer.lower) and the HRNet-W48 programs (BASELINE.json configs[4]) have NO reference oracle - autocast is CUDA-only
 and the reference hard-wires HRNet-W32.  This module restates the semantics the C library implements,
op by op, in torch-CPU arithmetic on the un-packed folded filters the packer keeps with keep_weights=True:

  * a 16-bit buffer holds values of its storage type (f16 / bf16); every op computes in float64 / float32 on those
    values and rounds its result ONCE (nearest even) when it writes a 16-bit buffer;
  * CONV: filters rounded to the storage type (fp32 programs: to fp32), exact products, float64 accumulation
    (the kernels accumulate in fp32: the difference is ~1e-7 relative, far below one 16-bit ulp, but it can move a
    value across a rounding boundary - comparisons allow a few ulps of the storage type), + bias (fp32, shared or per
    frame) + residual, ReLU;
  * the element-wise ops follow the kernels' fp32 expressions term by term;
  * the lowering's own constructions are read back into the convolutions they stand for: a CONV with ACRMI_CONV_SPLITK is
    ONE convolution over its concatenated K-slices, ACRMI_CONV_BIAS_MAP adds the position-bias map of the blob to every
    frame, PAIR1X1 is two 1x1 convolutions (64 -> 256 + residual + ReLU, then 256 -> 64 + ReLU), MAXPOOL and the 7x7 stem
    belong to the build-defined ResNet-50 (oracle/acr_net.resnet50_backbone); a CONV with nterms > 0 adds that many extra
    residual maps (nearest-upsampled by 2^shift) before its ReLU: the HR-module fuse sum (acr/model.py:672-686) folded into
    the last convolution of the x0 downsampling chain.

For fp32 W32 programs the same interpreter is cross-checked against oracle/acr_net.py (pinned to the reference), which
pins the interpreter's reading of the op list; tests/test_program_oracle.py.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this.
"""
import numpy as np
import torch
import torch.nn.functional as F

OP_U8NORM, OP_CONV, OP_FUSESUM, OP_BILINEAR2X, OP_POW11, OP_ATTPOOL, OP_PAREBIAS, OP_COORDFILL, OP_POINTHEADS, OP_STEM = range(1, 11)
OP_MAXPOOL, OP_PAIR1X1 = 11, 12
MODE_POINT = 2
CONV_BIAS_MAP = 8      # acrmi_op.flags of a CONV (include/acrmi.h)
CONV_SPLITK = 16
CONV_DUAL = 32
DT_F32, DT_F16, DT_BF16 = 0, 1, 2


def rnd(x, dt):
    """float tensor -> values representable in storage type dt, as float32 (round to nearest even)."""
    x = x.to(torch.float32)
    if dt == DT_F16:
        return x.to(torch.float16).to(torch.float32)
    if dt == DT_BF16:
        return x.to(torch.bfloat16).to(torch.float32)
    return x


def bilinear2x(x):
    """align_corners=True x2 bilinear upsampling of an NHWC map, in bilinear2x_kernel's fp32 expression."""
    B, H, W, C = x.shape
    Ho, Wo = 2 * H, 2 * W
    f32 = torch.float32
    sh = (torch.tensor(H - 1, dtype=f32) / torch.tensor(Ho - 1, dtype=f32))
    sw = (torch.tensor(W - 1, dtype=f32) / torch.tensor(Wo - 1, dtype=f32))
    fy = sh * torch.arange(Ho, dtype=f32)
    fx = sw * torch.arange(Wo, dtype=f32)
    y0, x0 = fy.to(torch.int64), fx.to(torch.int64)
    y1 = y0 + (y0 < H - 1).to(torch.int64)
    x1 = x0 + (x0 < W - 1).to(torch.int64)
    ly, lx = (fy - y0.to(f32)), (fx - x0.to(f32))
    hy, hx = 1.0 - ly, 1.0 - lx
    v00, v01 = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
    v10, v11 = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    hx_, lx_ = hx[None, None, :, None], lx[None, None, :, None]
    hy_, ly_ = hy[None, :, None, None], ly[None, :, None, None]
    return hy_ * (hx_ * v00 + lx_ * v01) + ly_ * (hx_ * v10 + lx_ * v11)


class Interp(object):
    def __init__(self, prog, B):
        self.prog, self.B = prog, B
        self.bufs = [torch.zeros(B, h, w, cs, dtype=torch.float32) for (h, w, cs, _p, _dt) in prog['bufs']]
        self.dts = [b[4] for b in prog['bufs']]
        self.blob = torch.from_numpy(np.asarray(prog['blob']))
        self.prog_dt = max(self.dts)

    def w(self, off, n):
        return self.blob[off:off + n].to(torch.float64)

    # ---- ops -------------------------------------------------------------------------------------------
    def conv(self, op, info):
        x = self.bufs[op.in_buf][..., op.in_coff:op.in_coff + op.groups * op.cin]
        wdt = self.dts[op.in_buf]                      # filters are stored in the input's type (fp32 programs: fp32)
        ws, bs = [], []
        for (w, b) in info['wb']:
            ws.append(rnd(torch.from_numpy(np.ascontiguousarray(w)), wdt).to(torch.float64))
            bs.append(torch.from_numpy(np.asarray(b, np.float32)).to(torch.float64))    # bias: fp32 in the blob
        splitk = bool(op.flags & CONV_SPLITK)          # the "groups" are K-slices of one convolution: same Cout
        if splitk:
            w, bs = torch.cat(ws, 1), bs[:1]
            y = F.conv2d(x.permute(0, 3, 1, 2).to(torch.float64), w, None, op.stride, op.ksize // 2, 1, 1)
        else:
            w = torch.cat(ws, 0)
            y = F.conv2d(x.permute(0, 3, 1, 2).to(torch.float64), w, None, op.stride, op.ksize // 2, 1, op.groups)
        y = y.permute(0, 2, 3, 1)
        if op.bias_per_frame:
            y = y + self.bufs[op.aux_buf][:, 0, 0, :y.shape[-1]].to(torch.float64)[:, None, None, :]
        else:
            y = y + torch.cat(bs)[None, None, None, :]
        y = y.to(torch.float32)                        # the kernels add bias / residual in fp32
        n = op.cout if splitk else op.groups * op.cout
        if op.flags & CONV_BIAS_MAP:                   # position-bias map in the blob: one map for every frame
            ho, wo, cs = y.shape[1], y.shape[2], (n + 3) // 4 * 4
            y = y + self.blob[op.w_off2:op.w_off2 + ho * wo * cs].view(1, ho, wo, cs)[..., :n]
        if op.res_buf >= 0:
            y = y + self.bufs[op.res_buf][..., op.res_coff:op.res_coff + n]
        dual = bool(op.flags & CONV_DUAL)              # the terms go into a SECOND output (aux_buf), not into this one
        if dual:
            if op.relu:
                y = torch.relu(y)
            self.bufs[op.out_buf][..., op.out_coff:op.out_coff + n] = rnd(y, self.dts[op.out_buf])
        for t in range(op.nterms):                     # extra residual terms: the HR fuse sum in this conv's epilogue
            v = self.bufs[op.term_buf[t]][..., op.term_coff[t]:op.term_coff[t] + n]
            sh = op.term_shift[t]
            if sh:
                v = v.repeat_interleave(1 << sh, 1).repeat_interleave(1 << sh, 2)    # nearest up (acr/model.py:639)
            y = y + v
        if dual:
            self.bufs[op.aux_buf][..., :n] = rnd(torch.relu(y), self.dts[op.aux_buf])
            return
        if op.relu:
            y = torch.relu(y)
        self.bufs[op.out_buf][..., op.out_coff:op.out_coff + n] = rnd(y, self.dts[op.out_buf])

    def stem(self, op, info, img):
        (w, b), = info['wb']
        x = (img.to(torch.float32) / 255.0) * 2.0 - 1.0                     # stem_kernel's table expression
        w = torch.from_numpy(np.asarray(w, np.float32)).to(torch.float64)   # pack_stem keeps fp32 filters
        y = F.conv2d(x.permute(0, 3, 1, 2).to(torch.float64), w, None, 2, op.ksize // 2).permute(0, 2, 3, 1)   # 3x3 / 7x7 (ResNet)
        y = (y + torch.from_numpy(np.asarray(b, np.float32)).to(torch.float64)).to(torch.float32)
        if op.relu:
            y = torch.relu(y)
        self.bufs[op.out_buf][..., op.out_coff:op.out_coff + 64] = rnd(y, self.dts[op.out_buf])

    def fuse_sum(self, op):
        acc = None
        for t in range(op.nterms):
            v = self.bufs[op.term_buf[t]][..., op.term_coff[t]:op.term_coff[t] + op.cout]
            sh = op.term_shift[t]
            if sh:
                v = v.repeat_interleave(1 << sh, 1).repeat_interleave(1 << sh, 2)    # nearest up (acr/model.py:639)
            acc = v.clone() if acc is None else acc + v
        if op.relu:
            acc = torch.relu(acc)
        self.bufs[op.out_buf][..., op.out_coff:op.out_coff + op.cout] = rnd(acc, self.dts[op.out_buf])

    def bilinear2x(self, op):
        x = self.bufs[op.in_buf][..., op.in_coff:op.in_coff + op.cin]
        self.bufs[op.out_buf][..., op.out_coff:op.out_coff + op.cin] = rnd(bilinear2x(x), self.dts[op.out_buf])

    def pair1x1(self, op, info):
        """out = relu(W3 in + b3 + res), aux = relu(W1 out + b1) (csrc/pair1x1.hip; fp32 programs)"""
        (w3, b3), (w1, b1) = [(torch.from_numpy(np.asarray(w, np.float64)), torch.from_numpy(np.asarray(b, np.float64)))
                              for (w, b) in info['wb']]
        t2 = self.bufs[op.in_buf][..., op.in_coff:op.in_coff + 64].to(torch.float64)
        y = torch.einsum('bhwc,oc->bhwo', t2, w3.reshape(256, 64)) + b3
        y = torch.relu(y.to(torch.float32) + self.bufs[op.res_buf][..., op.res_coff:op.res_coff + 256])
        self.bufs[op.out_buf][..., op.out_coff:op.out_coff + 256] = y
        t = torch.einsum('bhwc,oc->bhwo', y.to(torch.float64), w1.reshape(64, 256)) + b1
        self.bufs[op.aux_buf][..., :64] = torch.relu(t.to(torch.float32))

    def maxpool(self, op):
        x = self.bufs[op.in_buf][..., op.in_coff:op.in_coff + op.cin]
        y = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)      # exact in every storage type
        self.bufs[op.out_buf][..., op.out_coff:op.out_coff + op.cin] = y

    def pow11(self, op):
        b = self.bufs[op.out_buf]
        b[..., op.out_coff] = rnd(torch.pow(torch.tensor(1.1, dtype=torch.float32), b[..., op.out_coff]), self.dts[op.out_buf])

    def coordfill(self, op):
        b = self.bufs[op.out_buf]
        _, H, W, _ = b.shape
        f32 = torch.float32
        xs = (torch.arange(W, dtype=f32) / torch.tensor(W - 1, dtype=f32)) * 2.0 - 1.0
        ys = (torch.arange(H, dtype=f32) / torch.tensor(H - 1, dtype=f32)) * 2.0 - 1.0
        b[..., op.out_coff] = rnd(xs[None, None, :].expand(b.shape[0], H, W), self.dts[op.out_buf])
        b[..., op.out_coff + 1] = rnd(ys[None, :, None].expand(b.shape[0], H, W), self.dts[op.out_buf])

    def attpool(self, op):
        segm = self.bufs[op.in_buf]
        feat = self.bufs[op.res_buf][..., op.res_coff:op.res_coff + op.cin]
        B = segm.shape[0]
        logits = segm[:, ::2, ::2, 1:33].reshape(B, -1, 32).to(torch.float64)        # [B, pix, part]
        wts = torch.softmax(logits, 1)
        pooled = torch.einsum('bpj,bpc->bjc', wts, feat.reshape(B, -1, op.cin).to(torch.float64))
        self.bufs[op.out_buf].view(B, -1)[:, :32 * op.cin] = pooled.reshape(B, -1).to(torch.float32)

    def parebias(self, op):
        C, part0 = op.cin, op.flags
        B = self.B
        pooled = self.bufs[op.in_buf].view(B, -1)[:, :32 * C].reshape(B, 32, C).to(torch.float64)[:, part0:part0 + 16]   # [B,16,C]
        lc = self.w(op.w_off, 6 * 256 * 16).view(6, 256, 16)
        nsh = (64 if C == 320 else 256)
        lin_w = self.w(op.w_off2, 10 * nsh * 16).view(10, nsh, 16)
        lin_b = self.w(op.b_off2, 10)
        mix_wp = self.w(op.w_off3, 109 * 106).view(109, 106)
        mix_b = self.w(op.b_off, 109)
        off = torch.einsum('ocj,bjc->bjo', lc, pooled[:, :, :256]).reshape(B, 96)
        shp = lin_b + torch.einsum('kcj,bjc->bk', lin_w, pooled[:, :, C - nsh:] if C == 320 else pooled)
        pare = torch.cat([off, shp], 1)
        out = mix_b + pare @ mix_wp.t()
        self.bufs[op.out_buf][:, 0, 0, :109] = out.to(torch.float32)

    # ---- driver ----------------------------------------------------------------------------------------
    def step(self, op, info, img_u8):
        """Evaluates one dense op on the current buffers."""
        k = op.kind
        if k == OP_CONV:
            self.conv(op, info)
        elif k == OP_STEM:
            self.stem(op, info, img_u8)
        elif k == OP_FUSESUM:
            self.fuse_sum(op)
        elif k == OP_BILINEAR2X:
            self.bilinear2x(op)
        elif k == OP_MAXPOOL:
            self.maxpool(op)
        elif k == OP_PAIR1X1:
            self.pair1x1(op, info)
        elif k == OP_POW11:
            self.pow11(op)
        elif k == OP_COORDFILL:
            self.coordfill(op)
        elif k == OP_ATTPOOL:
            self.attpool(op)
        elif k == OP_PAREBIAS:
            self.parebias(op)
        else:
            raise ValueError('op kind %d is not part of the dense program' % k)

    def run(self, img_u8, after=None):
        """img_u8: torch uint8 [B,512,512,3].  Runs the dense variant of the program; returns self.
        after(n, op, info, self): called behind op n (tests plant faults there, so that later ops read them)."""
        for n, (op, info) in enumerate(zip(self.prog['ops'], self.prog['op_info'])):
            if op.mode == MODE_POINT:
                continue
            self.step(op, info, img_u8)
            if after is not None:
                after(n, op, info, self)
        return self

    def head_maps(self):
        """The reference's H11 dict (NCHW float32) from the interpreted head buffers."""
        hl = self.prog['heads']
        out = {}
        for si, side in enumerate('lr'):
            out[side + '_params_maps'] = self.bufs[hl.params_buf[si]][..., :109]
            out[side + '_center_map'] = self.bufs[hl.center_buf[si]][..., :1]
            out[side + '_prior_maps'] = self.bufs[hl.prior_buf[si]][..., :106]
        out['segms'] = self.bufs[hl.segm_buf][..., :33]
        return {k: v.permute(0, 3, 1, 2).contiguous() for k, v in out.items()}


@torch.no_grad()
def run_program(prog, img_u8):
    """prog = packer.lower(sd, keep_weights=True, ...); img_u8 uint8 [B,512,512,3] -> Interp (buffers + head_maps())."""
    if 'wb' not in next(i for i in prog['op_info'] if i['kind'] == OP_CONV):
        raise ValueError('lower the checkpoint with keep_weights=True')
    return Interp(prog, img_u8.shape[0]).run(img_u8)


# ---- per-op check of a program run --------------------------------------------------------------------------------
# The op kinds whose every output frame depends only on the same frame of their inputs: checking a subset of a batch's
# frames (the interpreter's batch = that subset) is valid only for these.  A new kind must be added here (and to
# Interp.step) before check_program accepts a program that uses it.
FRAME_LOCAL = (OP_CONV, OP_STEM, OP_FUSESUM, OP_BILINEAR2X, OP_MAXPOOL, OP_PAIR1X1, OP_POW11, OP_COORDFILL, OP_ATTPOOL,
               OP_PAREBIAS)
U32 = 2.0 ** -24       # unit round-off of fp32

# fp32 outputs: |got - want| <= ELEMENT_TOL[class] * 2^-24 * M per element, M = the 7x7 max of the op's sum of |terms|
# (check_program).  Each constant is the smallest power of two >= 2x the worst ratio measured on the MI355X over the
# programs, batches and both checkpoints of tests/test_gpu_program_ops.py (its per_op_report.json).
# A class measured bit-exact keeps the floor 1 (one rounding of M); maxpool is exact by construction (0: bit-equal).  An
# in-place chain is held to the looser class of its ops.  (Measured worst ratios in the comments.)
ELEMENT_TOL = {
    'direct': 32.0,         # 9.7 (the small-batch lowerings' head convs)
    'h16': 8.0,             # 2.8 (conv_h16_kernel's fp32 head outputs, 16-bit storage programs: tests/test_gpu_h16.py)
    'pair': 16.0,           # 4.5
    'stem': 16.0,           # 6.0 (ResNet-50's 7x7 stem)
    'f2x2': 8.0,            # 3.4
    'f2x2_lds': 8.0,        # 2.9
    'f2x2_splitk': 4.0,     # 1.5
    'f2x4': 16.0,           # 5.3
    'polyphase': 8.0,       # 3.9
    'split_f16x3': 32.0,    # 12.6 (hostile checkpoint)
    'split_bf16x3': 256.0,  # 115 (16-bit operand halves)
    'pow11': 4.0,           # 1.6 (on its own; every 1.1^x of the programs ends an in-place chain with a conv)
    'fusesum': 1.0, 'bilinear': 1.0, 'coordfill': 1.0,       # 0: bit-exact
    'maxpool': 0.0,
}
# ... and |got - want| <= LAYER_TOL[class] * max(1, max |want|) over the op's whole output (the bound of the earlier per-layer
# tests: 2e-5 for the fp32 kernels, 2e-6 for the layer1 pairs, 5e-6 / 1e-4 for the split-operand kernels)
LAYER_TOL = {'pair': 2e-6, 'split_f16x3': 5e-6, 'split_bf16x3': 1e-4}
LAYER_TOL_DEFAULT = 2e-5
ATTPOOL_TOL = 1e-5          # absolute on O(1) features (tests/test_gpu_kernels.py test_attpool_matches_oracle)
PAREBIAS_TOL = 2e-5         # rtol = atol (tests/test_gpu_network.py test_parebias_kernel_matches_oracle)
ALGO_CLASS = {'direct': 'direct', 'winograd_f2x2_3x3': 'f2x2', 'winograd_f2x2_3x3_lds': 'f2x2_lds',
              'winograd_f2x4_3x3': 'f2x4', 'polyphase_f2x2_s2': 'polyphase', 'split_f16x3': 'split_f16x3',
              'split_bf16x3': 'split_bf16x3'}
KIND_CLASS = {OP_STEM: 'stem', OP_FUSESUM: 'fusesum', OP_BILINEAR2X: 'bilinear', OP_MAXPOOL: 'maxpool', OP_PAIR1X1: 'pair',
              OP_POW11: 'pow11', OP_COORDFILL: 'coordfill', OP_ATTPOOL: 'attpool', OP_PAREBIAS: 'parebias'}


def op_class(prog, op, info):
    """Tolerance class of an op (ELEMENT_TOL / LAYER_TOL key)."""
    if op.kind != OP_CONV:
        return KIND_CLASS[op.kind]
    if prog['bufs'][op.in_buf][4] != DT_F32:
        return 'h16'                                   # conv_h16_kernel (16-bit storage programs)
    if op.flags & CONV_SPLITK:
        return 'f2x2_splitk'
    return ALGO_CLASS[info['algo']]


def written(op):
    """[(buf, region)] an op writes; region: ('ch', c0, c1) channels of every pixel, or ('flat', n) the first n floats of a
    frame."""
    k = op.kind
    if k == OP_CONV:
        n = op.cout if op.flags & CONV_SPLITK else op.groups * op.cout
        w = [(op.out_buf, ('ch', op.out_coff, op.out_coff + n))]
        return w + [(op.aux_buf, ('ch', 0, n))] if op.flags & CONV_DUAL else w
    if k == OP_PAIR1X1:
        return [(op.out_buf, ('ch', op.out_coff, op.out_coff + 256)), (op.aux_buf, ('ch', 0, 64))]
    if k == OP_STEM:
        return [(op.out_buf, ('ch', op.out_coff, op.out_coff + 64))]
    if k in (OP_BILINEAR2X, OP_MAXPOOL):
        return [(op.out_buf, ('ch', op.out_coff, op.out_coff + op.cin))]
    if k == OP_FUSESUM:
        return [(op.out_buf, ('ch', op.out_coff, op.out_coff + op.cout))]
    if k == OP_POW11:
        return [(op.out_buf, ('ch', op.out_coff, op.out_coff + 1))]
    if k == OP_COORDFILL:
        return [(op.out_buf, ('ch', op.out_coff, op.out_coff + 2))]
    if k == OP_ATTPOOL:
        return [(op.out_buf, ('flat', 32 * op.cin))]
    if k == OP_PAREBIAS:
        return [(op.out_buf, ('ch', 0, 109))]          # pixel (0, 0) only; the rest of the row buffer is 1x1
    raise ValueError('op kind %d: unknown outputs' % k)


def _view(t, region):
    if region[0] == 'ch':
        return t[..., region[1]:region[2]]
    return t.reshape(t.shape[0], -1)[:, :region[1]]


def _up(v, sh):
    return v.repeat_interleave(1 << sh, 1).repeat_interleave(1 << sh, 2) if sh else v


def _pool7(m):
    """7x7 stride-1 max over the pixels of an NHWC magnitude map: covers every output tile (F(2x4): 2 x 4) that holds the
    pixel - a Winograd kernel spreads the rounding error of a tile over all of its pixels."""
    return F.max_pool2d(m.permute(0, 3, 1, 2), 7, 1, 3).permute(0, 2, 3, 1)


def conv_magnitude(it, op, info, carry=None):
    """(M_out, M_aux) of a CONV in fp64 on the interpreter's current buffers, before the 7x7 max: |W| * |X| + |bias|
    (+ |bias map|) + |residual|, and + sum |terms| for the map that receives the terms (the first one unless CONV_DUAL).
    carry: {buf: magnitude} of buffers that hold an interpreter value (in-place chains): used in place of |residual|."""
    carry = carry or {}
    x = it.bufs[op.in_buf][..., op.in_coff:op.in_coff + op.groups * op.cin].permute(0, 3, 1, 2).to(torch.float64).abs()
    wdt = it.dts[op.in_buf]
    ws = [rnd(torch.from_numpy(np.ascontiguousarray(w)), wdt).to(torch.float64).abs() for (w, _b) in info['wb']]
    bs = [torch.from_numpy(np.asarray(b, np.float32)).to(torch.float64).abs() for (_w, b) in info['wb']]
    splitk = bool(op.flags & CONV_SPLITK)
    if splitk:
        m = F.conv2d(x, torch.cat(ws, 1), None, op.stride, op.ksize // 2, 1, 1)
        bs = bs[:1]
    else:
        m = F.conv2d(x, torch.cat(ws, 0), None, op.stride, op.ksize // 2, 1, op.groups)
    m = m.permute(0, 2, 3, 1)
    n = m.shape[-1]
    if op.bias_per_frame:
        m = m + it.bufs[op.aux_buf][:, 0, 0, :n].to(torch.float64).abs()[:, None, None, :]
    else:
        m = m + torch.cat(bs)[None, None, None, :]
    if op.flags & CONV_BIAS_MAP:
        ho, wo, cs = m.shape[1], m.shape[2], (n + 3) // 4 * 4
        m = m + it.blob[op.w_off2:op.w_off2 + ho * wo * cs].view(1, ho, wo, cs)[..., :n].to(torch.float64).abs()
    if op.res_buf >= 0:
        r = carry[op.res_buf] if op.res_buf in carry else it.bufs[op.res_buf].to(torch.float64).abs()
        m = m + r[..., op.res_coff:op.res_coff + n]
    m1 = m
    for t in range(op.nterms):
        m = m + _up(it.bufs[op.term_buf[t]][..., op.term_coff[t]:op.term_coff[t] + n].to(torch.float64).abs(), op.term_shift[t])
    return (m1, m) if op.flags & CONV_DUAL else (m, None)


def _magnitudes(it, op, info, img_u8, carry):
    """{label: M (fp64, before the 7x7 max) or None} of an op's fp32 outputs, on the buffers BEFORE the op runs."""
    k = op.kind
    d = lambda b: it.bufs[b].to(torch.float64).abs()
    if k == OP_CONV:
        m1, m2 = conv_magnitude(it, op, info, carry)
        return {'out': m1, 'aux': m2} if m2 is not None else {'out': m1}
    if k == OP_PAIR1X1:
        (w3, b3), (w1, b1) = [(torch.from_numpy(np.asarray(w, np.float64)).abs(), torch.from_numpy(np.asarray(b, np.float64)).abs())
                              for (w, b) in info['wb']]
        t2 = d(op.in_buf)[..., op.in_coff:op.in_coff + 64]
        mo = torch.einsum('bhwc,oc->bhwo', t2, w3.reshape(256, 64)) + b3 + d(op.res_buf)[..., op.res_coff:op.res_coff + 256]
        # the second GEMM reads the first one's result: its error is |W1| times the first output's error bound
        return {'out': mo, 'aux': torch.einsum('bhwc,oc->bhwo', mo, w1.reshape(64, 256)) + b1}
    if k == OP_STEM:
        (w, b), = info['wb']
        x = ((img_u8.to(torch.float32) / 255.0) * 2.0 - 1.0).permute(0, 3, 1, 2).to(torch.float64).abs()
        w = torch.from_numpy(np.asarray(w, np.float32)).to(torch.float64).abs()
        m = F.conv2d(x, w, None, 2, op.ksize // 2).permute(0, 2, 3, 1)
        return {'out': m + torch.from_numpy(np.asarray(b, np.float32)).to(torch.float64).abs()}
    if k == OP_FUSESUM:
        return {'out': sum(_up(d(op.term_buf[t])[..., op.term_coff[t]:op.term_coff[t] + op.cout], op.term_shift[t])
                           for t in range(op.nterms))}
    if k == OP_BILINEAR2X:
        return {'out': bilinear2x(it.bufs[op.in_buf][..., op.in_coff:op.in_coff + op.cin].abs()).to(torch.float64)}
    if k == OP_COORDFILL:
        return {'out': None}                          # |values| <= 1: M = 1
    if k == OP_POW11:
        # d(1.1^x) = ln(1.1) 1.1^x dx: an interpreter-held input (in-place chain) carries its own error bound
        mx = carry[op.out_buf][..., op.out_coff:op.out_coff + 1] if op.out_buf in carry else 0.0
        y = torch.pow(torch.tensor(1.1, dtype=torch.float32), it.bufs[op.out_buf][..., op.out_coff:op.out_coff + 1])
        return {'out': y.to(torch.float64).abs() * (1.0 + float(np.log(1.1)) * mx)}
    return {'out': None}                              # maxpool (exact), attpool / parebias (bounds of their kernel tests)


def check_program(prog, bufs, img_u8, frames=None, element_tol=None):
    """Per-op check of one run of a lowered program on the GPU.

    prog: packer.lower(..., keep_weights=True, keep_all=True) (no buffer reuse: every op's inputs survive the run);
    bufs: host float32 copies [F, h, w, cs] of the chosen frames of EVERY program buffer after the run; img_u8: the uint8
    input of those frames [F, 512, 512, 3]; frames: their indices in the call's batch (report only).

    Every dense op is re-evaluated by Interp, with the F frames as its batch, on the GPU's own input buffers, and every
    output it writes is compared (CONV_DUAL's second map and both PAIR1X1 maps included).  An op whose output a later op
    updates in place (a conv with res_buf == out_buf, POW11) keeps the interpreter's value, which flows into that op: the
    chain is compared as one unit.  fp32 outputs: |got - want| <= c_class 2^-24 M per element, M = maxpool7x7(|W| * |X| +
    |bias| + |residual| + sum |terms|) in fp64 on the same slices (ELEMENT_TOL), and <= LAYER_TOL x max(1, max |want|) over
    the output; 16-bit outputs: within one ulp of the storage type (+ the fp32 accumulation error), < 2 % not bit-equal.
    Every channel no op writes must still be exactly 0.0 (acrmi_set_program zeroes the buffers: a non-zero value there is a
    stray write).

    Returns {'rows': one per compared output (op, kind, algo, class, ratio = worst |got - want| over its bound's unit,
    where = (frame, y, x, c) of that element, rel_err = max |got - want| / max |want|, ...), 'checked': ops compared,
    'chained': ops compared through their in-place successor, 'worst_frac_16bit', 'failures': [dicts]}."""
    tol = dict(ELEMENT_TOL, **(element_tol or {}))
    B = img_u8.shape[0]
    frames = list(range(B)) if frames is None else list(frames)
    assert len(bufs) == len(prog['bufs']) and all(tuple(b.shape) == (B,) + tuple(d[:3]) for b, d in zip(bufs, prog['bufs']))
    if 'wb' not in next(i for i in prog['op_info'] if i['kind'] == OP_CONV):
        raise ValueError('lower the checkpoint with keep_weights=True')
    ops = [(n, op, info) for n, (op, info) in enumerate(zip(prog['ops'], prog['op_info'])) if op.mode != MODE_POINT]
    for n, op, info in ops:
        if op.kind not in FRAME_LOCAL:
            raise ValueError('op %d (%s): kind %d is not a known frame-local op' % (n, info['name'], op.kind))
    seen = set()
    for _n, op, _i in ops:                             # keep_all: no two ops write the same region (in place apart)
        for b, reg in written(op):
            key = (b,) + reg
            assert key not in seen or (op.kind == OP_POW11 or (op.kind == OP_CONV and op.res_buf == op.out_buf)), \
                'buffer %d is reused: lower with keep_all=True' % b
            seen.add(key)
    it = Interp(prog, B)
    it.bufs = [b.clone() for b in bufs]
    in_place = lambda o: o.kind == OP_POW11 or (o.kind == OP_CONV and o.res_buf == o.out_buf)
    carry, carry_cls, pending, rows, failures = {}, {}, {}, [], []
    checked, chained, worst = 0, 0, {'frac': 0.0}

    def compare(n, op, info, cls, label, b, reg, m, in_absmax):
        """One output region of op n against the interpreter; the GPU's values then replace the interpreter's."""
        want, got = _view(it.bufs[b], reg).to(torch.float64), _view(bufs[b], reg).to(torch.float64)
        d = (got - want).abs()
        d = torch.where(torch.isnan(d), torch.full_like(d, float('inf')), d)
        scale, err = float(want.abs().max()), float(d.max())
        row = {'op': info['name'], 'index': n, 'kind': int(op.kind), 'algo': info.get('algo'), 'kernel': info.get('kernel'),
               'class': cls, 'out': label, 'err': err, 'scale': scale, 'rel_err': err / max(scale, 1e-20),
               'in_absmax': in_absmax}
        bad = []
        if prog['bufs'][b][4] != DT_F32:
            # one ulp of the storage type + the kernels' fp32 accumulation error (absolute: it exceeds the spacing of
            # the storage type where large terms cancel to a tiny result)
            e = torch.floor(torch.log2(want.abs().clamp_min(1e-30)))
            if prog['bufs'][b][4] == DT_F16:
                e, mant = e.clamp_min(-14.0), 10
            else:
                mant = 7
            u = torch.pow(2.0, e - mant) + 2e-6 * max(1.0, scale)
            r = d / u
            frac = float((d > 0).double().mean())
            worst['frac'] = max(worst['frac'], frac)
            row.update(rule='ulp16', frac_not_bit_equal=frac)
            if bool((d > u * 1.001).any()):
                bad.append('ulp16')
            if frac >= 0.02:
                bad.append('frac16')
        elif cls == 'attpool':
            r = d / (ATTPOOL_TOL * max(1.0, scale))
            row['rule'] = 'attpool'
            if bool((r > 1.0).any()):
                bad.append('attpool')
        elif cls == 'parebias':
            r = d / (PAREBIAS_TOL * (1.0 + want.abs()))
            row['rule'] = 'parebias'
            if bool((r > 1.0).any()):
                bad.append('parebias')
        else:
            if m is None:
                m = want.abs() if cls == 'maxpool' else torch.ones_like(want)
            r = torch.where(d == 0, torch.zeros_like(d), d / (U32 * m))      # d > 0 where M = 0: inf
            row['rule'] = 'element'
            if bool((r > tol[cls]).any()):
                bad.append('element')
            if err > LAYER_TOL.get(cls, LAYER_TOL_DEFAULT) * max(1.0, scale):
                bad.append('layer')
        flat = int(torch.argmax(r))
        idx = np.unravel_index(flat, tuple(r.shape))
        where = [frames[int(idx[0])]] + [int(i) for i in idx[1:]]
        if reg[0] == 'ch':
            where[-1] += reg[1]
        row.update(ratio=float(r.reshape(-1)[flat]), where=where)
        rows.append(row)
        if bad:
            failures.append({'op': info['name'], 'index': n, 'out': label, 'rules': bad, 'ratio': row['ratio'],
                             'where': where, 'class': cls})
        _view(it.bufs[b], reg)[...] = _view(bufs[b], reg)           # later ops read the GPU's values

    def pooled(op, m, reg):
        """M of an output region: the 7x7 max for the convolutions, cut to the region's channels."""
        if m is None:
            return None
        if op.kind in (OP_CONV, OP_PAIR1X1, OP_STEM):
            m = _pool7(m)
        return m[..., :reg[2] - reg[1]] if reg[0] == 'ch' else m

    for j, (n, op, info) in enumerate(ops):
        cls = op_class(prog, op, info)
        if in_place(op) and op.out_buf in carry_cls:       # the chain is one unit: the looser class of its ops
            cls = max(cls, carry_cls[op.out_buf], key=lambda c: tol[c])
        outs = written(op)
        fp32_out = any(prog['bufs'][b][4] == DT_F32 for b, _ in outs)
        later = any(in_place(o) and o.out_buf == op.out_buf for _m, o, _i in ops[j + 1:])
        mags = _magnitudes(it, op, info, img_u8, carry) if (fp32_out or later) else {}
        in_absmax = float(it.bufs[op.in_buf].abs().max()) if op.in_buf >= 0 else 0.0
        it.step(op, info, img_u8)
        if later:
            # the GPU's buffer no longer holds this op's result: the interpreter's value (and its magnitude) flows into the
            # in-place successor, which compares the chain; channels the successor does not write are compared behind it
            b, reg = outs[0]
            m = torch.zeros(it.bufs[b].shape, dtype=torch.float64)
            _view(m, reg)[...] = mags['out'][..., :reg[2] - reg[1]]
            carry[b] = m
            carry_cls[b] = cls
            pending.setdefault(b, []).append((n, op, info, cls, reg, mags['out'], in_absmax))
            chained += 1
            continue
        for label, (b, reg) in zip(('out', 'aux'), outs):
            compare(n, op, info, cls, label, b, reg, pooled(op, mags.get(label), reg), in_absmax)
        if in_place(op) and op.out_buf in pending:
            reg_i = outs[0][1]
            for (pn, pop, pinfo, pcls, preg, pm, pabs) in pending.pop(op.out_buf):
                # the part of a chained predecessor's output that this op left alone
                for c0, c1 in ((preg[1], min(preg[2], reg_i[1])), (max(preg[1], reg_i[2]), preg[2])):
                    if c1 > c0:
                        pm_full = pooled(pop, pm, preg)
                        compare(pn, pop, pinfo, pcls, 'out', op.out_buf, ('ch', c0, c1),
                                pm_full[..., c0 - preg[1]:c1 - preg[1]], pabs)
            carry.pop(op.out_buf, None)
            carry_cls.pop(op.out_buf, None)
        checked += 1
    assert not pending, 'in-place chains without their last op: %s' % sorted(pending)

    # channels (and flat tails) no op writes: still exactly 0.0
    regions = {}
    for op in prog['ops']:
        if op.kind in FRAME_LOCAL:
            for b, reg in written(op):
                regions.setdefault(b, []).append(reg)
        else:                                          # point heads etc.: unknown layout, the buffers it touches are left out
            for b in (op.out_buf, op.aux_buf, op.res_buf):
                if b >= 0:
                    regions.setdefault(b, []).append(('all',))
    zero_checked = 0
    for b, t in enumerate(bufs):
        regs = regions.get(b, [])
        if any(r[0] == 'all' for r in regs):
            continue
        free = torch.ones(t.shape[1:], dtype=torch.bool)
        for reg in regs:
            if reg[0] == 'ch':
                free[..., reg[1]:reg[2]] = False
            else:
                free.view(-1)[:reg[1]] = False
        if not bool(free.any()):
            continue
        zero_checked += 1
        stray = (t[:, free] != 0)
        if bool(stray.any()):
            f, i = [int(v) for v in torch.nonzero(stray)[0]]
            pos = [int(v) for v in torch.nonzero(free)[i]]
            failures.append({'buf': b, 'rules': ['zero'], 'count': int(stray.sum()), 'where': [frames[f]] + pos,
                             'value': float(t[f][tuple(pos)])})
    return {'rows': rows, 'checked': checked, 'chained': chained, 'worst_frac_16bit': worst['frac'], 'failures': failures,
            'zero_checked_buffers': zero_checked}


def worst_by_class(rows):
    """{class: worst ratio} over check_program rows (the report of the measured tolerances)."""
    out = {}
    for r in rows:
        key = r['class'] if r['rule'] != 'ulp16' else r['class'] + '_ulp16'
        out[key] = max(out.get(key, 0.0), r['ratio'])
    return out
