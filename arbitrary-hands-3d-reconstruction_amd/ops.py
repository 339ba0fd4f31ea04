"""Stand-alone operator wrappers over the C ABI (NHWC fp32 device tensors in, device tensors out).
Same kernels the resident program uses; handy for parity tests and for embedding single ops."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .packer import (DT_BF16, DT_F16, PRECISIONS, pack_conv, pack_conv_h16, pack_conv_x3, pack_stem, pack_wino3, n_tiles_for,
                     winograd_weights, winograd2d_weights, winograd24_weights, polyphase2_weights)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _s(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.AcrmiError('device tensors required: libacrmi has no CPU path')


def to_nhwc(x_nchw, cs=None, device='cuda'):
    """[B,C,H,W] (any device) -> contiguous NHWC on `device` with channel stride cs (zero padded)."""
    B, Cc, H, W = x_nchw.shape
    cs = cs or (Cc + 3) // 4 * 4
    out = torch.zeros(B, H, W, cs, dtype=torch.float32, device=device)
    out[..., :Cc] = x_nchw.permute(0, 2, 3, 1).to(device)
    return out


def conv2d(x, weight, bias=None, stride=1, relu=False, residual=None, groups=1, cin=None, in_coff=0, out=None,
           out_coff=0, out_cs=None, frame_bias=None, algo='direct'):
    """x: NHWC [B,H,W,cs] device fp32; weight: [Cout_total, Cin/groups, k, k] (torch/numpy, host or device);
    padding = k//2 (the only padding the ACR network uses).  Returns NHWC [B,Ho,Wo,out_cs].
    residual: [B,Ho,Wo,rcs] added before the ReLU, or [1,Ho,Wo,rcs] = one map added to EVERY frame
    (ACRMI_CONV_BIAS_MAP: the position-bias map of the head convs; not with 'winograd2d_lds')."""
    _need_cuda(x, residual, out, frame_bias)
    w = weight.detach().cpu().numpy() if hasattr(weight, 'detach') else np.asarray(weight)
    cout_t, cin_g, k, _ = w.shape
    cout = cout_t // groups
    b = np.zeros(cout_t, np.float32) if bias is None else (
        bias.detach().cpu().numpy() if hasattr(bias, 'detach') else np.asarray(bias))
    if algo in ('split16', 'split_bf16'):
        if k not in (1, 3) or stride not in (1, 2) or (k == 1 and stride != 1):
            raise ValueError('the split-operand kernels are for 3x3 (stride 1 or 2) and 1x1 stride-1 convolutions')
        tr = None
    elif algo == 'polyphase2':
        if k != 3 or stride != 2:
            raise ValueError('the polyphase kernel is for 3x3 stride-2 convolutions')
        tr = polyphase2_weights
    elif algo in ('winograd', 'winograd2d', 'winograd2d_lds', 'winograd24'):
        if k != 3 or stride != 1:
            raise ValueError('winograd needs a 3x3 stride-1 convolution')
        tr = {'winograd': winograd_weights, 'winograd24': winograd24_weights}.get(algo, winograd2d_weights)
    elif algo == 'direct':
        tr = lambda t: t
    else:
        raise ValueError('algo must be "direct", "winograd", "winograd2d", "winograd2d_lds", "winograd24", "polyphase2", "split16" or "split_bf16"')
    algo_id = {'direct': 0, 'winograd': 1, 'winograd2d': 2, 'winograd2d_lds': 3, 'winograd24': 4, 'polyphase2': 5, 'split16': 6, 'split_bf16': 7}[algo]
    if algo_id == 3:
        if groups != 1 or cout != 32 or cin_g > 32:
            raise ValueError('winograd2d_lds needs groups = 1, Cout = 32, Cin <= 32')
        packed = [pack_wino3(w.astype(np.float64), b)]
    elif algo_id in (6, 7):
        packed = [pack_conv_x3([(w[g * cout:(g + 1) * cout].astype(np.float64), b[g * cout:(g + 1) * cout]) for g in range(groups)],
                               DT_BF16 if algo_id == 7 else DT_F16)]
    else:
        packed = [pack_conv(tr(w[g * cout:(g + 1) * cout].astype(np.float64)), b[g * cout:(g + 1) * cout])
                  for g in range(groups)]
    wp = torch.from_numpy(np.concatenate([p[0] for p in packed])).to(x.device)
    bp = torch.from_numpy(np.concatenate([p[1] for p in packed])).to(x.device)
    B, H, W, cs = x.shape
    cin = cin_g if cin is None else cin
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if out is None:
        out_cs = out_cs or (cout_t + 3) // 4 * 4
        out = torch.zeros(B, Ho, Wo, out_cs, dtype=torch.float32, device=x.device)
    bias_t, fstride = bp, 0
    if frame_bias is not None:
        bias_t, fstride = frame_bias.contiguous(), frame_bias.shape[-1]
    if residual is not None and residual.shape[0] == 1 and B > 1:
        algo_id |= _lib.CONV_BIAS_MAP
    L = _lib.lib()
    _lib.check(L.acrmi_conv2d(_p(x), B, H, W, cs, in_coff, cin, _p(wp), _p(bias_t), fstride, _p(residual),
                              residual.shape[-1] if residual is not None else 0, 0, _p(out), out.shape[-1], out_coff,
                              cout, k, stride, int(relu), groups, algo_id, _s(x)))
    return out


def conv2d_group(problems):
    """Up to two INDEPENDENT 3x3 stride-1 convolutions on the F(2x4,3x3) kernel as ONE launch (acrmi_conv2d_group): the
    second problem's work items follow the first's inside the persistent workgroups.  problems: dicts with x (NHWC fp32
    [B,H,W,cs] on the device) and weight ([Cout, Cin, 3, 3]), optionally bias, relu, residual ([B,H,W,rcs]) and frame_bias
    ([B, >= Cout rounded up to 64]).  Returns the outputs; each is bit-identical to conv2d(..., algo='winograd24').  Two
    problems that do not run on one kernel instantiation with a group form raise (there is no pair of launches instead)."""
    arr = (_lib.ConvProblem * len(problems))()
    outs, keep = [], []
    for q, pr in zip(arr, problems):
        x, residual, frame_bias = pr['x'], pr.get('residual'), pr.get('frame_bias')
        _need_cuda(x, residual, frame_bias)
        w = pr['weight']
        w = w.detach().cpu().numpy() if hasattr(w, 'detach') else np.asarray(w)
        cout, cin, k, _ = w.shape
        if k != 3:
            raise ValueError('conv2d_group takes 3x3 stride-1 convolutions')
        b = pr.get('bias')
        b = np.zeros(cout, np.float32) if b is None else (b.detach().cpu().numpy() if hasattr(b, 'detach') else np.asarray(b))
        wp, bp = pack_conv(winograd24_weights(w.astype(np.float64)), b)
        wp, bp = torch.from_numpy(wp).to(x.device), torch.from_numpy(bp).to(x.device)
        B, H, W, cs = x.shape
        out = torch.zeros(B, H, W, (cout + 3) // 4 * 4, dtype=torch.float32, device=x.device)
        bias_t, fstride = (bp, 0) if frame_bias is None else (frame_bias.contiguous(), frame_bias.shape[-1])
        keep += [wp, bp, bias_t]
        q.in_, q.w_packed, q.bias, q.res, q.out = [t.data_ptr() if t is not None else None for t in (x, wp, bias_t, residual, out)]
        q.B, q.H, q.W, q.in_cs, q.in_coff, q.cin = B, H, W, cs, 0, cin
        q.bias_frame_stride, q.res_cs, q.res_coff = fstride, (residual.shape[-1] if residual is not None else 0), 0
        q.out_cs, q.out_coff, q.cout, q.ksize, q.stride, q.relu, q.groups, q.algo = out.shape[-1], 0, cout, 3, 1, int(bool(pr.get('relu'))), 1, 4
        outs.append(out)
    _lib.check(_lib.lib().acrmi_conv2d_group(arr, len(problems), _s(problems[0]['x'])))
    return outs


def conv2d_splitk(x, weight, bias=None, splits=2, relu=False, residual=None, in_coff=0, out=None, out_coff=0, out_cs=None,
                  workspace=None):
    """3x3 stride-1 convolution as Winograd F(2x2,3x3) with the input channels split into `splits` slices that run as
    separate work items and meet in `workspace` (acrmi_conv2d_splitk; the small-batch form of the low-resolution HRNet
    branches).  x NHWC fp32 [B,H,W,cs]; weight [Cout, Cin, 3, 3] with Cin = splits * (a multiple of 32, >= 64).
    workspace: zeroed uint8 device tensor of conv2d_splitk_workspace() bytes (allocated here when None)."""
    _need_cuda(x, residual, out, workspace)
    w = weight.detach().cpu().numpy() if hasattr(weight, 'detach') else np.asarray(weight)
    cout, cin, k, _ = w.shape
    if k != 3 or cin % splits:
        raise ValueError('split-K needs a 3x3 convolution whose Cin is a multiple of the slice count')
    ks = cin // splits
    b = np.zeros(cout, np.float32) if bias is None else (
        bias.detach().cpu().numpy() if hasattr(bias, 'detach') else np.asarray(bias))
    packed = [pack_conv(winograd2d_weights(w[:, s * ks:(s + 1) * ks].astype(np.float64)), b) for s in range(splits)]
    wp = torch.from_numpy(np.concatenate([p[0] for p in packed])).to(x.device)
    bp = torch.from_numpy(np.concatenate([p[1] for p in packed])).to(x.device)
    B, H, W, cs = x.shape
    if out is None:
        out_cs = out_cs or (cout + 3) // 4 * 4
        out = torch.zeros(B, H, W, out_cs, dtype=torch.float32, device=x.device)
    L = _lib.lib()
    need = int(L.acrmi_conv2d_splitk_workspace(B, H, W, cout, splits))
    if workspace is None:
        workspace = torch.zeros(need, dtype=torch.uint8, device=x.device)
    _lib.check(L.acrmi_conv2d_splitk(_p(x), B, H, W, cs, in_coff, ks, splits, _p(wp), _p(bp), _p(residual),
                                     residual.shape[-1] if residual is not None else 0, 0, _p(out), out.shape[-1], out_coff,
                                     cout, int(relu), _p(workspace), workspace.numel(), _s(x)))
    return out


def to_nhwc16(x_nchw, precision='fp16', cs=None, device='cuda'):
    """[B,C,H,W] float (any device) -> contiguous NHWC float16 / bfloat16 on `device`, channel stride cs (a multiple
    of 8, zero padded): the activation layout of a 16-bit program."""
    B, Cc, H, W = x_nchw.shape
    cs = cs or (Cc + 7) // 8 * 8
    out = torch.zeros(B, H, W, cs, dtype=torch.float16 if precision == 'fp16' else torch.bfloat16, device=device)
    out[..., :Cc] = x_nchw.permute(0, 2, 3, 1).to(device).to(out.dtype)
    return out


def conv2d_h16(x, weight, bias=None, stride=1, relu=False, residual=None, groups=1, cin=None, in_coff=0, out=None,
               out_coff=0, out_cs=None, frame_bias=None, out_f32=False):
    """The convolution of a 16-bit program (acrmi_conv2d_h16): x NHWC float16 / bfloat16 [B,H,W,cs] on the device,
    weight [Cout_total, Cin/groups, k, k] and bias as float arrays (rounded once to x's type by the packer / kept fp32),
    fp32 accumulation, one rounding of the output.  out_f32: fp32 output and residual (the head exits)."""
    _need_cuda(x, residual, out, frame_bias)
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError('x must be float16 or bfloat16')
    dt = DT_F16 if x.dtype == torch.float16 else DT_BF16
    w = weight.detach().cpu().numpy() if hasattr(weight, 'detach') else np.asarray(weight)
    cout_t, cin_g, k, _ = w.shape
    cout = cout_t // groups
    b = np.zeros(cout_t, np.float32) if bias is None else (
        bias.detach().cpu().numpy() if hasattr(bias, 'detach') else np.asarray(bias))
    packed = [pack_conv_h16(w[g * cout:(g + 1) * cout].astype(np.float64), b[g * cout:(g + 1) * cout], dt) for g in range(groups)]
    wp = torch.from_numpy(np.concatenate([p[0] for p in packed]).view(np.int16)).to(x.device)
    bp = torch.from_numpy(np.concatenate([p[1] for p in packed])).to(x.device)
    B, H, W, cs = x.shape
    cin = cin_g if cin is None else cin
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    odt = torch.float32 if out_f32 else x.dtype
    if out is None:
        q = 4 if out_f32 else 8
        out_cs = out_cs or (cout_t + q - 1) // q * q
        out = torch.zeros(B, Ho, Wo, out_cs, dtype=odt, device=x.device)
    if out.dtype != odt or (residual is not None and residual.dtype != odt):
        raise ValueError('out / residual must be %s' % odt)
    bias_t, fstride = bp, 0
    if frame_bias is not None:
        bias_t, fstride = frame_bias.contiguous().float(), frame_bias.shape[-1]
    _lib.check(_lib.lib().acrmi_conv2d_h16(_p(x), B, H, W, cs, in_coff, cin, _p(wp), _p(bias_t), fstride, _p(residual),
                                           residual.shape[-1] if residual is not None else 0, 0, _p(out), out.shape[-1],
                                           out_coff, cout, k, stride, int(relu), groups, dt, int(bool(out_f32)), _s(x)))
    return out


def preprocess(bgr_frames):
    """uint8 BGR device frames [n,H,W,3] (all the same size) -> (uint8 RGB [n,512,512,3] device, offsets [n,10] host).
    The device counterpart of acr.utils.img_preprocess (reference acr/utils.py:1315-1337)."""
    _need_cuda(bgr_frames)
    if bgr_frames.dtype != torch.uint8 or bgr_frames.dim() != 4 or bgr_frames.shape[-1] != 3:
        raise ValueError('frames must be uint8 [n,H,W,3] BGR')
    n, H, W, _ = bgr_frames.shape
    out = torch.empty(n, 512, 512, 3, dtype=torch.uint8, device=bgr_frames.device)
    offsets = np.zeros((n, 10), np.float32)
    src = bgr_frames.contiguous()          # bound to a local until the call has been queued
    _lib.check(_lib.lib().acrmi_preprocess(_p(src), n, H, W, _p(out), offsets.ctypes.data_as(C.c_void_p), _s(src)))
    return out, torch.from_numpy(offsets)


def _bgr_frames(frames, need_cuda=True):
    """`frames` of preprocess_frames / preprocess_rois (a tensor [N,H,W,3] or a list of [H_i,W_i,3]) -> (acrmi_frame array,
    sizes [(H, W)], device, bound tensors): the counterpart of _nv12_frames.  Layout errors are ValueErrors raised before the
    device is looked at, for preprocess_frames too, which used to look at the device first (need_cuda=False: the caller has
    more to validate first and looks at the device itself)."""
    items = list(frames.unbind(0)) if isinstance(frames, torch.Tensor) and frames.dim() == 4 else list(frames)
    if not items:
        raise ValueError('no frames')
    keep, sizes = [], []
    arr = (_lib.Frame * len(items))()
    for i, f in enumerate(items):
        if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or f.dim() != 3 or f.shape[-1] != 3 or \
                f.device != items[0].device:
            raise ValueError('frames must be uint8 [H,W,3] BGR tensors on one device')
        f = f.contiguous()
        keep.append(f)                     # bound until the call has been queued
        H, W, _ = f.shape
        arr[i].bgr_dev, arr[i].H, arr[i].W = f.data_ptr(), H, W
        sizes.append((H, W))
    if need_cuda:
        _need_cuda(*keep)
    return arr, sizes, keep[0].device, keep


def preprocess_frames(bgr_frames):
    """A list of uint8 BGR device frames [H_i,W_i,3] of ANY sizes -> (uint8 RGB [n,512,512,3] device, offsets [n,10] host) in
    one call (acrmi_preprocess_frames: per-frame geometry in the kernel arguments).  img_preprocess is per image on the
    reference (acr/utils.py:1315-1337); folder mode mixes sizes (acr/main.py:144-205)."""
    arr, sizes, dev, keep = _bgr_frames(bgr_frames)
    n = len(sizes)
    out = torch.empty(n, 512, 512, 3, dtype=torch.uint8, device=dev)
    offsets = np.zeros((n, 10), np.float32)
    _lib.check(_lib.lib().acrmi_preprocess_frames(arr, n, _p(out), offsets.ctypes.data_as(C.c_void_p), _s(out)))
    del keep                               # (held until here: arr holds bare pointers into these tensors)
    return out, torch.from_numpy(offsets)


# ---- NV12 input (csrc/preprocess.hip, csrc/nv12.hip; DESIGN.md "NV12 input") ---------------------------------------------
def nv12_matrix(name_or_row='cv601'):
    """A matrix name ('cv601', 'bt601', 'bt601-full', 'bt709', 'bt709-full': acrmi_nv12_matrix) or a row of six integers
    (cy, cub, cug, cvg, cvr, y_off) -> the row as int32 numpy [6].  Pure host: works without a GPU."""
    if isinstance(name_or_row, str):
        which = _lib.NV12_MATRICES.get(name_or_row)
        if which is None:
            raise ValueError('unknown NV12 matrix %r: one of %s, or a row of six integers' % (name_or_row, sorted(_lib.NV12_MATRICES)))
        row = np.zeros(6, np.int32)
        _lib.check(_lib.lib().acrmi_nv12_matrix(which, row.ctypes.data_as(C.c_void_p)))
        return row
    row = np.asarray(name_or_row.cpu() if hasattr(name_or_row, 'cpu') else name_or_row)
    if row.shape != (6,) or row.dtype.kind not in 'iu' or np.abs(row.astype(np.int64)).max() >= 2 ** 31:
        raise ValueError('an NV12 matrix is a name or six int32 integers (cy, cub, cug, cvg, cvr, y_off)')
    return np.ascontiguousarray(row.astype(np.int32))


def _nv12_plane(t, what, i):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise ValueError('NV12 frame %d: %s must be a uint8 tensor' % (i, what))


def _nv12_item(item, i):
    """One item of `frames` -> (y_ptr, uv_ptr, H, W, y_pitch, uv_pitch, tensors to keep bound).  Strided views are taken as
    they are (pitch = stride(0)); nothing is copied."""
    if isinstance(item, torch.Tensor):                       # [H*3/2, W]: the Y rows, then the UV rows (OpenCV's layout)
        _nv12_plane(item, 'the surface', i)
        if item.dim() != 2 or item.shape[0] % 3:
            raise ValueError('NV12 frame %d: one tensor must be [H*3/2, W], got %s' % (i, tuple(item.shape)))
        H, W = item.shape[0] // 3 * 2, item.shape[1]
        if H < 2 or W < 2 or H % 2 or W % 2:
            raise ValueError('NV12 frame %d: H and W must be even and >= 2, got %d x %d' % (i, H, W))
        if item.stride(1) != 1 or item.stride(0) < W:
            raise ValueError('NV12 frame %d: rows must be dense (innermost stride 1, pitch >= W), got strides %s' % (i, item.stride()))
        p = item.stride(0)
        return item.data_ptr(), item.data_ptr() + H * p, H, W, p, p, (item,)
    if not isinstance(item, tuple) or len(item) != 2:
        raise ValueError('NV12 frame %d: a uint8 tensor [H*3/2, W] or a tuple (y [H,W], uv [H/2,W] or [H/2,W/2,2])' % i)
    y, uv = item
    _nv12_plane(y, 'y', i)
    _nv12_plane(uv, 'uv', i)
    if y.dim() != 2:
        raise ValueError('NV12 frame %d: y must be [H,W], got %s' % (i, tuple(y.shape)))
    H, W = y.shape
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError('NV12 frame %d: H and W must be even and >= 2, got %d x %d' % (i, H, W))
    if tuple(uv.shape) not in ((H // 2, W), (H // 2, W // 2, 2)):
        raise ValueError('NV12 frame %d: uv must be [H/2,W] or [H/2,W/2,2] for y %s, got %s' % (i, tuple(y.shape), tuple(uv.shape)))
    if y.stride(1) != 1 or y.stride(0) < W:
        raise ValueError('NV12 frame %d: y rows must be dense (innermost stride 1, pitch >= W), got strides %s' % (i, y.stride()))
    inner_ok = uv.stride(-1) == 1 and (uv.dim() == 2 or W == 2 or uv.stride(1) == 2)
    uv_pitch = uv.stride(0) if H > 2 else W                  # (a single row has no pitch to speak of)
    if not inner_ok or uv_pitch < W:
        raise ValueError('NV12 frame %d: uv rows must be dense interleaved U, V bytes (pitch >= W), got strides %s' % (i, uv.stride()))
    if y.device != uv.device:
        raise ValueError('NV12 frame %d: y and uv are on different devices' % i)
    return y.data_ptr(), uv.data_ptr(), H, W, y.stride(0), uv_pitch, (y, uv)


def _nv12_frames(frames, need_cuda=True):
    """`frames` of preprocess_nv12 / nv12_to_bgr -> (acrmi_nv12_frame array, sizes [(H, W)], device, bound tensors).  Layout
    errors are ValueErrors raised before the device is looked at (need_cuda=False: the caller has more to validate first and
    looks at the device itself)."""
    if isinstance(frames, torch.Tensor) and frames.dim() == 3:       # [n, H*3/2, W]: n surfaces of one size
        items = list(frames.unbind(0))
    elif isinstance(frames, (torch.Tensor, tuple)):                  # a single item: a batch of one
        items = [frames]
    else:
        items = list(frames)
    if not items:
        raise ValueError('no frames')
    arr = (_lib.NV12Frame * len(items))()
    keep, sizes = [], []
    for i, item in enumerate(items):
        yp, uvp, H, W, ypitch, uvpitch, bound = _nv12_item(item, i)
        if max(ypitch, uvpitch) >= 2 ** 31:
            raise ValueError('NV12 frame %d: pitch beyond int32' % i)
        arr[i].y_dev, arr[i].uv_dev, arr[i].H, arr[i].W, arr[i].y_pitch, arr[i].uv_pitch = yp, uvp, H, W, ypitch, uvpitch
        keep.extend(bound)                                           # bound until the call has been queued
        sizes.append((H, W))
    if any(t.device != keep[0].device for t in keep):
        raise ValueError('NV12 frames must all be on one device')
    if need_cuda:
        _need_cuda(*keep)
    return arr, sizes, keep[0].device, keep


def preprocess_nv12(frames, matrix='cv601'):
    """NV12 frames in HBM -> (uint8 RGB [n,512,512,3] device, offsets [n,10] host) in one call (acrmi_preprocess_nv12): colour
    conversion by the integer rule of include/acrmi.h, white square pad and OpenCV's cubic resize fused - byte for byte
    preprocess_frames(nv12_to_bgr(frames)), without the full-resolution frame.
    frames: a list whose items are each one uint8 device tensor [H*3/2, W] (the Y rows, then the interleaved UV rows: OpenCV's
    layout) or a TUPLE (y [H,W], uv [H/2,W] or [H/2,W/2,2]); one such item alone is a batch of one, a tensor [n,H*3/2,W] is n
    frames.  H, W even.  Rows may be strided views (innermost stride 1, pitch = stride(0)): nothing is copied.
    matrix: a name or six integers (nv12_matrix)."""
    coef = nv12_matrix(matrix)
    arr, sizes, dev, keep = _nv12_frames(frames)
    n = len(sizes)
    out = torch.empty(n, 512, 512, 3, dtype=torch.uint8, device=dev)
    offsets = np.zeros((n, 10), np.float32)
    _lib.check(_lib.lib().acrmi_preprocess_nv12(arr, n, coef.ctypes.data_as(C.c_void_p), _p(out),
                                                offsets.ctypes.data_as(C.c_void_p), _s(out)))
    del keep
    return out, torch.from_numpy(offsets)


def nv12_to_bgr(frames, matrix='cv601', rgb=False):
    """NV12 frames (as preprocess_nv12 takes them) -> the full-resolution uint8 frames, BGR (RGB with rgb=True), by the same
    integer rule (acrmi_nv12_to_rgb): a tensor [n,H,W,3] when all sizes agree, otherwise a list of [H_i,W_i,3] in input order."""
    coef = nv12_matrix(matrix)
    arr, sizes, dev, keep = _nv12_frames(frames)
    n = len(sizes)
    if all(s == sizes[0] for s in sizes):
        out = torch.empty(n, sizes[0][0], sizes[0][1], 3, dtype=torch.uint8, device=dev)
        dst = [out[i] for i in range(n)]
    else:
        out = dst = [torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for H, W in sizes]
    ptrs = (C.c_void_p * n)(*[d.data_ptr() for d in dst])
    _lib.check(_lib.lib().acrmi_nv12_to_rgb(arr, n, coef.ctypes.data_as(C.c_void_p), 0 if rgb else 1, ptrs, _s(dst[0])))
    del keep
    return out


# ---- NV12 output (csrc/nv12_out.hip, csrc/nv12_out_plan.h; DESIGN.md "NV12 output") --------------------------------------
def nv12_out_matrix(name_or_row='cv601'):
    """A matrix name (those of nv12_matrix: acrmi_nv12_out_matrix) or a row of ten integers (cry, cgy, cby, cru, cgu, cbu, crv,
    cgv, cbv, y_off) -> the row as int32 numpy [10].  Pure host: works without a GPU."""
    if isinstance(name_or_row, str):
        which = _lib.NV12_MATRICES.get(name_or_row)
        if which is None:
            raise ValueError('unknown NV12 matrix %r: one of %s, or a row of ten integers' % (name_or_row, sorted(_lib.NV12_MATRICES)))
        row = np.zeros(10, np.int32)
        _lib.check(_lib.lib().acrmi_nv12_out_matrix(which, row.ctypes.data_as(C.c_void_p)))
        return row
    row = np.asarray(name_or_row.cpu() if hasattr(name_or_row, 'cpu') else name_or_row)
    if row.shape != (10,) or row.dtype.kind not in 'iu' or int(row.min()) < -2 ** 31 or int(row.max()) >= 2 ** 31:
        raise ValueError('an NV12 output matrix is a name or ten int32 integers (cry, cgy, cby, cru, cgu, cbu, crv, cgv, cbv, y_off)')
    return np.ascontiguousarray(row.astype(np.int32))


def _nv12_matrix_pair(matrix='cv601'):
    """`matrix` of nv12_compose: a name, which selects the input and the output row, or a pair (row6, row10), each a name or a
    row of integers -> (int32 [6], int32 [10])."""
    if isinstance(matrix, str):
        return nv12_matrix(matrix), nv12_out_matrix(matrix)
    if isinstance(matrix, (tuple, list)) and len(matrix) == 2 and not all(isinstance(v, (int, np.integer)) for v in matrix):
        return nv12_matrix(matrix[0]), nv12_out_matrix(matrix[1])
    raise ValueError('matrix must be a name or a pair (row of six integers, row of ten integers): the input and the output rule')


def _nv12_surfaces(out, sizes, dev, what):
    """`out=` of bgr_to_nv12 / nv12_compose (surfaces to write into, in the layouts of _nv12_frames), or None: new tight
    surfaces - one tensor [n, H*3/2, W] when all sizes agree, else a list -> (what the call returns, acrmi_nv12_surface array,
    bound tensors)."""
    n = len(sizes)
    if out is None:
        if all(s == sizes[0] for s in sizes):
            out = torch.empty(n, sizes[0][0] * 3 // 2, sizes[0][1], dtype=torch.uint8, device=dev)
        else:
            out = [torch.empty(H * 3 // 2, W, dtype=torch.uint8, device=dev) for H, W in sizes]
    arr, out_sizes, out_dev, keep = _nv12_frames(out, need_cuda=False)
    if out_sizes != sizes:
        raise ValueError('%s: out= holds surfaces of %s (H, W), the frames are %s' % (what, out_sizes, sizes))
    if out_dev != dev:
        raise ValueError('%s: out= is on another device than the frames' % what)
    su = (_lib.NV12Surface * n)()
    for i in range(n):
        su[i].y_dev, su[i].uv_dev, su[i].H, su[i].W = arr[i].y_dev, arr[i].uv_dev, arr[i].H, arr[i].W
        su[i].y_pitch, su[i].uv_pitch = arr[i].y_pitch, arr[i].uv_pitch
    return out, su, keep


def _even_sizes(sizes, what):
    for i, (H, W) in enumerate(sizes):
        if H < 2 or W < 2 or H % 2 or W % 2:
            raise ValueError('%s: frame %d: NV12 needs H and W even and >= 2, got %d x %d' % (what, i, H, W))


def bgr_to_nv12(frames, matrix='cv601', bgr=True, out=None):
    """Packed uint8 device frames - a tensor [n,H,W,3] or a list of [H_i,W_i,3] of different sizes, BGR (RGB with bgr=False) -> NV12
    surfaces by the integer rule of include/acrmi.h (acrmi_rgb_to_nv12): luma per pixel, chroma from the mean of each 2x2 block.
    H, W even.  matrix: a name, a row of ten integers, or the pair nv12_compose takes (its output row is used).
    -> one uint8 tensor [n, H*3/2, W] (the Y rows, then the interleaved UV rows: what preprocess_nv12 takes) when all sizes
    agree, else a list of [H_i*3/2, W_i] in input order; or `out`: surfaces to write into, in any layout preprocess_nv12
    accepts (strided views are taken as they are, pitch = stride(0); nothing beyond W bytes of a row is written)."""
    if isinstance(matrix, str) or (isinstance(matrix, (tuple, list)) and len(matrix) == 2):
        coef = _nv12_matrix_pair(matrix)[1]
    else:
        coef = nv12_out_matrix(matrix)
    src, sizes, dev, keep = _bgr_frames(frames, need_cuda=False)
    _even_sizes(sizes, 'bgr_to_nv12')
    out, su, keep_out = _nv12_surfaces(out, sizes, dev, 'bgr_to_nv12')
    _need_cuda(*keep)
    n = len(sizes)
    ptrs = (C.c_void_p * n)(*[src[i].bgr_dev for i in range(n)])
    _lib.check(_lib.lib().acrmi_rgb_to_nv12(ptrs, su, n, coef.ctypes.data_as(C.c_void_p), 1 if bgr else 0, _s(keep[0])))
    del keep, keep_out
    return out


def nv12_compose(surfaces, drawn, matrix='cv601', bgr=True, out=None):
    """The drawn frames `drawn` (as bgr_to_nv12 takes them) over the NV12 surfaces they were drawn from (as preprocess_nv12
    takes them): new bytes only where a drawn pixel differs from what nv12_to_bgr makes of the surface, the surface's own bytes
    everywhere else (acrmi_nv12_compose) - nv12_compose(s, nv12_to_bgr(s)) is s, byte for byte.  matrix: a name, or a pair
    (row6, row10) of the input and the output rule.  -> as bgr_to_nv12; out= may be `surfaces` itself (in place)."""
    coef6, coef10 = _nv12_matrix_pair(matrix)
    arr, sizes, dev, keep = _nv12_frames(surfaces, need_cuda=False)
    src, drawn_sizes, drawn_dev, keep_drawn = _bgr_frames(drawn, need_cuda=False)
    if drawn_sizes != sizes:
        raise ValueError('nv12_compose: the drawn frames are %s (H, W), the surfaces %s' % (drawn_sizes, sizes))
    if drawn_dev != dev:
        raise ValueError('nv12_compose: the drawn frames are on another device than the surfaces')
    out, su, keep_out = _nv12_surfaces(out, sizes, dev, 'nv12_compose')
    _need_cuda(*keep)
    n = len(sizes)
    ptrs = (C.c_void_p * n)(*[src[i].bgr_dev for i in range(n)])
    _lib.check(_lib.lib().acrmi_nv12_compose(arr, ptrs, su, n, coef6.ctypes.data_as(C.c_void_p), coef10.ctypes.data_as(C.c_void_p),
                                            1 if bgr else 0, _s(keep[0])))
    del keep, keep_drawn, keep_out
    return out


# ---- regions of interest (csrc/preprocess.hip, csrc/roi_plan.h; DESIGN.md "Regions of interest") ---------------------
def _roi_int_box(H, W, box, i=0):
    """(l, t, r, b), ints or floats -> the integer box with the same crop amounts: the reference turns a bbox into
    crop_trbl = (int(max(0, t)), int(max(0, W - r)), int(max(0, H - b)), int(max(0, l))) (acr/utils.py:1289-1292), int()
    truncating, so r = 100.7 in a 200-wide frame crops 99 on the right."""
    vals = np.asarray(box.cpu() if hasattr(box, 'cpu') else box)
    if vals.shape != (4,) or vals.dtype.kind not in 'iuf' or not np.isfinite(vals.astype(np.float64)).all():
        raise ValueError('region %d: a box is four finite numbers (l, t, r, b), got %r' % (i, box))
    l, t, r, b = (v.item() for v in vals)
    cap = 2 ** 30      # a crop beyond the frame leaves no pixel whatever its size: keep the integers within int32
    ct, cr, cb, cl = (min(int(max(0, v)), cap) for v in (t, W - r, H - b, l))
    return cl, ct, W - cr, H - cb


def roi_offsets(H, W, box):
    """The `offsets` row float32 numpy [10] = [padded h, padded w, crop t, r, b, l, pad t, r, b, l] of the box (l, t, r, b),
    r and b exclusive, in an H x W frame (acrmi_roi_offsets; the reference's image_crop_pad with a bbox, acr/utils.py:1287-1301).
    A box that leaves no pixel of the frame is a ValueError.  Pure host: works without a GPU."""
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        raise ValueError('the frame must have pixels, got %d x %d' % (H, W))
    roi = _lib.Roi(0, *_roi_int_box(H, W, box))
    row = np.zeros(10, np.float32)
    _lib.check(_lib.lib().acrmi_roi_offsets(H, W, C.byref(roi), None, row.ctypes.data_as(C.c_void_p)))
    return row


def _rois(boxes, box_frame, sizes):
    """boxes [n,4], box_frame [n] or None, the frames' [(H, W)] -> the acrmi_roi array."""
    boxes = boxes.cpu() if hasattr(boxes, 'cpu') else boxes
    boxes = [np.asarray(b) for b in boxes] if isinstance(boxes, (list, tuple)) else np.asarray(boxes)
    n = len(boxes)
    if n == 0 or any(np.shape(b) != (4,) for b in boxes):
        raise ValueError('boxes must be [n,4] rows (l, t, r, b), n >= 1')
    if box_frame is None:
        if n != len(sizes):
            raise ValueError('box_frame is needed when there is not one box per frame (%d boxes, %d frames)' % (n, len(sizes)))
        frame_of = list(range(n))
    else:
        bf = np.asarray(box_frame.cpu() if hasattr(box_frame, 'cpu') else box_frame)
        if bf.shape != (n,) or bf.dtype.kind not in 'iu':
            raise ValueError('box_frame must hold one integer per box')
        frame_of = [int(f) for f in bf]
    arr = (_lib.Roi * n)()
    for i, f in enumerate(frame_of):
        if not 0 <= f < len(sizes):
            raise ValueError('region %d: frame index %d outside [0, %d)' % (i, f, len(sizes)))
        arr[i] = _lib.Roi(f, *_roi_int_box(sizes[f][0], sizes[f][1], boxes[i], i))
    return arr


def preprocess_rois(frames, boxes, box_frame=None, pixel_format='bgr', matrix='cv601'):
    """Regions of frames in HBM -> (uint8 RGB [n,512,512,3] device, offsets [n,10] host) in one call (acrmi_preprocess_rois /
    acrmi_preprocess_rois_nv12): region i is the box boxes[i] = (l, t, r, b), r and b exclusive, of frame box_frame[i], clamped
    to that frame, and is pre-processed as a frame of its own size - byte for byte preprocess_frames on a copy of the window,
    without the copy.  Its offsets row carries the crop, so pj2d_org lands in the pixels of the original frame.
    frames: what preprocess / preprocess_frames take ('bgr': a uint8 tensor [N,H,W,3] or a list of [H_i,W_i,3]) or what
    preprocess_nv12 takes ('nv12', with `matrix`).  box_frame: integers [n], default arange(n), which needs one box per frame;
    frames may repeat, be skipped and come in any order.  Float boxes become crop amounts by the reference's
    int(max(0, .)) truncation.  A box that leaves no pixel of its frame is a ValueError that names the region."""
    L = _lib.lib()
    if pixel_format == 'nv12':
        coef = nv12_matrix(matrix)
        arr, sizes, dev, keep = _nv12_frames(frames, need_cuda=False)
    elif pixel_format != 'bgr':
        raise ValueError("pixel_format must be 'bgr' or 'nv12', got %r" % (pixel_format,))
    else:
        arr, sizes, dev, keep = _bgr_frames(frames, need_cuda=False)
    rois = _rois(boxes, box_frame, sizes)      # layouts, boxes and frame indices are ValueErrors before the device is looked at
    _need_cuda(*keep)
    n = len(rois)
    out = torch.empty(n, 512, 512, 3, dtype=torch.uint8, device=dev)
    offsets = np.zeros((n, 10), np.float32)
    if pixel_format == 'nv12':
        _lib.check(L.acrmi_preprocess_rois_nv12(arr, len(sizes), rois, n, coef.ctypes.data_as(C.c_void_p), _p(out),
                                                offsets.ctypes.data_as(C.c_void_p), _s(out)))
    else:
        _lib.check(L.acrmi_preprocess_rois(arr, len(sizes), rois, n, _p(out), offsets.ctypes.data_as(C.c_void_p), _s(out)))
    del keep
    return out, torch.from_numpy(offsets)


# ---- tracking on the device (csrc/track.hip, csrc/track_plan.h, csrc/preprocess.hip; DESIGN.md "Tracking on the device") ----
def _raw_stream(stream, device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream) if stream is None else C.c_void_p(stream)


def _device_boxes(boxes):
    """The boxes of preprocess_rois_device: a contiguous int32 tensor [n,4], n >= 1 (its device is looked at later)."""
    if not isinstance(boxes, torch.Tensor) or boxes.dtype != torch.int32 or boxes.dim() != 2 or boxes.shape[1] != 4 or \
            boxes.shape[0] < 1 or not boxes.is_contiguous():
        raise ValueError('boxes must be a contiguous int32 CUDA tensor [n,4], n >= 1 (host, float or list boxes: ops.preprocess_rois)')
    return boxes.shape[0]


def _box_frames(box_frame, n, n_frames):
    """box_frame (host integers [n], or None = frame i, one box per frame) -> int32 numpy [n] or None."""
    if box_frame is None:
        if n != n_frames:
            raise ValueError('box_frame is needed when there is not one box per frame (%d boxes, %d frames)' % (n, n_frames))
        return None
    if isinstance(box_frame, torch.Tensor) and box_frame.is_cuda:
        raise ValueError('box_frame is a host list of integers')
    bf = np.asarray(box_frame)
    if bf.shape != (n,) or bf.dtype.kind not in 'iu':
        raise ValueError('box_frame must hold one integer per box')
    for i, f in enumerate(bf):
        if not 0 <= int(f) < n_frames:
            raise ValueError('region %d: frame index %d outside [0, %d)' % (i, int(f), n_frames))
    return np.ascontiguousarray(bf, dtype=np.int32)


def _track_out(t, shape, dtype, dev, name):
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != dev:
        raise ValueError('%s must be a contiguous %s tensor %s on the frames\' device' % (name, dtype, tuple(shape)))
    return t


def region_frame_sizes(frames, box_frame=None, pixel_format='bgr'):
    """(H, W) of the frame of every region, as track_boxes takes it: one pair when all frames have one size, else a list of
    one pair per region."""
    if pixel_format == 'nv12':
        sizes = _nv12_frames(frames, need_cuda=False)[1]
    elif isinstance(frames, torch.Tensor) and frames.dim() == 4:
        sizes = [tuple(frames.shape[1:3])] * frames.shape[0]
    else:
        sizes = [tuple(f.shape[:2]) for f in frames]
    if all(s == sizes[0] for s in sizes):
        return tuple(int(v) for v in sizes[0])
    return [sizes[int(f)] for f in (range(len(sizes)) if box_frame is None else box_frame)]


def whole_frame_boxes(frames, pixel_format='bgr'):
    """The box (0, 0, W, H) of every frame as the int32 device tensor [n_frames,4] preprocess_rois_device takes: the first
    frames of a video, before there are key points to track."""
    if pixel_format not in ('bgr', 'nv12'):
        raise ValueError("pixel_format must be 'bgr' or 'nv12', got %r" % (pixel_format,))
    _, sizes, dev, keep = (_nv12_frames if pixel_format == 'nv12' else _bgr_frames)(frames, need_cuda=False)
    _need_cuda(*keep)
    return torch.tensor([[0, 0, W, H] for H, W in sizes], dtype=torch.int32).to(dev)


def preprocess_rois_device(frames, boxes, box_frame=None, pixel_format='bgr', matrix='cv601', out=None, offsets=None, status=None,
                           stream=None):
    """preprocess_rois with the boxes in DEVICE memory (acrmi_preprocess_rois_dev / acrmi_preprocess_rois_nv12_dev): region i
    is the box boxes[i] of frame box_frame[i], boxes a contiguous int32 CUDA tensor [n,4] on the frames' device - what
    track_boxes wrote, never seen by the host.  -> (uint8 RGB [n,512,512,3], offsets float32 [n,10], status int32 [n]), all on
    the device.  The kernel clamps every box to its frame itself; a box that leaves no pixel cannot be refused here, it takes
    the whole frame and its status is 1 (0: the box as given).  The bytes and the offsets rows are those of preprocess_rois
    for the same boxes.  box_frame: host integers, as preprocess_rois.  out / offsets / status: tensors to write into.
    stream: a raw hipStream_t to queue on instead of the current stream.  Nothing here waits for the device."""
    if pixel_format == 'nv12':
        coef = nv12_matrix(matrix)
        arr, sizes, dev, keep = _nv12_frames(frames, need_cuda=False)
    elif pixel_format != 'bgr':
        raise ValueError("pixel_format must be 'bgr' or 'nv12', got %r" % (pixel_format,))
    else:
        arr, sizes, dev, keep = _bgr_frames(frames, need_cuda=False)
    n = _device_boxes(boxes)
    bf = _box_frames(box_frame, n, len(sizes))
    if not boxes.is_cuda or boxes.device != dev:
        raise ValueError('boxes must be a contiguous int32 CUDA tensor [n,4] on the frames\' device (host boxes: ops.preprocess_rois)')
    _need_cuda(*keep)
    out = _track_out(out, (n, 512, 512, 3), torch.uint8, dev, 'out')
    offsets = _track_out(offsets, (n, 10), torch.float32, dev, 'offsets')
    status = _track_out(status, (n,), torch.int32, dev, 'status')
    bfp = None if bf is None else bf.ctypes.data_as(C.c_void_p)
    L = _lib.lib()
    if pixel_format == 'nv12':
        _lib.check(L.acrmi_preprocess_rois_nv12_dev(arr, len(sizes), bfp, _p(boxes), n, coef.ctypes.data_as(C.c_void_p), _p(out),
                                                    _p(offsets), _p(status), _raw_stream(stream, dev)))
    else:
        _lib.check(L.acrmi_preprocess_rois_dev(arr, len(sizes), bfp, _p(boxes), n, _p(out), _p(offsets), _p(status),
                                               _raw_stream(stream, dev)))
    del keep
    return out, offsets, status


def check_track_args(scale, min_size):
    """scale: a finite number > 0; min_size: an integer >= 1 -> (float, int)."""
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.integer, np.floating)) or not np.isfinite(scale) or scale <= 0:
        raise ValueError('scale must be a finite number > 0, got %r' % (scale,))
    if isinstance(min_size, bool) or not isinstance(min_size, (int, np.integer)) or min_size < 1 or min_size >= 2 ** 31:
        raise ValueError('min_size must be an integer >= 1, got %r' % (min_size,))
    return float(scale), int(min_size)


def _host_frame_hw(frame_hw, n):
    """The host forms of frame_hw -> int numpy (2,) or (n,2); a device tensor -> None.  Does not look at the device."""
    if isinstance(frame_hw, torch.Tensor) and frame_hw.is_cuda:
        return None
    hw = np.asarray(frame_hw.numpy() if isinstance(frame_hw, torch.Tensor) else frame_hw)
    if hw.shape not in ((2,), (n, 2)) or hw.dtype.kind not in 'iu' or (hw <= 0).any() or (hw >= 2 ** 31).any():
        raise ValueError('frame_hw must be (H, W) or one (H, W) per region, positive integers')
    return hw


def frame_hw_device(frame_hw, n, dev):
    """frame_hw of track_boxes -> the int32 device table [n,2]: a device tensor is used as it is; (H, W) is written by two
    fills; one pair per region on the host goes through pinned memory.  No form waits for the device."""
    hw = _host_frame_hw(frame_hw, n)
    if hw is None:
        if frame_hw.dtype != torch.int32 or tuple(frame_hw.shape) != (n, 2) or not frame_hw.is_contiguous() or frame_hw.device != dev:
            raise ValueError('a device frame_hw must be a contiguous int32 tensor [n,2] on the key points\' device')
        return frame_hw
    if hw.shape == (2,):
        t = torch.empty(n, 2, dtype=torch.int32, device=dev)
        t[:, 0] = int(hw[0])
        t[:, 1] = int(hw[1])
        return t
    return torch.from_numpy(np.ascontiguousarray(hw, dtype=np.int32)).pin_memory().to(dev, non_blocking=True)


def track_boxes(pj2d_org, slots, frame_hw, scale=1.5, min_size=64, out=None, stream=None):
    """The boxes of the NEXT frame from the key points of this one, on the device (acrmi_track_boxes): pj2d_org [n,2,21,2] and
    slots [n,2,176] as Engine.forward(..., project=True, offsets=) returns them -> int32 [n,4] rows (l, t, r, b) on the device.
    The rule is acr.utils.boxes_from_keypoints on the fp32 points of the hands whose flag is set, integer for integer, with
    one clause more: a result without pixels is the whole frame (DESIGN.md "Tracking on the device").  frame_hw: (H, W), or one
    pair per region on the host, or an int32 device tensor [n,2], which is used as it is.  out: the tensor to write.  stream:
    a raw hipStream_t to queue on instead of the current stream.  Nothing here waits for the device."""
    scale, min_size = check_track_args(scale, min_size)
    if not isinstance(pj2d_org, torch.Tensor) or not isinstance(slots, torch.Tensor) or pj2d_org.dim() != 4 or \
            tuple(pj2d_org.shape[1:]) != (2, 21, 2) or tuple(slots.shape) != (pj2d_org.shape[0], 2, _lib.SLOT) or \
            pj2d_org.dtype != torch.float32 or slots.dtype != torch.float32 or pj2d_org.shape[0] < 1:
        raise ValueError('pj2d_org must be float32 [n,2,21,2] and slots float32 [n,2,%d], n >= 1' % _lib.SLOT)
    n = pj2d_org.shape[0]
    dev = pj2d_org.device
    _host_frame_hw(frame_hw, n)      # the host forms: checked before the device is looked at
    _need_cuda(pj2d_org, slots)
    if slots.device != dev:
        raise ValueError('pj2d_org and slots are on different devices')
    hw = frame_hw_device(frame_hw, n, dev)
    out = _track_out(out, (n, 4), torch.int32, dev, 'out')
    pj, sl = pj2d_org.contiguous(), slots.contiguous()
    _lib.check(_lib.lib().acrmi_track_boxes(_p(pj), _p(sl), _p(hw), n, scale, min_size, _p(out), _raw_stream(stream, dev)))
    return out


# ---- tracks: hand identity across frames with max_hand > 1 (csrc/assoc_plan.h, csrc/heads.hip) ----
def check_track_table(table, K):
    """`table=` of associate_hands / Engine.forward(tracks=): an open engine.TrackTable of K slots per side."""
    if getattr(table, 'handle', None) is None or getattr(table, 'max_hand', None) is None:
        raise ValueError('the track table must be an open TrackTable')
    if int(table.max_hand) != int(K):
        raise ValueError('the TrackTable holds %d slots per side, the slots %d hands' % (table.max_hand, K))
    return table


def track_stream_ids(tracks, table, B):
    """`tracks=`: one stream id per frame (-1 = leave the frame alone) -> host int32 [B], checked against the table."""
    from .engine import stream_ids
    ids = stream_ids(tracks, B)
    if ids.size and (int(ids.min()) < -1 or int(ids.max()) >= int(table.capacity)):
        raise ValueError('tracks: an id outside -1..%d' % (int(table.capacity) - 1))
    return ids


def associate_hands(slots, tracks, table, smooth=True, ctx=None, stream=None):
    """Which hand of each frame continues which track (acrmi_associate): slots [B,K,2,176] ([B,2,176]: K = 1) as
    decode(max_hand=K) / decode_maps_multi leave them, reordered IN PLACE so that row k of a side is the hand of track slot k
    of the frame's stream; tracks: the stream of each frame (-1 = leave the frame as it is), frames that share an id are one
    sequence in batch order; table: an engine.TrackTable of K slots.  smooth: the rows that continue or start a track go
    through that slot's own One-Euro filter (ctx: the context whose ACRMI_OPT_SMOOTH_COEFF applies; None = the default).
    -> (track_ids, perm), int32 [B,K,2]: the id of the slot's track (-1: no hand of it in this frame) and the rank that moved
    there.  Nothing here waits for the device."""
    if not isinstance(slots, torch.Tensor) or slots.dtype != torch.float32 or slots.dim() not in (3, 4) or \
            tuple(slots.shape[-2:]) != (2, _lib.SLOT) or slots.shape[0] < 1 or not slots.is_contiguous():
        raise ValueError('slots must be a contiguous float32 tensor [B,K,2,%d] or [B,2,%d], B >= 1' % (_lib.SLOT, _lib.SLOT))
    B, K = slots.shape[0], (1 if slots.dim() == 3 else slots.shape[1])
    if not 1 <= K <= _lib.MAX_HAND:
        raise ValueError('slots hold %d hands per side: 1..%d' % (K, _lib.MAX_HAND))
    check_track_table(table, K)
    ids = track_stream_ids(tracks, table, B)
    _need_cuda(slots)
    dev = slots.device
    track_ids = torch.empty(B, K, 2, dtype=torch.int32, device=dev)
    perm = torch.empty(B, K, 2, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().acrmi_associate(ctx, table.handle, _p(slots), B, K, ids.ctypes.data_as(C.c_void_p), int(bool(smooth)),
                                          _p(track_ids), _p(perm), _raw_stream(stream, dev)), ctx)
    return track_ids, perm


def assoc_step_host(rows, state, gate=8, max_miss=5):
    """The association rule for one frame of one (stream, side) on the host (acrmi_assoc_step; no device): rows float32
    [K,>=2] in rank order (flag and flat index in columns 0 and 1), state int32 [41] updated in place
    -> (track_ids, perm, born), int32 [K]."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if rows.ndim != 2 or rows.shape[1] < 2 or not isinstance(state, np.ndarray) or state.dtype != np.int32 or \
            state.shape != (_lib.ASSOC_STATE,) or not state.flags['C_CONTIGUOUS']:
        raise ValueError('rows must be [K,>=2] and state a contiguous int32 array [%d]' % _lib.ASSOC_STATE)
    K = rows.shape[0]
    out = np.zeros((3, max(K, 1)), np.int32)
    _lib.check(_lib.lib().acrmi_assoc_step(K, int(gate), int(max_miss), rows.ctypes.data_as(C.c_void_p), rows.shape[1],
                                           state.ctypes.data_as(C.c_void_p), out[0].ctypes.data_as(C.c_void_p),
                                           out[1].ctypes.data_as(C.c_void_p), out[2].ctypes.data_as(C.c_void_p)))
    return out[0, :K], out[1, :K], out[2, :K]


def cam_trans(joints, pj2d, focal_length=600.0, img_size=512.0):
    """joints [n,21,3], pj2d [n,21,2] (device fp32) -> cam_trans [n,3]: the reference's closed-form least squares
    (acr/utils.py:430-472, unit confidences) on the device."""
    _need_cuda(joints, pj2d)
    n = joints.shape[0]
    if tuple(joints.shape[1:]) != (21, 3) or tuple(pj2d.shape) != (n, 21, 2):
        raise ValueError('joints must be [n,21,3] and pj2d [n,21,2]')
    out = torch.empty(n, 3, dtype=torch.float32, device=joints.device)
    j, p = joints.contiguous().float(), pj2d.contiguous().float()
    _lib.check(_lib.lib().acrmi_cam_trans(_p(j), _p(p), n, float(focal_length), float(img_size), _p(out), _s(joints)))
    return out


def u8norm(img):
    _need_cuda(img)
    B, H, W, _ = img.shape
    out = torch.empty(B, H, W, 4, dtype=torch.float32, device=img.device)
    src = img.contiguous()                 # bound to a local until the call has been queued
    _lib.check(_lib.lib().acrmi_u8norm(_p(src), B * H * W, _p(out), _s(src)))
    return out


def stem_conv(img, w, b, relu=True):
    """uint8 RGB [B,H,W,3] on the device + conv1 filters [64,3,3,3] / bias [64] (host arrays, BN folded) ->
    relu(conv3x3 stride 2 pad 1 of (img/255*2-1)) NHWC [B,H/2,W/2,64] (acr/model.py:832,589-603) in one kernel."""
    _need_cuda(img)
    B, H, W, _ = img.shape
    wp, bp = pack_stem(np.asarray(w, np.float64), np.asarray(b, np.float64))
    wd, bd = torch.from_numpy(wp).to(img.device), torch.from_numpy(bp).to(img.device)
    out = torch.empty(B, H // 2, W // 2, 64, dtype=torch.float32, device=img.device)
    src = img.contiguous()
    _lib.check(_lib.lib().acrmi_stem_conv(_p(src), B, H, W, _p(wd), _p(bd), _p(out), 64, 0, int(relu), _s(src)))
    return out


def bilinear2x(x, channels=None):
    _need_cuda(x)
    B, H, W, cs = x.shape
    Cc = channels or cs
    out = torch.zeros(B, 2 * H, 2 * W, Cc, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().acrmi_bilinear2x(_p(x), B, H, W, cs, Cc, _p(out), Cc, _s(x)))
    return out


def fuse_sum(terms, shifts, relu=True):
    _need_cuda(*terms)
    B, H, W, Cc = terms[0].shape
    n = len(terms)
    out = torch.empty(B, H, W, Cc, dtype=torch.float32, device=terms[0].device)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in terms])
    cs = (C.c_int * n)(*[t.shape[-1] for t in terms])
    sh = (C.c_int * n)(*shifts)
    _lib.check(_lib.lib().acrmi_fuse_sum(n, ptrs, cs, sh, B, H, W, Cc, _p(out), Cc, int(relu), _s(out)))
    return out


def attpool(segm, feat, channels):
    """segm NHWC [B,256,256,cs] logits, feat NHWC [B,128,128,cs]; -> pooled [B,32,channels]."""
    _need_cuda(segm, feat)
    B = segm.shape[0]
    ws = torch.empty(int(_lib.lib().acrmi_attpool_ws_floats(B, channels)), dtype=torch.float32, device=segm.device)
    pooled = torch.empty(B, 32, channels, dtype=torch.float32, device=segm.device)
    _lib.check(_lib.lib().acrmi_attpool(_p(segm), segm.shape[-1], _p(feat), feat.shape[-1], channels, B, _p(ws),
                                        _p(pooled), _s(segm)))
    return pooled


def parebias(pooled, lc_w, lin_w, lin_b, mix_wp, mix_b, part0):
    """pooled [B,32,C] device (C = 320: contact 256 | shape 64) + the reference's raw weights (host arrays:
    contact_layers.{2,3}.weight -> [6,256,16], cam_shape_layers.{2,3} -> [10,1024] / [10], the pare columns of
    contact_layers.{4,5} -> [109,106] / bias [109]) -> per-frame mix-conv bias [B,112] (acr/model.py:141-164)."""
    _need_cuda(pooled)
    B, _, Cc = pooled.shape
    dev = pooled.device
    w = [torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float32))).to(dev) for a in (lc_w, lin_w, lin_b, mix_wp, mix_b)]
    out = torch.zeros(B, 112, dtype=torch.float32, device=dev)
    src = pooled.contiguous().float()
    _lib.check(_lib.lib().acrmi_parebias(_p(src), Cc, int(part0), _p(w[0]), _p(w[1]), _p(w[2]), _p(w[3]), _p(w[4]), B,
                                         _p(out), 112, _s(src)))
    return out


def decode_maps(l_center, r_center, l_params, r_params, l_prior, r_prior, conf_thresh=0.35, prior_gate=None):
    """NHWC device maps -> slots [B,2,176].  conf_thresh = args().centermap_conf_thresh (strict >).
    prior_gate: int32 device tensor [B] (acrmi_decode_maps_gated) or None = the per-frame prior rule."""
    _need_cuda(l_center, r_center, l_params, r_params, l_prior, r_prior, prior_gate)
    B = l_center.shape[0]
    slots = torch.empty(B, 2, _lib.SLOT, dtype=torch.float32, device=l_center.device)
    gate = None if prior_gate is None else prior_gate.to(torch.int32).contiguous()
    if gate is not None and gate.numel() != B:
        raise ValueError('prior_gate must hold one int per frame')
    _lib.check(_lib.lib().acrmi_decode_maps_gated(_p(l_center), _p(r_center), l_center.shape[-1], _p(l_params), _p(r_params),
                                                  l_params.shape[-1], _p(l_prior), _p(r_prior), l_prior.shape[-1], B,
                                                  float(conf_thresh), _p(gate), _p(slots), _s(slots)))
    return slots


def decode_maps_multi(l_center, r_center, l_params, r_params, l_prior, r_prior, max_hand, conf_thresh=0.35):
    """NHWC device maps -> slots [B,max_hand,2,176]: the max_hand (1.._lib.MAX_HAND) best centres of each map per frame, pair
    k = (left rank k, right rank k), every hand's prior from its nearest flagged partner of the other side
    (acrmi_decode_maps_multi).  max_hand = 1 is decode_maps with one more dimension."""
    _need_cuda(l_center, r_center, l_params, r_params, l_prior, r_prior)
    K = int(max_hand)
    if K != max_hand or not 1 <= K <= _lib.MAX_HAND:
        raise ValueError('max_hand %r: an integer in 1..%d' % (max_hand, _lib.MAX_HAND))
    B = l_center.shape[0]
    slots = torch.empty(B, K, 2, _lib.SLOT, dtype=torch.float32, device=l_center.device)
    _lib.check(_lib.lib().acrmi_decode_maps_multi(_p(l_center), _p(r_center), l_center.shape[-1], _p(l_params), _p(r_params),
                                                  l_params.shape[-1], _p(l_prior), _p(r_prior), l_prior.shape[-1], B, K,
                                                  float(conf_thresh), _p(slots), _s(slots)))
    return slots


def prior_gate(slots):
    """acrmi_prior_gate (stand-alone form): slots [B,2,176] of a first decode -> int32 [B] for decode_maps(prior_gate=...):
    the reference's batch-wide prior decision (acr/result_parser.py:42-47,102-145), computed on the device."""
    _need_cuda(slots)
    if slots.dtype != torch.float32 or not slots.is_contiguous():
        raise ValueError('slots must be a contiguous float32 device tensor')
    gate = torch.empty(slots.shape[0], dtype=torch.int32, device=slots.device)
    _lib.check(_lib.lib().acrmi_prior_gate(None, _p(slots), slots.shape[0], _p(gate), _s(slots)))
    return gate


# ---- mesh overlay (csrc/render.hip; DESIGN.md "Rendering") -------------------------------------------------------------
HAND_COLORS_RGB = ((0.46, 0.59, 0.64), (0.94, 0.71, 0.53))      # left, right (reference acr/visualization.py:76)


def mesh_topology(faces, n_verts):
    """faces [F,3] (numpy / torch integers) of a mesh with n_verts vertices -> the int32 blob acrmi_rasterize reads
    ([F, V | faces | CSR row | CSR col]: faces + the vertex -> faces table, acrmi_mesh_topology).  Pure host: works
    without a GPU.  Upload it once (`torch.from_numpy(blob).cuda()`) and hand it to render_meshes for every call."""
    f = faces.detach().cpu().numpy() if hasattr(faces, 'detach') else np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError('faces must be [F,3]')
    f = np.ascontiguousarray(f.astype(np.int32))
    L = _lib.lib()
    n = _lib.check(L.acrmi_mesh_topology(None, f.shape[0], int(n_verts), None, 0))
    blob = np.empty(n, np.int32)
    _lib.check(L.acrmi_mesh_topology(f.ctypes.data_as(C.c_void_p), f.shape[0], int(n_verts), blob.ctypes.data_as(C.c_void_p), n))
    return blob


def view_from_offsets(offsets):
    """`offsets` rows [N,10] (ops.preprocess / acr.utils.img_preprocess) -> the viewport rows [N,4] render_meshes takes:
    the 512 canvas mapped into the original frame exactly like pj2d -> pj2d_org (x_org = x_512 * padded_w / 512 + left).
    The rule is stated once, in csrc/region_view_plan.h (region_view_row)."""
    o = torch.as_tensor(offsets, dtype=torch.float32)
    return torch.stack([o[:, 0] / 512., o[:, 1] / 512., o[:, 5] - o[:, 9], o[:, 2] - o[:, 6]], 1)


def _topology_on(t, n_verts, device):
    if isinstance(t, torch.Tensor) and t.dim() == 1 and t.dtype == torch.int32:
        blob = t
    elif isinstance(t, np.ndarray) and t.ndim == 1 and t.dtype == np.int32:
        blob = torch.from_numpy(t)
    else:
        blob = torch.from_numpy(mesh_topology(t, n_verts))
    return blob.to(device).contiguous()


def render_meshes(verts, faces, images, mesh_frame=None, trans=None, colors=None, view=None, focal_length=1265.,
                  visible_weight=0.9, out=None, return_ids=False, topo_index=None, mesh_view=None, vertex_colors=None):
    """Draws M meshes over N equal-sized frames on the GPU (acrmi_rasterize; the reference's Visualizer 'mesh' view,
    acr/visualization.py:100-218, with the conventions of DESIGN.md "Rendering").
    verts [M,V,3] device fp32 (metres, camera axes); trans [M,3] added to them (cam_trans) or None.
    faces: [F,3] integers, or a mesh_topology blob (host or device int32) - or a pair of either for meshes of two
    topologies with the same V and F (left / right MANO), chosen per mesh by topo_index [M] (0 / 1).
    images uint8 [N,H,W,3] device; mesh_frame [M] = the frame each mesh is drawn into, -1 = not drawn (default: mesh m
    into frame m when M == N, into frame m // (M / N) when N divides M).  colors [M,3] or [3] in the images' channel
    order (default: the reference's right-hand colour as RGB).  view [N,4] = scale x, scale y, shift x, shift y of the 512
    canvas (view_from_offsets) or None = the 512 network input.  mesh_view [M,4]: such a row per MESH instead (exclusive with
    view; meshes of several regions of interest in one frame, DESIGN.md "Views over regions") - the depth that is compared
    is then mesh_view[m,0] / Z, one virtual camera per frame, and a mesh whose scale is not > 0 is not drawn.
    vertex_colors [M,V,3] device fp32 (what ops.vertex_colors returns): a base colour in [0,1] per VERTEX, in the images'
    channel order, interpolated perspective-correctly over every triangle (acrmi_rasterize_colored); it
    replaces `colors` for every mesh of the call, with view= and with mesh_view=.
    out: uint8 tensor like images (may BE images: in place).
    Returns out, or (out, ids int32 [N,H,W]: mesh * F + face of the visible triangle, -1 = none) with return_ids."""
    if view is not None and mesh_view is not None:
        raise ValueError('view (one row per frame) and mesh_view (one row per mesh) exclude each other')
    _need_cuda(verts, images, out)
    if verts.dim() != 3 or verts.shape[-1] != 3 or verts.shape[0] < 1:
        raise ValueError('verts must be [M,V,3]')
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3 or images.shape[0] < 1:
        raise ValueError('images must be uint8 [N,H,W,3]')
    dev = images.device
    M, V, _ = verts.shape
    N, H, W, _ = images.shape
    pair = isinstance(faces, (tuple, list)) and len(faces) == 2 and not np.isscalar(faces[0]) and np.ndim(faces[0]) >= 1
    topos = [_topology_on(t, V, dev) for t in (faces if pair else [faces])]
    head = [t[:2].tolist() for t in topos]      # (one small D2H copy per topology; [F, V])
    F = head[0][0]
    if any(h != [F, V] for h in head):
        raise ValueError('topology is for (faces, verts) = %s, verts have %d vertices' % (head, V))
    v = verts.to(dev, torch.float32).contiguous()
    t = None if trans is None else trans.to(dev, torch.float32).contiguous().view(M, 3)
    if mesh_frame is None:
        if M % N:
            raise ValueError('mesh_frame is needed when the frames do not divide the meshes')
        mesh_frame = torch.arange(M, dtype=torch.int32) // (M // N)
    mf = torch.as_tensor(mesh_frame).to(dev, torch.int32).contiguous()
    if mf.numel() != M:
        raise ValueError('mesh_frame must hold one int per mesh')
    ti = None
    if topo_index is not None:
        ti = torch.as_tensor(topo_index).to(dev, torch.int32).contiguous()
        if ti.numel() != M or not pair:
            raise ValueError('topo_index needs a pair of topologies and one int per mesh')
    c = torch.as_tensor(HAND_COLORS_RGB[1] if colors is None else colors, dtype=torch.float32)
    c = (c.view(1, 3).repeat(M, 1) if c.numel() == 3 else c.reshape(M, 3)).to(dev).contiguous()
    vw = None
    if view is not None:
        vw = torch.as_tensor(view, dtype=torch.float32).to(dev).contiguous()
        if tuple(vw.shape) != (N, 4):
            raise ValueError('view must be [N,4]')
    if mesh_view is not None:
        vw = torch.as_tensor(mesh_view, dtype=torch.float32).to(dev).contiguous()
        if tuple(vw.shape) != (M, 4):
            raise ValueError('mesh_view must be [M,4]')
    vc = None
    if vertex_colors is not None:
        _need_cuda(vertex_colors)
        if tuple(vertex_colors.shape) != (M, V, 3):
            raise ValueError('vertex_colors must be [M,V,3]')
        vc = vertex_colors.to(dev, torch.float32).contiguous()
    src = images.contiguous()
    if out is None:
        out = torch.empty_like(src)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (N, H, W, 3) or not out.is_contiguous() or out.device != dev:
        raise ValueError('out must be a contiguous uint8 tensor shaped like images, on their device')
    ids = torch.empty(N, H, W, dtype=torch.int32, device=dev) if return_ids else None
    L = _lib.lib()
    ws = torch.empty(int(L.acrmi_render_workspace(M, F)) + 256, dtype=torch.uint8, device=dev)
    ws_p = (ws.data_ptr() + 255) // 256 * 256
    head = (_p(v), _p(t), M, V, F, _p(topos[0]), _p(topos[1]) if pair else None, _p(ti), _p(mf), _p(c))
    tail = (float(focal_length), float(visible_weight), _p(src), _p(out), N, H, W, _p(ids), C.c_void_p(ws_p), _s(src))
    if vc is not None:
        _lib.check(L.acrmi_rasterize_colored(*head, _p(vc), _p(vw), int(mesh_view is not None), *tail))
    else:
        call = L.acrmi_rasterize if mesh_view is None else L.acrmi_rasterize_views
        _lib.check(call(*head, _p(vw), *tail))
    return (out, ids) if return_ids else out


# ---- per-vertex colours: the contact and error views (csrc/vertex_color.hip) ------------------------
FLAG_COLOR = (1.0, 0.0, 1.0)      # magenta: no entry of the default table, in either channel order


def check_color_range(lo, hi):
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo) or not (abs(lo) <= 3.4028234e38 and abs(hi) <= 3.4028234e38):
        raise ValueError('lo and hi must be finite fp32 values with hi > lo')
    return lo, hi


def _lut_arg(lut):
    if lut is None:
        return None
    t = np.ascontiguousarray(np.asarray(lut.cpu() if isinstance(lut, torch.Tensor) else lut))
    if t.dtype != np.uint8 or t.shape != (256, 3):
        raise ValueError('lut must be uint8 [256,3]')
    return t


def vertex_colors(values, lo, hi, flags=None, base=None, flag_color=FLAG_COLOR, lut=None, reverse=False, bgr=False, out=None,
                  stream=None):
    """A scalar per vertex -> a colour per vertex for render_meshes(vertex_colors=) on the GPU (acrmi_vertex_colors; DESIGN.md
    section 22).  values [M,V] device fp32; flags [M,V] device int32 or None.  Per vertex: flag != 0 -> flag_color; else a NaN
    value -> base (the mesh keeps its flat colour there); else t = (v - lo) / (hi - lo) clamped to [0,1], entry int(t * 255)
    of the table - 255 minus it with reverse=True - divided by 255.  base [M,3] or [3] (default: the reference's right-hand
    colour, as render_meshes), flag_color [3], in the images' channel order; lut uint8 [256,3] in that order, None = the
    default jet of overlay_tables(bgr).  lo, hi: finite, hi > lo (ValueError).  Returns fp32 [M,V,3] on the device of values;
    nothing waits for the host."""
    _need_cuda(values, flags, out)
    if values.dim() != 2 or values.shape[1] < 1:
        raise ValueError('values must be [M,V]')
    lo, hi = check_color_range(lo, hi)
    dev = values.device
    M, V = values.shape
    if M * V * 3 > 0x7fffffff:
        raise ValueError('%d meshes of %d vertices are beyond 2^31 - 1 colour values' % (M, V))
    val = values.to(dev, torch.float32).contiguous()
    fl = None
    if flags is not None:
        if tuple(flags.shape) != (M, V):
            raise ValueError('flags must be [M,V] like values')
        fl = flags.to(dev, torch.int32).contiguous()
    b = torch.as_tensor(HAND_COLORS_RGB[1] if base is None else base, dtype=torch.float32)
    if b.numel() not in (3, 3 * M):
        raise ValueError('base must be [M,3] or [3]')
    b = (b.reshape(1, 3).repeat(M, 1) if b.numel() == 3 and M != 1 else b.reshape(M, 3)).to(dev).contiguous()
    fc = np.ascontiguousarray(np.asarray(flag_color, np.float32))
    if fc.shape != (3,):
        raise ValueError('flag_color must be [3]')
    table = _lut_arg(lut)
    if out is None:
        out = torch.empty(M, V, 3, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (M, V, 3) or not out.is_contiguous() or out.device != dev:
        raise ValueError('out must be a contiguous fp32 tensor [M,V,3] on the device of values')
    st = _s(val) if stream is None else C.c_void_p(stream)
    _lib.check(_lib.lib().acrmi_vertex_colors(_p(val), _p(fl), _p(b), M, V, lo, hi, int(bool(reverse)), fc.ctypes.data_as(C.c_void_p),
                                              None if table is None else table.ctypes.data_as(C.c_void_p), int(bool(bgr)), _p(out), st))
    return out


def contact_values(con, B, K=1, max_depth=None, stream=None):
    """What mesh_contact / mesh_surface_contact (or Engine.contact) returned for the B * K * K pairs of B rows at K hands per side
    (pair (b*K + i)*K + j = left rank i, right rank j; direction 0 = the left hand) -> per HAND and vertex, on the GPU
    (acrmi_contact_values): 'value' fp32 [B,K,2,V] = metres to the nearest hand of the other side in the
    row (NaN when no pair of the hand was computed), 'flag' int32 [B,K,2,V] = 1 where the vertex is inside one of them by the
    measure's own rule (side < 0, respectively crossings odd) within max_depth.  con: a dict with 'd2' [B*K*K,2,V] and 'side'
    (nearest-vertex measure) or 'cross' (surface measure).  Nothing waits for the host."""
    d2 = con['d2']
    surface = con.get('cross') is not None
    other = con['cross'] if surface else con.get('side')
    if other is None:
        raise ValueError("con must hold 'd2' and one of 'side' (mesh_contact) and 'cross' (mesh_surface_contact)")
    _need_cuda(d2, other)
    B, K = int(B), int(K)
    if B < 0 or not 1 <= K <= _lib.MAX_HAND:
        raise ValueError('B >= 0 and K in 1..%d' % _lib.MAX_HAND)
    if d2.dim() != 3 or d2.shape[0] != B * K * K or d2.shape[1] != 2 or d2.shape[2] < 1 or tuple(other.shape) != tuple(d2.shape):
        raise ValueError('d2 and %s must be [%d,2,V]' % ('cross' if surface else 'side', B * K * K))
    max_depth = float(CONTACT_MAX_DEPTH if max_depth is None else max_depth)      # (a parameter, not a measurement)
    if not max_depth >= 0:
        raise ValueError('max_depth must be >= 0 (inf allowed)')
    dev, V = d2.device, d2.shape[2]
    d2 = d2.to(dev, torch.float32).contiguous()
    other = other.to(dev, torch.int32 if surface else torch.float32).contiguous()
    value = torch.empty(B, K, 2, V, dtype=torch.float32, device=dev)
    flag = torch.empty(B, K, 2, V, dtype=torch.int32, device=dev)
    st = _s(d2) if stream is None else C.c_void_p(stream)
    _lib.check(_lib.lib().acrmi_contact_values(_p(d2), None if surface else _p(other), _p(other) if surface else None, B, K, V,
                                               max_depth, _p(value), _p(flag), st))
    return {'value': value, 'flag': flag}


# ---- contact and interpenetration between meshes (csrc/contact.hip) --------------------------------
CONTACT_DIST, CONTACT_MAX_DEPTH = 0.005, 0.02      # metres; defaults of PARAMETERS, not measurements


def mesh_orientation(verts, faces):
    """+1 / -1: the sign of the signed volume sum v0 . (v1 x v2) of a closed mesh (verts [V,3], faces [F,3]) in float64; +1
    when it is exactly 0.  +1 means the face normals (v1 - v0) x (v2 - v0) point outwards - the `sign` mesh_contact takes.
    Pure host: works without a GPU."""
    v = verts.detach().cpu().numpy() if hasattr(verts, 'detach') else np.asarray(verts)
    f = faces.detach().cpu().numpy() if hasattr(faces, 'detach') else np.asarray(faces)
    v = v.astype(np.float64)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError('verts must be [V,3] and faces [F,3]')
    f = f.astype(np.int64)
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError('a face names a vertex outside [0, %d)' % v.shape[0])
    vol = float((v[f[:, 0]] * np.cross(v[f[:, 1]], v[f[:, 2]])).sum())
    return -1 if vol < 0 else 1


def check_contact_params(contact_dist, max_depth):
    contact_dist, max_depth = float(contact_dist), float(max_depth)
    if not (0 <= contact_dist < float('inf')) or not (max_depth >= 0):
        raise ValueError('contact_dist must be finite and >= 0, max_depth >= 0 (inf allowed)')
    return contact_dist, max_depth


SURFACE_FACE_TILE, SURFACE_MAX_FACES = 256, 8000      # = csrc/surface_contact_plan.h

# The two measures (Engine.contact's modes), each described once.  outputs: the per-vertex tensors [n_pairs, 2, V] + tail, in the
# order the entry points take them, ahead of sum_f / sum_i of the widths `sums`; summary: the views of the two summaries the
# result adds; workspace / op / ctx: the workspace size, the stateless and the context entry point; sign: it takes the
# orientation signs (ahead of the pairs / of contact_dist).
CONTACT_MEASURES = {
    'vertex': dict(
        outputs=(('nn', (), torch.int32), ('d2', (), torch.float32), ('side', (), torch.float32)), sums=(4, 6), sign=True,
        summary=lambda f, i: {'min_d2': f[:, 0], 'closest': i[:, 0:2], 'n_contact': i[:, 2:4], 'n_inside': i[:, 4:6],
                              'depth2': f[:, 1:3]},
        workspace=lambda L, M, V, F: L.acrmi_contact_workspace(M, V), op='acrmi_mesh_contact', ctx='acrmi_contact'),
    'surface': dict(
        outputs=(('face', (), torch.int32), ('d2', (), torch.float32), ('point', (3,), torch.float32), ('cross', (), torch.int32)),
        sums=(4, 8), sign=False,
        summary=lambda f, i: {'min_d2': f[:, 0:2], 'closest': i[:, 0:4].unflatten(1, (2, 2)), 'n_contact': i[:, 4:6],
                              'n_inside': i[:, 6:8], 'depth2': f[:, 2:4]},
        workspace=lambda L, M, V, F: L.acrmi_surface_contact_workspace(M, V, F), op='acrmi_mesh_surface_contact',
        ctx='acrmi_surface_contact')}


def measure_outputs(m, n_pairs, V, dev):
    """The raw output tensors of measure m (an entry of CONTACT_MEASURES) for n_pairs pairs of V vertices, in the order its entry
    points take them."""
    raw = {name: torch.empty((n_pairs, 2, V) + tail, dtype=dt, device=dev) for name, tail, dt in m['outputs']}
    raw['sum_f'] = torch.empty((n_pairs, m['sums'][0]), dtype=torch.float32, device=dev)
    raw['sum_i'] = torch.empty((n_pairs, m['sums'][1]), dtype=torch.int32, device=dev)
    return raw


def measure_result(m, raw):
    """The raw outputs -> the dict the measure's operator returns (views of the summaries, no copy, no host visit)."""
    return dict({name: raw[name] for name, _, _ in m['outputs']}, **m['summary'](raw['sum_f'], raw['sum_i']))


def contact_outputs(n_pairs, V, dev):
    """The raw output tensors of acrmi_mesh_contact / acrmi_contact for n_pairs pairs of V vertices."""
    return measure_outputs(CONTACT_MEASURES['vertex'], n_pairs, V, dev)


def contact_result(raw):
    """The raw outputs -> the dict mesh_contact returns (views of the summaries, no copy, no host visit)."""
    return measure_result(CONTACT_MEASURES['vertex'], raw)


def surface_contact_outputs(n_pairs, V, dev):
    """The raw output tensors of acrmi_mesh_surface_contact / acrmi_surface_contact for n_pairs pairs of V vertices."""
    return measure_outputs(CONTACT_MEASURES['surface'], n_pairs, V, dev)


def surface_contact_result(raw):
    """The raw outputs -> the dict mesh_surface_contact returns (views of the summaries, no copy, no host visit)."""
    return measure_result(CONTACT_MEASURES['surface'], raw)


def mesh_contact(verts, faces, pairs, trans=None, topo_index=None, sign=None, contact_dist=CONTACT_DIST,
                 max_depth=CONTACT_MAX_DEPTH):
    """Contact and interpenetration between pairs of meshes on the GPU (acrmi_mesh_contact): the nearest-vertex half-space
    heuristic of DESIGN.md section 19 - not a point-to-triangle distance, not a true inside test; meaningful for closed
    meshes.  verts [M,V,3] device fp32 (metres), trans [M,3] added to them (cam_trans) or None.  faces: as render_meshes -
    [F,3] integers or a mesh_topology blob, or a pair of either chosen per mesh by topo_index [M] (0 / 1).  sign [M] (+1 / -1,
    mesh_orientation of each mesh's topology) or None = all +1.  pairs [n,2] mesh indices (a, b): a host list / array is
    checked here (an index >= M is a ValueError; < 0 = skip the pair), a device tensor is not read - the kernel treats every
    index outside [0, M) as a skipped pair.  contact_dist / max_depth in metres (max_depth may be inf).
    Returns device tensors, nothing is copied to the host: 'nn' int32, 'd2', 'side' fp32 [n,2,V] (direction 0: the vertices of
    a against b; 1: those of b against a; nearest vertex, its squared distance, the side value - inside where negative);
    'min_d2' [n] with 'closest' [n,2] = (i, j); 'n_contact', 'n_inside' int32 [n,2]; 'depth2' [n,2] = the largest d2 among the
    inside vertices (its square root: the penetration depth estimate).  A skipped pair: nn -1, d2 inf, side 0, zero counts,
    closest (-1, -1)."""
    return _mesh_measure('vertex', verts, faces, pairs, trans, topo_index, sign, contact_dist, max_depth)


def mesh_surface_contact(verts, faces, pairs, trans=None, topo_index=None, contact_dist=CONTACT_DIST, max_depth=CONTACT_MAX_DEPTH):
    """The surface contact measure between pairs of meshes on the GPU (acrmi_mesh_surface_contact): the
    distance from every vertex to the other mesh's SURFACE (closest point of every triangle) and containment by the parity of
    the crossings of the +Z ray, exact on a closed mesh.  Every vertex meets every face: it costs more than mesh_contact.
    verts, faces, pairs, trans, topo_index, contact_dist, max_depth: as mesh_contact, with the same host checks; there is no
    sign - the rule does not depend on the winding.  At most 4000 vertices and 8000 faces.
    Returns device tensors, nothing is copied to the host, direction 0 = the vertices of a against b, 1 = those of b against
    a: 'face' int32 [n,2,V] (the nearest face, -1: none), 'd2' [n,2,V] (squared distance to it), 'point' [n,2,V,3] (the point
    on it), 'cross' int32 [n,2,V] (crossings; odd = inside); 'min_d2' [n,2] with 'closest' [n,2,2] = (i, face) per direction;
    'n_contact', 'n_inside' int32 [n,2]; 'depth2' [n,2] = the largest d2 among the inside vertices.  A skipped pair: face -1,
    d2 inf, point 0, cross 0, zero counts, closest (-1, -1)."""
    return _mesh_measure('surface', verts, faces, pairs, trans, topo_index, None, contact_dist, max_depth)


def _mesh_measure(mode, verts, faces, pairs, trans, topo_index, sign, contact_dist, max_depth):
    """mesh_contact / mesh_surface_contact: the host checks, the outputs, the aligned workspace and the call."""
    m = CONTACT_MEASURES[mode]
    _need_cuda(verts)
    if verts.dim() != 3 or verts.shape[-1] != 3 or verts.shape[0] < 1:
        raise ValueError('verts must be [M,V,3]')
    contact_dist, max_depth = check_contact_params(contact_dist, max_depth)
    v, t, topos, ti, pr = _contact_inputs(verts, faces, pairs, trans, topo_index)
    dev = v.device
    M, V, _ = v.shape
    n, F = pr.shape[0], int(topos[2])
    sg = None
    if sign is not None:
        sg = torch.as_tensor(sign).to(dev, torch.int32).contiguous()
        if sg.numel() != M:
            raise ValueError('sign must hold one int per mesh')
    raw = measure_outputs(m, n, V, dev)
    L = _lib.lib()
    ws = torch.empty(int(m['workspace'](L, M, V, F)) + 16, dtype=torch.uint8, device=dev)
    ws_p = (ws.data_ptr() + 15) // 16 * 16
    _lib.check(getattr(L, m['op'])(_p(v), _p(t), M, V, F, _p(topos[0]), _p(topos[1]), _p(ti), *((_p(sg),) if m['sign'] else ()),
                                   _p(pr), n, contact_dist, max_depth, *[_p(x) for x in raw.values()], C.c_void_p(ws_p), _s(v)))
    return measure_result(m, raw)


def _contact_inputs(verts, faces, pairs, trans, topo_index):
    """The host checks mesh_contact and mesh_surface_contact share -> (verts, trans or None, (topology, second topology or
    None, F), topo_index or None, pairs [n,2] int32), all on the device of verts."""
    dev = verts.device
    M, V, _ = verts.shape
    if isinstance(pairs, torch.Tensor) and pairs.is_cuda:
        pr = pairs.to(dev, torch.int32).contiguous()
    else:
        host = np.asarray(pairs.cpu() if isinstance(pairs, torch.Tensor) else pairs)
        if host.size and not np.issubdtype(host.dtype, np.integer):
            raise ValueError('pairs must be integers')
        host = host.reshape(-1, 2) if host.size else np.zeros((0, 2), np.int32)
        if host.size and host.max() >= M:
            raise ValueError('a pair names mesh %d, there are %d meshes' % (int(host.max()), M))
        pr = torch.from_numpy(np.ascontiguousarray(host.astype(np.int32))).to(dev)
    if pr.dim() != 2 or pr.shape[1] != 2:
        raise ValueError('pairs must be [n,2]')
    pair = isinstance(faces, (tuple, list)) and len(faces) == 2 and not np.isscalar(faces[0]) and np.ndim(faces[0]) >= 1
    topos = [_topology_on(t, V, dev) for t in (faces if pair else [faces])]
    head = [t[:2].tolist() for t in topos]      # (one small D2H copy per topology; [F, V])
    F = head[0][0]
    if any(h != [F, V] for h in head):
        raise ValueError('topology is for (faces, verts) = %s, verts have %d vertices' % (head, V))
    v = verts.to(dev, torch.float32).contiguous()
    t = None if trans is None else trans.to(dev, torch.float32).contiguous().view(M, 3)
    ti = None
    if topo_index is not None:
        ti = torch.as_tensor(topo_index).to(dev, torch.int32).contiguous()
        if ti.numel() != M or not pair:
            raise ValueError('topo_index needs a pair of topologies and one int per mesh')
    return v, t, (topos[0], topos[1] if pair else None, F), ti, pr


# ---- scoring against ground truth (csrc/score.hip) -------------------------------------------------
def score_outputs(N, n, dev, xform=False, pairs=False):
    """The raw output tensors of acrmi_pose_errors for N rows of n points, in the order it takes them."""
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    return {'e_ra': f(N, n), 'e_pa': f(N, n), 'row_f': f(N, 4), 'row_i': torch.empty(N, 2, dtype=torch.int32, device=dev),
            'xform': f(N, 8) if xform else None, 'pair_err': f(N // 2) if pairs else None}


def score_result(raw):
    """The raw outputs -> the dict pose_errors returns (views, no copy, no host visit)."""
    rf, ri = raw['row_f'], raw['row_i']
    res = {'e_ra': raw['e_ra'], 'e_pa': raw['e_pa'], 'row_f': rf, 'row_i': ri, 'mean_ra': rf[:, 0], 'mean_pa': rf[:, 1],
           'scale': rf[:, 2], 'root_err': rf[:, 3], 'n_ra': ri[:, 0], 'n_pa': ri[:, 1]}
    res.update({k: raw[k] for k in ('xform', 'pair_err') if raw.get(k) is not None})
    return res


def pose_errors(pred, gt, valid=None, root=-1, origin=None, group=None, flags=None, trans=None, n_groups=1, xform=False,
                pairs=False):
    """Errors of predicted against true points on the GPU (acrmi_pose_errors; the rule: DESIGN.md section 21): per point the
    root-aligned error and the error after the best similarity transform (Procrustes, Horn's quaternion method, six Jacobi
    sweeps), fp64 arithmetic on fp32 inputs.  pred, gt [N,n,3] device fp32 (a row = one hand, n <= 4000); valid [N,n] (non-zero =
    the point counts) or None; root: the index of the point both sets are centred on, or -1: then origin = (pred origins
    [N,3], gt origins [N,3]) or None = no alignment.  group int32 [N] with n_groups: a row is scored when its group is in [0,
    n_groups) and its flag (flags fp32 [N], None = all set) is > 0.5.  trans [N,3]: the camera translation of every row, for
    the absolute root error and - pairs=True, rows 2p and 2p + 1 the left and right hand of pair p - the MRRPE terms.
    Returns device tensors, nothing is copied to the host: 'e_ra', 'e_pa' [N,n] (-1 = not counted), 'row_f' [N,4] = ('mean_ra',
    'mean_pa', 'scale', 'root_err'), 'row_i' int32 [N,2] = ('n_ra', 'n_pa'), and with xform=True 'xform' [N,8] (quaternion w x y
    z, scale, translation: pred -> gt), with pairs=True 'pair_err' [N // 2]."""
    _need_cuda(pred)
    if pred.dim() != 3 or pred.shape[-1] != 3 or tuple(gt.shape) != tuple(pred.shape):
        raise ValueError('pred and gt must be [N,n,3], shaped alike')
    dev = pred.device
    N, n, _ = pred.shape
    if not 1 <= n <= 4000:
        raise ValueError('n = %d: 1..4000 points' % n)
    root = int(root)
    if not -1 <= root < n:
        raise ValueError('root %d outside -1..%d' % (root, n - 1))
    f32 = lambda t, shape, name: _score_arg(t, dev, torch.float32, shape, name)
    p, g = pred.to(dev, torch.float32).contiguous(), gt.to(dev, torch.float32).contiguous()
    v = _score_arg(valid, dev, torch.uint8, (N, n), 'valid', as_bool=True)
    if origin is not None and len(origin) != 2:
        raise ValueError('origin is a pair (pred origins, gt origins), each [N,3]')
    o = [None, None] if origin is None else [f32(t, (N, 3), 'origin') for t in origin]
    t, fl = f32(trans, (N, 3), 'trans'), f32(flags, (N,), 'flags')
    gr = _score_arg(group, dev, torch.int32, (N,), 'group')
    raw = score_outputs(N, n, dev, xform, pairs)
    _lib.check(_lib.lib().acrmi_pose_errors(_p(p), _p(g), _p(v), N, n, root, _p(o[0]), _p(o[1]), _p(t), _p(gr), int(n_groups), _p(fl),
                                            *[_p(x) for x in raw.values()], _s(p)))
    return score_result(raw)


def _score_arg(t, dev, dtype, shape, name, as_bool=False):
    """An optional argument of the scoring calls on the device, contiguous, of `dtype` and `shape` (None stays None)."""
    if t is None:
        return None
    t = torch.as_tensor(t)
    if tuple(t.shape) != tuple(shape):
        raise ValueError('%s must be %s, got %s' % (name, list(shape), list(t.shape)))
    if as_bool and t.dtype != torch.uint8:
        t = t != 0
    return t.to(dev, dtype).contiguous()


def score_accumulate(board, pair_board, res, n_groups, n_bins, bin_width, group=None, flags=None, stream=None):
    """Adds the rows of one pose_errors result `res` to a board (acrmi_score_accumulate): board / pair_board are int64 device
    tensors of acrmi_score_board_bytes / acrmi_score_pair_bytes (pair_board may be None); group and flags as pose_errors took
    them.  Asynchronous; engine.ScoreBoard is the object that owns such buffers."""
    e = res['e_ra']
    N, n = e.shape
    dev = e.device
    gr = _score_arg(group, dev, torch.int32, (N,), 'group')
    fl = _score_arg(flags, dev, torch.float32, (N,), 'flags')
    _lib.check(_lib.lib().acrmi_score_accumulate(_p(e), _p(res['e_pa']), N, n, _p(gr), int(n_groups), _p(fl), _p(res.get('pair_err')),
                                                 int(n_bins), float(bin_width), _p(board), _p(pair_board),
                                                 _s(e) if stream is None else C.c_void_p(stream)))


# ---- matching decoded hands to ground truth (csrc/match.hip) ----------------------------------------
def match_outputs(B, K, G, dev):
    """The raw output tensors of acrmi_match_hands, in the order it takes them."""
    i = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    return {'match': i(B, K, 2), 'pred_of': i(B, G, 2), 'cost': torch.empty(B, K, 2, dtype=torch.float32, device=dev),
            'counts': i(B, 2, 3), 'group': i(B, G, 2)}


def check_match_params(gate, min_points, n):
    """gate finite and >= 0, or +inf; min_points an integer in 1..n; else ValueError.  -> (float, int)."""
    gate = float(gate)
    if not gate >= 0:
        raise ValueError('gate %r: finite and >= 0, or inf' % (gate,))
    if int(min_points) != min_points or not 1 <= min_points <= n:
        raise ValueError('min_points %r: an integer in 1..%d' % (min_points, n))
    return gate, int(min_points)


def match_hands(pred, truth, flags=None, valid=None, truth_valid=None, trans=None, group=None, gate=float('inf'), min_points=1):
    """The exact assignment of predicted to true hands per (frame, side) on the GPU (acrmi_match_hands; the rule: DESIGN.md
    section 24): pred [B,K,2,n,D], truth [B,G,2,n,D] device fp32 (K, G in 1..8, n <= 256, D = 2 or 3); the cost of a pair is the
    mean distance over its counted points, the matching has the most allowed pairs and among those the smallest cost sum.
    flags fp32 [B,K,2] (a prediction is looked at when its flag is > 0.5; None = all; a strided view such as slots[..., 0] is
    read in place), valid [B,G,2,n] (non-zero = the point counts), truth_valid [B,G,2], trans [B,K,2,D] (added to the
    prediction), group int32 [B,G,2] (default the side), gate: the largest cost of an allowed pair, min_points: the fewest
    counted points of one.  Returns device tensors, nothing is copied to the host: 'match' int32 [B,K,2] (the truth of each
    prediction or -1), 'pred_of' int32 [B,G,2], 'cost' fp32 [B,K,2] (-1 = unmatched), 'counts' int32 [B,2,3] (TP, FP, FN per
    side), 'group' int32 [B,G,2] (-1 where the truth is not valid)."""
    _need_cuda(pred, truth)
    if pred.dim() != 5 or truth.dim() != 5 or pred.shape[2] != 2 or tuple(truth.shape[2:]) != tuple(pred.shape[2:]) or \
            truth.shape[0] != pred.shape[0]:
        raise ValueError('pred must be [B,K,2,n,D] and truth [B,G,2,n,D]')
    dev = pred.device
    B, K, _, n, D = pred.shape
    G = truth.shape[1]
    if not (1 <= K <= 8 and 1 <= G <= 8 and 1 <= n <= 256 and D in (2, 3)):
        raise ValueError('K = %d, G = %d in 1..8, n = %d in 1..256, D = %d in (2, 3)' % (K, G, n, D))
    gate, min_points = check_match_params(gate, min_points, n)
    p, t = pred.to(dev, torch.float32).contiguous(), truth.to(dev, torch.float32).contiguous()
    v = _score_arg(valid, dev, torch.uint8, (B, G, 2, n), 'valid', as_bool=True)
    tv = _score_arg(truth_valid, dev, torch.uint8, (B, G, 2), 'truth_valid', as_bool=True)
    tr = _score_arg(trans, dev, torch.float32, (B, K, 2, D), 'trans')
    gr = _score_arg(group, dev, torch.int32, (B, G, 2), 'group')
    fl, stride = _match_flags(flags, B, K, dev)
    raw = match_outputs(B, K, G, dev)
    _lib.check(_lib.lib().acrmi_match_hands(_p(p), _p(t), _p(v), _p(tv), _p(fl), stride, _p(tr), _p(gr), B, K, G, n, D, gate, min_points,
                                            *[_p(x) for x in raw.values()], _s(p)))
    return raw


def _match_flags(flags, B, K, dev):
    """flags [B,K,2] -> (the tensor whose data pointer the library reads, the stride in floats between two flags).  An fp32
    device view whose [B,K,2] elements lie a constant number of floats apart is read in place, anything else is copied."""
    if flags is None:
        return None, 1
    flags = torch.as_tensor(flags)
    if tuple(flags.shape) != (B, K, 2):
        raise ValueError('flags must be %s, got %s' % ([B, K, 2], list(flags.shape)))
    if flags.dtype == torch.float32 and flags.device == dev and B * K * 2 > 0:
        st = flags.stride()
        step = st[2]
        if step >= 1 and st[1] == 2 * step and st[0] == 2 * K * step:
            return flags, int(step)
    return flags.to(dev, torch.float32).contiguous(), 1


def match_gather(src, index):
    """dst[b,q,s,...] = src[b, index[b,q,s], s, ...] on the GPU (acrmi_match_gather): src fp32 [B,Ks,2,...], index int32 [B,Kd,2]
    -> [B,Kd,2,...]; an index outside [0, Ks) gives a row of zeros (every index is range-checked on the device)."""
    _need_cuda(src, index)
    if src.dim() < 3 or src.shape[2] != 2 or index.dim() != 3 or index.shape[0] != src.shape[0] or index.shape[2] != 2:
        raise ValueError('src must be [B,Ks,2,...] and index [B,Kd,2]')
    if src.dtype != torch.float32:
        raise ValueError('src must be float32, got %s' % src.dtype)
    B, Ks, Kd = src.shape[0], src.shape[1], index.shape[1]
    tail = tuple(src.shape[3:])
    W = 1
    for d in tail:
        W *= d
    if not (1 <= Ks <= 8 and 1 <= Kd <= 8 and W >= 1):
        raise ValueError('Ks = %d, Kd = %d in 1..8, rows of at least one float' % (Ks, Kd))
    s, ix = src.contiguous(), index.to(src.device, torch.int32).contiguous()
    dst = torch.empty((B, Kd, 2) + tail, dtype=torch.float32, device=src.device)
    _lib.check(_lib.lib().acrmi_match_gather(_p(s), _p(ix), B, Ks, Kd, W, _p(dst), _s(s)))
    return dst


def match_accumulate(board_words, counts, cost, stream=None):
    """Adds 'counts' [B,2,3] and 'cost' [B,K,2] of one match_hands result to a board (acrmi_match_accumulate): board_words an
    int64 device tensor of acrmi_match_board_bytes.  Asynchronous; engine.MatchBoard is the object that owns such a buffer."""
    _need_cuda(board_words, counts, cost)
    if counts.dim() != 3 or tuple(counts.shape[1:]) != (2, 3) or cost.dim() != 3 or cost.shape[0] != counts.shape[0] or cost.shape[2] != 2:
        raise ValueError('counts must be [B,2,3] and cost [B,K,2]')
    if board_words.dtype != torch.int64 or board_words.numel() != 8 or not board_words.is_contiguous():
        raise ValueError('board_words must be a contiguous int64 tensor of 8 words')
    c, f = counts.to(torch.int32).contiguous(), cost.to(torch.float32).contiguous()
    _lib.check(_lib.lib().acrmi_match_accumulate(_p(c), _p(f), c.shape[0], f.shape[1], _p(board_words),
                                                 _s(c) if stream is None else C.c_void_p(stream)))


# ---- key-point skeleton and heat-map views (csrc/overlay.hip; DESIGN.md "Key-point and heat-map views") ----------------
# mano/skeleton.txt (first 21 rows) of the reference: five fingers of four joints, tip to base, then the wrist (no parent)
SKELETON_PARENTS = (1, 2, 3, 20, 5, 6, 7, 20, 9, 10, 11, 20, 13, 14, 15, 20, 17, 18, 19, 20, -1)
# skeleton joint i is MANO joint MANO2INTERHAND[i] (acr/visualization.py:25)
MANO2INTERHAND = (4, 3, 2, 1, 8, 7, 6, 5, 12, 11, 10, 9, 16, 15, 14, 13, 20, 19, 18, 17, 0)
# get_keypoint_rgb (acr/visualization.py:331-381) for that skeleton, by skeleton joint
SKELETON_COLORS_RGB = ((230, 230, 0), (255, 51, 51), (255, 102, 102), (255, 153, 153),
                       (230, 230, 0), (51, 255, 51), (102, 255, 102), (153, 255, 153),
                       (230, 230, 0), (255, 153, 51), (255, 178, 102), (255, 204, 153),
                       (230, 230, 0), (51, 153, 255), (102, 178, 255), (153, 204, 255),
                       (230, 230, 0), (255, 51, 255), (255, 102, 255), (255, 153, 255), (230, 230, 0))


def overlay_tables(bgr=False):
    """The library's default tables (acrmi_overlay_tables; pure host): (colors uint8 [21,3] by skeleton joint, lut uint8
    [256,3] - the piece-wise linear jet of include/acrmi.h), RGB or flipped."""
    colors, lut = np.empty((21, 3), np.uint8), np.empty((256, 3), np.uint8)
    _lib.check(_lib.lib().acrmi_overlay_tables(int(bool(bgr)), colors.ctypes.data_as(C.c_void_p), lut.ctypes.data_as(C.c_void_p)))
    return colors, lut


def _check_images(images, name='images'):
    if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3 \
            or images.shape[0] < 1:
        raise ValueError('%s must be a uint8 tensor [N,H,W,3]' % name)


def _check_dst(dst, src, name='dst'):
    if dst.dtype != torch.uint8 or tuple(dst.shape) != tuple(src.shape) or not dst.is_contiguous() or dst.device != src.device:
        raise ValueError('%s must be a contiguous uint8 tensor shaped like images, on their device' % name)


def draw_skeletons(kps, images, hand_frame=None, colors=None, line_width=3, circle_rad=3, bgr=False, dst=None):
    """Draws the 21 key points of M hands as coloured skeletons over N equal-sized frames on the GPU (acrmi_draw_skeletons;
    the reference's Visualizer 'pj2d' view, acr/visualization.py:228-278, with the integer rule of DESIGN.md "Key-point and
    heat-map views").  kps [M,21,2] device fp32, pixels of the image, MANO joint order; images uint8 [N,H,W,3] device;
    hand_frame [M] = the frame each hand is drawn into, -1 = not drawn (default: hand m into frame m // (M / N));
    colors uint8 [21,3] by skeleton joint in the images' channel order (default: the reference's, flipped with bgr=True);
    dst: uint8 tensor like images to draw into (may BE images: in place).  Returns dst."""
    _check_images(images)
    if not isinstance(kps, torch.Tensor) or kps.dim() != 3 or tuple(kps.shape[1:]) != (21, 2) or kps.shape[0] < 1 or \
            kps.dtype != torch.float32:
        raise ValueError('kps must be a float32 tensor [M,21,2]')
    _need_cuda(kps, images, dst)
    dev = images.device
    M, N = kps.shape[0], images.shape[0]
    if hand_frame is None:
        if M % N:
            raise ValueError('hand_frame is needed when the frames do not divide the hands')
        hand_frame = torch.arange(M, dtype=torch.int32) // (M // N)
    hf = torch.as_tensor(hand_frame).to(dev, torch.int32).contiguous()
    if hf.numel() != M:
        raise ValueError('hand_frame must hold one int per hand')
    col = None
    if colors is not None:
        col = np.ascontiguousarray(np.asarray(colors.cpu() if hasattr(colors, 'cpu') else colors))
        if col.shape != (21, 3) or col.dtype != np.uint8:
            raise ValueError('colors must be uint8 [21,3]')
    k = kps.to(dev).contiguous()
    src = images.contiguous()
    if dst is None:
        dst = torch.empty_like(src)
    else:
        _check_dst(dst, src)
    _lib.check(_lib.lib().acrmi_draw_skeletons(_p(k), _p(hf), M, None if col is None else col.ctypes.data_as(C.c_void_p),
                                               int(bool(bgr)), int(line_width), int(circle_rad), _p(src), _p(dst), N,
                                               src.shape[1], src.shape[2], _s(src)))
    return dst


def _maps_arg(maps, images, n, per, rows=None):
    """The maps of draw_heatmaps / draw_region_heatmaps, checked -> (fp32, contiguous, on the images' device; pointer to the
    right maps or None; whether there are two per row)."""
    if not isinstance(maps, torch.Tensor) or not maps.is_floating_point() or maps.dim() not in (3, 4) or \
            (maps.dim() == 4 and maps.shape[1] != 2) or maps.shape[0] < 1 or (rows is not None and maps.shape[0] != rows):
        raise ValueError('maps must be a float tensor [%s,2,h,w] or [%s,h,w] with one row per %s' % (n, n, per))
    m = maps.to(images.device, torch.float32).contiguous()      # (16-bit maps convert exactly)
    two = m.dim() == 4
    return m, C.c_void_p(m.data_ptr() + 4 * m.shape[-2] * m.shape[-1]) if two else None, two


def draw_heatmaps(maps, images, view=None, weight=0.7, bgr=False, lut=None):
    """Heat maps in false colour over N frames on the GPU (acrmi_draw_heatmaps; the reference's 'centermap' view,
    acr/visualization.py:246-300: bilinear to the frame, * 255 truncated to a byte, colour table, weight * colour +
    (1 - weight) * frame - rule and table in DESIGN.md "Key-point and heat-map views"; the table is a piece-wise linear
    jet, not cv2's).  maps device float [N,2,h,w] (left, right: one launch, the frames are read once) or [N,h,w];
    images uint8 [N,H,W,3] device; view [N,4] (view_from_offsets) = where the 512 canvas the maps cover sits in the frames,
    None = it is the whole frame.  lut: uint8 [256,3] in the images' channel order (default: the library's, flipped with
    bgr=True).  Returns uint8 [2,N,H,W,3] for [N,2,h,w] maps, [N,H,W,3] for [N,h,w]."""
    _check_images(images)
    m, right, two = _maps_arg(maps, images, 'N', 'image', images.shape[0])
    _need_cuda(maps, images)
    dev = images.device
    N, H, W, _ = images.shape
    h, w = m.shape[-2:]
    vw = None
    if view is not None:
        vw = torch.as_tensor(view, dtype=torch.float32).to(dev).contiguous()
        if tuple(vw.shape) != (N, 4):
            raise ValueError('view must be [N,4]')
    tab = _lut_arg(lut)
    src = images.contiguous()
    out = torch.empty((2 if two else 1, N, H, W, 3), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().acrmi_draw_heatmaps(_p(m), right, (2 if two else 1) * h * w, N, h, w, _p(vw), float(weight),
                                              None if tab is None else tab.ctypes.data_as(C.c_void_p), int(bool(bgr)),
                                              _p(src), _p(out[0]), _p(out[1]) if two else None, H, W, _s(src)))
    return out if two else out[0]


def check_regions(offsets, region_frame, n=None):
    """`offsets` [n,10] and `region_frame` [n] of views over regions, checked on the host without reading them: -> (n, offsets,
    region_frame) with lists / numpy turned into CPU tensors of the right type.  Device tensors pass as they are."""
    o = offsets if isinstance(offsets, torch.Tensor) else torch.as_tensor(np.asarray(offsets, np.float32))
    if o.dim() != 2 or o.shape[1] != 10 or o.shape[0] < 1 or (n is not None and o.shape[0] != n):
        raise ValueError('offsets must be [n,10], one row per region%s (got %s)' % ('' if n is None else ': n = %d' % n, tuple(o.shape)))
    n = o.shape[0]
    rf = region_frame if isinstance(region_frame, torch.Tensor) else torch.as_tensor(np.asarray(region_frame))
    if rf.dim() != 1 or rf.shape[0] != n or rf.is_floating_point() or rf.dtype == torch.bool:
        raise ValueError('region_frame must hold one integer per region: [%d] (got %s %s)' % (n, rf.dtype, tuple(rf.shape)))
    return n, o, rf


def draw_region_heatmaps(maps, images, offsets, region_frame, weight=0.7, bgr=False, lut=None, dst=None):
    """Heat maps of n REGIONS of interest in false colour over the N frames they were cut from (acrmi_draw_region_heatmaps;
    DESIGN.md "Views over regions").  maps device float [n,2,h,w] (left, right) or [n,h,w], one per region; images uint8
    [N,H,W,3] device; offsets [n,10] = the regions' `offsets` rows and region_frame [n] = the frame of each (host values or
    device tensors: the kernel reads them).  Region i tints the pixels of ITS window in frame region_frame[i] as
    draw_heatmaps would with view_from_offsets(offsets[i]); where windows overlap the larger colour index wins; every other
    pixel is the input byte for byte.  weight, bgr, lut: as draw_heatmaps.  dst: uint8 [2,N,H,W,3] (or [N,H,W,3] for [n,h,w]
    maps) to draw into; dst[0] (dst) may BE images.  Returns uint8 [2,N,H,W,3], or [N,H,W,3] for [n,h,w] maps."""
    _check_images(images)
    m, rp, two = _maps_arg(maps, images, 'n', 'region')
    n, o, rf = check_regions(offsets, region_frame, maps.shape[0])
    _need_cuda(maps, images)
    dev = images.device
    N, H, W, _ = images.shape
    h, w = m.shape[-2:]
    o = o.to(dev, torch.float32).contiguous()
    rf = rf.to(dev, torch.int32).contiguous()
    tab = _lut_arg(lut)
    src = images.contiguous()
    shape = (2, N, H, W, 3) if two else (N, H, W, 3)
    if dst is None:
        dst = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif dst.dtype != torch.uint8 or tuple(dst.shape) != shape or not dst.is_contiguous() or dst.device != dev:
        raise ValueError('dst must be a contiguous uint8 tensor %s on the images\' device' % (shape,))
    left, right = (dst[0], dst[1]) if two else (dst, None)
    _lib.check(_lib.lib().acrmi_draw_region_heatmaps(_p(m), rp, (2 if two else 1) * h * w, n, h, w, _p(o), _p(rf), float(weight),
                                                     None if tab is None else tab.ctypes.data_as(C.c_void_p), int(bool(bgr)),
                                                     _p(src), _p(left), _p(right), N, H, W, _s(src)))
    return dst


# ---- the part segmentation as an output (csrc/segm_plan.h) ----------------------------------------
SEGM_NONE = _lib.SEGM_NONE


def segm_colors(classes=33, bgr=False):
    """The default colours of the 'segm' view, uint8 [classes,3] (acrmi_segm_tables): right parts on the upper half of the heat
    maps' jet, left parts on the lower half, row 0 (background, never drawn) zero."""
    tab = np.zeros((int(classes), 3), np.uint8)
    _lib.check(_lib.lib().acrmi_segm_tables(int(bool(bgr)), int(classes), tab.ctypes.data_as(C.c_void_p)))
    return tab


def _segm_logits(logits, classes):
    """logits NHWC [N,h,w,cs] fp32 on the device, possibly a channel slice of a wider buffer -> (tensor, classes, pix_stride,
    frame_stride)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 4 or logits.dtype != torch.float32:
        raise ValueError('logits must be a float32 tensor [N,h,w,C] (NHWC)')
    _need_cuda(logits)
    N, h, w, cs = logits.shape
    st = logits.stride()
    if st[3] != 1 or (w > 1 and st[1] != w * st[2]) or st[2] < cs or (N > 1 and st[0] < h * w * st[2]):
        logits = logits.contiguous()
        st = logits.stride()
    return logits, int(cs if classes is None else classes), int(st[2]), int(st[0]) if N > 1 else int(max(st[0], h * w * st[2]))


def _segm_call(logits, classes, hw, images, view, offsets, weight, bgr, colors, dst, labels, stream=None):
    logits, Cn, ps, fs = _segm_logits(logits, classes)
    N, h, w, _ = logits.shape
    dev = logits.device
    src = out = None
    if images is not None:
        _check_images(images)
        _need_cuda(images)
        if images.shape[0] != N:
            raise ValueError('one image per frame of logits')
        src = images.contiguous()
        H, W = src.shape[1:3]
        if dst is None:
            out = torch.empty_like(src)
        else:
            _check_dst(dst, src)
            out = dst
    else:
        H, W = (512, 512) if hw is None else (int(hw[0]), int(hw[1]))
    if view is not None and offsets is not None:
        raise ValueError('view or offsets, not both')
    vw = off = None
    if view is not None:
        vw = torch.as_tensor(view, dtype=torch.float32).to(dev).contiguous()
        if tuple(vw.shape) != (N, 4):
            raise ValueError('view must be [N,4]')
    if offsets is not None:
        off = torch.as_tensor(offsets, dtype=torch.float32).to(dev).contiguous()
        if tuple(off.shape) != (N, 10):
            raise ValueError('offsets must be [N,10]')
    tab = None
    if colors is not None:
        tab = np.ascontiguousarray(np.asarray(colors.cpu() if hasattr(colors, 'cpu') else colors))
        if tab.shape != (Cn, 3) or tab.dtype != np.uint8:
            raise ValueError('colors must be uint8 [%d,3]' % Cn)
    lab = torch.empty((N, H, W), dtype=torch.uint8, device=dev) if labels else None
    _lib.check(_lib.lib().acrmi_segm_labels(_p(logits), fs, ps, N, h, w, Cn, _p(vw), _p(off), float(weight),
                                            None if tab is None else tab.ctypes.data_as(C.c_void_p), int(bool(bgr)), _p(src), _p(out),
                                            _p(lab), H, W, _s(logits) if stream is None else C.c_void_p(stream)))
    return out, lab


def segm_labels(logits, hw=None, view=None, offsets=None, classes=None):
    """Part logits -> a label per pixel of N frames of hw = (H, W) pixels (default 512 x 512) on the GPU (acrmi_segm_labels;
    DESIGN.md section 23): the bilinear LOGITS of every class at the pixel's canvas coordinate, then the strict arg-max (the
    lowest class wins a tie, a NaN never wins) - not nearest labels.  logits device fp32 NHWC [N,h,w,C] (a channel slice of
    a wider buffer is read in place; classes: the first `classes` channels, default all), C odd in 3..63.  view [N,4]
    (view_from_offsets) or offsets [N,10]: where the 512 canvas the map covers sits in the frames; neither: it is the whole
    frame.  Label 0 = background, 1 .. (C-1)/2 the right hand's parts, the rest the left hand's; SEGM_NONE (255) where the
    canvas does not cover the pixel.  Returns uint8 [N,H,W]."""
    return _segm_call(logits, classes, hw, None, view, offsets, 0.7, False, None, None, True)[1]


def draw_segm(logits, images, view=None, offsets=None, weight=0.7, bgr=False, colors=None, dst=None, labels=False, classes=None):
    """The part labels of segm_labels in colour over N frames, in the same launch (acrmi_segm_labels): a pixel with a hand
    part's label becomes floor(weight * colour[label] + (1 - weight) * pixel), every other pixel stays byte for byte.  images
    uint8 [N,H,W,3] device; colors uint8 [C,3] in the images' channel order (default segm_colors(C, bgr)); dst: tensor like
    images to draw into (may BE images).  Returns the frames, or (frames, labels uint8 [N,H,W]) with labels=True."""
    if images is None:
        raise ValueError('images: the frames to draw over')
    out, lab = _segm_call(logits, classes, None, images, view, offsets, weight, bgr, colors, dst, labels)
    return (out, lab) if labels else out


def segm_stats(labels, classes=33, ids=None, n_faces=None, stream=None):
    """Statistics of label maps uint8 [N,H,W] on the GPU (acrmi_segm_stats) -> {'counts': int32 [N,C]
    pixels per label (255 is not counted), 'boxes': int32 [N,2,4] the smallest (l, t, r, b) around each side's pixels (side 0
    left, 1 right; r, b exclusive; zeros when the side has none)}, and with ids - int32 [N,H,W] of render(...,
    return_ids=True) for the same frames, n_faces the faces of a mesh - 'agree': int32 [N,2,3] = (pixels in mask and silhouette,
    mask pixels, silhouette pixels) per side.  Integers only; IoU = inter / (mask + sil - inter) is the caller's division."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.dim() != 3:
        raise ValueError('labels must be a uint8 tensor [N,H,W]')
    _need_cuda(labels, ids)
    lab = labels.contiguous()
    N, H, W = lab.shape
    dev = lab.device
    if ids is not None:
        if ids.dtype != torch.int32 or tuple(ids.shape) != (N, H, W):
            raise ValueError('ids must be int32 [N,H,W] like labels')
        if n_faces is None or int(n_faces) <= 0:
            raise ValueError('ids needs n_faces, the number of faces of a mesh')
        ids = ids.contiguous()
    L = _lib.lib()
    ws = torch.empty(max(int(L.acrmi_segm_stats_ws_ints(N, H, W)), 1), dtype=torch.int32, device=dev)
    res = {'counts': torch.empty(N, int(classes), dtype=torch.int32, device=dev),
           'boxes': torch.empty(N, 2, 4, dtype=torch.int32, device=dev)}
    if ids is not None:
        res['agree'] = torch.empty(N, 2, 3, dtype=torch.int32, device=dev)
    _lib.check(L.acrmi_segm_stats(_p(lab), _p(ids), int(n_faces or 0), N, H, W, int(classes), _p(res['counts']), _p(res['boxes']),
                                  _p(res.get('agree')), _p(ws), _s(lab) if stream is None else C.c_void_p(stream)))
    return res
