"""Thin functional wrappers over the C-ABI HIP library: shape checks on the host, raw pointers down.

Every function here requires CUDA (=HIP) tensors and enqueues on torch's current stream.  No
fallbacks: a CPU tensor or a missing library raises ``HipLibraryError``.
"""
import ctypes
import math
import os
from ctypes import c_float, c_int, c_long, c_void_p

import numpy as np
import torch

from ._lib import check, lib, lib_color_jitter, lib_weight_average, ptr, require_cuda, stream_ptr, to_device_async

DT = {torch.bfloat16: 0, torch.float32: 1}

_L = lib      # the loaded library, every entry point typed from include/cddmsl_hip.h (_lib.py)


class _Profiler:
    """Optional per-kernel timing with HIP events recorded on the launch stream (torch's current stream is the
    stream every kernel of this library is enqueued on).  Used by bench.py for the roofline object."""

    def __init__(self):
        self.on = False
        self.only = None
        self.events = []
        self.shapes = []

    def enable(self, only=None):
        """``only``: a set of profiler row names -- launches of other kernels record no events at all (an event pair per
        launch on ~1000 launches costs ~5 % of the step; inside bench.py's timed region only the dominant kernel is timed)."""
        self.on, self.only, self.events, self.shapes = True, (set(only) if only else None), [], []

    def begin(self, name=None, plan=None):
        """``name``: the row this launch will be booked under, if known before the launch; ``plan``: a callable that runs
        the entry point in plan-only mode (no launch) for entry points whose kernel is chosen inside the library."""
        if not self.on:
            return None
        if self.only is not None:
            if name is None and plan is not None:
                L = _L()
                L.cddmsl_plan_only(1)
                try:
                    plan()
                finally:
                    L.cddmsl_plan_only(0)
                name = _CONV_KERNEL.get(L.cddmsl_last_kernel())
            if name not in self.only:
                return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def end(self, e0, name, flops=0.0, shape=None, nbytes=0.0):
        if e0 is None:
            return
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.events.append((name, flops, e0, e1, nbytes))
        if shape is not None:
            self.shapes.append((name, shape, flops, e0, e1, nbytes))

    def by_shape(self):
        """(name, shape) -> [launches, ms, flops, algorithmic bytes]; call before collect()."""
        torch.cuda.synchronize()
        out = {}
        for name, shape, flops, e0, e1, nbytes in self.shapes:
            d = out.setdefault((name, shape), [0, 0.0, 0.0, 0.0])
            d[0] += 1
            d[1] += e0.elapsed_time(e1)
            d[2] += flops
            d[3] += nbytes
        return out

    def collect(self):
        torch.cuda.synchronize()
        out = {}
        for name, flops, e0, e1, nbytes in self.events:
            d = out.setdefault(name, {"flops": 0.0, "ms": 0.0, "launches": 0, "bytes": 0.0})
            d["flops"] += flops
            d["bytes"] += nbytes
            d["ms"] += e0.elapsed_time(e1)
            d["launches"] += 1
        self.on, self.only, self.events = False, None, []
        return out


PROFILE = _Profiler()
# cddmsl_last_kernel() ids -> profiler row names (one row per KERNEL, so the roofline object describes one kernel)
_CONV_KERNEL = {10: "k_conv_fwd256_fp8", 11: "k_conv_fwd2", 1: "k_conv_fwd", 2: "k_conv_fwd_reg", 3: "k_conv_fwd256", 4: "k_conv_wgrad", 5: "k_conv_wgrad_dma", 6: "k_wgrad256", 7: "k_gemm_tn_stream", 8: "k_conv3x3_small", 9: "k_gemm_tn_small", 12: "k_wgrad256_fp8",
                13: "k_bottleneck64"}


def _timed(name):
    def deco(fn):
        def wrapper(*a, **k):
            e0 = PROFILE.begin(name)
            r = fn(*a, **k)
            PROFILE.end(e0, name)
            return r
        wrapper.__name__, wrapper.__doc__ = fn.__name__, fn.__doc__
        return wrapper
    return deco


def _dt(t):
    if t.dtype not in DT:
        raise TypeError(f"unsupported dtype {t.dtype}: the kernels compute in bf16 or f32")
    return DT[t.dtype]


def _conv_input_pixels(N, H, W, Ho, Wo, KH, KW, stride, pool):
    """input pixels a convolution reads at least once (rows x columns its taps cover, per image)"""
    if pool:
        return N * min(H, 2 * Ho) * min(W, 2 * Wo)
    rows = min(H, Ho * min(KH, stride) if stride > KH else (Ho - 1) * stride + KH)
    cols = min(W, Wo * min(KW, stride) if stride > KW else (Wo - 1) * stride + KW)
    return N * rows * cols


class OutSpec:
    """Where a convolution puts its result when two launches' outputs have to end up adjacent (rows [0, N) and [N, 2N) of ONE
    buffer) without a concatenation copy: the first launch (``full`` None) allocates the double buffer, writes its half and
    records it; the second (``full`` set) writes rows [N, 2N).  Anything that does not fit leaves ``full`` / ``used`` untouched
    and the caller falls back to ``torch.cat``."""

    def __init__(self):
        self.full, self.used = None, 0


def conv_fwd(x, w, scale=None, bias=None, residual=None, relu=False, relu_mask=None, stride=1, pad=0,
             pool=False, out_f32=False, residual_pooled=False, emit8=None, out_spec=None):
    """x NHWC [N,H,W,Cin]; w [Cout,KH,KW,Cin] (same dtype).  Returns NHWC [N,Ho,Wo,Cout].
    y = relu?(acc*scale[n] + bias[n] + residual), zeroed where relu_mask <= 0 (ReLU backward).
    pool=True: 1x1 conv over the 2x2 average-pooled input (AvgPool2d(2) fused into the loader).
    residual_pooled=True: ``residual`` is [N, Ho//2, Wo//2, Cout] and every output pixel adds a quarter of its pooled pixel
    (the backward of AvgPool2d(2) fused into the epilogue; pooled tensor < 2 GiB -- see ``pooled_residual_ok``)."""
    require_cuda(x, w, scale, bias, residual, relu_mask)
    ensure_workspace(x.device)                       # (the split-K tail of badly quantised launches goes through it)
    assert x.dim() == 4 and w.dim() == 4 and x.is_contiguous() and w.is_contiguous()
    assert x.dtype == w.dtype
    N, H, W, Cin = x.shape
    Cout, KH, KW, Cin2 = w.shape
    assert Cin == Cin2, (x.shape, w.shape)
    if pool:
        Ho, Wo = H // 2, W // 2
    else:
        Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    ydt = torch.float32 if out_f32 else x.dtype
    if out_spec is not None and out_spec.full is None:
        out_spec.full = torch.empty((2 * N, Ho, Wo, Cout), device=x.device, dtype=ydt)
        y, out_spec.used = out_spec.full[:N], 1
    elif out_spec is not None and out_spec.used == 1 and tuple(out_spec.full.shape) == (2 * N, Ho, Wo, Cout) and out_spec.full.dtype == ydt:
        y, out_spec.used = out_spec.full[N:], 2
    else:
        y = torch.empty((N, Ho, Wo, Cout), device=x.device, dtype=ydt)
    for v in (scale, bias):
        assert v is None or (v.dtype == torch.float32 and v.numel() == Cout and v.is_contiguous())
    res_f32 = residual is not None and residual.dtype == torch.float32 and x.dtype != torch.float32
    if res_f32:       # f32 residual stream on the bf16 kernels: f32 output, vector epilogue
        assert out_f32 and relu_mask is None and not pool and Cout % 8 == 0
    if residual_pooled:
        assert residual is not None and not res_f32 and residual.dtype == x.dtype and residual.is_contiguous()
        assert tuple(residual.shape) == (N, Ho // 2, Wo // 2, Cout) and pooled_residual_ok(residual), residual.shape
    for v in (residual, relu_mask):
        assert v is None or (v is residual and residual_pooled) or (
            (v.dtype == x.dtype or (v is residual and res_f32)) and v.is_contiguous() and v.numel() == y.numel())
    y8 = None
    if emit8 is not None:     # fp8 configuration: (scale [1], amax [64]) of the consuming convolution's slot -> e4m3 copy of y, as y._fp8
        assert x.dtype == torch.bfloat16 and not out_f32 and not pool and not residual_pooled and not res_f32
        y8 = torch.empty(y.shape, device=x.device, dtype=torch.uint8)

    def launch():
        if y8 is not None:
            return _L().cddmsl_conv_fwd_q8(ptr(x), ptr(w), ptr(y), ptr(scale), ptr(bias), ptr(residual), ptr(relu_mask),
                                           N, H, W, Cin, Cout, KH, KW, stride, pad, int(relu), ptr(y8), ptr(emit8[0]), ptr(emit8[1]), stream_ptr())
        return _L().cddmsl_conv_fwd(ptr(x), ptr(w), ptr(y), ptr(scale), ptr(bias), ptr(residual), ptr(relu_mask),
                                    N, H, W, Cin, Cout, KH, KW, stride, pad, int(pool), Cout, Cout, Cout,
                                    int(relu), int(out_f32) | (2 if res_f32 else 0) | (4 if residual_pooled else 0), _dt(x), stream_ptr())
    e0 = PROFILE.begin(plan=launch) if PROFILE.on else None
    st = launch()
    check(st, "cddmsl_conv_fwd")
    PROFILE.end(e0, _CONV_KERNEL.get(_L().cddmsl_last_kernel(), "conv_fwd") if e0 is not None else "conv_fwd",
                2.0 * N * Ho * Wo * Cout * KH * KW * Cin,    # algorithmic 2*M*N*K
                (N * Ho * Wo, Cout, KH * KW * Cin, KH, int(pool), stride),
                # algorithmic HBM bytes: every operand once -- of x, the pixels the taps reach (a strided 1x1 convolution, e.g. the
                # attention pool's query projection over every 56th token row, reads one input row per output row, not the tensor)
                nbytes=float(_conv_input_pixels(N, H, W, Ho, Wo, KH, KW, stride, bool(pool)) * Cin * x.element_size()
                             + w.numel() * w.element_size() + y.numel() * y.element_size()
                             + (residual.numel() * residual.element_size() if residual is not None else 0)
                             + (relu_mask.numel() * relu_mask.element_size() if relu_mask is not None else 0)))
    if y8 is not None:
        y._fp8 = (y8, emit8[0].data_ptr())
    return y


def conv3x3_pool_fwd(x, w, scale, bias, relu_mask=None, stride=1):
    """The stem's third convolution and its AvgPool2d(2) in one launch: x [N,H,W,32] bf16, w [64,3,3,32] -> [N,H//2,W//2,64] =
    avgpool2_fwd(conv_fwd(x, w, scale, bias, relu=True, pad=1)), bit-identical; the full-resolution map is never written.  The library
    refuses (``HipLibraryError``) anything but that layer: f32, other widths, ``stride`` != 1, a ``relu_mask``."""
    require_cuda(x, w, scale, bias, relu_mask)
    assert x.dim() == 4 and w.dim() == 4 and x.is_contiguous() and w.is_contiguous() and x.dtype == w.dtype
    N, H, W, Cin = x.shape
    Cout, KH, KW, Cin2 = w.shape
    assert (KH, KW, Cin2) == (3, 3, Cin), (x.shape, w.shape)
    for v in (scale, bias):
        assert v is not None and v.dtype == torch.float32 and v.numel() == Cout and v.is_contiguous()
    assert relu_mask is None or (relu_mask.dtype == x.dtype and relu_mask.is_contiguous())
    y = torch.empty((N, H // 2, W // 2, Cout), device=x.device, dtype=x.dtype)

    def launch():
        return _L().cddmsl_conv3x3_pool_fwd(ptr(x), ptr(w), ptr(y), ptr(scale), ptr(bias), ptr(relu_mask), N, H, W, Cin, Cout, stride,
                                            _dt(x), stream_ptr())
    e0 = PROFILE.begin(plan=launch) if PROFILE.on else None
    check(launch(), "cddmsl_conv3x3_pool_fwd")
    # booked under the row of the unfused launch (same M, N, K: the convolution is computed at the even rows / columns in full);
    # algorithmic bytes: x and w once, the POOLED map written
    Mc = N * (H // 2) * (W // 2) * 4
    PROFILE.end(e0, "k_conv3x3_small", 2.0 * Mc * Cout * 9 * Cin, (Mc, Cout, 9 * Cin, 3, 2, 1),
                nbytes=float(x.numel() * x.element_size() + w.numel() * w.element_size() + y.numel() * y.element_size()))
    return y


def bottleneck64_ok(o1, w2, w3, wd=None, w1n=None):
    """does the fused frozen-bottleneck kernel take this block?  bf16, packed tensors, 64 planes (conv2 64 -> 64 3x3, conv3 64 -> 256,
    an optional 64 -> 256 downsample convolution and an optional 256 -> 64 conv1 of the next block), every tensor below 2 GiB."""
    if not (o1.is_cuda and o1.dtype == torch.bfloat16 and o1.dim() == 4 and o1.is_contiguous() and o1.shape[3] == 64):
        return False
    want = ((w2, (64, 3, 3, 64)), (w3, (256, 1, 1, 64)), (wd, (256, 1, 1, 64)), (w1n, (64, 1, 1, 256)))
    if any(w is not None and (tuple(w.shape) != s or w.dtype != torch.bfloat16 or not w.is_contiguous()) for w, s in want):
        return False
    N, H, W, _ = o1.shape
    return N > 0 and bool(_L().cddmsl_bottleneck64_ok(N, H, W, 0))


def bottleneck64_fwd(o1, w2, bn2, w3, bn3, residual=None, x0=None, wd=None, bnd=None, w1n=None, bn1n=None):
    """One frozen 64-plane Bottleneck behind its conv1 in one launch (``bottleneck64_ok``): o1 [N,H,W,64] -> out [N,H,W,256] =
    relu(bn3(conv3(relu(bn2(conv2(o1))))) + residual), bit-identical to the three ``conv_fwd`` launches.  The residual is given
    or, with ``wd`` / ``bnd``, computed as bnd(x0 . wd) from the block's input ``x0``.  With ``w1n`` / ``bn1n`` (conv1 of the next
    block) also returns o1n [N,H,W,64] = relu(bn1n(out . w1n)); else None.  bn* = (scale, bias) f32."""
    require_cuda(o1, w2, w3, residual, x0, wd, w1n)
    assert bottleneck64_ok(o1, w2, w3, wd, w1n) and (residual is None) != (wd is None)
    N, H, W, _ = o1.shape
    for t, c in ((residual, 256), (x0 if wd is not None else None, 64)):
        assert t is None or (t.dtype == torch.bfloat16 and t.is_contiguous() and tuple(t.shape) == (N, H, W, c))
    for bn, c in ((bn2, 64), (bn3, 256), (bnd, 256), (bn1n, 64)):
        assert bn is None or all(v.dtype == torch.float32 and v.numel() == c and v.is_contiguous() and v.is_cuda for v in bn)
    assert (wd is None) == (bnd is None) and (w1n is None) == (bn1n is None) and (wd is None or x0 is not None)
    out = torch.empty((N, H, W, 256), device=o1.device, dtype=o1.dtype)
    o1n = torch.empty((N, H, W, 64), device=o1.device, dtype=o1.dtype) if w1n is not None else None
    sd, bd = bnd if bnd is not None else (None, None)
    s1n, b1n = bn1n if bn1n is not None else (None, None)
    e0 = PROFILE.begin(name="k_bottleneck64") if PROFILE.on else None
    check(_L().cddmsl_bottleneck64_fwd(ptr(o1), ptr(w2), ptr(bn2[0]), ptr(bn2[1]), ptr(w3), ptr(bn3[0]), ptr(bn3[1]), ptr(residual),
                                       ptr(x0 if wd is not None else None), ptr(wd), ptr(sd), ptr(bd), ptr(w1n), ptr(s1n), ptr(b1n),
                                       ptr(out), ptr(o1n), N, H, W, 0, stream_ptr()), "cddmsl_bottleneck64_fwd")
    M = N * H * W
    kn = 576 * 64 + 64 * 256 + (64 * 256 if wd is not None else 0) + (256 * 64 if w1n is not None else 0)
    # algorithmic HBM bytes: o1, the residual or x0, out, o1n and the weights once each (o2 and the computed residual never exist)
    PROFILE.end(e0, "k_bottleneck64", 2.0 * M * kn, (M, 256, 576, 3, int(wd is not None), int(w1n is not None)),
                nbytes=float(2 * M * (64 + (64 if wd is not None else 256) + 256 + (64 if w1n is not None else 0)) + 2 * kn))
    return out, o1n


def conv_emit8_ok(M, Cout, KH, KW, Cin_chunks_ok=True):
    """can a bf16 launch carry the e4m3 second output? (the 256x256 kernel's epilogue writes it: whole 256-wide tiles, >= 160 tiles)"""
    return Cout % 256 == 0 and KH * KW <= 31 and ((M + 255) // 256) * (Cout // 256) >= 160 and Cin_chunks_ok and os.environ.get("CDDMSL_GEMM256", "1") != "0"


# ------------------------------------------------------------------------------------------------ e4m3 (fp8) configuration
FP8_MAX = 448.0      # largest finite OCP e4m3fn magnitude


@_timed("quantize_fp8")
def quantize_fp8(x, scale=None, amax=None):
    """x (bf16 or f32, contiguous, numel % 8 == 0) -> uint8 tensor of OCP e4m3 bytes = sat(x * scale[0]).  ``scale`` / ``amax``:
    1-element f32 device tensors; max|x| is atomically max-ed into ``amax`` (delayed scaling: next step's scale)."""
    require_cuda(x, scale, amax)
    assert x.is_contiguous() and x.dtype in (torch.bfloat16, torch.float32) and x.numel() % 8 == 0
    y = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    check(_L().cddmsl_quantize_fp8(ptr(x), ptr(y), ptr(scale), ptr(amax), x.numel(), 0 if x.dtype == torch.bfloat16 else 1, stream_ptr()),
          "cddmsl_quantize_fp8")
    return y


def conv_fwd_fp8_ok(M, Cin, Cout, KH, KW, pad):
    """shapes the e4m3 kernel takes AND wins on: whole 256-wide tiles, enough of them to fill the chip, a reduction long enough to
    be MFMA-bound in bf16 (short reductions are bound by their output traffic, which fp8 operands do not shrink)"""
    min_tiles = int(os.environ.get("CDDMSL_FP8_MIN_TILES", "160"))      # (tests lower both to reach the kernel at small sizes)
    min_k = int(os.environ.get("CDDMSL_FP8_MIN_K", "2048"))
    return Cin % 128 == 0 and Cout % 256 == 0 and KH * KW <= 31 and 2 * pad <= KH - 1 and ((M + 255) // 256) * (Cout // 256) >= min_tiles \
        and KH * KW * Cin >= min_k


def conv_fwd_fp8(x8, w8, scale=None, bias=None, residual=None, relu=False, relu_mask=None, pad=0, out_f32=False, emit8=None):
    """x8 uint8 (e4m3) NHWC [N,H,W,Cin]; w8 uint8 [Cout,KH,KW,Cin].  y (bf16, or f32) = epilogue(sum x8 * w8): ``scale`` must carry
    the two dequantisation factors (x the FrozenBN scale).  stride 1."""
    require_cuda(x8, w8, scale, bias, residual, relu_mask)
    assert x8.dtype == torch.uint8 and w8.dtype == torch.uint8 and x8.is_contiguous() and w8.is_contiguous()
    N, H, W, Cin = x8.shape
    Cout, KH, KW, Cin2 = w8.shape
    assert Cin == Cin2
    Ho, Wo = H + 2 * pad - KH + 1, W + 2 * pad - KW + 1
    y = torch.empty((N, Ho, Wo, Cout), device=x8.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    for v in (scale, bias):
        assert v is None or (v.dtype == torch.float32 and v.numel() == Cout and v.is_contiguous())
    for v in (residual, relu_mask):
        assert v is None or (v.dtype == torch.bfloat16 and v.is_contiguous() and v.numel() == y.numel())

    y8 = torch.empty(y.shape, device=x8.device, dtype=torch.uint8) if emit8 is not None else None
    assert emit8 is None or not out_f32

    def launch():
        return _L().cddmsl_conv_fwd_fp8(ptr(x8), ptr(w8), ptr(y), ptr(scale), ptr(bias), ptr(residual), ptr(relu_mask),
                                        N, H, W, Cin, Cout, KH, KW, pad, int(relu), int(out_f32), ptr(y8),
                                        ptr(emit8[0]) if emit8 else c_void_p(0), ptr(emit8[1]) if emit8 else c_void_p(0), stream_ptr())
    e0 = PROFILE.begin(name="k_conv_fwd256_fp8") if PROFILE.on else None
    check(launch(), "cddmsl_conv_fwd_fp8")
    PROFILE.end(e0, "k_conv_fwd256_fp8", 2.0 * N * Ho * Wo * Cout * KH * KW * Cin, (N * Ho * Wo, Cout, KH * KW * Cin, KH, 0, 1),
                nbytes=float(x8.numel() + w8.numel() + y.numel() * y.element_size() + (residual.numel() * 2 if residual is not None else 0)
                             + (relu_mask.numel() * 2 if relu_mask is not None else 0)))
    if y8 is not None:
        y._fp8 = (y8, emit8[0].data_ptr())
    return y


@_timed("fp8_dot_nt")
def fp8_dot_nt(a8, b8, alpha=None):
    """a8 [R,K], b8 [N,K] uint8 (e4m3), N <= 32, K % 64 == 0 -> [R,N] f32 = alpha[0] * a . b^T"""
    require_cuda(a8, b8, alpha)
    R, K = a8.shape
    N = b8.shape[0]
    assert a8.dtype == torch.uint8 and b8.dtype == torch.uint8 and a8.is_contiguous() and b8.is_contiguous() and b8.shape[1] == K
    c = torch.empty((R, N), device=a8.device, dtype=torch.float32)
    check(_L().cddmsl_fp8_dot_nt(ptr(a8), ptr(b8), ptr(c), ptr(alpha), R, N, K, N, stream_ptr()), "cddmsl_fp8_dot_nt")
    return c


def pooled_residual_ok(t):
    """the fused AvgPool2d(2)-backward residual is buffer-addressed from the tensor base: below 2 GiB, rows of whole 16-B chunks"""
    return t.numel() * t.element_size() < 2 ** 31 and t.shape[-1] % 8 == 0


def linear_fwd(x, w, scale=None, bias=None, residual=None, relu=False, relu_mask=None, out_f32=False):
    """x [M,K] @ w[N,K]^T with the conv epilogue (a 1x1 conv over M 'pixels')."""
    M, K = x.shape
    y = conv_fwd(x.view(1, 1, M, K), w.view(w.shape[0], 1, 1, K), scale, bias,
                 None if residual is None else residual.view(1, 1, M, -1), relu,
                 None if relu_mask is None else relu_mask.view(1, 1, M, -1), out_f32=out_f32)
    return y.view(M, w.shape[0])


_WORKSPACE = {}
WORKSPACE_BYTES = 288 << 20      # the largest split reduction of the 16 x 800x1333 step needs 258 MiB (1 008 blocks x 256 KiB)


def ensure_workspace(device):
    """Registers (once per device) the scratch the weight-gradient kernels' split reductions go through: see cddmsl_set_workspace."""
    key = torch.device(device).index or 0
    if key not in _WORKSPACE:
        ws = torch.empty(WORKSPACE_BYTES, dtype=torch.uint8, device=device)
        check(_L().cddmsl_set_workspace(ptr(ws), ctypes.c_long(ws.numel())), "cddmsl_set_workspace")
        _WORKSPACE[key] = ws
    return _WORKSPACE[key]


def conv_wgrad(x, dy, w_shape, scale=None, stride=1, pad=0, pool=False, out=None):
    """dW[Cout,KH,KW,Cin] (f32) += scale[n] * sum_m dY[m,n] * im2col(x)[m,k].  x NHWC, dy NHWC."""
    require_cuda(x, dy, scale, out)
    Cout, KH, KW, Cin = w_shape
    N, H, W, Cin2 = x.shape
    assert Cin == Cin2 and x.dtype == dy.dtype and x.is_contiguous() and dy.is_contiguous()
    assert dy.shape[-1] == Cout and dy.numel() // Cout == (N * (H // 2) * (W // 2) if pool else
                                                          N * ((H + 2 * pad - KH) // stride + 1) * ((W + 2 * pad - KW) // stride + 1))
    if out is None:
        out = torch.zeros(w_shape, device=x.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == tuple(w_shape)
    ensure_workspace(x.device)
    def launch():
        return _L().cddmsl_conv_wgrad(ptr(x), ptr(dy), ptr(out), ptr(scale), N, H, W, Cin, Cout, KH, KW, stride, pad,
                                      int(pool), Cout, _dt(x), stream_ptr())
    e0 = PROFILE.begin(plan=launch) if PROFILE.on else None
    st = launch()
    check(st, "cddmsl_conv_wgrad")
    PROFILE.end(e0, _CONV_KERNEL.get(_L().cddmsl_last_kernel(), "conv_wgrad") if e0 is not None else "conv_wgrad",
                2.0 * (dy.numel() // Cout) * Cout * KH * KW * Cin,
                (dy.numel() // Cout, Cout, KH * KW * Cin, KH, int(pool), stride),
                # algorithmic HBM bytes: both operands once (a long reduction into a small dW is bound by reading them, not by the MFMAs)
                nbytes=float(_conv_input_pixels(N, H, W, (H // 2) if pool else (H + 2 * pad - KH) // stride + 1,
                                                 (W // 2) if pool else (W + 2 * pad - KW) // stride + 1, KH, KW, stride, bool(pool)) * Cin * x.element_size()
                             + dy.numel() * dy.element_size() + out.numel() * 4))
    return out


def conv_wgrad_fp8_ok(M, Cin, Cout, KH, KW, pad, min_m=None, taps_only=True):
    """shapes the e4m3 weight-gradient kernel takes AND wins on: whole 256 x 256 output tiles of a "same" convolution and a reduction
    long enough to fill the chip.  ``taps_only``: 1x1 layers only where the caller says their e4m3 copies come for free (written by the
    producing epilogues: the RoI head's conv1 / conv3); the kernel itself runs ~2x the bf16 one on every shape measured."""
    # (default: the RoI head's 3x3 layers; a caller whose copies cost nothing extra passes its own bound; tests lower it to reach the kernel at small sizes)
    min_m = int(os.environ.get("CDDMSL_FP8_WGRAD_MIN_M", "300000" if min_m is None else str(min_m)))
    return os.environ.get("CDDMSL_FP8_WGRAD", "1") != "0" and (KH * KW > 1 or not taps_only) and M >= min_m \
        and bool(_L().cddmsl_conv_wgrad_fp8_ok(Cin, Cout, KH, KW, pad, Cout))


def conv_wgrad_fp8(x8, dy8, w_shape, scale, pad=0, out=None):
    """dW[Cout,KH,KW,Cin] (f32) += scale[n] * sum_m dy8[m,n] * im2col(x8)[m,k]; x8, dy8 uint8 (e4m3) NHWC, stride 1, "same" padding.
    ``scale`` must carry the two dequantisation factors (x the FrozenBN scale)."""
    require_cuda(x8, dy8, scale, out)
    Cout, KH, KW, Cin = w_shape
    N, H, W, Cin2 = x8.shape
    assert Cin == Cin2 and x8.dtype == torch.uint8 and dy8.dtype == torch.uint8 and x8.is_contiguous() and dy8.is_contiguous()
    assert dy8.shape[-1] == Cout and dy8.numel() // Cout == N * H * W and 2 * pad == KH - 1
    assert scale is not None and scale.dtype == torch.float32 and scale.numel() == Cout and scale.is_contiguous()
    if out is None:
        out = torch.zeros(w_shape, device=x8.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == tuple(w_shape)
    ensure_workspace(x8.device)
    def launch():
        return _L().cddmsl_conv_wgrad_fp8(ptr(x8), ptr(dy8), ptr(out), ptr(scale), N, H, W, Cin, Cout, KH, KW, pad, Cout, stream_ptr())
    e0 = PROFILE.begin(name="k_wgrad256_fp8") if PROFILE.on else None
    check(launch(), "cddmsl_conv_wgrad_fp8")
    PROFILE.end(e0, "k_wgrad256_fp8", 2.0 * (N * H * W) * Cout * KH * KW * Cin, (N * H * W, Cout, KH * KW * Cin, KH, 0, 1),
                nbytes=float(x8.numel() + dy8.numel() + out.numel() * 4))
    return out


@_timed("weight_prep")
def weight_prep(w_master, scale, dtype, want_fwd=True, want_dgrad=True):
    """f32 master [Cout,KH,KW,Cin] -> (fwd weights, dgrad weights [Cin,KH,KW,Cout] flipped, *scale[cout])."""
    require_cuda(w_master, scale)
    assert w_master.dtype == torch.float32 and w_master.is_contiguous() and w_master.dim() == 4
    Cout, KH, KW, Cin = w_master.shape
    wf = torch.empty((Cout, KH, KW, Cin), device=w_master.device, dtype=dtype) if want_fwd else None
    wd = torch.empty((Cin, KH, KW, Cout), device=w_master.device, dtype=dtype) if want_dgrad else None
    st = _L().cddmsl_weight_prep(ptr(w_master), ptr(scale), ptr(wf), ptr(wd), Cout, KH, KW, Cin, DT[dtype], stream_ptr())
    check(st, "cddmsl_weight_prep")
    return wf, wd


@_timed("weight_prep")
def weight_prep_multi(table, count, dtype):
    """``table``: int64 device tensor [count, 8] = {w, scale, wf, wd pointers, Cout, KH, KW, Cin} -> all copies in one launch"""
    require_cuda(table)
    assert table.dtype == torch.int64 and table.is_contiguous() and table.shape == (count, 8)
    check(_L().cddmsl_weight_prep_multi(ptr(table), count, DT[dtype], stream_ptr()), "cddmsl_weight_prep_multi")


# ------------------------------------------------------------------------------------------------ elementwise
def _f3(v):
    return (c_float * 3)(*[float(x) for x in v])


def _image_table(images_u8):
    """host arrays (device pointers, heights, widths) of a list of CHW images: the batched preprocessing entries' image table"""
    import ctypes
    n = len(images_u8)
    ptrs = (ctypes.c_void_p * n)(*[im.data_ptr() for im in images_u8])
    hs = (ctypes.c_int * n)(*[int(im.shape[1]) for im in images_u8])
    ws = (ctypes.c_int * n)(*[int(im.shape[2]) for im in images_u8])
    return ptrs, hs, ws


@_timed("preprocess")
def preprocess(images_u8, Hp, Wp, mean, std, dtype, Cp=None, div255=True):
    """list of u8 CHW device tensors -> normalised, zero-padded NHWC [N,Hp,Wp,Cp] (rcnn.py:758-768).
    div255: CLIP models take x/255 (rcnn.py:87-91); stock models normalise raw 0-255 pixels."""
    require_cuda(*images_u8)
    Cp = Cp or (8 if dtype == torch.bfloat16 else 4)
    out = torch.empty((len(images_u8), Hp, Wp, Cp), device=images_u8[0].device, dtype=dtype)
    m, s = _f3(mean), _f3(std)
    for im in images_u8:
        assert im.dtype == torch.uint8 and im.dim() == 3 and im.shape[0] == 3 and im.is_contiguous()
    ptrs, hs, ws = _image_table(images_u8)
    check(_L().cddmsl_preprocess_batch(ptrs, hs, ws, len(images_u8), ptr(out), Hp, Wp, Cp, m, s, int(div255), DT[dtype], stream_ptr()),
          "cddmsl_preprocess_batch")
    return out


@_timed("preprocess224")
def preprocess224(images_u8, Hp, Wp, mean, std, dtype, size=224, Cp=None):
    """rcnn.py:161-179: /255 -> pad to (Hp,Wp) -> bicubic short side `size` -> center crop -> normalise; NHWC out."""
    require_cuda(*images_u8)
    Cp = Cp or (8 if dtype == torch.bfloat16 else 4)
    if Wp <= Hp:
        RW, RH = size, int(size * Hp / Wp)
    else:
        RH, RW = size, int(size * Wp / Hp)
    top, left = int(round((RH - size) / 2.0)), int(round((RW - size) / 2.0))
    out = torch.empty((len(images_u8), size, size, Cp), device=images_u8[0].device, dtype=dtype)
    m, s = _f3(mean), _f3(std)
    for im in images_u8:
        assert im.dtype == torch.uint8 and im.dim() == 3 and im.is_contiguous()
    ptrs, hs, ws = _image_table(images_u8)
    check(_L().cddmsl_preprocess224_batch(ptrs, hs, ws, len(images_u8), ptr(out), Hp, Wp, RH, RW, top, left, size, Cp,
                                           m, s, DT[dtype], stream_ptr()), "cddmsl_preprocess224_batch")
    return out


from .resample import resample_table as _resample_table  # noqa: E402  (pure numpy: the loader's workers build the same tables)


def tta_view_list(sizes, flip):
    """the reference's view order (test_time_augmentation.py:79-86): [s0, s0 mirrored, s1, s1 mirrored, ...] -> [(newh, neww, flipped)]"""
    return [(int(nh), int(nw), f) for nh, nw in sizes for f in ((False, True) if flip else (False,))]


@_timed("tta_views")
def tta_views(image_u8, sizes, flip, mean, std, dtype, batch_size=3, div255=True):
    """Test-time-augmentation views of ONE u8 CHW device image, made on the device: for every (newh, neww) of ``sizes`` the PIL
    bilinear resize (bit-equal to ``Image.resize((neww, newh), BILINEAR)``), with ``flip`` also its left-right mirror, normalised
    and zero-padded like ``preprocess``.  Returns the reference's batches (test_time_augmentation.py:162-186): a list of groups
    ``(NHWC tensor [g, Hp, Wp, Cp], [(newh, neww), ...])`` of ``batch_size`` views in the order [s0, s0 mirrored, s1, ...] (the last
    group may be short), each padded to its own largest view.  One launch per size writes the view and its mirror, each into its
    own group's slot; a size equal to the image's makes the plain view a copy."""
    import numpy as np
    require_cuda(image_u8)
    assert image_u8.dtype == torch.uint8 and image_u8.dim() == 3 and image_u8.shape[0] == 3 and image_u8.is_contiguous()
    assert batch_size >= 1
    h, w = int(image_u8.shape[1]), int(image_u8.shape[2])
    Cp = 8 if dtype == torch.bfloat16 else 4
    sizes = [(int(a), int(b)) for a, b in sizes]
    views = tta_view_list(sizes, flip)
    groups = []
    for g0 in range(0, len(views), batch_size):
        vs = views[g0:g0 + batch_size]
        Hp, Wp = max(v[0] for v in vs), max(v[1] for v in vs)
        groups.append((torch.empty((len(vs), Hp, Wp, Cp), device=image_u8.device, dtype=dtype), [(v[0], v[1]) for v in vs]))
    # every table of the call in ONE int32 upload
    parts, where, off = [], {}, 0
    for insize, outsize in sorted({(w, nw) for _, nw in sizes if nw != w} | {(h, nh) for nh, _ in sizes if nh != h}):
        lo, n, k, ks = _resample_table(insize, outsize)
        where[(insize, outsize)] = (off, off + outsize, off + 2 * outsize, ks)
        parts += [lo, n, k.reshape(-1)]
        off += 2 * outsize + outsize * ks
    tab = None
    if parts:
        tab = to_device_async(torch.from_numpy(np.concatenate(parts)), image_u8.device)

    def axis(insize, outsize):
        if insize == outsize:
            return c_void_p(0), c_void_p(0), c_void_p(0), 0
        a, b, c, ks = where[(insize, outsize)]
        base = tab.data_ptr()
        return c_void_p(base + 4 * a), c_void_p(base + 4 * b), c_void_p(base + 4 * c), ks

    m, s = _f3(mean), _f3(std)
    per = 2 if flip else 1
    for i, (nh, nw) in enumerate(sizes):
        v0 = i * per
        t0, t1 = groups[v0 // batch_size][0], (groups[(v0 + 1) // batch_size][0] if flip else None)
        check(_L().cddmsl_tta_view(ptr(image_u8), h, w, nh, nw, *axis(w, nw), *axis(h, nh),
                                   ptr(t0), v0 % batch_size, t0.shape[1], t0.shape[2],
                                   ptr(t1), (v0 + 1) % batch_size if flip else 0, t1.shape[1] if flip else 0, t1.shape[2] if flip else 0,
                                   Cp, m, s, int(div255), DT[dtype], stream_ptr()), "cddmsl_tta_view")
    return groups


class ResizeItem(ctypes.Structure):
    """``cddmsl_resize_item`` of include/cddmsl_hip.h"""
    _fields_ = [("src_off", c_long), ("dst_off", c_long)] + [(k, c_int) for k in (
        "h", "w", "newh", "neww", "flip", "reverse_channels", "xtab", "xks", "ytab", "yks")]


def resize_batch_u8(src, dst, tab, items):
    """The loader's resize + mirror for a whole batch in one launch (a launch per 32 items beyond that), on the current stream.
    ``src``: device uint8 buffer holding the decoded images, interleaved [h, w, 3]; ``dst``: device uint8 buffer that receives the
    planar [3, newh, neww] results; ``tab``: device int32 buffer of ``resample.packed_table`` tables (None when no axis changes);
    ``items``: one ``(src_off, dst_off, h, w, newh, neww, flip, reverse_channels, xtab, xks, ytab, yks)`` per image -- byte offsets
    into ``src`` / ``dst``, int32 positions into ``tab`` with -1 for an axis that keeps its size.  Bit-equal to
    ``PIL.Image.resize((neww, newh), BILINEAR)``, then ``[:, ::-1]`` with bit 0 of flip, ``[::-1]`` with bit 1 (0 none, 1 left-right,
    2 top-bottom, 3 both) and ``[:, :, ::-1]`` with reverse_channels, transposed to CHW.  The library checks every item (buffer sizes,
    flip in 0..3) before it launches; a refusal raises."""
    require_cuda(src, dst, tab)
    assert src.dtype == torch.uint8 and dst.dtype == torch.uint8 and src.is_contiguous() and dst.is_contiguous()
    assert tab is None or (tab.dtype == torch.int32 and tab.is_contiguous())
    arr = (ResizeItem * max(len(items), 1))(*[ResizeItem(*(int(v) for v in it)) for it in items])
    check(_L().cddmsl_resize_batch_u8(ptr(src), src.numel(), ptr(dst), dst.numel(), ptr(tab), 0 if tab is None else tab.numel(),
                                      ctypes.cast(arr, c_void_p), len(items), stream_ptr()), "cddmsl_resize_batch_u8")
    return dst


class JitterItem(ctypes.Structure):
    """``cddmsl_jitter_item`` of include/cddmsl_color_jitter.h"""
    _fields_ = [("off", c_long)] + [(k, c_int) for k in (
        "h", "w", "ops", "bgr", "b_dw", "b_sw", "c_dw", "c_sw", "s_dw", "s_sw", "light_r", "light_g", "light_b", "reserved")]


def color_jitter_batch_u8(buf, items):
    """INPUT.COLOR_JITTER for a whole batch in place, on the current stream (a sum and an apply launch per 32 items).  ``buf``: device
    uint8 buffer holding planar [3, h, w] images; ``items``: one ``(off, h, w, params, bgr)`` per image -- byte offset into ``buf``,
    the parameters ``augment.ColorJitter.draw`` gave (None or {}: the image is left alone), and whether plane 0 is blue.  Bit-equal to
    ``augment.color_jitter_u8`` on each image; bytes outside the images are not touched.  Returns the int64 per-item byte sums the
    contrast step used (0 where it is off), or None when no item has contrast.  The library checks every item before it launches; a
    refusal raises."""
    from .augment import CONTRAST, descriptor
    require_cuda(buf)
    assert buf.dtype == torch.uint8 and buf.is_contiguous()
    desc = [descriptor(off, h, w, params, bgr) for off, h, w, params, bgr in items]
    arr = (JitterItem * max(len(desc), 1))(*[JitterItem(*d) for d in desc])
    sums = torch.empty(len(desc), dtype=torch.int64, device=buf.device) if any(d[3] & CONTRAST for d in desc) else None
    check(lib_color_jitter().cddmsl_color_jitter_batch_u8(ptr(buf), buf.numel(), ctypes.cast(arr, c_void_p), len(desc), ptr(sums), stream_ptr()),
          "cddmsl_color_jitter_batch_u8")
    return sums


@_timed("avgpool2_fwd")
def avgpool2_fwd(x):
    require_cuda(x)
    N, H, W, C = x.shape
    y = torch.empty((N, H // 2, W // 2, C), device=x.device, dtype=x.dtype)
    check(_L().cddmsl_avgpool2_fwd(ptr(x), ptr(y), N, H, W, C, _dt(x), stream_ptr()), "cddmsl_avgpool2_fwd")
    return y


@_timed("avgpool2_fwd")
def avgpool2_fwd_bits(x):
    """(avgpool2_fwd(x), bits): bits [N,H//2,W//2,C//8] int32, byte (dy*2+dx) of a word = the 8 bits x[2oy+dy][2ox+dx][8c+j] > 0 (bit j)
    -- the ReLU mask ``avgpool2_bwd_bits`` needs, at 1/16 of x's bytes.  bf16 only."""
    require_cuda(x)
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    N, H, W, C = x.shape
    y = torch.empty((N, H // 2, W // 2, C), device=x.device, dtype=x.dtype)
    bits = torch.empty((N, H // 2, W // 2, C // 8), device=x.device, dtype=torch.int32)
    check(_L().cddmsl_avgpool2_fwd_bits(ptr(x), ptr(y), ptr(bits), N, H, W, C, _dt(x), stream_ptr()), "cddmsl_avgpool2_fwd_bits")
    return y, bits


@_timed("avgpool2_bwd")
def avgpool2_bwd_bits(dy, in_shape, bits):
    """avgpool2_bwd(dy, in_shape, mask=x) with the mask given as ``avgpool2_fwd_bits(x)[1]``; bit-identical.  bf16 only."""
    require_cuda(dy, bits)
    N, H, W, C = in_shape
    assert dy.dtype == torch.bfloat16 and dy.is_contiguous() and tuple(dy.shape) == (N, H // 2, W // 2, C)
    assert bits.dtype == torch.int32 and bits.is_contiguous() and tuple(bits.shape) == (N, H // 2, W // 2, C // 8)
    dx = torch.empty(in_shape, device=dy.device, dtype=dy.dtype)
    check(_L().cddmsl_avgpool2_bwd_bits(ptr(dy), ptr(bits), ptr(dx), N, H, W, C, _dt(dy), stream_ptr()), "cddmsl_avgpool2_bwd_bits")
    return dx


@_timed("avgpool2_bwd")
def avgpool2_bwd(dy, in_shape, mask=None, add=None, emit8=None):
    """dx = up(dy)/4 (+ add), zeroed where mask <= 0.  in_shape = (N,H,W,C) of the pooled tensor's input.  ``emit8`` (scale, amax),
    bf16 only: the pass also writes dx's e4m3 copy (attached as ``dx._fp8``) and records max|dx|."""
    require_cuda(dy, mask, add)
    N, H, W, C = in_shape
    assert dy.is_contiguous() and tuple(dy.shape) == (N, H // 2, W // 2, C)
    dx = torch.empty(in_shape, device=dy.device, dtype=dy.dtype)
    if emit8 is not None and dy.dtype == torch.bfloat16:
        y8 = torch.empty(in_shape, device=dy.device, dtype=torch.uint8)
        check(_L().cddmsl_avgpool2_bwd_q8(ptr(dy), ptr(mask), ptr(add), ptr(dx), N, H, W, C, ptr(y8), ptr(emit8[0]), ptr(emit8[1]), stream_ptr()),
              "cddmsl_avgpool2_bwd_q8")
        dx._fp8 = (y8, emit8[0].data_ptr())
        return dx
    check(_L().cddmsl_avgpool2_bwd(ptr(dy), ptr(mask), ptr(add), ptr(dx), N, H, W, C, _dt(dy), stream_ptr()), "cddmsl_avgpool2_bwd")
    return dx


@_timed("attn_tokens_fwd")
def attn_tokens_fwd(x, pos, tp=None):
    """x [K,P,C] (T), pos [P+1,C] f32 -> tok [K,TP,C] (TP >= P+1 token rows per region; pad rows are zero)"""
    require_cuda(x, pos)
    K, P, C = x.shape
    tp = tp or P + 1
    assert pos.dtype == torch.float32 and tuple(pos.shape) == (P + 1, C) and x.is_contiguous() and pos.is_contiguous()
    tok = torch.empty((K, tp, C), device=x.device, dtype=x.dtype)
    check(_L().cddmsl_attn_tokens_fwd(ptr(x), ptr(pos), ptr(tok), K, P, tp, C, _dt(x), stream_ptr()), "cddmsl_attn_tokens_fwd")
    return tok


@_timed("attn_tokens_fwd")
def attn_tokens_fwd_mask(x, pos, tp=None):
    """the same, plus mbits [K,C] int64: bit p of a column's word = (x[k,p,col] > 0) -- the pooled map's ReLU mask for ``attnpool_dx``"""
    require_cuda(x, pos)
    K, P, C = x.shape
    tp = tp or P + 1
    assert pos.dtype == torch.float32 and tuple(pos.shape) == (P + 1, C) and x.is_contiguous() and pos.is_contiguous() and P <= 64
    tok = torch.empty((K, tp, C), device=x.device, dtype=x.dtype)
    mbits = torch.empty((K, C), device=x.device, dtype=torch.int64)
    check(_L().cddmsl_attn_tokens_fwd_mask(ptr(x), ptr(pos), ptr(tok), ptr(mbits), K, P, tp, C, _dt(x), stream_ptr()), "cddmsl_attn_tokens_fwd_mask")
    return tok, mbits


def rpn_losses(logits, deltas, pos, neg, midx, gt, gt_off, anchors, weights, inv_norm, gout=None):
    """forward: -> [2] f32 (loss_rpn_cls, loss_rpn_loc); backward (gout [2]): -> (dlogits, ddeltas), zero except at the sampled anchors"""
    require_cuda(logits, deltas, pos, neg, midx, gt, gt_off, anchors)
    for t in (logits, deltas, gt, anchors):
        assert t.dtype == torch.float32 and t.is_contiguous()
    for t in (pos, neg, midx, gt_off):
        assert t.dtype == torch.int64 and t.is_contiguous()
    A = anchors.shape[0]
    assert deltas.numel() == 4 * logits.numel() and midx.numel() == logits.numel()
    args = (ptr(logits), ptr(deltas), ptr(pos), pos.numel(), ptr(neg), neg.numel(), ptr(midx), ptr(gt), ptr(gt_off), ptr(anchors), A,
            *[float(w) for w in weights], float(inv_norm))
    if gout is None:
        out = torch.empty(2, device=logits.device, dtype=torch.float32)
        check(_L().cddmsl_rpn_losses(*args, ptr(out), None, None, None, stream_ptr()), "cddmsl_rpn_losses")
        return out
    dl, dd = torch.zeros_like(logits), torch.zeros_like(deltas)
    g = gout.contiguous().float()
    check(_L().cddmsl_rpn_losses(*args, None, ptr(g), ptr(dl), ptr(dd), stream_ptr()), "cddmsl_rpn_losses(backward)")
    return dl, dd


def box_l1(deltas, fg, cls, src, tgt, weights, inv_norm, gout=None):
    """forward: -> [1] f32 sum_{fg} |deltas[r, 4 cls[r]..+4] - get_deltas(src[r], tgt[r])| * inv_norm; backward (gout [1]): -> ddeltas"""
    require_cuda(deltas, fg, src, tgt)
    assert deltas.dtype == torch.float32 and deltas.dim() == 2 and deltas.is_contiguous() and fg.dtype == torch.int64 and fg.is_contiguous()
    assert src.dtype == tgt.dtype == torch.float32 and src.is_contiguous() and tgt.is_contiguous() and (cls is None or (cls.dtype == torch.int64 and cls.is_contiguous()))
    args = (ptr(deltas), deltas.shape[1], ptr(fg), fg.numel(), ptr(cls), ptr(src), ptr(tgt), *[float(w) for w in weights], float(inv_norm))
    if gout is None:
        out = torch.empty(1, device=deltas.device, dtype=torch.float32)
        check(_L().cddmsl_box_l1(*args, ptr(out), None, None, stream_ptr()), "cddmsl_box_l1")
        return out
    dd = torch.zeros_like(deltas)
    g = gout.contiguous().float().view(1)
    check(_L().cddmsl_box_l1(*args, None, ptr(g), ptr(dd), stream_ptr()), "cddmsl_box_l1(backward)")
    return dd


LOC_TYPES = {"smooth_l1": 0, "giou": 1}


def rpn_losses_reg(logits, deltas, pos, neg, midx, gt, gt_off, anchors, weights, inv_norm, loc_type, beta, scale_clamp, gout=None):
    """``rpn_losses`` with the box-regression term of ``loc_type`` ("smooth_l1" with ``beta``, or "giou" of the decoded anchors,
    dw / dh clamped at ``scale_clamp``): cddmsl_rpn_losses_reg"""
    require_cuda(logits, deltas, pos, neg, midx, gt, gt_off, anchors)
    for t in (logits, deltas, gt, anchors):
        assert t.dtype == torch.float32 and t.is_contiguous()
    for t in (pos, neg, midx, gt_off):
        assert t.dtype == torch.int64 and t.is_contiguous()
    A = anchors.shape[0]
    assert deltas.numel() == 4 * logits.numel() and midx.numel() == logits.numel()
    args = (ptr(logits), ptr(deltas), ptr(pos), pos.numel(), ptr(neg), neg.numel(), ptr(midx), ptr(gt), ptr(gt_off), ptr(anchors), A,
            *[float(w) for w in weights], float(inv_norm), LOC_TYPES[loc_type], float(beta), float(scale_clamp))
    if gout is None:
        out = torch.empty(2, device=logits.device, dtype=torch.float32)
        check(_L().cddmsl_rpn_losses_reg(*args, ptr(out), None, None, None, stream_ptr()), "cddmsl_rpn_losses_reg")
        return out
    dl, dd = torch.zeros_like(logits), torch.zeros_like(deltas)
    g = gout.contiguous().float()
    check(_L().cddmsl_rpn_losses_reg(*args, None, ptr(g), ptr(dl), ptr(dd), stream_ptr()), "cddmsl_rpn_losses_reg(backward)")
    return dl, dd


def box_reg_loss(deltas, fg, cls, src, tgt, weights, inv_norm, loc_type, beta, scale_clamp, gout=None):
    """``box_l1`` with the term of ``loc_type`` ("smooth_l1" with ``beta``, or "giou" of the decoded proposals): cddmsl_box_reg_loss"""
    require_cuda(deltas, fg, src, tgt)
    assert deltas.dtype == torch.float32 and deltas.dim() == 2 and deltas.is_contiguous() and fg.dtype == torch.int64 and fg.is_contiguous()
    assert src.dtype == tgt.dtype == torch.float32 and src.is_contiguous() and tgt.is_contiguous() and (cls is None or (cls.dtype == torch.int64 and cls.is_contiguous()))
    args = (ptr(deltas), deltas.shape[1], ptr(fg), fg.numel(), ptr(cls), ptr(src), ptr(tgt), *[float(w) for w in weights], float(inv_norm),
            LOC_TYPES[loc_type], float(beta), float(scale_clamp))
    if gout is None:
        out = torch.empty(1, device=deltas.device, dtype=torch.float32)
        check(_L().cddmsl_box_reg_loss(*args, ptr(out), None, None, stream_ptr()), "cddmsl_box_reg_loss")
        return out
    dd = torch.zeros_like(deltas)
    g = gout.contiguous().float().view(1)
    check(_L().cddmsl_box_reg_loss(*args, None, ptr(g), ptr(dd), stream_ptr()), "cddmsl_box_reg_loss(backward)")
    return dd


def attnpool_dx_ok(K, H, P, TP, C, dtype):
    return dtype == torch.bfloat16 and P == 49 and TP == 56 and 2 * H <= 64 and (2 * H) % 8 == 0 and C % 128 == 0 and 0 < K <= 65535 * 8


@_timed("attnpool_dx")
def attnpool_dx(pds, zu, g0, mbits, P, gpos=None):
    """pds [K,2H,TP] = [p ; ds], zu [K,2H,C] = [dZ ; U] (bf16), g0 [K,C] f32, mbits [K,C] int64 -> dx [K,P,C] bf16 (masked),
    gpos [P+1,C] f32 accumulated when given: the token-gradient product with its epilogue fused (cddmsl_attnpool_dx)"""
    require_cuda(pds, zu, g0, mbits)
    K, H2, TP = pds.shape
    C = zu.shape[2]
    assert pds.dtype == zu.dtype == torch.bfloat16 and g0.dtype == torch.float32 and mbits.dtype == torch.int64
    assert pds.is_contiguous() and zu.is_contiguous() and g0.is_contiguous() and mbits.is_contiguous() and tuple(zu.shape) == (K, H2, C)
    assert tuple(g0.shape) == (K, C) and tuple(mbits.shape) == (K, C) and (gpos is None or (gpos.dtype == torch.float32 and tuple(gpos.shape) == (P + 1, C) and gpos.is_contiguous()))
    dx = torch.empty((K, P, C), device=pds.device, dtype=pds.dtype)
    check(_L().cddmsl_attnpool_dx(ptr(pds), ptr(zu), ptr(g0), ptr(mbits), ptr(dx), ptr(gpos), K, H2, P, TP, C, 0, stream_ptr()), "cddmsl_attnpool_dx")
    return dx


@_timed("attn_tokens_bwd")
def attn_tokens_bwd(dtok, P, relu_mask=None, gpos=None, want_dx=True):
    """dtok [K,TP,C] -> dx [K,P,C], zeroed where relu_mask [K,P,C] <= 0; gpos (f32 [P+1,C], accumulated into) += the
    per-token column sums of dtok (the positional embedding's gradient) in the same pass"""
    require_cuda(dtok, relu_mask, gpos)
    K, TP, C = dtok.shape
    assert dtok.is_contiguous()
    assert relu_mask is None or (relu_mask.is_contiguous() and relu_mask.dtype == dtok.dtype and relu_mask.numel() == K * P * C)
    assert gpos is None or (gpos.is_contiguous() and gpos.dtype == torch.float32 and tuple(gpos.shape) == (P + 1, C))
    assert want_dx or gpos is not None
    dx = torch.empty((K, P, C), device=dtok.device, dtype=dtok.dtype) if want_dx else None
    check(_L().cddmsl_attn_tokens_bwd(ptr(dtok), ptr(relu_mask), ptr(dx), ptr(gpos), K, P, TP, C, _dt(dtok), stream_ptr()), "cddmsl_attn_tokens_bwd")
    return dx


@_timed("attnpool_softmax")
def attnpool_softmax_fwd(S, P1, scale, dtype):
    """S [K,H,TP] f32 -> (p [K,H,P1] f32 = softmax(S[..., :P1] * scale), pT [K,TP,H] dtype with zero rows past P1)"""
    require_cuda(S)
    K, H, TP = S.shape
    assert S.dtype == torch.float32 and S.is_contiguous() and P1 <= TP
    p = torch.empty((K, H, P1), device=S.device, dtype=torch.float32)
    pT = torch.empty((K, TP, H), device=S.device, dtype=dtype)
    check(_L().cddmsl_attnpool_softmax_fwd(ptr(S), ptr(p), ptr(pT), K, H, P1, TP, float(scale), DT[dtype], stream_ptr()), "cddmsl_attnpool_softmax_fwd")
    return p, pT


@_timed("attnpool_softmax")
def attnpool_softmax_bwd(p, dP, scale, dtype):
    """p [K,H,P1] f32, dP [K,H,TP] f32 -> (dsT [K,TP,H], pds [K,2H,TP] = [p ; ds]) in dtype, zero past P1"""
    require_cuda(p, dP)
    K, H, P1 = p.shape
    TP = dP.shape[2]
    assert p.dtype == dP.dtype == torch.float32 and p.is_contiguous() and dP.is_contiguous() and dP.shape[:2] == (K, H)
    dsT = torch.empty((K, TP, H), device=p.device, dtype=dtype)
    pds = torch.empty((K, 2 * H, TP), device=p.device, dtype=dtype)
    check(_L().cddmsl_attnpool_softmax_bwd(ptr(p), ptr(dP), ptr(dsT), ptr(pds), K, H, P1, TP, float(scale), DT[dtype], stream_ptr()), "cddmsl_attnpool_softmax_bwd")
    return dsT, pds


def _eptr(t, elem_offset=0):
    return ctypes.c_void_p(t.data_ptr() + elem_offset * t.element_size())


@_timed("gemm_nt_batched")
def gemm_nt_batched(a, w, c, M, N, K, lda, ldb, ldc, batch, sa, sw, sc, a_off=0, w_off=0, c_off=0, bias=None):
    """C_b[m][n] = sum_k A_b[m][k] * B_b[n][k] for b < batch; raw strided views of the tensors a, w, c (element offsets /
    strides).  c's dtype decides f32 vs compute-dtype output."""
    require_cuda(a, w, c, bias)
    assert a.dtype == w.dtype and c.dtype in (a.dtype, torch.float32)
    out_f32 = int(c.dtype == torch.float32 and a.dtype != torch.float32)
    check(_L().cddmsl_gemm_nt_batched(_eptr(a, a_off), _eptr(w, w_off), _eptr(c, c_off), ptr(bias), M, N, K, lda, ldb, ldc, batch,
                                      sa, sw, sc, out_f32, _dt(a), stream_ptr()), "cddmsl_gemm_nt_batched")


@_timed("gemm_tn_batched")
def gemm_tn_batched(a, b, out, M, N, K, lda, ldb, ldo, batch, sa, sb, so, a_off=0, b_off=0, o_off=0, accumulate=False):
    """out_b[n][k] (+)= sum_m A_b[m][n] * B_b[m][k].  accumulate=True: f32 atomic adds into `out` (f32); otherwise a plain
    store in out's dtype (f32 or the compute dtype)."""
    require_cuda(a, b, out)
    assert a.dtype == b.dtype
    if accumulate:
        assert out.dtype == torch.float32
        mode = 0
    else:
        mode = 1 if (out.dtype == torch.float32 and a.dtype != torch.float32) else (1 if out.dtype == torch.float32 else 2)
        assert out.dtype in (a.dtype, torch.float32)
    check(_L().cddmsl_gemm_tn_batched(_eptr(a, a_off), _eptr(b, b_off), _eptr(out, o_off), M, N, K, lda, ldb, ldo, batch, sa, sb, so,
                                      mode, _dt(a), stream_ptr()), "cddmsl_gemm_tn_batched")


@_timed("relu_bwd")
def relu_bwd(g, y):
    """dx = g * (y > 0) in y's dtype; g may be f32 while y is bf16."""
    require_cuda(g, y)
    assert g.is_contiguous() and y.is_contiguous() and g.numel() == y.numel()
    g_f32 = int(g.dtype == torch.float32 and y.dtype != torch.float32)
    assert g_f32 or g.dtype == y.dtype
    dx = torch.empty_like(y)
    check(_L().cddmsl_relu_bwd(ptr(g), ptr(y), ptr(dx), y.numel(), g_f32, _dt(y), stream_ptr()), "cddmsl_relu_bwd")
    return dx


@_timed("colsum")
def colsum(x2d, period=1, out=None):
    """f32 column sums of x [rows, cols] (rows folded modulo `period`)."""
    require_cuda(x2d, out)
    rows, cols = x2d.shape
    assert x2d.is_contiguous()
    if out is None:
        out = torch.zeros((period, cols) if period > 1 else (cols,), device=x2d.device, dtype=torch.float32)
    check(_L().cddmsl_colsum(ptr(x2d), ptr(out), rows, cols, period, _dt(x2d), stream_ptr()), "cddmsl_colsum")
    return out


# ---- sparse backward pass of the RPN head: the bookkeeping kernels around the GEMM entry points (csrc/rpn_sparse.hip)
def _rows_profiled(name, launch, what, shape, nbytes, flops=0.0):
    # (FLOP model: the copies and the scan do none; the gather-sum adds each partial row once)
    e0 = PROFILE.begin(name) if PROFILE.on else None
    check(launch(), what)
    PROFILE.end(e0, name, float(flops), shape, nbytes=float(nbytes))


def rpn_active_rows(dy2d, cap, overflow):
    """The rows of ``dy2d`` [positions, cols] (f32 or the compute dtype) that hold a non-zero, compacted in ascending order:
    ``rows`` [cap] int32 (-1 behind the last one) and ``slot`` [positions] int32 (index into rows, -1 = inactive).  More than
    ``cap`` active rows set ``overflow`` [1] int32 and are dropped: whoever owns the flag reads it and raises."""
    require_cuda(dy2d, overflow)
    M, cols = dy2d.shape
    assert dy2d.is_contiguous() and dy2d.dtype in DT and cap > 0 and overflow.dtype == torch.int32
    marks = torch.empty(M, device=dy2d.device, dtype=torch.int32)
    rows = torch.empty(cap, device=dy2d.device, dtype=torch.int32)
    slot = torch.empty(M, device=dy2d.device, dtype=torch.int32)
    f32 = int(dy2d.dtype == torch.float32)
    _rows_profiled("rpn_mark_rows", lambda: _L().cddmsl_rpn_mark_rows(ptr(dy2d), ptr(marks), M, cols, f32, 1 if f32 else 0, stream_ptr()),
                   "cddmsl_rpn_mark_rows", (M, cols), dy2d.numel() * dy2d.element_size() + 4 * M)
    _rows_profiled("rpn_compact_rows", lambda: _L().cddmsl_rpn_compact_rows(ptr(marks), ptr(rows), ptr(slot), ptr(overflow), M, cap, stream_ptr()),
                   "cddmsl_rpn_compact_rows", (M, cap), 12 * M + 4 * cap)                 # (the marks twice, the slots once)
    return rows, slot


def rpn_gather_rows(src2d, rows, dtype):
    """``src2d[rows]`` in ``dtype`` (src f32 or ``dtype``), zero rows where ``rows`` < 0"""
    require_cuda(src2d, rows)
    cap, cols = rows.numel(), src2d.shape[1]
    assert src2d.is_contiguous() and rows.dtype == torch.int32 and src2d.dtype in (dtype, torch.float32)
    out = torch.empty((cap, cols), device=src2d.device, dtype=dtype)
    _rows_profiled("rpn_gather_rows", lambda: _L().cddmsl_rpn_gather_rows(ptr(src2d), ptr(rows), ptr(out), cap, cols,
                                                                         int(src2d.dtype == torch.float32 and dtype != torch.float32), DT[dtype], stream_ptr()),
                   "cddmsl_rpn_gather_rows", (cap, cols), cap * cols * (src2d.element_size() + out.element_size()) + 4 * cap)
    return out


def rpn_im2col_rows(x, rows, KH, KW, pad):
    """The im2col rows of the positions ``rows`` of x NHWC: [cap, KH*KW*Cin], tap-major then channel (the order of a
    [Cout][KH][KW][Cin] filter), zeros where a tap leaves its image"""
    require_cuda(x, rows)
    N, H, W, C = x.shape
    cap = rows.numel()
    assert x.is_contiguous() and rows.dtype == torch.int32
    out = torch.empty((cap, KH * KW * C), device=x.device, dtype=x.dtype)
    _rows_profiled("rpn_im2col_rows", lambda: _L().cddmsl_rpn_im2col_rows(ptr(x), ptr(rows), ptr(out), cap, N, H, W, C, KH, KW, pad, _dt(x), stream_ptr()),
                   "cddmsl_rpn_im2col_rows", (cap, KH * KW * C), 2 * out.numel() * out.element_size() + 4 * cap)
    return out


def rpn_dx_gather(P, slot, x_shape, KH, KW, pad, dtype):
    """dx NHWC ``x_shape`` = per pixel the sum, in tap order, of the rows P[tap][slot[neighbour]] (P [KH*KW, cap, Cin] f32)"""
    require_cuda(P, slot)
    N, H, W, C = x_shape
    taps, cap, C2 = P.shape
    assert P.dtype == torch.float32 and P.is_contiguous() and taps == KH * KW and C2 == C and slot.numel() == N * H * W and slot.dtype == torch.int32
    dx = torch.empty(tuple(x_shape), device=P.device, dtype=dtype)
    # bytes: dx once, the slots, and every partial row once (a row of P[tap] is read by exactly one pixel)
    _rows_profiled("rpn_dx_gather", lambda: _L().cddmsl_rpn_dx_gather(ptr(P), ptr(slot), ptr(dx), cap, N, H, W, C, KH, KW, pad, DT[dtype], stream_ptr()),
                   "cddmsl_rpn_dx_gather", (N * H * W, C, cap), dx.numel() * dx.element_size() + 4 * slot.numel() + P.numel() * 4, flops=P.numel())
    return dx


def same_layout(a, b):
    """Same shape and the same element order in memory (strides of size-1 dims are irrelevant)."""
    return a.shape == b.shape and all(sa == sb for sa, sb, n in zip(a.stride(), b.stride(), a.shape) if n > 1)


@_timed("sgd_clip_step")
def sgd_clip_step(params, grads, moms, norm_ws, lr, momentum, wd, clip, first_step):
    """Fused per-parameter grad-norm clip + SGD(momentum, wd) over a list of f32 tensors (solver/build.py:59-130)."""
    n = len(params)
    if n == 0:
        return
    require_cuda(*params, *grads, *moms, norm_ws)
    assert len(grads) == n and len(moms) == n
    assert norm_ws.dtype == torch.float32 and norm_ws.is_contiguous() and norm_ws.numel() >= n, "norm_ws holds one f32 per tensor"
    for p, g, m in zip(params, grads, moms):
        assert p.dtype == g.dtype == m.dtype == torch.float32
        assert same_layout(p, g) and same_layout(p, m), "param/grad/momentum must share a memory layout"
    P = (c_void_p * n)(*[p.data_ptr() for p in params])
    G = (c_void_p * n)(*[g.data_ptr() for g in grads])
    M = (c_void_p * n)(*[m.data_ptr() for m in moms])
    S = (c_long * n)(*[p.numel() for p in params])
    check(_L().cddmsl_sgd_clip_step(P, G, M, S, n, ptr(norm_ws), lr, momentum, wd, clip, int(first_step), stream_ptr()),
          "cddmsl_sgd_clip_step")


SGD_CLIP_MODES = {"none": 0, "value": 1, "l2": 2, "l1": 3, "inf": 4}


@_timed("sgd_step_groups")
def sgd_step_groups(params, grads, moms, norm_ws, lrs, wds, momentum, nesterov, clip_mode, clip_value, first_step):
    """torch.optim.SGD with one lr and one weight decay per tensor, optional Nesterov momentum and per-parameter gradient clipping
    over a list of f32 tensors (solver/build.py:23-40,113-217).  ``clip_mode``: SGD_CLIP_MODES (0 none, 1 value, 2 / 3 / 4 the
    L2 / L1 / inf norm); the norm modes leave sum g^2, sum |g| or max |g| of tensor i in ``norm_ws[i]``."""
    n = len(params)
    assert len(lrs) == n and len(wds) == n, "one lr and one weight decay per tensor"
    if n == 0:
        return
    require_cuda(*params, *grads, *moms, norm_ws)
    assert len(grads) == n and len(moms) == n
    assert norm_ws.dtype == torch.float32 and norm_ws.is_contiguous() and norm_ws.numel() >= n, "norm_ws holds one f32 per tensor"
    for p, g, m in zip(params, grads, moms):
        assert p.dtype == g.dtype == m.dtype == torch.float32
        assert same_layout(p, g) and same_layout(p, m), "param/grad/momentum must share a memory layout"
    P = (c_void_p * n)(*[p.data_ptr() for p in params])
    G = (c_void_p * n)(*[g.data_ptr() for g in grads])
    M = (c_void_p * n)(*[m.data_ptr() for m in moms])
    S = (c_long * n)(*[p.numel() for p in params])
    LR = (c_float * n)(*lrs)
    WD = (c_float * n)(*wds)
    check(_L().cddmsl_sgd_step_groups(P, G, M, S, LR, WD, n, ptr(norm_ws), momentum, int(nesterov), int(clip_mode), clip_value,
                                      int(first_step), stream_ptr()), "cddmsl_sgd_step_groups")


@_timed("weight_average")
def weight_average(avgs, params, w, copy):
    """The averaged weights after a step, over lists of f32 tensors: ``copy``: avg = param bit for bit; else avg += w (param - avg),
    ``w`` in [0, 1] (EMA: 1 - decay; running mean of n + 1 snapshots: 1 / (n + 1)).  ``params`` are only read."""
    n = len(avgs)
    assert len(params) == n, "one averaged tensor per parameter"
    if n == 0:
        return
    require_cuda(*avgs, *params)
    for e, p in zip(avgs, params):
        assert e.dtype == p.dtype == torch.float32
        assert same_layout(e, p), "averaged tensor and parameter must share a memory layout"
        # the kernel walks numel() elements from data_ptr(): the elements must fill that span (contiguous in some dimension order)
        assert p.numel() == 0 or sum((n_ - 1) * s_ for n_, s_ in zip(p.shape, p.stride())) + 1 == p.numel(), "tensors must be dense"
    E = (c_void_p * n)(*[e.data_ptr() for e in avgs])
    P = (c_void_p * n)(*[p.data_ptr() for p in params])
    S = (c_long * n)(*[p.numel() for p in params])
    check(lib_weight_average().cddmsl_weight_average(E, P, S, n, float(w), int(bool(copy)), stream_ptr()), "cddmsl_weight_average")


# ------------------------------------------------------------------------------------------------ RoIAlign
@_timed("roi_align_forward")
def roi_align_forward(x, rois, ph, pw, spatial_scale, sampling_ratio, aligned, dbg_grid=None, with_pooled=False, extra_rows=0):
    """x NHWC [N,H,W,C]; rois [K,5] f32 (batch_idx,x0,y0,x1,y1) -> [K,ph,pw,C]  (layers/roi_align.py:49-65).
    ``with_pooled``: also returns AvgPool2d(2) of the result [K,ph/2,pw/2,C] (bit-identical to avgpool2_fwd of it).
    ``extra_rows``: the outputs are allocated with that many more (unwritten) leading rows behind the K crops, for a caller that
    appends maps of the same geometry without a concatenation copy."""
    require_cuda(x, rois)
    assert rois.dim() == 2 and rois.size(1) == 5 and rois.dtype == torch.float32 and rois.is_contiguous()
    N, H, W, C = x.shape
    K = rois.shape[0]
    y = torch.empty((K + extra_rows, ph, pw, C), device=x.device, dtype=x.dtype)
    yp = torch.empty((K + extra_rows, ph // 2, pw // 2, C), device=x.device, dtype=x.dtype) if with_pooled else None
    check(_L().cddmsl_roi_align_forward(ptr(x), ptr(rois), ptr(y), ptr(yp), ptr(dbg_grid), N, C, H, W, K, ph, pw, spatial_scale,
                                         sampling_ratio, int(aligned), _dt(x), stream_ptr()), "cddmsl_roi_align_forward")
    return (y, yp) if with_pooled else y


@_timed("roi_align_forward")
def roi_align_forward_affine(x, rois, ph, pw, spatial_scale, sampling_ratio, aligned, scale=None, bias=None, relu=False,
                             pooled_only=False, extra_rows=0, emit8=None):
    """RoIAlign of a map that already went through a 1x1 convolution (layers.RoIStageFn):
    ``pooled_only=False``: y [K,ph,pw,C] = relu?(scale * roi_align(x) + bias) (per channel, f32 scale / bias);
    ``pooled_only=True``: only AvgPool2d(2) of the crops, [K,ph/2,pw/2,C] = scale * avgpool2(roi_align(x)) + bias (the affine after the
    average; no ReLU: the library refuses it) -- the full-resolution crops are never written."""
    require_cuda(x, rois)
    assert rois.dim() == 2 and rois.size(1) == 5 and rois.dtype == torch.float32 and rois.is_contiguous()
    assert (scale is None) == (bias is None)
    N, H, W, C = x.shape
    K = rois.shape[0]
    if pooled_only:
        y, yp = None, torch.empty((K + extra_rows, ph // 2, pw // 2, C), device=x.device, dtype=x.dtype)
    else:
        y, yp = torch.empty((K + extra_rows, ph, pw, C), device=x.device, dtype=x.dtype), None
    assert scale is None or (scale.dtype == torch.float32 and scale.numel() == C and bias.numel() == C and scale.is_contiguous() and bias.is_contiguous())
    y8 = None
    if emit8 is not None:     # e4m3 copy of the crops for the convolution that consumes them (fp8 configuration), as y._fp8
        assert not pooled_only and x.dtype == torch.bfloat16
        y8 = torch.empty(y.shape, device=x.device, dtype=torch.uint8)
    check(_L().cddmsl_roi_align_forward_affine(ptr(x), ptr(rois), ptr(y), ptr(yp), ptr(scale), ptr(bias), int(relu), N, C, H, W, K,
                                                ph, pw, spatial_scale, sampling_ratio, int(aligned), _dt(x), ptr(y8),
                                                ptr(emit8[0]) if emit8 else c_void_p(0), ptr(emit8[1]) if emit8 else c_void_p(0), stream_ptr()),
          "cddmsl_roi_align_forward_affine")
    if y8 is not None:
        y._fp8 = (y8, emit8[0].data_ptr())
    return yp if pooled_only else y


@_timed("roi_align_backward")
def roi_align_backward(dy, rois, roi_start, in_shape, spatial_scale, sampling_ratio, aligned, pooled=False):
    """dy [K,ph,pw,C] -> dx NHWC in_shape.  rois must be grouped by image; roi_start int32 [N+1] prefix offsets.
    ``pooled``: dy is the gradient of AvgPool2d(2) of the crops (the RoIAlign grid is 2ph x 2pw)."""
    require_cuda(dy, rois, roi_start)
    N, H, W, C = in_shape
    K, ph, pw, _ = dy.shape
    assert roi_start.dtype == torch.int32 and roi_start.numel() == N + 1 and dy.is_contiguous()
    dx = torch.empty(in_shape, device=dy.device, dtype=dy.dtype)
    ay = workspace("roi_ay", max(K, 1) * H * ph * 4, dy.device)
    ax = workspace("roi_ax", max(K, 1) * W * pw * 4, dy.device)
    fp = workspace("roi_fp", max(K, 1) * 16, dy.device)
    fn = _L().cddmsl_roi_align_backward_pooled if pooled else _L().cddmsl_roi_align_backward
    check(fn(ptr(dy), ptr(rois), ptr(roi_start), ptr(dx), ptr(ay), ptr(ax), ptr(fp), N, C, H, W, K,
             ph, pw, spatial_scale, sampling_ratio, int(aligned), _dt(dy), stream_ptr()), "cddmsl_roi_align_backward")
    return dx


def roi_align_nchw(input, rois, output_size, spatial_scale, sampling_ratio, aligned):
    """torchvision.ops.roi_align as layers/roi_align.py:58-65 calls it: input [N,C,H,W], rois [K,5] in any order -> [K,C,ph,pw]"""
    require_cuda(input, rois)
    assert rois.dim() == 2 and rois.size(1) == 5 and rois.dtype == torch.float32 and rois.is_contiguous() and input.is_contiguous()
    N, C, H, W = input.shape
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else output_size
    K = rois.shape[0]
    out = torch.zeros((K, C, ph, pw), device=input.device, dtype=input.dtype)
    _with_temp(_L().cddmsl_roi_align_nchw_anyorder, "cddmsl_roi_align_nchw_anyorder", "roi_nchw", input.device, ptr(input), ptr(rois), ptr(out),
               N, C, H, W, K, ph, pw, spatial_scale, sampling_ratio, int(aligned), _dt(input))
    return out


def roi_align_backward_nchw(grad, rois, input_shape, spatial_scale, sampling_ratio, aligned):
    """its backward: grad [K,C,ph,pw] -> grad_input [N,C,H,W]"""
    require_cuda(grad, rois)
    assert rois.dtype == torch.float32 and rois.is_contiguous() and grad.is_contiguous()
    N, C, H, W = input_shape
    K, _, ph, pw = grad.shape
    dx = torch.zeros(tuple(input_shape), device=grad.device, dtype=grad.dtype)
    _with_temp(_L().cddmsl_roi_align_backward_nchw_anyorder, "cddmsl_roi_align_backward_nchw_anyorder", "roi_nchw_b", grad.device, ptr(grad), ptr(rois),
               ptr(dx), N, C, H, W, K, ph, pw, spatial_scale, sampling_ratio, int(aligned), _dt(grad))
    return dx


# ------------------------------------------------------------------------------------------------ boxes
def anchors(cell, Hf, Wf, stride, offset):
    require_cuda(cell)
    A = cell.shape[0]
    out = torch.empty((Hf * Wf * A, 4), device=cell.device, dtype=torch.float32)
    check(_L().cddmsl_anchors(ptr(cell), ptr(out), Hf, Wf, A, stride, offset, stream_ptr()), "cddmsl_anchors")
    return out


_WS = {}


def workspace(key, nbytes, device):
    """Persistent scratch buffers (NMS masks, sort temp storage ...): allocated once per (key, size) and reused, so the
    hot loop never goes back to the allocator for its 100+ MB workspaces."""
    k = (key, device)         # (a torch.device hashes by type and index; a str() per call shows on the GPT-2 decode step)
    buf = _WS.get(k)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 16), device=device, dtype=torch.uint8)
        _WS[k] = buf
    return buf


def _with_temp(fn, what, key, device, *head):
    """Query-then-run for an entry point whose parameters end in (temp, temp_bytes, stream): ``fn(*head, NULL, &bytes, stream)``
    reports the scratch it needs, the persistent ``workspace(key)`` supplies it, and the same call with the buffer does the work."""
    nbytes = ctypes.c_size_t(0)
    check(fn(*head, None, ctypes.byref(nbytes), stream_ptr()), what + "(size)")
    ws = workspace(key, max(nbytes.value, 1), device)
    check(fn(*head, ptr(ws), ctypes.byref(nbytes), stream_ptr()), what)


INSTANCE_ID_LO, INSTANCE_ID_HI = 24, 34000      # ids the instance-box kernel reports: [24, 34000)


def instance_boxes(maps):
    """Instance-id maps [B,H,W] (uint16 or int32, on the GPU) -> (records int32 [B,R,6], counts int32 [B]), enqueued on the current
    stream, no synchronisation.  records[b,:counts[b]] = (id, xmin, ymin, xmax, ymax, npixels) for every id in [24, 34000) present in
    map b, ascending id; counts[b] == -1 flags a map holding an id >= 34000 (``instance_boxes_host`` raises on it)."""
    require_cuda(maps)
    assert maps.dim() == 3 and maps.is_contiguous(), maps.shape
    if maps.dtype not in (torch.uint16, torch.int32):
        raise TypeError(f"instance maps must be uint16 or int32, got {maps.dtype}")
    B, H, W = maps.shape
    R = min(H * W, INSTANCE_ID_HI - INSTANCE_ID_LO)
    records = torch.empty((B, R, 6), device=maps.device, dtype=torch.int32)
    counts = torch.empty(B, device=maps.device, dtype=torch.int32)
    dt = 0 if maps.dtype == torch.uint16 else 1
    nbytes = ctypes.c_size_t(0)
    check(_L().cddmsl_instance_boxes(ptr(maps), B, H, W, dt, None, R, None, None, ctypes.byref(nbytes), stream_ptr()),
          "cddmsl_instance_boxes(size)")
    ws = torch.empty(nbytes.value, device=maps.device, dtype=torch.uint8)      # torch's caching allocator, stream-ordered
    check(_L().cddmsl_instance_boxes(ptr(maps), B, H, W, dt, ptr(records), R, ptr(counts), ptr(ws), ctypes.byref(nbytes), stream_ptr()),
          "cddmsl_instance_boxes")
    return records, counts


def instance_boxes_host(maps):
    """``instance_boxes`` + readback: a list of B numpy int32 arrays [n_b, 6].  Raises ``HipLibraryError`` (status 1,
    CDDMSL_ERR_ARG) if a map holds an id >= 34000 -- such ids have no Cityscapes label and are never dropped silently."""
    import numpy as np
    from ._lib import HipLibraryError, Readback
    records, counts = instance_boxes(maps)
    n = Readback(counts).get().tolist()
    bad = [b for b, c in enumerate(n) if c < 0]
    if bad:
        raise HipLibraryError(f"cddmsl_instance_boxes failed with status 1: map(s) {bad} hold an instance id >= {INSTANCE_ID_HI}")
    top = max(n, default=0)
    host = Readback(records[:, :top]).get().numpy() if top else None
    return [host[b, :c].copy() if c else np.zeros((0, 6), dtype=np.int32) for b, c in enumerate(n)]


@_timed("sort_desc")
def sort_desc(keys):
    """Stable descending sort of each row of keys [N,total] f32 -> (sorted keys, int32 order)."""
    require_cuda(keys)
    N, total = keys.shape
    assert keys.dtype == torch.float32 and keys.is_contiguous()
    dev = keys.device
    offs = torch.arange(0, (N + 1) * total, total, device=dev, dtype=torch.int32)
    keys_out = torch.empty_like(keys)
    idx = torch.empty((N, total), device=dev, dtype=torch.int32)
    order = torch.empty((N, total), device=dev, dtype=torch.int32)
    _with_temp(_L().cddmsl_sort_desc, "cddmsl_sort_desc", "sort", dev, ptr(keys), ptr(keys_out), ptr(idx), ptr(order), ptr(offs), N, total)
    return keys_out, order


@_timed("nms")
def nms_anyorder(boxes, scores, iou_threshold):
    """torchvision.ops.nms(boxes [K,4], scores [K], thr) -> (keep int64 [K] (kept indices, descending score, then -1), nkeep int32 [1])"""
    require_cuda(boxes, scores)
    K = boxes.shape[0]
    assert boxes.dtype == scores.dtype == torch.float32 and boxes.is_contiguous() and scores.is_contiguous() and scores.numel() == K
    keep = torch.empty(K, device=boxes.device, dtype=torch.int64)
    nkeep = torch.zeros(1, device=boxes.device, dtype=torch.int32)
    _with_temp(_L().cddmsl_nms_anyorder, "cddmsl_nms_anyorder", "nms_any", boxes.device, ptr(boxes), ptr(scores), ptr(keep), ptr(nkeep), K, iou_threshold)
    return keep, nkeep


SOFT_NMS_METHODS = {"gaussian": 0, "linear": 1, "hard": 2}
SOFT_NMS_MAX_CANDIDATES = 32768      # cddmsl_soft_nms: candidates per call, any split over categories


@_timed("soft_nms")
def soft_nms(boxes, scores, idxs, method, sigma, iou_threshold, prune_threshold, max_keep=-1):
    """layers/soft_nms.py batched_soft_nms(boxes [K,4], scores [K], idxs [K] int64, ...) on the per-category walk kernel ->
    (keep int64 [K]: kept input indices in pick order, then -1; keep_scores f32 [K]: their rescored scores, valid up to nkeep;
    nkeep int32 [1]), all on the device, no synchronisation.  ``method``: "gaussian" / "linear" / "hard" (or 0 / 1 / 2);
    ``max_keep`` >= 0 stops every category's walk after that many picks and cuts the output there (the first max_keep entries
    of the uncapped result)."""
    require_cuda(boxes, scores, idxs)
    K = boxes.shape[0]
    assert boxes.dtype == scores.dtype == torch.float32 and idxs.dtype == torch.int64 and scores.numel() == idxs.numel() == K
    assert boxes.is_contiguous() and scores.is_contiguous() and idxs.is_contiguous()
    if isinstance(method, str):
        if method not in SOFT_NMS_METHODS:
            raise NotImplementedError("{} soft nms method not implemented.".format(method))
        method = SOFT_NMS_METHODS[method]
    keep = torch.empty(K, device=boxes.device, dtype=torch.int64)
    keep_scores = torch.empty(K, device=boxes.device, dtype=torch.float32)
    nkeep = torch.zeros(1, device=boxes.device, dtype=torch.int32)
    _with_temp(_L().cddmsl_soft_nms, "cddmsl_soft_nms", "soft_nms", boxes.device, ptr(boxes), ptr(scores), ptr(idxs), ptr(keep), ptr(keep_scores),
               ptr(nkeep), K, int(method), float(sigma), float(iou_threshold), float(prune_threshold), int(max_keep))
    return keep, keep_scores, nkeep


# cddmsl_coco_match: what one (image, class) may hold; an image beyond a cap comes back flagged in ``over`` and is matched on the host
COCO_MATCH_MAX_DETS = 1024           # detections of one class in one image (so any image with up to 1024 detections fits)
COCO_MATCH_MAX_GT = 256              # ground-truth boxes of one class in one image
COCO_MATCH_MAX_KEPT = 128            # kept detections per (image, class): the ``max_dets`` argument


def _upload(array, device):
    return to_device_async(torch.from_numpy(np.ascontiguousarray(array)), device)


def _pack_ground_truth(items, fields, device):
    """What the three ground-truth classes' ``from_host`` share.  ``items``: one tuple of numpy arrays per image (or row), ``fields``: a
    ``(dtype, trailing shape)`` per tuple member -> the members concatenated over the items ([G, *trailing], contiguous, zero rows
    for an empty list) followed by ``off`` int64 [len(items) + 1], the running sum of the items' lengths; all uploaded without a
    synchronisation."""
    cols = [[np.asarray(it[k], dtype=dt).reshape(-1, *tail) for it in items] for k, (dt, tail) in enumerate(fields)]
    arrays = [np.concatenate(col) if col else np.zeros((0, *tail), dtype=dt) for col, (dt, tail) in zip(cols, fields)]
    off = np.concatenate([[0], np.cumsum([len(a) for a in cols[0]])]).astype(np.int64)
    return [_upload(a, device) for a in arrays + [off]]


class CocoGroundTruth:
    """A data set's ground truth on the device, as cddmsl_coco_match reads it: ``xywh`` f64 [G, 4], ``area`` f64 [G], ``crowd`` u8 [G],
    ``cls`` int64 [G] concatenated over the images, ``off`` int64 [n_images + 1]; plus the walk's constants ``thrs`` f64 [T] and
    ``rngs`` f64 [A, 2].  Built once per evaluator from host arrays (``from_host``)."""

    def __init__(self, xywh, area, crowd, cls, off, thrs, rngs):
        require_cuda(xywh, area, crowd, cls, off, thrs, rngs)
        G = area.numel()
        assert xywh.dtype == area.dtype == thrs.dtype == rngs.dtype == torch.float64 and crowd.dtype == torch.uint8
        assert cls.dtype == off.dtype == torch.int64 and tuple(xywh.shape) == (G, 4) and crowd.numel() == cls.numel() == G
        assert off.numel() >= 1 and rngs.dim() == 2 and rngs.shape[1] == 2 and thrs.dim() == 1
        assert all(t.is_contiguous() for t in (xywh, area, crowd, cls, off, thrs, rngs))
        self.xywh, self.area, self.crowd, self.cls, self.off, self.thrs, self.rngs = xywh, area, crowd, cls, off, thrs, rngs
        self.n_images = off.numel() - 1

    @classmethod
    def from_host(cls, per_image, thrs, rngs, device):
        """``per_image``: [(xywh [g,4], area [g], crowd [g] bool, class [g])] numpy, in data-set order"""
        packed = _pack_ground_truth(per_image, [(np.float64, (4,)), (np.float64, ()), (np.uint8, ()), (np.int64, ())], device)
        return cls(*packed, _upload(np.asarray(thrs, dtype=np.float64), device), _upload(np.asarray(rngs, dtype=np.float64).reshape(-1, 2), device))


@_timed("coco_match")
def coco_match(dt_boxes, dt_scores, dt_cls, dt_off, img_idx, gt, num_classes, max_dets=100):
    """``COCOeval.evaluateImg`` for every (image, class, area range, IoU threshold) of a batch in one launch (cddmsl_coco_match),
    bit-identical to ``evaluation._coco_match`` per (image, class, range).  ``dt_boxes`` f32 [D, 4] XYXY, ``dt_scores`` f32 [D],
    ``dt_cls`` int64 [D]: the batch's detections, image after image, with offsets ``dt_off`` int64 [B + 1]; ``img_idx`` int64 [B]:
    the images' indices into ``gt`` (a ``CocoGroundTruth``).  All on the device; nothing is read back and nothing synchronises.
    -> (rank int32 [D]: position in the stable descending-score order of the detection's (image, class), -1 when dropped;
    matched, ignored int64 [D]: bit ``a * T + t``; over int32 [B]: 1 = the image exceeds a cap (COCO_MATCH_MAX_DETS /
    COCO_MATCH_MAX_GT of one class), its outputs are incomplete and the caller has to match it on the host)."""
    require_cuda(dt_boxes, dt_scores, dt_cls, dt_off, img_idx)
    D, B = dt_scores.numel(), img_idx.numel()
    assert dt_boxes.dtype == dt_scores.dtype == torch.float32 and dt_cls.dtype == dt_off.dtype == img_idx.dtype == torch.int64
    assert tuple(dt_boxes.shape) == (D, 4) and dt_cls.numel() == D and dt_off.numel() == B + 1
    assert dt_boxes.is_contiguous() and dt_scores.is_contiguous() and dt_cls.is_contiguous() and dt_off.is_contiguous() and img_idx.is_contiguous()
    if not 1 <= max_dets <= COCO_MATCH_MAX_KEPT:
        raise ValueError(f"coco_match: max_dets {max_dets} outside [1, {COCO_MATCH_MAX_KEPT}]")
    dev = dt_boxes.device
    rank = torch.empty(D, device=dev, dtype=torch.int32)
    matched = torch.empty(D, device=dev, dtype=torch.int64)
    ignored = torch.empty(D, device=dev, dtype=torch.int64)
    over = torch.empty(B, device=dev, dtype=torch.int32)
    check(_L().cddmsl_coco_match(ptr(dt_boxes), ptr(dt_scores), ptr(dt_cls), ptr(dt_off), ptr(img_idx), B, D, ptr(gt.xywh), ptr(gt.area),
                                 ptr(gt.crowd), ptr(gt.cls), ptr(gt.off), gt.n_images, ptr(gt.thrs), gt.thrs.numel(), ptr(gt.rngs),
                                 gt.rngs.shape[0], int(num_classes), int(max_dets), ptr(rank), ptr(matched), ptr(ignored), ptr(over),
                                 stream_ptr()), "cddmsl_coco_match")
    return rank, matched, ignored, over


# cddmsl_proposal_cover: what one image may hold; an image beyond a cap comes back flagged in ``over`` and is walked on the host
PROPOSAL_COVER_MAX_PROPOSALS = 2048  # proposals of one image (the RPN's post-NMS top-k is 2000 in training, 1000 at test time)
PROPOSAL_COVER_MAX_GT = 512          # ground-truth boxes of one image
PROPOSAL_COVER_MAX_LIMITS = 4        # proposal limits per launch
PROPOSAL_COVER_MAX_RANGES = 8        # area ranges per launch (one bit each in ``rng``)


class ProposalGroundTruth:
    """A data set's ground truth on the device, as cddmsl_proposal_cover reads it: ``boxes`` f32 [G, 4] XYXY, ``rng`` u8 [G] (bit a =
    the box counts in area range a; a crowd box has no bit) concatenated over the images, ``off`` int64 [n_images + 1]; plus the
    walk's ``limits`` int32 [L] (a value >= PROPOSAL_COVER_MAX_PROPOSALS is "no limit") and the number of ranges ``A``.  Built once
    per evaluator from host arrays (``from_host``)."""

    def __init__(self, boxes, rng, off, limits, num_ranges):
        require_cuda(boxes, rng, off, limits)
        G = rng.numel()
        assert boxes.dtype == torch.float32 and rng.dtype == torch.uint8 and off.dtype == torch.int64 and limits.dtype == torch.int32
        assert tuple(boxes.shape) == (G, 4) and off.dim() == 1 and off.numel() >= 1 and limits.dim() == 1
        assert all(t.is_contiguous() for t in (boxes, rng, off, limits))
        if not 1 <= limits.numel() <= PROPOSAL_COVER_MAX_LIMITS:
            raise ValueError(f"proposal_cover: {limits.numel()} limits outside [1, {PROPOSAL_COVER_MAX_LIMITS}]")
        if not 1 <= num_ranges <= PROPOSAL_COVER_MAX_RANGES:
            raise ValueError(f"proposal_cover: {num_ranges} area ranges outside [1, {PROPOSAL_COVER_MAX_RANGES}]")
        self.boxes, self.rng, self.off, self.limits, self.num_ranges = boxes, rng, off, limits, int(num_ranges)
        self.n_images, self.n_boxes = off.numel() - 1, G

    @classmethod
    def from_host(cls, per_image, limits, num_ranges, device):
        """``per_image``: [(boxes [g, 4] f32 XYXY, rng [g] u8)] numpy, in data-set order; ``limits``: ints, None = no limit"""
        lim = np.asarray([PROPOSAL_COVER_MAX_PROPOSALS if l is None else min(max(int(l), 0), PROPOSAL_COVER_MAX_PROPOSALS) for l in limits],
                         dtype=np.int32)
        return cls(*_pack_ground_truth(per_image, [(np.float32, (4,)), (np.uint8, ())], device), _upload(lim, device), num_ranges)


@_timed("proposal_cover")
def proposal_cover(boxes, logits, off, img_idx, cover_off, num_slots, gt):
    """The per-image walk of ``_evaluate_box_proposals`` for every (image, limit, area range) of a batch in one launch
    (cddmsl_proposal_cover), bit-identical to ``evaluation.proposal_cover_host`` per image.  ``boxes`` f32 [P, 4] XYXY, ``logits`` f32
    [P]: the batch's proposals, image after image in any order inside an image, with offsets ``off`` int64 [B + 1]; ``img_idx`` int64
    [B]: the images' indices into ``gt`` (a ``ProposalGroundTruth``); ``cover_off`` int64 [B + 1]: the running sum of the batch
    images' ground-truth counts, ``num_slots`` its last value (a host int).  All on the device; nothing is read back and nothing
    synchronises.
    -> (cover f32 [L, A, num_slots]: per ground-truth box -1 = not counted (outside the range, or an image without proposals), else the
    IoU the walk recorded on it, 0.0 when the walk ended before it; over int32 [B]: 1 = the image exceeds a cap
    (PROPOSAL_COVER_MAX_PROPOSALS / PROPOSAL_COVER_MAX_GT), none of its slots is written and the caller has to walk it on the host)."""
    require_cuda(boxes, logits, off, img_idx, cover_off)
    P, B = logits.numel(), img_idx.numel()
    assert boxes.dtype == logits.dtype == torch.float32 and off.dtype == img_idx.dtype == cover_off.dtype == torch.int64
    assert tuple(boxes.shape) == (P, 4) and off.numel() == B + 1 and cover_off.numel() == B + 1
    assert boxes.is_contiguous() and logits.is_contiguous() and off.is_contiguous() and img_idx.is_contiguous() and cover_off.is_contiguous()
    dev = boxes.device
    L, A = gt.limits.numel(), gt.num_ranges
    cover = torch.empty((L, A, int(num_slots)), device=dev, dtype=torch.float32)
    over = torch.empty(B, device=dev, dtype=torch.int32)
    check(_L().cddmsl_proposal_cover(ptr(boxes), ptr(logits), ptr(off), ptr(img_idx), B, P, ptr(gt.boxes), ptr(gt.rng), ptr(gt.off),
                                     gt.n_images, gt.n_boxes, ptr(gt.limits), L, A, ptr(cover_off), int(num_slots), ptr(cover), ptr(over),
                                     stream_ptr()), "cddmsl_proposal_cover")
    return cover, over


VOC_MATCH_MAX_THRS = 16              # cddmsl_voc_match: IoU thresholds per launch (one bit each in the u16 masks)


class VocGroundTruth:
    """A VOC test set's ground truth on the device, as cddmsl_voc_match reads it: ``boxes`` f64 [G, 4] (the 1-based integers of the
    XML), ``difficult`` u8 [G], ``off`` int64 [R + 1] over the R = classes * images rows (row = class * n_images + image index), and
    the thresholds ``thrs`` f64 [T] as the host compares them.  Built once per evaluator (``from_host``)."""

    def __init__(self, boxes, difficult, off, thrs):
        require_cuda(boxes, difficult, off, thrs)
        G = difficult.numel()
        assert boxes.dtype == thrs.dtype == torch.float64 and difficult.dtype == torch.uint8 and off.dtype == torch.int64
        assert tuple(boxes.shape) == (G, 4) and off.dim() == 1 and off.numel() >= 1 and thrs.dim() == 1
        assert 1 <= thrs.numel() <= VOC_MATCH_MAX_THRS, f"voc_match: {thrs.numel()} thresholds outside [1, {VOC_MATCH_MAX_THRS}]"
        assert all(t.is_contiguous() for t in (boxes, difficult, off, thrs))
        self.boxes, self.difficult, self.off, self.thrs = boxes, difficult, off, thrs
        self.n_rows, self.n_boxes = off.numel() - 1, G

    @classmethod
    def from_host(cls, rows, thrs, device):
        """``rows``: [(bbox [g, 4], difficult [g])] numpy, one per (class, image) in row order"""
        rows = [(b, np.asarray(d).astype(np.uint8)) for b, d in rows]          # (difficult is a bool array)
        return cls(*_pack_ground_truth(rows, [(np.float64, (4,)), (np.uint8, ())], device), _upload(np.asarray(thrs, dtype=np.float64), device))


@_timed("voc_match")
def voc_match(boxes, perm, seg_off, seg_gt, gt):
    """``evaluation.class_ap``'s greedy walk for every (class, image) segment at every threshold of ``gt.thrs`` in one launch
    (cddmsl_voc_match), bit-identical to it.  ``boxes`` f32 [D, 4] XYXY as the model left them (the kernel rounds them the way the
    reference's result lines do), ``perm`` int64 [P]: detection indices segment by segment, inside a segment in ``class_ap``'s
    visiting order, each detection at most once; ``seg_off`` int64 [S + 1]; ``seg_gt`` int64 [S]: the segments' rows in ``gt`` (a
    ``VocGroundTruth``), each row at most once.  All on the device; nothing is read back and nothing synchronises.
    -> (tp, fp: int16 [D] holding the u16 masks, bit t = the flag at ``gt.thrs[t]``; bad int32 [S]: 1 = the segment's offsets or
    entries were out of range and skipped)."""
    require_cuda(boxes, perm, seg_off, seg_gt)
    D, S = boxes.shape[0], seg_gt.numel()
    if boxes.dtype != torch.float32:
        raise TypeError(f"voc_match: boxes are {boxes.dtype}, the kernel reads f32")
    assert perm.dtype == seg_off.dtype == seg_gt.dtype == torch.int64 and tuple(boxes.shape) == (D, 4) and seg_off.numel() == S + 1
    assert perm.dim() == seg_off.dim() == seg_gt.dim() == 1
    assert boxes.is_contiguous() and perm.is_contiguous() and seg_off.is_contiguous() and seg_gt.is_contiguous()
    if S >= 2 ** 31:
        raise ValueError(f"voc_match: {S} segments in one launch (the grid holds 2^31 - 1)")
    dev = boxes.device
    flags = torch.empty((2, D), device=dev, dtype=torch.int16)
    bad = torch.empty(S, device=dev, dtype=torch.int32)
    ws = workspace("voc_match", max(2 * gt.n_boxes, 1), dev)          # the claimed bits: one u16 per ground-truth box
    check(_L().cddmsl_voc_match(ptr(boxes), D, ptr(perm), perm.numel(), ptr(seg_off), ptr(seg_gt), S, ptr(gt.boxes), ptr(gt.difficult), ptr(gt.off),
                                gt.n_rows, gt.n_boxes, ptr(gt.thrs), gt.thrs.numel(), ptr(flags[0]), ptr(flags[1]), ptr(bad), ptr(ws),
                                stream_ptr()), "cddmsl_voc_match")
    return flags[0], flags[1], bad


OPENSET_MAX_CLASSES = 16384          # cddmsl_openset_logits / _select: classes of the test vocabulary


@_timed("openset_logits")
def openset_logits(x, wn, temperature, eps=1e-12, ld=None):
    """x [R, D] f32, wn [K, D] f32 unit rows -> (logits [R, ld] f32 with column K exactly 0, stats [R, 2] f32 = (row max, sum
    exp(logit - max)) over the K+1 logits): the open-vocabulary classifier on the exact-f32 MFMA (cddmsl_openset_logits).
    ``ld`` (default K + 1) is the row pitch; columns beyond K are left as allocated."""
    require_cuda(x, wn)
    R, D = x.shape
    K = wn.shape[0]
    ld = K + 1 if ld is None else int(ld)
    assert x.dtype == wn.dtype == torch.float32 and x.is_contiguous() and wn.is_contiguous() and wn.dim() == 2 and wn.shape[1] == D
    logits = torch.empty((R, max(ld, 0)), device=x.device, dtype=torch.float32)
    stats = torch.empty((R, 2), device=x.device, dtype=torch.float32)
    check(_L().cddmsl_openset_logits(ptr(x), ptr(wn), ptr(logits), ptr(stats), R, D, K, ld, float(temperature), float(eps), stream_ptr()),
          "cddmsl_openset_logits")
    return logits, stats


def openset_cap(R, K, score_thresh, with_objectness):
    """Candidate slots ``openset_select`` allocates: a softmax row holds at most ceil(1 / thresh) - and never more than K - entries
    above ``thresh``; with the objectness product (the square root of a product with an unbounded factor) any entry may pass."""
    if with_objectness or not score_thresh > 0.0:
        return R * K
    return R * min(K, int(math.ceil(1.0 / score_thresh)))


@_timed("openset_select")
def openset_select_raw(logits, stats, K, boxes, objectness, img_h, img_w, score_thresh, cap):
    """cddmsl_openset_select without the readback -> (cand_row int32 [cap], cand_cls int32 [cap], cand_score f32 [cap], cand_box
    f32 [cap, 4], valid u8 [R], count int32 [1]); count is the full number of candidates, only the first ``cap`` are written."""
    require_cuda(logits, stats, boxes, objectness)
    R, ld = logits.shape
    assert logits.dtype == stats.dtype == boxes.dtype == torch.float32 and logits.is_contiguous() and stats.is_contiguous() and boxes.is_contiguous()
    assert tuple(stats.shape) == (R, 2) and boxes.dim() == 2 and boxes.shape[0] == R
    assert objectness is None or (objectness.dtype == torch.float32 and objectness.is_contiguous() and objectness.numel() == R)
    dev = logits.device
    cap = int(cap)
    cand_row = torch.empty(cap, device=dev, dtype=torch.int32)
    cand_cls = torch.empty(cap, device=dev, dtype=torch.int32)
    cand_score = torch.empty(cap, device=dev, dtype=torch.float32)
    cand_box = torch.empty((cap, 4), device=dev, dtype=torch.float32)
    valid = torch.empty(R, device=dev, dtype=torch.uint8)
    count = torch.zeros(1, device=dev, dtype=torch.int32)
    _with_temp(_L().cddmsl_openset_select, "cddmsl_openset_select", "openset_select", dev, ptr(logits), ptr(stats), ld, ptr(boxes), boxes.shape[1],
               ptr(objectness), R, int(K), float(img_h), float(img_w), float(score_thresh),
               ptr(cand_row), ptr(cand_cls), ptr(cand_score), ptr(cand_box), ptr(valid), ptr(count), cap)
    return cand_row, cand_cls, cand_score, cand_box, valid, count


def openset_select(logits, stats, K, boxes, objectness, img_h, img_w, score_thresh, cap=None):
    """fast_rcnn_inference_single_image up to its NMS on the open-vocabulary logits: softmax from ``stats``, optional geometric
    mean with ``objectness`` [R], rows with a non-finite box or score dropped, boxes clipped to the image, entries above
    ``score_thresh`` in (row, class) order -> (rows int32 [n], classes int32 [n], scores f32 [n], boxes f32 [n, 4], valid u8 [R]).
    ONE host readback (n).  ``cap`` defaults to ``openset_cap``; more candidates than ``cap`` raise ValueError, never a truncation."""
    R = logits.shape[0]
    if cap is None:
        cap = openset_cap(R, K, score_thresh, objectness is not None)
    cand_row, cand_cls, cand_score, cand_box, valid, count = openset_select_raw(logits, stats, K, boxes, objectness, img_h, img_w,
                                                                                score_thresh, cap)
    n = int(count[0])
    if n > cap:
        raise ValueError(f"openset_select: {n} candidates exceed the {cap} slots of this call")
    return cand_row[:n], cand_cls[:n], cand_score[:n], cand_box[:n], valid


@_timed("rpn_decode")
def rpn_decode(order, deltas, cell, img_hw, Hf, Wf, topk, stride, offset, weights, scale_clamp, min_size):
    """Decode + clip the top-k sorted anchors of every image -> boxes [N,topk,4] f32, valid u8 [N,topk]."""
    require_cuda(order, deltas, cell, img_hw)
    N = deltas.shape[0]
    A = cell.shape[0]
    assert deltas.dtype == torch.float32 and deltas.is_contiguous() and img_hw.dtype == torch.int32
    boxes = torch.empty((N, topk, 4), device=deltas.device, dtype=torch.float32)
    valid = torch.empty((N, topk), device=deltas.device, dtype=torch.uint8)
    check(_L().cddmsl_rpn_decode(ptr(order), ptr(deltas), ptr(cell), ptr(img_hw), ptr(boxes), ptr(valid), N, Hf, Wf, A, topk,
                                  stride, offset, *[float(w) for w in weights], scale_clamp, min_size, stream_ptr()),
          "cddmsl_rpn_decode")
    return boxes, valid


@_timed("nms")
def nms(boxes, valid, thr, max_keep):
    """boxes [N,n,4] f32 score-descending, valid u8 [N,n] -> keep int32 [N,max_keep] (positions), nkeep int32 [N]."""
    require_cuda(boxes, valid)
    N, n, _ = boxes.shape
    assert boxes.dtype == torch.float32 and boxes.is_contiguous() and valid.dtype == torch.uint8 and valid.is_contiguous()
    nw = (n + 63) // 64
    mask = workspace("nms_mask", max(N * n * nw, 1) * 8, boxes.device)
    keep = torch.full((N, max_keep), -1, device=boxes.device, dtype=torch.int32)
    nkeep = torch.zeros(N, device=boxes.device, dtype=torch.int32)
    check(_L().cddmsl_nms(ptr(boxes), ptr(valid), ptr(mask), ptr(keep), ptr(nkeep), N, n, thr, max_keep, stream_ptr()), "cddmsl_nms")
    return keep, nkeep


@_timed("iou_match")
def iou_match(gt, preds, thresholds, labels, allow_low_quality, out_matches=None, out_labels=None):
    """Fused pairwise_iou + Matcher for one image: gt [G,4], preds [P,4] -> (matches int64 [P], labels int8 [P]).
    ``out_*``: optional contiguous destination rows (callers that batch several images write into slices of one tensor)."""
    require_cuda(gt, preds)
    G, P = gt.shape[0], preds.shape[0]
    assert gt.dtype == preds.dtype == torch.float32 and gt.is_contiguous() and preds.is_contiguous()
    matches = torch.empty(P, device=preds.device, dtype=torch.int64) if out_matches is None else out_matches
    lab = torch.empty(P, device=preds.device, dtype=torch.int8) if out_labels is None else out_labels
    assert matches.dtype == torch.int64 and lab.dtype == torch.int8 and matches.is_contiguous() and lab.is_contiguous()
    assert matches.numel() == P and lab.numel() == P
    best = torch.empty(max(G, 1), device=preds.device, dtype=torch.int32)
    nthr = len(thresholds)
    t0 = float(thresholds[0])
    t1 = float(thresholds[1]) if nthr > 1 else 0.0
    l = list(labels) + [0]
    check(_L().cddmsl_iou_match(ptr(gt), G, ptr(preds), P, ptr(matches), ptr(lab), ptr(best), nthr, t0, t1, l[0], l[1], l[2],
                                 int(allow_low_quality), stream_ptr()), "cddmsl_iou_match")
    return matches, lab


@_timed("iou_match")
def iou_match_batched(gt_list, preds, pred_counts, thresholds, labels, allow_low_quality):
    """Fused pairwise_iou + Matcher for ALL images in one launch pair.  ``gt_list``: per-image [G_i, 4] f32 tensors;
    ``preds``: [P, 4] shared by every image (``pred_counts`` None; returns [N, P] tensors) or the images' predictions
    concatenated [sum P_i, 4] with ``pred_counts`` = [P_i] (returns [sum P_i] tensors)."""
    require_cuda(preds, *gt_list)
    dev = preds.device
    N = len(gt_list)
    ng = [int(g.shape[0]) for g in gt_list]
    total_g = sum(ng)
    gt = torch.cat(gt_list).float().contiguous() if total_g else torch.zeros((1, 4), device=dev)
    gt_off = to_device_async(torch.tensor([0] + ng, dtype=torch.int32).cumsum(0).to(torch.int32), dev)
    assert preds.dtype == torch.float32 and preds.is_contiguous()
    if pred_counts is None:
        P, pred_off, shape = preds.shape[0], None, (N, preds.shape[0])
    else:
        P, shape = max(pred_counts) if pred_counts else 0, (sum(pred_counts),)
        pred_off = to_device_async(torch.tensor([0] + list(pred_counts), dtype=torch.int32).cumsum(0).to(torch.int32), dev)
    matches = torch.empty(shape, device=dev, dtype=torch.int64)
    lab = torch.empty(shape, device=dev, dtype=torch.int8)
    best = torch.empty(max(total_g, 1), device=dev, dtype=torch.int32)
    nthr = len(thresholds)
    t0 = float(thresholds[0])
    t1 = float(thresholds[1]) if nthr > 1 else 0.0
    l = list(labels) + [0]
    check(_L().cddmsl_iou_match_batched(ptr(gt), ptr(gt_off), ptr(preds), ptr(pred_off), ptr(matches), ptr(lab), ptr(best), N, P,
                                         max(ng) if ng else 0, total_g, nthr, t0, t1, l[0], l[1], l[2], int(allow_low_quality),
                                         stream_ptr()), "cddmsl_iou_match_batched")
    return matches, lab


# ------------------------------------------------------------------------------------------------ attention pool / losses
def l2norm_fwd(x, eps):
    require_cuda(x)
    R, D = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    y = torch.empty_like(x)
    inv = torch.empty(R, device=x.device, dtype=torch.float32)
    check(_L().cddmsl_l2norm_fwd(ptr(x), ptr(y), ptr(inv), R, D, eps, stream_ptr()), "cddmsl_l2norm_fwd")
    return y, inv


def l2norm_bwd(dy, y, inv):
    require_cuda(dy, y, inv)
    dy = dy.contiguous()
    assert y.dim() == 2 and y.dtype == dy.dtype == inv.dtype == torch.float32 and y.is_contiguous() and inv.is_contiguous()
    assert dy.shape == y.shape and inv.numel() == y.shape[0]
    dx = torch.empty_like(y)
    check(_L().cddmsl_l2norm_bwd(ptr(dy), ptr(y), ptr(inv), ptr(dx), y.shape[0], y.shape[1], stream_ptr()), "cddmsl_l2norm_bwd")
    return dx


def cosine_logits_fwd(x, wn, temperature, eps=1e-12):
    require_cuda(x, wn)
    R, D = x.shape
    Kc = wn.shape[0]
    assert x.dtype == wn.dtype == torch.float32 and x.is_contiguous() and wn.is_contiguous() and wn.dim() == 2 and wn.shape[1] == D
    scores = torch.empty((R, Kc + 1), device=x.device, dtype=torch.float32)
    inv = torch.empty(R, device=x.device, dtype=torch.float32)
    check(_L().cddmsl_cosine_logits_fwd(ptr(x), ptr(wn), ptr(scores), ptr(inv), R, D, Kc, temperature, eps, stream_ptr()),
          "cddmsl_cosine_logits_fwd")
    return scores, inv


def cosine_logits_bwd(ds, x, wn, inv, temperature, dx=None):
    require_cuda(ds, x, wn, inv, dx)
    R, D = x.shape
    ds = ds.contiguous()
    assert x.dtype == wn.dtype == inv.dtype == ds.dtype == torch.float32 and x.is_contiguous() and wn.is_contiguous() and inv.is_contiguous()
    assert wn.dim() == 2 and wn.shape[1] == D and tuple(ds.shape) == (R, wn.shape[0] + 1) and inv.numel() == R
    acc = dx is not None
    if dx is None:
        dx = torch.empty_like(x)
    assert dx.dtype == torch.float32 and dx.is_contiguous() and dx.shape == x.shape
    check(_L().cddmsl_cosine_logits_bwd(ptr(ds), ptr(x), ptr(wn), ptr(inv), ptr(dx), R, D, wn.shape[0], temperature, int(acc),
                                         stream_ptr()), "cddmsl_cosine_logits_bwd")
    return dx


def contrastive_fwd(S):
    require_cuda(S)
    n = S.shape[0]
    assert S.dtype == torch.float32 and S.shape == (n, n) and S.is_contiguous()
    rl = torch.empty(n, device=S.device, dtype=torch.float32)
    cl = torch.empty(n, device=S.device, dtype=torch.float32)
    loss = torch.empty(1, device=S.device, dtype=torch.float32)
    check(_L().cddmsl_contrastive_fwd(ptr(S), ptr(rl), ptr(cl), ptr(loss), n, n, stream_ptr()), "cddmsl_contrastive_fwd")
    return loss, rl, cl


def contrastive_bwd(S, rl, cl, gloss):
    require_cuda(S, rl, cl, gloss)
    n = S.shape[0]
    assert S.dtype == rl.dtype == cl.dtype == torch.float32 and tuple(S.shape) == (n, n) and S.is_contiguous()
    assert rl.is_contiguous() and cl.is_contiguous() and rl.numel() == n and cl.numel() == n and gloss.numel() == 1
    dS = torch.empty_like(S)
    check(_L().cddmsl_contrastive_bwd(ptr(S), ptr(rl), ptr(cl), ptr(gloss.reshape(1).float().contiguous()), ptr(dS), n, n, stream_ptr()),
          "cddmsl_contrastive_bwd")
    return dS


@_timed("layernorm")
def layernorm_fwd(x, gamma, beta, out_dtype, eps=1e-5):
    """x [R,D] f32 -> (y [R,D] out_dtype, mean [R], rstd [R])"""
    require_cuda(x, gamma, beta)
    R, D = x.shape
    assert x.dtype == gamma.dtype == beta.dtype == torch.float32 and x.is_contiguous() and gamma.is_contiguous() and beta.is_contiguous()
    assert gamma.numel() == D and beta.numel() == D
    y = torch.empty((R, D), device=x.device, dtype=out_dtype)
    mean = torch.empty(R, device=x.device, dtype=torch.float32)
    rstd = torch.empty(R, device=x.device, dtype=torch.float32)
    check(_L().cddmsl_layernorm_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), R, D, eps, DT[out_dtype], stream_ptr()),
          "cddmsl_layernorm_fwd")
    return y, mean, rstd


@_timed("layernorm")
def layernorm_bwd(dy, x, gamma, mean, rstd, accumulate_into=None, emit_bf16=False):
    """dx = LN'(dy); with ``accumulate_into`` (f32 [R,D], contiguous) the result is ADDED to that tensor in place and it is returned.
    ``emit_bf16``: returns (dx, dx_bf16) -- dx_bf16 = dx.to(bfloat16) written by the same kernel, or None where the rows took the
    scalar kernel (which writes no copy)."""
    require_cuda(dy, x, gamma, mean, rstd, accumulate_into)
    R, D = x.shape
    dy = dy.contiguous()
    assert x.dtype == gamma.dtype == mean.dtype == rstd.dtype == torch.float32 and x.is_contiguous() and gamma.is_contiguous()
    assert mean.is_contiguous() and rstd.is_contiguous() and gamma.numel() == D and mean.numel() == R and rstd.numel() == R and dy.shape == x.shape
    if accumulate_into is None:
        dx, acc = torch.empty_like(x), 0
    else:
        assert accumulate_into.dtype == torch.float32 and accumulate_into.is_contiguous() and accumulate_into.shape == x.shape
        dx, acc = accumulate_into, 1
    if emit_bf16:
        dxb, did = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16), c_int(0)
        check(_L().cddmsl_layernorm_bwd_emit(ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dxb), R, D, acc, _dt(dy),
                                             ctypes.byref(did), stream_ptr()), "cddmsl_layernorm_bwd_emit")
        return dx, (dxb if did.value else None)
    check(_L().cddmsl_layernorm_bwd(ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), R, D, acc, _dt(dy), stream_ptr()),
          "cddmsl_layernorm_bwd")
    return dx


def _attn_views(q, kv, t, heads):
    assert q.dim() == 2 and kv.dim() == 2 and q.is_contiguous() and kv.is_contiguous() and q.dtype == kv.dtype == torch.bfloat16
    R, d = q.shape
    assert kv.shape == (R, 2 * d) and R % t == 0 and d % heads == 0
    return R // t, d, d // heads


@_timed("attn_small")
def attn_small_fwd(q, kv, t, heads, scale):
    """q [n*t, d], kv [n*t, 2d] (keys | values), bf16 -> o [n*t, d] = softmax(q_h k_h^T * scale) v_h per (sequence, head)"""
    require_cuda(q, kv)
    n, d, dh = _attn_views(q, kv, t, heads)
    o = torch.empty_like(q)
    vptr = c_void_p(kv.data_ptr() + d * 2)
    check(_L().cddmsl_attn_small_fwd(ptr(q), ptr(kv), vptr, ptr(o), n, t, heads, dh, d, 2 * d, 2 * d, d, float(scale), 0, stream_ptr()),
          "cddmsl_attn_small_fwd")
    return o


@_timed("attn_last")
def attn_last_fwd(q, kv, t, heads, scale):
    """one query row per sequence: q [n, d], kv [n*t, 2d] (keys | values) bf16 -> (o [n, d] bf16, p [n, heads, t] f32)"""
    require_cuda(q, kv)
    n, d = q.shape
    assert q.dtype == kv.dtype == torch.bfloat16 and q.is_contiguous() and kv.is_contiguous() and tuple(kv.shape) == (n * t, 2 * d)
    o = torch.empty((n, d), device=q.device, dtype=q.dtype)
    p = torch.empty((n, heads, t), device=q.device, dtype=torch.float32)
    check(_L().cddmsl_attn_last_fwd(ptr(q), ptr(kv), ptr(o), ptr(p), n, t, heads, d // heads, d, 2 * d, d, d, float(scale), 0, stream_ptr()),
          "cddmsl_attn_last_fwd")
    return o, p


@_timed("attn_last")
def attn_last_bwd(q, kv, do, p, t, heads, scale):
    """-> (dq [n, d], dkv [n*t, 2d]) bf16"""
    require_cuda(q, kv, do, p)
    n, d = q.shape
    do = do.contiguous()
    assert do.shape == (n, d) and do.dtype == q.dtype and p.is_contiguous()
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    check(_L().cddmsl_attn_last_bwd(ptr(q), ptr(kv), ptr(do), ptr(p), ptr(dq), ptr(dkv), n, t, heads, d // heads, d, 2 * d, d, d, float(scale), 0,
                                    stream_ptr()), "cddmsl_attn_last_bwd")
    return dq, dkv


@_timed("attn_small")
def attn_small_fwd_qkv(qkv, t, heads, scale):
    """qkv [n*t, 3d] (queries | keys | values: ONE projection GEMM's output), bf16 -> o [n*t, d]"""
    require_cuda(qkv)
    assert qkv.dim() == 2 and qkv.is_contiguous() and qkv.dtype == torch.bfloat16 and qkv.shape[1] % 3 == 0 and qkv.shape[0] % t == 0
    R, d = qkv.shape[0], qkv.shape[1] // 3
    o = torch.empty((R, d), device=qkv.device, dtype=qkv.dtype)
    base = qkv.data_ptr()
    check(_L().cddmsl_attn_small_fwd(c_void_p(base), c_void_p(base + d * 2), c_void_p(base + 4 * d), ptr(o), R // t, t, heads, d // heads,
                                     3 * d, 3 * d, 3 * d, d, float(scale), 0, stream_ptr()), "cddmsl_attn_small_fwd")
    return o


@_timed("attn_small")
def attn_small_bwd_qkv(qkv, do, t, heads, scale):
    """-> dqkv [n*t, 3d] bf16 (the three gradients side by side: ONE input-gradient GEMM follows)"""
    require_cuda(qkv, do)
    R, d = qkv.shape[0], qkv.shape[1] // 3
    do = do.contiguous()
    assert do.shape == (R, d) and do.dtype == qkv.dtype
    dqkv = torch.empty_like(qkv)
    base, gbase = qkv.data_ptr(), dqkv.data_ptr()
    check(_L().cddmsl_attn_small_bwd(c_void_p(base), c_void_p(base + d * 2), c_void_p(base + 4 * d), ptr(do), c_void_p(gbase),
                                     c_void_p(gbase + d * 2), c_void_p(gbase + 4 * d), R // t, t, heads, d // heads, 3 * d, 3 * d, 3 * d, d,
                                     float(scale), 0, stream_ptr()), "cddmsl_attn_small_bwd")
    return dqkv


@_timed("text_embed")
def text_embed(ids, tok, pos):
    """ids [n, t] int64 (contiguous, every id in [0, vocab)), tok [vocab, W] bf16 / f32, pos [>= t, W] f32 -> x [n*t, W] f32 =
    tok[ids] + pos[position]"""
    require_cuda(ids, tok, pos)
    assert ids.dim() == 2 and ids.dtype == torch.int64 and ids.is_contiguous() and tok.is_contiguous() and pos.is_contiguous()
    assert pos.dtype == torch.float32 and tok.shape[1] == pos.shape[1] and pos.shape[0] >= ids.shape[1]
    n, t = ids.shape
    W = tok.shape[1]
    x = torch.empty((n * t, W), device=ids.device, dtype=torch.float32)
    check(_L().cddmsl_text_embed(ptr(ids), ptr(tok), ptr(pos), ptr(x), n * t, t, W, tok.shape[0], DT[tok.dtype], stream_ptr()),
          "cddmsl_text_embed")
    return x


@_timed("attn_causal")
def attn_causal_fwd(qkv, t, heads, scale):
    """qkv [n*t, 3W] bf16 (queries | keys | values, the in-projection's output) -> o [n*t, W] bf16, causal (keys j <= query i)"""
    require_cuda(qkv)
    assert qkv.dim() == 2 and qkv.is_contiguous() and qkv.dtype == torch.bfloat16 and qkv.shape[1] % 3 == 0 and qkv.shape[0] % t == 0
    R, W = qkv.shape[0], qkv.shape[1] // 3
    o = torch.empty((R, W), device=qkv.device, dtype=qkv.dtype)
    check(_L().cddmsl_attn_causal_fwd(ptr(qkv), ptr(o), R // t, t, heads, W // heads, 3 * W, W, float(scale), 0, stream_ptr()),
          "cddmsl_attn_causal_fwd")
    return o


@_timed("quick_gelu")
def quick_gelu_(x):
    """x * sigmoid(1.702 x) in place (bf16 or f32, contiguous); returns x"""
    require_cuda(x)
    assert x.is_contiguous()
    check(_L().cddmsl_quick_gelu(ptr(x), x.numel(), DT[x.dtype], stream_ptr()), "cddmsl_quick_gelu")
    return x


@_timed("text_pool")
def text_pool(x, rows, gamma, beta, group=1, out_dtype=torch.float32, eps=1e-5):
    """x [R, W] f32, rows [nout * group] int64 (row indices into x) -> [nout, W] out_dtype: the mean over each group of ``group``
    consecutive entries of rows of LayerNorm(x[row]) (gamma, beta)"""
    require_cuda(x, rows, gamma, beta)
    assert x.dtype == torch.float32 and x.is_contiguous() and rows.dtype == torch.int64 and rows.is_contiguous()
    assert rows.numel() % group == 0 and gamma.numel() == beta.numel() == x.shape[1]
    nout = rows.numel() // group
    y = torch.empty((nout, x.shape[1]), device=x.device, dtype=out_dtype)
    check(_L().cddmsl_text_pool(ptr(x), ptr(rows), ptr(gamma), ptr(beta), ptr(y), x.shape[0], nout, group, x.shape[1], eps,
                                DT[out_dtype], stream_ptr()), "cddmsl_text_pool")
    return y


# ---- GPT-2 decoder (modeling/gpt2.py) ----------------------------------------------------------------------------------------
def skinny_gemm_workspace(M, N, K):
    return int(_L().cddmsl_skinny_gemm_workspace(M, N, K))


@_timed("skinny_gemm")
def skinny_gemm(x, w, bias=None, residual=None, epi=0, out=None):
    """x [M, K] bf16 (M <= 64) @ w [N, K]^T bf16 + bias f32 -> y: epi 0 bf16, 1 f32 (+ residual f32), 2 gelu_new -> bf16.
    ``out`` may be ``residual`` (in place)."""
    require_cuda(x, w, bias, residual, out)
    assert x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.is_contiguous() and w.is_contiguous() and x.dim() == 2
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K
    for v in (bias,):
        assert v is None or (v.dtype == torch.float32 and v.is_contiguous() and v.numel() == N)
    assert residual is None or (epi == 1 and residual.dtype == torch.float32 and residual.is_contiguous() and residual.shape == (M, N))
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=torch.float32 if epi == 1 else torch.bfloat16)
    nb = skinny_gemm_workspace(M, N, K)
    check(0 if nb >= 0 else 1, "cddmsl_skinny_gemm_workspace")
    ws = workspace("gpt2", max(nb, 1 << 20), x.device)    # shared with the LM head (one stream, in order); not regrown up to M = 64
    check(_L().cddmsl_skinny_gemm(ptr(x), ptr(w), ptr(bias), ptr(residual), ptr(out), ptr(ws), ws.numel(), M, N, K, epi, stream_ptr()),
          "cddmsl_skinny_gemm")
    return out


@_timed("lm_head_argmax")
def lm_head_argmax(h, wte, ids=None, logits=False):
    """h [M, K] bf16 (M <= 64), wte [V, K] bf16 -> ids [M] int64 = argmax over v of h @ wte^T (lowest index on ties);
    ``ids`` may be a strided int64 column view to write into.  ``logits``: also return the f32 logits [M, V]."""
    require_cuda(h, wte, ids)
    assert h.dtype == torch.bfloat16 and wte.dtype == torch.bfloat16 and h.is_contiguous() and wte.is_contiguous()
    M, K = h.shape
    V = wte.shape[0]
    assert wte.shape[1] == K
    if ids is None:
        ids = torch.empty(M, device=h.device, dtype=torch.int64)
    assert ids.dtype == torch.int64 and ids.dim() == 1 and ids.numel() == M
    lg = torch.empty((M, V), device=h.device, dtype=torch.float32) if logits else None
    nb = int(_L().cddmsl_lm_head_workspace(M, V))
    check(0 if nb >= 0 else 1, "cddmsl_lm_head_workspace")
    ws = workspace("gpt2", max(nb, 1 << 20), h.device)
    check(_L().cddmsl_lm_head_argmax(ptr(h), ptr(wte), ptr(ids), ids.stride(0), ptr(lg), ptr(ws), ws.numel(), M, V, K, stream_ptr()),
          "cddmsl_lm_head_argmax")
    return (ids, lg) if logits else ids


@_timed("decode_attn")
def decode_attn(qkv, kc, vc, L, heads, scale, out=None):
    """qkv [n, >= 3W] bf16 (this step's c_attn output), kc / vc [n, Lmax, W] bf16 caches holding positions 0..L-2 -> o [n, W] bf16;
    writes this step's keys / values to position L - 1 of the caches"""
    require_cuda(qkv, kc, vc, out)
    n, Lmax, W = kc.shape
    assert qkv.dtype == kc.dtype == vc.dtype == torch.bfloat16 and kc.is_contiguous() and vc.is_contiguous() and vc.shape == kc.shape
    assert qkv.dim() == 2 and qkv.shape[0] == n and qkv.stride(1) == 1 and qkv.shape[1] >= 3 * W and W == heads * 64
    if out is None:
        out = torch.empty((n, W), device=qkv.device, dtype=torch.bfloat16)
    check(_L().cddmsl_decode_attn(ptr(qkv), ptr(kc), ptr(vc), ptr(out), n, heads, 64, L, Lmax, qkv.stride(0), float(scale), 0,
                                  stream_ptr()), "cddmsl_decode_attn")
    return out


@_timed("pos_embed")
def pos_embed(wpe, pos0, t, ids=None, tab=None, src=None, out=None):
    """x [rows, W] f32 = (tab[ids[r]] or src[r]) + wpe[pos0 + r % t]; ids a 1-D int64 (possibly strided) view, tab [vocab, W] bf16
    or f32; src [rows, W] f32"""
    require_cuda(wpe, ids, tab, src, out)
    assert (ids is None) != (src is None) and wpe.dtype == torch.float32 and wpe.is_contiguous()
    W = wpe.shape[1]
    if ids is not None:
        assert ids.dtype == torch.int64 and ids.dim() == 1 and tab is not None and tab.is_contiguous() and tab.shape[1] == W
        rows, ld, vocab, dt = ids.numel(), ids.stride(0), tab.shape[0], DT[tab.dtype]
    else:
        assert src.dtype == torch.float32 and src.is_contiguous() and src.shape[-1] == W
        rows, ld, vocab, dt = src.numel() // W, 1, 0, 1
    if out is None:
        out = torch.empty((rows, W), device=wpe.device, dtype=torch.float32)
    check(_L().cddmsl_pos_embed(ptr(ids), max(ld, 1), ptr(tab), ptr(src), ptr(wpe), ptr(out), rows, t, pos0, W, vocab, wpe.shape[0], dt,
                                stream_ptr()), "cddmsl_pos_embed")
    return out


@_timed("lm_head_topk")
def lm_head_topk(h, wte, B, logits=False):
    """h [M, K] bf16 (M <= 64), wte [V, K] bf16 -> (vals [M, B] f32, idx [M, B] int32, logZ [M] f32[, logits [M, V] f32]): per row
    the B largest logits of h @ wte^T, larger value first and lower index among equal values, and the row's log-sum-exp"""
    require_cuda(h, wte)
    assert h.dtype == torch.bfloat16 and wte.dtype == torch.bfloat16 and h.is_contiguous() and wte.is_contiguous() and h.dim() == 2
    M, K = h.shape
    V = wte.shape[0]
    assert wte.shape[1] == K
    vals = torch.empty((M, max(B, 0)), device=h.device, dtype=torch.float32)
    idx = torch.empty((M, max(B, 0)), device=h.device, dtype=torch.int32)
    logZ = torch.empty(M, device=h.device, dtype=torch.float32)
    lg, ws = None, None
    if logits:
        lg = torch.empty((M, V), device=h.device, dtype=torch.float32)
    else:
        nb = int(_L().cddmsl_lm_head_topk_workspace(M, V))
        check(0 if nb >= 0 else 1, "cddmsl_lm_head_topk_workspace")
        ws = workspace("gpt2_topk", nb, h.device)
    check(_L().cddmsl_lm_head_topk(ptr(h), ptr(wte), ptr(vals), ptr(idx), ptr(logZ), ptr(lg), ptr(ws), 0 if ws is None else ws.numel(),
                                   M, V, K, B, stream_ptr()), "cddmsl_lm_head_topk")
    return (vals, idx, logZ, lg) if logits else (vals, idx, logZ)


class BeamState:
    """the per-beam tables of one chunk of captions, as ``beam_step`` reads and writes them: sum [n, B] f32, len [n, B] int32,
    stop [n, B] uint8, hist [n, B, T] int32 (-1 past a beam's length), anc [n * B, T - 1] uint8 (which beam slot wrote step t of the
    beam's cache history), and of the last step src [n, B] int32 and next_tok [n * B] int64"""

    def __init__(self, n, B, T, device):
        self.n, self.B, self.T = n, B, T
        self.sum = torch.zeros((n, B), device=device, dtype=torch.float32)
        self.len = torch.zeros((n, B), device=device, dtype=torch.int32)
        self.stop = torch.zeros((n, B), device=device, dtype=torch.uint8)
        self.hist = torch.full((n, B, T), -1, device=device, dtype=torch.int32)
        self.anc = torch.zeros((n * B, max(T - 1, 1)), device=device, dtype=torch.uint8)[:, :T - 1]
        self.src = torch.zeros((n, B), device=device, dtype=torch.int32)
        self.next_tok = torch.zeros(n * B, device=device, dtype=torch.int64)


@_timed("beam_step")
def beam_step(vals, idx, logZ, old, new, step, stop_id=None):
    """one beam-selection step: reads the rows' top-B ``vals`` / ``idx`` / ``logZ`` (``lm_head_topk``) and the BeamState ``old``,
    writes the BeamState ``new`` (a distinct object: every permuted table is double-buffered).  ``step`` = tokens already in the
    history; step 0 takes one row per caption and ignores ``old``'s contents."""
    n, B, T = new.n, new.B, new.T
    require_cuda(vals, idx, logZ, old.sum, new.sum)
    rows = n if step == 0 else n * B
    assert old is not new and (old.n, old.B, old.T) == (n, B, T)
    assert vals.dtype == torch.float32 and idx.dtype == torch.int32 and logZ.dtype == torch.float32
    assert vals.is_contiguous() and idx.is_contiguous() and logZ.is_contiguous()
    assert tuple(vals.shape) == tuple(idx.shape) == (rows, B) and logZ.numel() == rows
    anc_in, anc_out = (old.anc, new.anc) if T > 1 else (None, None)
    assert anc_in is None or (anc_in.stride(0) == max(T - 1, 1) and anc_out.stride(0) == max(T - 1, 1))
    check(_L().cddmsl_beam_step(ptr(vals), ptr(idx), ptr(logZ), ptr(old.sum), ptr(old.len), ptr(old.stop), ptr(old.hist), ptr(anc_in),
                                ptr(new.sum), ptr(new.len), ptr(new.stop), ptr(new.hist), ptr(anc_out), ptr(new.src), ptr(new.next_tok),
                                n, B, T, step, -1 if stop_id is None else int(stop_id), stream_ptr()), "cddmsl_beam_step")
    return new


@_timed("decode_attn_beam")
def decode_attn_beam(qkv, pk, pv, gk, gv, anc, L, B, heads, scale, out=None):
    """qkv [rows, >= 3W] bf16 (row = caption * B + beam), prefix caches pk / pv [rows / B, P, W] bf16 shared by a caption's beams,
    generated caches gk / gv [rows, Tg, W] bf16 read through anc [rows, >= L - 1 - P] uint8 (row stride anc.stride(0)) -> o [rows, W]
    bf16; writes this step's keys / values to position L - 1 - P of row r of the generated caches"""
    require_cuda(qkv, pk, pv, gk, gv, anc, out)
    rows, Tg, W = gk.shape
    ncap, P, _ = pk.shape
    assert qkv.dtype == pk.dtype == pv.dtype == gk.dtype == gv.dtype == torch.bfloat16 and anc.dtype == torch.uint8
    assert pk.is_contiguous() and pv.is_contiguous() and gk.is_contiguous() and gv.is_contiguous()
    assert pv.shape == pk.shape and gv.shape == gk.shape and pk.shape[2] == W and W == heads * 64 and (rows % B or ncap * B == rows)
    assert qkv.dim() == 2 and qkv.shape[0] == rows and qkv.stride(1) == 1 and qkv.shape[1] >= 3 * W
    assert anc.dim() == 2 and anc.shape[0] == rows and anc.shape[1] >= L - 1 - P and (anc.shape[1] == 0 or anc.stride(1) == 1)
    ldanc = anc.stride(0) if anc.shape[1] else 0
    if out is None:
        out = torch.empty((rows, W), device=qkv.device, dtype=torch.bfloat16)
    check(_L().cddmsl_decode_attn_beam(ptr(qkv), ptr(pk), ptr(pv), ptr(gk), ptr(gv), ptr(anc if anc.shape[1] else None), ptr(out), rows, B,
                                       heads, 64, P, L, Tg, ldanc, qkv.stride(0), float(scale), 0, stream_ptr()), "cddmsl_decode_attn_beam")
    return out


@_timed("gelu_new")
def gelu_new_(x):
    """GPT-2's tanh GELU in place (bf16 or f32, contiguous); returns x"""
    require_cuda(x)
    assert x.is_contiguous()
    check(_L().cddmsl_gelu_new(ptr(x), x.numel(), DT[x.dtype], stream_ptr()), "cddmsl_gelu_new")
    return x


@_timed("attn_small")
def attn_small_bwd(q, kv, do, t, heads, scale):
    """-> (dq [n*t, d], dkv [n*t, 2d]) bf16"""
    require_cuda(q, kv, do)
    n, d, dh = _attn_views(q, kv, t, heads)
    do = do.contiguous()
    assert do.shape == q.shape and do.dtype == q.dtype
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    vptr, dvptr = c_void_p(kv.data_ptr() + d * 2), c_void_p(dkv.data_ptr() + d * 2)
    check(_L().cddmsl_attn_small_bwd(ptr(q), ptr(kv), vptr, ptr(do), ptr(dq), ptr(dkv), dvptr, n, t, heads, dh, d, 2 * d, 2 * d, d,
                                     float(scale), 0, stream_ptr()), "cddmsl_attn_small_bwd")
    return dq, dkv


def focal_ce_fwd(logits, target, gamma, bg_class, bg_weight):
    require_cuda(logits, target)
    R, C = logits.shape
    assert logits.dtype == torch.float32 and logits.is_contiguous() and target.dtype == torch.int64 and target.is_contiguous() and target.numel() == R
    row = torch.empty(R, device=logits.device, dtype=torch.float32)
    probs = torch.empty_like(logits)
    check(_L().cddmsl_focal_ce_fwd(ptr(logits), ptr(target), ptr(row), ptr(probs), R, C, gamma, bg_class, bg_weight, stream_ptr()),
          "cddmsl_focal_ce_fwd")
    return row, probs


def focal_ce_bwd(logits, target, probs, gscale, gamma, bg_class, bg_weight):
    require_cuda(logits, target, probs, gscale)
    assert logits.dim() == 2 and logits.dtype == probs.dtype == torch.float32 and logits.is_contiguous() and probs.is_contiguous()
    assert probs.shape == logits.shape and target.dtype == torch.int64 and target.is_contiguous() and target.numel() == logits.shape[0]
    assert gscale.numel() == 1
    d = torch.empty_like(logits)
    check(_L().cddmsl_focal_ce_bwd(ptr(logits), ptr(target), ptr(probs), ptr(gscale.reshape(1).float().contiguous()), ptr(d), logits.shape[0],
                                   logits.shape[1], gamma, bg_class, bg_weight, stream_ptr()), "cddmsl_focal_ce_bwd")
    return d


def maxpool3s2_fwd(x):
    """F.max_pool2d(x, 3, 2, 1) on NHWC"""
    require_cuda(x)
    N, H, W, C = x.shape
    y = torch.empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), device=x.device, dtype=x.dtype)
    check(_L().cddmsl_maxpool3s2_fwd(ptr(x), ptr(y), N, H, W, C, _dt(x), stream_ptr()), "cddmsl_maxpool3s2_fwd")
    return y


def upsample_zero2(t, in_shape, mask=None, add=None):
    """dx[:, ::2, ::2] = t, zero elsewhere (+ add), zeroed where mask <= 0: input gradient of a stride-2 1x1 conv."""
    require_cuda(t, mask, add)
    N, H, W, C = in_shape
    assert t.is_contiguous() and tuple(t.shape) == (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C)
    dx = torch.empty(in_shape, device=t.device, dtype=t.dtype)
    check(_L().cddmsl_upsample_zero2(ptr(t), ptr(mask), ptr(add), ptr(dx), N, H, W, C, _dt(t), stream_ptr()), "cddmsl_upsample_zero2")
    return dx


def meanpool_fwd(x):
    """x [K,P,C] (T) -> [K,C] f32"""
    require_cuda(x)
    K, P, C = x.shape
    y = torch.empty((K, C), device=x.device, dtype=torch.float32)
    check(_L().cddmsl_meanpool_fwd(ptr(x), ptr(y), K, P, C, _dt(x), stream_ptr()), "cddmsl_meanpool_fwd")
    return y


def meanpool_bwd(dy, P, dtype):
    require_cuda(dy)
    K, C = dy.shape
    dx = torch.empty((K, P, C), device=dy.device, dtype=dtype)
    check(_L().cddmsl_meanpool_bwd(ptr(dy.contiguous().float()), ptr(dx), K, P, C, DT[dtype], stream_ptr()), "cddmsl_meanpool_bwd")
    return dx


# ------------------------------------------------------------------------------------------------ ClipCap mapper training
def _rows_view(x, what):
    """(ld, cols) of a 2-D bf16 / f32 tensor whose rows may be the leading columns of a wider buffer"""
    assert x.dim() == 2 and (x.shape[1] == 1 or x.stride(1) == 1) and x.stride(0) >= x.shape[1], f"{what}: rows of unit-stride columns"
    return x.stride(0), x.shape[1]


@_timed("k_attn_causal_bwd")
def attn_causal_bwd(qkv, do, t, heads, scale, out=None):
    """Backward of ``attn_causal_fwd``: qkv [n*t, 3W] bf16 (row stride >= 3W), do [n*t, W] bf16 (row stride >= W) -> dqkv
    (dq | dk | dv, qkv's row stride; ``out`` to write into a given buffer)."""
    require_cuda(qkv, do, out)
    ldqkv, W3 = _rows_view(qkv, "qkv")
    ldo, W = _rows_view(do, "do")
    assert qkv.dtype == do.dtype == torch.bfloat16 and W3 == 3 * W and W % heads == 0 and qkv.shape[0] == do.shape[0] and qkv.shape[0] % t == 0
    if out is None:
        out = torch.empty_strided(qkv.shape, qkv.stride(), device=qkv.device, dtype=qkv.dtype) if ldqkv != W3 else torch.empty_like(qkv)
    assert out.dtype == qkv.dtype and out.shape == qkv.shape and out.stride() == qkv.stride(), "dqkv takes qkv's layout"
    check(_L().cddmsl_attn_causal_bwd(ptr(qkv), ptr(do), ptr(out), qkv.shape[0] // t, t, heads, W // heads, ldqkv, ldo, float(scale), 0,
                                      stream_ptr()), "cddmsl_attn_causal_bwd")
    return out


@_timed("gelu_new_bwd")
def gelu_new_bwd(x_pre, dy):
    """dx = dy * gelu_new'(x_pre): x_pre is the c_fc output from before the activation (bf16 or f32, contiguous)"""
    require_cuda(x_pre, dy)
    assert x_pre.is_contiguous() and dy.is_contiguous() and x_pre.dtype == dy.dtype and x_pre.shape == dy.shape
    dx = torch.empty_like(x_pre)
    check(_L().cddmsl_gelu_new_bwd(ptr(x_pre), ptr(dy), ptr(dx), x_pre.numel(), _dt(x_pre), stream_ptr()), "cddmsl_gelu_new_bwd")
    return dx


@_timed("k_token_ce_fwd")
def token_ce_fwd(logits, target, V=None, ignore_index=0):
    """F.cross_entropy(logits[:, :V], target, ignore_index=...) for f32 logits [R, ld] (ld % 8 == 0; columns >= V are padding).
    -> (loss, lse [R], count): loss a 0-dim f32 tensor, the mean over the ``count`` rows whose target is not ``ignore_index``.
    Raises ``ValueError`` when no row counts (one readback of the count: the division is the host's)."""
    require_cuda(logits, target)
    ld, cols = _rows_view(logits, "logits")
    V = cols if V is None else V
    R = logits.shape[0]
    assert logits.dtype == torch.float32 and target.dtype == torch.int64 and target.is_contiguous() and target.numel() == R and 0 < V <= cols
    lse = torch.empty(R, device=logits.device, dtype=torch.float32)
    row = torch.empty(R, device=logits.device, dtype=torch.float32)
    sc = torch.zeros(2, device=logits.device, dtype=torch.float32)
    check(_L().cddmsl_token_ce_fwd(ptr(logits), ld, ptr(target), R, V, ignore_index, ptr(lse), ptr(row), ptr(sc), stream_ptr()),
          "cddmsl_token_ce_fwd")
    count = int(sc[1].item())
    if count == 0:
        raise ValueError("token_ce: every target equals ignore_index, the mean over no rows is undefined")
    return sc[0] / count, lse, count


@_timed("k_token_ce_bwd")
def token_ce_bwd(logits, target, lse, gscale, V=None, ignore_index=0, out_dtype=torch.float32, inplace=False):
    """d loss / d logits = (softmax - onehot) * gscale on the rows that count, zero on ignored rows and padding columns.
    ``gscale`` = upstream gradient / count, a float.  ``inplace`` (f32 only) writes over ``logits``."""
    require_cuda(logits, target, lse)
    ld, cols = _rows_view(logits, "logits")
    V = cols if V is None else V
    R = logits.shape[0]
    assert logits.dtype == lse.dtype == torch.float32 and target.dtype == torch.int64 and target.is_contiguous() and lse.is_contiguous()
    assert target.numel() == R and lse.numel() == R and 0 < V <= cols
    # the kernel walks whole rows of ld columns (the padding is read and discarded, written as zero): the last row's must exist
    assert (logits.storage_offset() + R * ld) * 4 <= logits.untyped_storage().nbytes(), "logits: the last row is shorter than ld"
    if inplace:
        assert out_dtype == torch.float32, "only an f32 gradient can overwrite the f32 logits"
        d = logits
    else:
        # (whole rows of ld columns: the kernel zeroes the padding columns too)
        d = torch.empty((R, ld), device=logits.device, dtype=out_dtype)[:, :cols]
    check(_L().cddmsl_token_ce_bwd(ptr(logits), ld, ptr(target), ptr(lse), float(gscale), ptr(d), R, V, ignore_index, DT[out_dtype],
                                   stream_ptr()), "cddmsl_token_ce_bwd")
    return d


@_timed("layernorm_bwd_params")
def layernorm_bwd_params(dy, x, mean, rstd, dgamma=None, dbeta=None):
    """The LayerNorm affine gradients: dgamma = sum_r dy (x - mean) rstd, dbeta = sum_r dy, f32 [D].  Given ``dgamma`` / ``dbeta``
    (both), the sums are ADDED to them in place."""
    require_cuda(dy, x, mean, rstd, dgamma, dbeta)
    R, D = x.shape
    dy = dy.contiguous()
    assert x.dtype == mean.dtype == rstd.dtype == torch.float32 and x.is_contiguous() and mean.is_contiguous() and rstd.is_contiguous()
    assert dy.shape == x.shape and mean.numel() == R and rstd.numel() == R and (dgamma is None) == (dbeta is None)
    acc = 0 if dgamma is None else 1
    if dgamma is None:
        dgamma, dbeta = torch.empty(D, device=x.device, dtype=torch.float32), torch.empty(D, device=x.device, dtype=torch.float32)
    assert dgamma.dtype == dbeta.dtype == torch.float32 and dgamma.is_contiguous() and dbeta.is_contiguous() and dgamma.numel() == dbeta.numel() == D
    L = _L()
    need = L.cddmsl_layernorm_bwd_params_workspace(R, D)
    if need < 0:
        raise ValueError(f"layernorm_bwd_params: R={R}, D={D} is outside the contract")
    ws = workspace("ln_params", need, x.device)
    check(L.cddmsl_layernorm_bwd_params(ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(dgamma), ptr(dbeta), ptr(ws), ws.numel(), R, D, acc,
                                        _dt(dy), stream_ptr()), "cddmsl_layernorm_bwd_params")
    return dgamma, dbeta


@_timed("adamw_step")
def adamw_step(params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step):
    """torch.optim.AdamW (amsgrad off) over a list of f32 tensors in one launch family; ``step`` >= 1 is the step being taken."""
    n = len(params)
    if n == 0:
        return
    require_cuda(*params, *grads, *exp_avg, *exp_avg_sq)
    assert len(grads) == n and len(exp_avg) == n and len(exp_avg_sq) == n and step >= 1
    for p, g, m, v in zip(params, grads, exp_avg, exp_avg_sq):
        assert p.dtype == g.dtype == m.dtype == v.dtype == torch.float32
        assert same_layout(p, g) and same_layout(p, m) and same_layout(p, v), "param/grad/moments must share a memory layout"
    P = (c_void_p * n)(*[p.data_ptr() for p in params])
    G = (c_void_p * n)(*[g.data_ptr() for g in grads])
    M = (c_void_p * n)(*[m.data_ptr() for m in exp_avg])
    Vv = (c_void_p * n)(*[v.data_ptr() for v in exp_avg_sq])
    S = (c_long * n)(*[p.numel() for p in params])
    check(_L().cddmsl_adamw_step(P, G, M, Vv, S, n, lr, beta1, beta2, eps, weight_decay, int(step), stream_ptr()), "cddmsl_adamw_step")
