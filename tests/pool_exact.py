"""Bit-for-bit checks of the pooling / streaming kernels of cddmsl_amd/csrc/elementwise.hip against torch f32 elementwise arithmetic on
the stored operands, rounded once to the output type (imported by tests/test_gpu_pool_exact.py; not a conftest).  Every launch goes
through the C-ABI with a NaN-filled output buffer longer than the view: the view must be written completely, the tail not at all.

``python -m pool_exact`` runs every check at shapes of at least 3 * 256 * 5 chunks and prints one line per kernel: started with
CDDMSL_GRID_CAP=3 in the environment (the cap is read once per process), every thread of the grid-stride kernels loops several times."""
import ctypes
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import exact_gemm as X  # noqa: E402
import exact_roi as R  # noqa: E402

DEV = "cuda"
TAIL = 64
DTYPES = (torch.bfloat16, torch.float32)


def _L():
    from cddmsl_amd import hip
    return hip._L()


def _st():
    from cddmsl_amd import hip
    return hip.stream_ptr()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _dt(dtype):
    return 0 if dtype == torch.bfloat16 else 1


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _rand(shape, seed, dtype, s=1.0):
    return (torch.randn(shape, device=DEV, generator=_gen(seed)) * s).to(dtype)


def _out(shape, dtype):
    """a NaN-filled buffer of prod(shape) + TAIL elements -> (buffer, view of ``shape``)"""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + TAIL,), float("nan"), device=DEV, dtype=dtype)
    return buf, buf[:n].view(shape)


def _written(buf, view, what):
    assert bool(torch.isfinite(view.float()).all()), f"{what}: an element of the output was not written (or is not finite)"
    assert bool(torch.isnan(buf[view.numel():].float()).all()), f"{what}: an element past the output was written"


def _store(v32, dtype):
    """the f32 value rounded once to the output type (exact_gemm.round_bf16: nearest, ties to even)"""
    assert v32.dtype == torch.float32
    return X.round_bf16(v32).to(torch.bfloat16) if dtype == torch.bfloat16 else v32


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(got, exp, what):
    bad = _bits(got) != _bits(exp)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at {i}: got "
                             f"{float(got.reshape(-1)[i])!r}, expected {float(exp.reshape(-1)[i])!r}")


# ---------------------------------------------------------------------------------------------------------------- avgpool2
def avgpool2_fwd(N, H, W, C, dtype, seed=1):
    x = _rand((N, H, W, C), seed, dtype)
    buf, y = _out((N, H // 2, W // 2, C), dtype)
    assert _L().cddmsl_avgpool2_fwd(_p(x), _p(buf), N, H, W, C, _dt(dtype), _st()) == 0
    _written(buf, y, "avgpool2_fwd")
    f = x.float()[:, :H // 2 * 2, :W // 2 * 2]
    a0, a1, a2, a3 = f[:, 0::2, 0::2], f[:, 0::2, 1::2], f[:, 1::2, 0::2], f[:, 1::2, 1::2]
    _same_bits(y, _store(((a0 + a1) + (a2 + a3)) * 0.25, dtype), f"avgpool2_fwd {(N, H, W, C)} {dtype}")


def _up_exp(dy, N, H, W, C, mask, add, dtype, quarter, stride_only):
    """dx of avgpool2_bwd (quarter: every pixel of a 2x2 group gets dy / 4; the floor-dropped row / column 0) or of upsample_zero2
    (stride_only: even (y, x) get t), then + add, then zero where mask <= 0 -- f32, in the kernel's order"""
    v = torch.zeros(N, H, W, C, device=DEV, dtype=torch.float32)
    g = dy.float()
    if stride_only:
        v[:, 0::2, 0::2] = g
    else:
        Ho, Wo = H // 2, W // 2
        v[:, :2 * Ho, :2 * Wo] = (g * 0.25).repeat_interleave(2, 1).repeat_interleave(2, 2)
    if add is not None:
        v = v + add.float()
    if mask is not None:
        v = torch.where(mask.float() > 0, v, torch.zeros_like(v))
    return v


def _mask_add(N, H, W, C, dtype, mask, add, seed):
    m = _rand((N, H, W, C), seed + 1, dtype) if mask else None
    if m is not None:
        m.view(-1)[::7] = 0.0
        m.view(-1)[3::11] = -0.0
    a = _rand((N, H, W, C), seed + 2, dtype) if add else None
    return m, a


def avgpool2_bwd(N, H, W, C, dtype, mask, add, seed=2):
    dy = _rand((N, H // 2, W // 2, C), seed, dtype)
    m, a = _mask_add(N, H, W, C, dtype, mask, add, seed)
    buf, dx = _out((N, H, W, C), dtype)
    assert _L().cddmsl_avgpool2_bwd(_p(dy), _p(m), _p(a), _p(buf), N, H, W, C, _dt(dtype), _st()) == 0
    _written(buf, dx, "avgpool2_bwd")
    exp = _up_exp(dy, N, H, W, C, m, a, dtype, True, False)
    _same_bits(dx, _store(exp, dtype), f"avgpool2_bwd {(N, H, W, C)} {dtype} mask={mask} add={add}")


def avgpool2_bwd_q8(N, H, W, C, mask, add, q8=24.0, seed=3):
    """the fp8 form (bf16): dx bit for bit; the e4m3 copy of the f32 value times q8 (check_e4m3 with an exact operand: only a tie may
    go either way; some values saturate at this q8); amax8 = max |f32 value| exactly"""
    dtype = torch.bfloat16
    dy = _rand((N, H // 2, W // 2, C), seed, dtype, 40.0)
    m, a = _mask_add(N, H, W, C, dtype, mask, add, seed)
    buf, dx = _out((N, H, W, C), dtype)
    b8 = torch.full((N * H * W * C + TAIL,), 0x7F, device=DEV, dtype=torch.uint8)        # (0x7f: e4m3's NaN)
    y8 = b8[:N * H * W * C].view(N, H, W, C)
    q = torch.tensor([q8], device=DEV, dtype=torch.float32)
    amax = torch.zeros(64, device=DEV, dtype=torch.float32)
    assert _L().cddmsl_avgpool2_bwd_q8(_p(dy), _p(m), _p(a), _p(buf), N, H, W, C, _p(b8), _p(q), _p(amax), _st()) == 0
    _written(buf, dx, "avgpool2_bwd_q8")
    assert bool((b8[y8.numel():] == 0x7F).all()), "avgpool2_bwd_q8: a byte past the e4m3 copy was written"
    exp = _up_exp(dy, N, H, W, C, m, a, dtype, True, False)
    _same_bits(dx, _store(exp, dtype), f"avgpool2_bwd_q8 dx {(N, H, W, C)} mask={mask} add={add}")
    ok, r, w = R.check_e4m3(y8, exp, torch.zeros_like(exp, dtype=torch.float64), q8)
    assert ok, f"avgpool2_bwd_q8 y8: |err| / (half ulp) {r:.3g} at {w}: code {int(y8.reshape(-1)[w])}, value {float(exp.reshape(-1)[w]) * q8!r}"
    assert float((exp.abs() * q8).max()) > 448.0, "no value saturates: choose a larger q8"
    assert float(amax.max()) == float(exp.abs().max()), (float(amax.max()), float(exp.abs().max()))


# ---------------------------------------------------------------------------------------------------------------- stock ResNet pieces
def maxpool3s2_fwd(N, H, W, C, dtype, seed=4):
    x = _rand((N, H, W, C), seed, dtype)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    buf, y = _out((N, Ho, Wo, C), dtype)
    assert _L().cddmsl_maxpool3s2_fwd(_p(x), _p(buf), N, H, W, C, _dt(dtype), _st()) == 0
    _written(buf, y, "maxpool3s2_fwd")                            # (finite: no -inf from an all-padding window)
    exp = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(y.float(), exp), f"maxpool3s2_fwd {(N, H, W, C)} {dtype}: {int((y.float() != exp).sum())} elements differ"


def upsample_zero2(N, H, W, C, dtype, mask, add, seed=5):
    t = _rand((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), seed, dtype)
    m, a = _mask_add(N, H, W, C, dtype, mask, add, seed)
    buf, dx = _out((N, H, W, C), dtype)
    assert _L().cddmsl_upsample_zero2(_p(t), _p(m), _p(a), _p(buf), N, H, W, C, _dt(dtype), _st()) == 0
    _written(buf, dx, "upsample_zero2")
    exp = _up_exp(t, N, H, W, C, m, a, dtype, False, True)
    _same_bits(dx, _store(exp, dtype), f"upsample_zero2 {(N, H, W, C)} {dtype} mask={mask} add={add}")


def _div(t, P):
    """t / P as one IEEE f32 division, on the host (a device division by a scalar may be a multiplication by its reciprocal)"""
    c = t.cpu()
    return (c / torch.full_like(c, float(P))).to(DEV)


def meanpool_fwd(K, P, C, dtype, seed=6):
    """a sequential f32 sum over P, then one division"""
    x = _rand((K, P, C), seed, dtype)
    buf, y = _out((K, C), torch.float32)
    assert _L().cddmsl_meanpool_fwd(_p(x), _p(buf), K, P, C, _dt(dtype), _st()) == 0
    _written(buf, y, "meanpool_fwd")
    s = torch.zeros(K, C, device=DEV, dtype=torch.float32)
    for p in range(P):
        s = s + x[:, p].float()
    _same_bits(y, _div(s, P), f"meanpool_fwd {(K, P, C)} {dtype}")


def meanpool_bwd(K, P, C, dtype, seed=7):
    dy = _rand((K, C), seed, torch.float32)
    buf, dx = _out((K, P, C), dtype)
    assert _L().cddmsl_meanpool_bwd(_p(dy), _p(buf), K, P, C, _dt(dtype), _st()) == 0
    _written(buf, dx, "meanpool_bwd")
    _same_bits(dx, _store(_div(dy, P).unsqueeze(1).expand(K, P, C).contiguous(), dtype), f"meanpool_bwd {(K, P, C)} {dtype}")


def relu_bwd(n, dtype, g_f32, seed=8):
    """dx = g where y > 0 else 0, in y's dtype; the mask holds zeros, negative zeros and denormals of both signs"""
    y = _rand((n,), seed, dtype)
    y[0::5] = 0.0
    y[1::13] = -0.0
    yb = _bits(y)                                                 # (denormals by bit pattern: 2^-130 in bf16, 2^-140 in f32)
    yb[2::17] = 0x0008 if dtype == torch.bfloat16 else 0x0200
    yb[3::19] = -0x8000 + 0x0008 if dtype == torch.bfloat16 else -0x80000000 + 0x0200
    pos = _bits(y) > 0                                            # y > 0 read from the bits: no flush-to-zero can enter the expectation
    g = _rand((n,), seed + 1, torch.float32 if g_f32 else dtype)
    g[4::23] = -0.0
    buf, dx = _out((n,), dtype)
    assert _L().cddmsl_relu_bwd(_p(g), _p(y), _p(buf), n, int(g_f32), _dt(dtype), _st()) == 0
    _written(buf, dx, "relu_bwd")
    exp = torch.where(pos, g.float(), torch.zeros(n, device=DEV))
    _same_bits(dx, _store(exp, dtype), f"relu_bwd n={n} {dtype} g_f32={g_f32}")


# ---------------------------------------------------------------------------------------------------------------- the child process
def run_all_large():
    """every check at >= 3 * 256 * 5 chunks of 16 bytes: with a grid of 3 blocks every thread loops at least 5 times"""
    for dtype in DTYPES:
        per = 8 if dtype == torch.bfloat16 else 4
        C = 16 * per                                              # 16 chunks per pixel
        avgpool2_fwd(2, 23, 31, C, dtype)                         # 2 * 11 * 15 * 16 = 5280 output chunks
        avgpool2_bwd(2, 11, 15, C, dtype, True, True)             # 5280 chunks, odd H and W
        avgpool2_bwd(2, 12, 10, C, dtype, False, False)
        maxpool3s2_fwd(2, 23, 29, C, dtype)                       # 2 * 12 * 15 * 16 = 5760
        upsample_zero2(2, 11, 15, C, dtype, True, True)
        upsample_zero2(2, 12, 10, C, dtype, False, False)
        relu_bwd(3 * 256 * 5 * per + 16 * per, dtype, False)
        meanpool_fwd(40, 49, 100, dtype)
        meanpool_bwd(40, 49, 100, dtype)
    relu_bwd(3 * 256 * 5 * 8 + 128, torch.bfloat16, True)
    avgpool2_bwd_q8(2, 11, 15, 128, True, True)
    torch.cuda.synchronize()
    for k in ("avgpool2_fwd", "avgpool2_bwd", "avgpool2_bwd_q8", "maxpool3s2_fwd", "upsample_zero2", "meanpool_fwd", "meanpool_bwd", "relu_bwd"):
        print(f"{k}: ok (CDDMSL_GRID_CAP={os.environ.get('CDDMSL_GRID_CAP', 'unset')})")


if __name__ == "__main__":
    run_all_large()
