"""GPU: three full-tensor passes folded into the kernels next to them, each bit for bit against the launches it replaces.

1. ``cddmsl_conv3x3_pool_fwd``: the stem's third convolution writing AvgPool2d(2) of its result, against ``conv_fwd`` + ``avgpool2_fwd``;
   one case against a float64 restatement of the chain.
2. ``cddmsl_avgpool2_fwd_bits`` / ``cddmsl_avgpool2_bwd_bits``: the pooling forward recording its input's ReLU mask as one byte per 16-byte
   chunk, the backward reading it; ``layers.res_stage`` / ``layers.roi_stage`` with CDDMSL_POOL_MASK_BITS 1 against 0.
3. ``cddmsl_layernorm_bwd_emit``: the LayerNorm backward also storing the bf16 copy of its result; the mapper under autograd with
   CDDMSL_LN_EMIT_BF16 1 against 0.

Raw C-ABI launches write into NaN-filled buffers longer than the result (tests/pool_exact.py): all of the result must be written,
nothing behind it."""
import ctypes

import pytest
import torch

import exact_gemm as X
import pool_exact as P

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
ERR_ARG = 1


# ================================================================================================ 1. stem: conv3 writes the pooled map
STEM_SHAPES = [(1, 2, 2), (2, 6, 10), (1, 7, 9), (1, 4, 34), (3, 8, 16)]


def _stem_operands(N, H, W, seed, cin=32, cout=64, dtype=BF):
    """random inputs of both signs, bf16 weights of a 288-long reduction, a FrozenBN affine with some negative scales"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, cin, generator=g).to(dtype)
    w = (torch.randn(cout, 3, 3, cin, generator=g) * (9 * cin) ** -0.5).to(dtype)
    scale = ((torch.rand(cout, generator=g) + 0.5) * torch.where(torch.rand(cout, generator=g) < 0.25, -1.0, 1.0)).contiguous()
    bias = (torch.randn(cout, generator=g) * 0.3).contiguous()
    return x, w, scale, bias


def _stem_raw(x, w, scale, bias, buf, mask=None, stride=1, dtype=0):
    N, H, W, Cin = x.shape
    return P._L().cddmsl_conv3x3_pool_fwd(P._p(x), P._p(w), P._p(buf), P._p(scale), P._p(bias), P._p(mask), N, H, W, Cin, w.shape[0], stride,
                                          dtype, P._st())


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=["one_pooled_pixel", "tile_across_images", "odd_row_col", "partial_last_tile", "whole_tiles"])
def test_stem_pool_equals_conv_then_pool(shape):
    """(1,2,2): one pooled pixel whose window touches all four image edges; (2,6,10): 15 pooled pixels per image, the second tile
    straddles the two images; (1,7,9): the odd last row and column are dropped; (1,4,34): 17 pooled pixels per row, a partial last
    tile, windows on the left and right edges; (3,8,16): whole tiles only"""
    from cddmsl_amd import hip
    N, H, W = shape
    x, w, scale, bias = (t.to(DEV) for t in _stem_operands(N, H, W, 11 + H * W))
    buf, y = P._out((N, H // 2, W // 2, 64), BF)
    assert _stem_raw(x, w, scale, bias, buf) == 0
    assert hip._L().cddmsl_last_kernel() == 8
    P._written(buf, y, f"conv3x3_pool_fwd {shape}")
    full = hip.conv_fwd(x, w, scale, bias, relu=True, pad=1)
    ref = hip.avgpool2_fwd(full)
    torch.cuda.synchronize()
    P._same_bits(y, ref, f"conv3x3_pool_fwd {shape}")
    assert torch.equal(hip.conv3x3_pool_fwd(x, w, scale, bias), ref)                # (the wrapper stem_nhwc calls)
    if N * H * W >= 60:
        frac0 = float((full == 0).float().mean())
        assert 0.05 < frac0 < 0.95, frac0                                           # the ReLU is exercised both ways


def test_stem_pool_against_float64_chain():
    """(1,7,9) against the chain in float64 on the bf16 operands: exact convolution, affine, ReLU, bf16 rounding (ties to even), the
    2x2 average, bf16 rounding.  Every element within ONE bf16 ulp of the float64 value.

    Why one ulp can occur at all: the kernel's f32 accumulation differs from the exact sum by at most C_ACC * 2^-24 * sum|x*w| (tests/
    exact_gemm.py), about 2^-16 of the layer's magnitude, so a rounded conv value equals the correctly rounded exact one except where
    the exact value lies that close to a tie -- then it is the neighbouring bf16 number.  Such a flip moves the average by a quarter
    of that value's ulp, at most one ulp of the average (the value is at most four times the average), and the final rounding is
    monotone.  Where the float64 value is exactly 0 (all four pre-ReLU values <= 0) an ulp is not defined: there the kernel's value
    may be positive by at most the accumulation bound of the window's four sums (times |scale|), which is the tolerance used."""
    from cddmsl_amd import hip
    N, H, W = 1, 7, 9
    x, w, scale, bias = _stem_operands(N, H, W, 5)
    f64 = lambda t: t.to(torch.float64)
    conv = lambda a, b: torch.nn.functional.conv2d(a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    pre = conv(f64(x), f64(w)) * f64(scale) + f64(bias)
    act = X.round_bf16(pre.clamp_min(0))[:, :H // 2 * 2, :W // 2 * 2]
    ref = X.round_bf16((act[:, 0::2, 0::2] + act[:, 0::2, 1::2] + act[:, 1::2, 0::2] + act[:, 1::2, 1::2]) * 0.25)
    absprod = (conv(f64(x).abs(), f64(w).abs()) * f64(scale).abs())[:, :H // 2 * 2, :W // 2 * 2]
    acc_tol = X.C_ACC * 2.0 ** -24 * torch.maximum(torch.maximum(absprod[:, 0::2, 0::2], absprod[:, 0::2, 1::2]),
                                                   torch.maximum(absprod[:, 1::2, 0::2], absprod[:, 1::2, 1::2]))
    tol = torch.where(ref != 0, X.ulp_bf16(torch.where(ref != 0, ref, torch.ones_like(ref))), acc_tol)
    got = f64(hip.conv3x3_pool_fwd(*(t.to(DEV) for t in (x, w, scale, bias))).cpu())
    err = (got - ref).abs()
    print(f"stem pool vs float64: {int((err > 0).sum())} of {err.numel()} elements differ, max err / tol {float((err / tol).max()):.3g}, "
          f"{int((ref == 0).sum())} exact zeros")
    assert got.shape == ref.shape == (1, 3, 4, 64)
    assert bool((err <= tol).all()), float((err / tol).max())
    assert 0 < int((ref == 0).sum()) < ref.numel()


@pytest.mark.parametrize("what", ["f32", "cout32", "stride2", "mask"])
def test_stem_pool_refusals(what):
    """what the kernel is not built for is CDDMSL_ERR_ARG at the entry point, and nothing is written"""
    dtype = torch.float32 if what == "f32" else BF
    x, w, scale, bias = (t.to(DEV) for t in _stem_operands(1, 4, 6, 3, cout=32 if what == "cout32" else 64, dtype=dtype))
    buf, y = P._out((1, 2, 3, w.shape[0]), dtype)
    mask = torch.ones(1, 4, 6, w.shape[0], device=DEV, dtype=dtype) if what == "mask" else None
    st = _stem_raw(x, w, scale, bias, buf, mask=mask, stride=2 if what == "stride2" else 1, dtype=1 if what == "f32" else 0)
    torch.cuda.synchronize()
    assert st == ERR_ARG, (what, st)
    assert bool(torch.isnan(buf.float()).all())


# ================================================================================================ 2. ReLU mask bits from the pooling kernel
BITS_SHAPES = [(2, 4, 6, 8), (1, 5, 7, 64), (3, 14, 14, 512), (1, 2, 2, 8)]
_pool_cache = {}


def _pool_case(shape):
    """x with exact +0, -0, negative values and one NaN; dy; and the reference results of the existing kernels -- computed once per
    shape and shared by the forward and the backward test"""
    if shape not in _pool_cache:
        from cddmsl_amd import hip
        N, H, W, C = shape
        x = P._rand(shape, 21 + C + H, BF)
        flat = x.view(-1)
        flat[::7] = 0.0
        flat[3::11] = -0.0
        flat[flat.numel() // 2 + 1] = float("nan")
        dy = P._rand((N, H // 2, W // 2, C), 22 + C + H, BF)
        assert bool((x < 0).any()) and bool((x == 0).any()) and int(torch.isnan(x).sum()) == 1
        _pool_cache[shape] = (x, dy, hip.avgpool2_fwd(x), hip.avgpool2_bwd(dy, shape, mask=x))
    return _pool_cache[shape]


def _pack_bits(x):
    """[N,H//2,W//2,C//8] int32 of the definition: byte (dy*2+dx), bit j = x[2oy+dy][2ox+dx][8c+j] > 0"""
    N, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    pos = (x.float() > 0)[:, :2 * Ho, :2 * Wo].view(N, Ho, 2, Wo, 2, C // 8, 8).to(torch.int64)
    word = torch.zeros(N, Ho, Wo, C // 8, device=x.device, dtype=torch.int64)
    for dy in range(2):
        for dx in range(2):
            for j in range(8):
                word |= pos[:, :, dy, :, dx, :, j] << (8 * (dy * 2 + dx) + j)
    return torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32)


@pytest.mark.parametrize("shape", BITS_SHAPES, ids=["one_chunk", "odd", "roi_crop", "one_window"])
def test_avgpool2_fwd_bits(shape):
    N, H, W, C = shape
    x, _, y_ref, _ = _pool_case(shape)
    ybuf, y = P._out((N, H // 2, W // 2, C), BF)
    bbuf = torch.full((y.numel() // 8 + P.TAIL,), 0x5A5A5A5A, device=DEV, dtype=torch.int32)
    assert P._L().cddmsl_avgpool2_fwd_bits(P._p(x), P._p(ybuf), P._p(bbuf), N, H, W, C, 0, P._st()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(ybuf[y.numel():].float()).all()) and bool((bbuf[y.numel() // 8:] == 0x5A5A5A5A).all())
    assert torch.equal(y.view(torch.int16), y_ref.view(torch.int16)), "pooled values differ from avgpool2_fwd (NaN included)"
    assert torch.equal(bbuf[:y.numel() // 8].view(N, H // 2, W // 2, C // 8), _pack_bits(x))


@pytest.mark.parametrize("shape", BITS_SHAPES, ids=["one_chunk", "odd", "roi_crop", "one_window"])
def test_avgpool2_bwd_bits(shape):
    from cddmsl_amd import hip
    N, H, W, C = shape
    x, dy, _, dx_ref = _pool_case(shape)
    _, bits = hip.avgpool2_fwd_bits(x)
    buf, dx = P._out(shape, BF)
    assert P._L().cddmsl_avgpool2_bwd_bits(P._p(dy), P._p(bits), P._p(buf), N, H, W, C, 0, P._st()) == 0
    torch.cuda.synchronize()
    P._written(buf, dx, f"avgpool2_bwd_bits {shape}")
    P._same_bits(dx, dx_ref, f"avgpool2_bwd_bits {shape}")
    if H % 2:
        assert bool((dx[:, H - 1] == 0).all()) and bool((dx[:, :, W - 1] == 0).all())      # the floor-dropped row and column
    assert torch.equal(hip.avgpool2_bwd_bits(dy, shape, bits), dx_ref)


def test_pool_bits_refuse_f32():
    x = torch.zeros(1, 4, 4, 8, device=DEV)
    y, bits = torch.zeros(1, 2, 2, 8, device=DEV), torch.zeros(1, 2, 2, 1, device=DEV, dtype=torch.int32)
    assert P._L().cddmsl_avgpool2_fwd_bits(P._p(x), P._p(y), P._p(bits), 1, 4, 4, 8, 1, P._st()) == ERR_ARG
    assert P._L().cddmsl_avgpool2_bwd_bits(P._p(y), P._p(bits), P._p(x), 1, 4, 4, 8, 1, P._st()) == ERR_ARG


def _blocks(cin, planes, strides, seed):
    """CLIP Bottlenecks as layers.BlockParams, trainable: the first with a downsample convolution"""
    from cddmsl_amd import layers
    g = torch.Generator().manual_seed(seed)

    def conv_w(co, ci, k):
        w = (torch.randn(co, ci, k, k, generator=g) * (ci * k * k) ** -0.5).to(DEV).contiguous(memory_format=torch.channels_last)
        return torch.nn.Parameter(w, requires_grad=True)

    def bn(c):
        return ((torch.rand(c, generator=g) + 0.5).to(DEV), (torch.randn(c, generator=g) * 0.3).to(DEV))
    blocks = []
    for bi, stride in enumerate(strides):
        blocks.append(layers.BlockParams(conv_w(planes, cin, 1), conv_w(planes, planes, 3), conv_w(4 * planes, planes, 1),
                                         conv_w(4 * planes, cin, 1) if bi == 0 else None, bn(planes), bn(planes), bn(4 * planes),
                                         bn(4 * planes) if bi == 0 else None, stride, False))
        cin = 4 * planes
    return blocks


def _stage_run(kind, switch, monkeypatch):
    """one stage forward + backward under CDDMSL_POOL_MASK_BITS=switch -> (tensors by name, profiler rows of its pooling launches)"""
    from cddmsl_amd import hip, layers
    monkeypatch.setenv("CDDMSL_POOL_MASK_BITS", switch)
    g = torch.Generator().manual_seed(9)
    if kind == "res":
        blocks = _blocks(32, 16, (2,), 31)
        x = torch.randn(2, 10, 12, 32, generator=g).clamp_min(0).to(DEV, BF).requires_grad_(True)
    else:
        blocks = _blocks(32, 32, (2, 1), 32)
        x = torch.randn(2, 10, 12, 32, generator=g).clamp_min(0).to(DEV, BF).requires_grad_(True)
        rois = torch.tensor([[0, 8.0, 4.0, 120.0, 90.0], [1, -10.0, 30.0, 70.0, 170.0], [1, 100.0, 60.0, 190.0, 150.0]], device=DEV)
        roi_start = torch.tensor([0, 1, 3], device=DEV, dtype=torch.int32)
    hip.PROFILE.enable()
    if kind == "res":
        y = layers.res_stage(x, blocks, False)
    else:
        y = layers.roi_stage(x, rois, roi_start, blocks, False, 14, 1.0 / 16, 0)
    gy = torch.randn(y.shape, generator=g).to(DEV, BF)
    y.backward(gy)
    rows = [e[0] for e in hip.PROFILE.events if e[0].startswith("avgpool2")]
    hip.PROFILE.collect()
    torch.cuda.synchronize()
    res = {"y": y.detach(), "dx": x.grad}
    for bi, bp in enumerate(blocks):
        for wi, w in enumerate(bp.w):
            if w is not None:
                res[f"block{bi}.w{wi}"] = w.grad
    return {k: v.detach().clone() for k, v in res.items()}, rows


@pytest.mark.parametrize("kind", ["res", "roi"])
def test_stage_mask_bits_on_equals_off(kind, monkeypatch):
    """layers.res_stage on one stride-2 block / layers.roi_stage with 3 RoIs (a stride-2 and a stride-1 block) on a 2 x 10 x 12 x 32
    map, bf16, forward and backward: with the mask kept as bits the output, the input gradient and every weight gradient are
    bit-identical to keeping o2, and the same number of pooling launches run"""
    on, rows_on = _stage_run(kind, "1", monkeypatch)
    off, rows_off = _stage_run(kind, "0", monkeypatch)
    assert set(on) == set(off) and sorted(rows_on) == sorted(rows_off) and "avgpool2_bwd" in rows_on, (rows_on, rows_off)
    for k in off:
        assert off[k] is not None and on[k].dtype == off[k].dtype and torch.equal(on[k], off[k]), k
    assert float(on["dx"].float().abs().max()) > 0


def test_stage_keeps_bits_instead_of_o2(monkeypatch):
    """what the autograd node holds for a pooled block: int32 mask words of 1/16 of o2's bytes with the switch on, o2 with it off"""
    from cddmsl_amd import layers
    blocks = _blocks(32, 16, (2,), 31)
    x = torch.randn(2, 10, 12, 32).clamp_min(0).to(DEV, BF).requires_grad_(True)
    for switch, dtype, shape in (("1", torch.int32, (2, 5, 6, 2)), ("0", BF, (2, 10, 12, 16))):
        monkeypatch.setenv("CDDMSL_POOL_MASK_BITS", switch)
        y = layers.res_stage(x, blocks, False)
        o2 = y.grad_fn.saved_tensors[2]
        assert o2.dtype == dtype and tuple(o2.shape) == shape, (switch, o2.dtype, o2.shape)


# ================================================================================================ 3. LayerNorm backward emits the bf16 copy
@pytest.mark.parametrize("accumulate", [False, True], ids=["plain", "accumulate"])
@pytest.mark.parametrize("R,D", [(3, 768), (65, 768), (4, 256)])
def test_layernorm_bwd_emit(R, D, accumulate):
    from cddmsl_amd import hip
    g = torch.Generator().manual_seed(40 + R)
    x = (torch.randn(R, D, generator=g) * 2 + 0.5).to(DEV)
    gamma, beta = (torch.rand(D, generator=g) + 0.5).to(DEV), torch.randn(D, generator=g).to(DEV)
    dy = torch.randn(R, D, generator=g).to(DEV, BF)
    acc0 = torch.randn(R, D, generator=g).to(DEV)
    _, mean, rstd = hip.layernorm_fwd(x, gamma, beta, BF)
    ref = hip.layernorm_bwd(dy, x, gamma, mean, rstd, accumulate_into=acc0.clone() if accumulate else None)
    dxbuf, dx = P._out((R, D), torch.float32)
    bbuf, dxb = P._out((R, D), BF)
    if accumulate:
        dx.copy_(acc0)
    did = ctypes.c_int(-1)
    st = P._L().cddmsl_layernorm_bwd_emit(P._p(dy), P._p(x), P._p(gamma), P._p(mean), P._p(rstd), P._p(dxbuf), P._p(bbuf), R, D, int(accumulate), 0,
                                          ctypes.byref(did), P._st())
    torch.cuda.synchronize()
    assert st == 0 and did.value == 1
    P._written(dxbuf, dx, "layernorm_bwd_emit dx")
    P._written(bbuf, dxb, "layernorm_bwd_emit dx_bf16")
    assert torch.equal(dx.view(torch.int32), ref.view(torch.int32)), "dx differs from cddmsl_layernorm_bwd"
    assert torch.equal(dxb.view(torch.int16), dx.to(BF).view(torch.int16)), "dx_bf16 is not dx.to(bfloat16)"
    got = hip.layernorm_bwd(dy, x, gamma, mean, rstd, accumulate_into=acc0.clone() if accumulate else None, emit_bf16=True)
    assert torch.equal(got[0], ref) and torch.equal(got[1], ref.to(BF))


def test_layernorm_bwd_emit_scalar_rows_emit_nothing():
    """D = 40 takes the scalar kernel: dx as before, no copy (the caller casts as before)"""
    from cddmsl_amd import hip
    g = torch.Generator().manual_seed(4)
    x, gamma, beta = torch.randn(5, 40, generator=g).to(DEV), torch.rand(40, generator=g).to(DEV) + 0.5, torch.zeros(40, device=DEV)
    dy = torch.randn(5, 40, generator=g).to(DEV, BF)
    _, mean, rstd = hip.layernorm_fwd(x, gamma, beta, BF)
    dx, dxb = hip.layernorm_bwd(dy, x, gamma, mean, rstd, emit_bf16=True)
    assert dxb is None and torch.equal(dx, hip.layernorm_bwd(dy, x, gamma, mean, rstd))


def _mapper_run(switch, monkeypatch):
    from cddmsl_amd import layers, synthetic
    from cddmsl_amd.modeling.clipcap import TransformerMapper
    monkeypatch.setenv("CDDMSL_LN_EMIT_BF16", switch)
    m = TransformerMapper(num_layers=2)
    m.load_state_dict(synthetic.make_mapper_state_dict(1, layers=2))
    m.to(DEV)
    x = torch.randn(2, 1024, generator=torch.Generator().manual_seed(8)).to(DEV).requires_grad_(True)
    gy = torch.randn(2, 40, 768, generator=torch.Generator().manual_seed(9)).to(DEV)
    y = m(x)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU], record_shapes=True) as prof:
        y.backward(gy)
        torch.cuda.synchronize()
    rows = 2 * 80
    numel = lambda shp: int(torch.tensor(list(shp)).prod()) if len(shp) else 0
    casts = [e for e in prof.events() if e.name == "aten::_to_copy" and e.input_shapes and numel(e.input_shapes[0]) == rows * 768]
    layers._BF16_OF.clear()
    return y.detach().clone(), x.grad.detach().clone(), len(casts)


def test_mapper_emit_on_equals_off(monkeypatch):
    """Two full layers, 2 sequences (160 rows), ``TransformerMapper`` under autograd in bf16: the output and the input gradient are
    bit-identical with CDDMSL_LN_EMIT_BF16 1 and 0.  The f32 -> bf16 casts of [160, 768] in the backward pass: four with the switch
    off (the MLP's and the attention projection's, per layer); with it on, every gradient a LayerNorm backward wrote arrives with its
    copy -- the one cast left is of the gradient that enters the top layer from the loss, which no LayerNorm wrote."""
    y1, g1, n1 = _mapper_run("1", monkeypatch)
    y0, g0, n0 = _mapper_run("0", monkeypatch)
    assert bool(torch.isfinite(y0).all()) and bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
    assert torch.equal(y1, y0) and torch.equal(g1, g0)
    assert n0 == 4 and n1 == 1, (n0, n1)
