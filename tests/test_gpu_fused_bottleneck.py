"""GPU: the fused frozen-bottleneck kernel (cddmsl_bottleneck64_fwd) against the launches it replaces.

Every case runs one 64-plane Bottleneck behind its conv1 twice on the same random bf16 inputs and weights -- through
``hip.bottleneck64_fwd`` and through the separate ``hip.conv_fwd`` launches (what CDDMSL_FUSED_BOTTLENECK=0 runs) -- and
demands ``torch.equal`` on every output: the fused kernel performs the same operations in the same order.  One small case is
anchored independently, against a float64 CPU restatement of the chain."""
import os

import pytest
import torch

from exact_gemm import round_bf16, ulp_bf16

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (name, residual given?, conv1 of the next block?)
VARIANTS = [("res", True, False), ("res_next", True, True), ("down_next", False, True), ("down", False, False)]


def _weights(seed):
    """bf16 weights and non-trivial FrozenBN (scale, bias) of one block + the next block's conv1; scales and biases are negative
    for some channels, so whole channels and scattered elements are zeroed by the ReLUs."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)

    def bn(c):
        scale = (torch.rand(c, generator=g) + 0.5) * torch.where(torch.rand(c, generator=g) < 0.25, -1.0, 1.0)
        return scale.contiguous(), (rn(c) * 0.3).contiguous()
    return {
        "w2": (rn(64, 3, 3, 64) * 576 ** -0.5).bfloat16(), "bn2": bn(64),
        "w3": (rn(256, 1, 1, 64) * 64 ** -0.5).bfloat16(), "bn3": bn(256),
        "wd": (rn(256, 1, 1, 64) * 64 ** -0.5).bfloat16(), "bnd": bn(256),
        "w1n": (rn(64, 1, 1, 256) * 256 ** -0.5).bfloat16(), "bn1n": bn(64),
    }


def _inputs(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    relu_rand = lambda c: torch.randn(N, H, W, c, generator=g).clamp_min(0).bfloat16()      # (post-ReLU activations)
    return {"o1": relu_rand(64), "x0": relu_rand(64), "residual": torch.randn(N, H, W, 256, generator=g).bfloat16()}


def _dev(d):
    return {k: (tuple(t.to(DEV) for t in v) if isinstance(v, tuple) else v.to(DEV)) for k, v in d.items()}


def _separate(hip, wt, inp, given, nxt):
    """today's launches: conv2, the downsample convolution, conv3 with the residual add, conv1 of the next block"""
    o2 = hip.conv_fwd(inp["o1"], wt["w2"], *wt["bn2"], relu=True, pad=1)
    idn = inp["residual"] if given else hip.conv_fwd(inp["x0"], wt["wd"], *wt["bnd"])
    out = hip.conv_fwd(o2, wt["w3"], *wt["bn3"], residual=idn, relu=True)
    return out, (hip.conv_fwd(out, wt["w1n"], *wt["bn1n"], relu=True) if nxt else None)


def _fused(hip, wt, inp, given, nxt):
    kw = dict(residual=inp["residual"]) if given else dict(x0=inp["x0"], wd=wt["wd"], bnd=wt["bnd"])
    if nxt:
        kw.update(w1n=wt["w1n"], bn1n=wt["bn1n"])
    out, o1n = hip.bottleneck64_fwd(inp["o1"], wt["w2"], wt["bn2"], wt["w3"], wt["bn3"], **kw)
    assert hip._L().cddmsl_last_kernel() == 13
    return out, o1n


def _check_equal(shape, given, nxt, seed=0):
    from cddmsl_amd import hip
    wt, inp = _dev(_weights(seed)), _dev(_inputs(*shape, seed + 100))
    out_f, o1n_f = _fused(hip, wt, inp, given, nxt)
    out_s, o1n_s = _separate(hip, wt, inp, given, nxt)
    torch.cuda.synchronize()
    assert out_f.shape == out_s.shape and torch.equal(out_f, out_s), f"out differs in {int((out_f != out_s).sum())} elements"
    frac0 = float((out_s == 0).float().mean())
    assert 0.02 < frac0 < 0.98, frac0                                   # the ReLU is exercised both ways
    assert (o1n_f is None) == (not nxt)
    if nxt:
        assert torch.equal(o1n_f, o1n_s), f"o1n differs in {int((o1n_f != o1n_s).sum())} elements"


@pytest.mark.parametrize("name,given,nxt", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_partial_tile_and_borders(name, given, nxt):
    """2 x 9 x 13 (M = 234): a partial last tile, every border and corner tap masked, an image boundary inside a tile"""
    _check_equal((2, 9, 13), given, nxt)


@pytest.mark.parametrize("shape", [(2, 8, 16), (1, 1, 40), (1, 40, 1)], ids=["whole_tiles", "one_row", "one_column"])
@pytest.mark.parametrize("name,given,nxt", [VARIANTS[1], VARIANTS[2]], ids=["res_next", "down_next"])
def test_whole_tiles_and_degenerate_images(shape, name, given, nxt):
    """2 x 8 x 16: whole tiles only; 1 x 1 x 40 / 1 x 40 x 1: every vertical / horizontal neighbour is padding"""
    _check_equal(shape, given, nxt, seed=1)


@pytest.mark.parametrize("name,given,nxt", [VARIANTS[1], VARIANTS[2]], ids=["res_next", "down_next"])
def test_more_tiles_than_waves(name, given, nxt):
    """2 x 200 x 170 (M = 68 000 > 2048 waves x 32 pixels): the grid-stride loop and the reuse of a wave's LDS slot between tiles"""
    _check_equal((2, 200, 170), given, nxt, seed=2)


def _layer1_blocks(planes, frozen, dtype, seed=5):
    """three CLIP Bottlenecks (stride 1; the first with a downsample convolution) as layers.BlockParams"""
    from cddmsl_amd import layers
    g = torch.Generator().manual_seed(seed)

    def conv_w(co, ci, k):
        w = (torch.randn(co, ci, k, k, generator=g) * (ci * k * k) ** -0.5).to(DEV).contiguous(memory_format=torch.channels_last)
        return torch.nn.Parameter(w, requires_grad=not frozen)

    def bn(c):
        return ((torch.rand(c, generator=g) + 0.5).to(DEV), (torch.randn(c, generator=g) * 0.3).to(DEV))
    blocks, cin = [], planes
    for bi in range(3):
        blocks.append(layers.BlockParams(conv_w(planes, cin, 1), conv_w(planes, planes, 3), conv_w(4 * planes, planes, 1),
                                         conv_w(4 * planes, cin, 1) if bi == 0 else None, bn(planes), bn(planes), bn(4 * planes),
                                         bn(4 * planes) if bi == 0 else None, 1, frozen))
        cin = 4 * planes
    x = torch.randn(2, 24, 40, planes, generator=g).clamp_min(0).to(DEV, dtype)
    return blocks, x


def _run_stage(blocks, x, frozen, switch):
    """res_stage under CDDMSL_FUSED_BOTTLENECK=switch -> (output, profiler row names of its convolution launches)"""
    from cddmsl_amd import hip, layers
    old = os.environ.get("CDDMSL_FUSED_BOTTLENECK")
    os.environ["CDDMSL_FUSED_BOTTLENECK"] = switch
    try:
        hip.PROFILE.enable()
        y = layers.res_stage(x, blocks, frozen)
        names = [e[0] for e in hip.PROFILE.events if e[0].startswith("k_")]      # (the convolution kernels, not the weight preparation)
        hip.PROFILE.collect()
    finally:
        if old is None:
            del os.environ["CDDMSL_FUSED_BOTTLENECK"]
        else:
            os.environ["CDDMSL_FUSED_BOTTLENECK"] = old
    return y, names


def test_stage_switch_on_equals_off():
    """frozen layer1 through res_stage on 2 x 24 x 40: one conv1 launch + one fused launch per block, equal to today's ten launches"""
    blocks, x = _layer1_blocks(64, True, torch.bfloat16)
    y_on, k_on = _run_stage(blocks, x, True, "1")
    y_off, k_off = _run_stage(blocks, x, True, "0")
    assert k_on.count("k_bottleneck64") == 3 and len(k_on) == 4, k_on
    assert "k_bottleneck64" not in k_off and len(k_off) == 10, k_off
    assert y_on.shape == (2, 24, 40, 256) and torch.equal(y_on, y_off)


@pytest.mark.parametrize("what", ["f32", "trainable", "planes128"])
def test_stage_refuses_what_the_kernel_does_not_take(what):
    """f32, a trainable stage and 128 planes keep today's launches with the switch on"""
    planes, frozen, dtype = (128 if what == "planes128" else 64), what != "trainable", (torch.float32 if what == "f32" else torch.bfloat16)
    blocks, x = _layer1_blocks(planes, frozen, dtype)
    if what == "trainable":
        x.requires_grad_(True)
    y, names = _run_stage(blocks, x, frozen, "1")
    assert "k_bottleneck64" not in names and len(names) == 10, names
    assert y.shape == (2, 24, 40, 4 * planes) and bool(torch.isfinite(y.float()).all())


def test_refused_arguments_are_errors():
    """the entry point itself: no f32, not both / neither source of the residual"""
    from cddmsl_amd import hip
    from cddmsl_amd._lib import HipLibraryError, ptr, stream_ptr
    L = hip._L()
    assert L.cddmsl_bottleneck64_ok(2, 9, 13, 0) == 1 and L.cddmsl_bottleneck64_ok(2, 9, 13, 1) == 0
    assert L.cddmsl_bottleneck64_ok(16, 800, 1333, 0) == 0       # a [M][256] tensor past 2 GiB
    wt, inp = _dev(_weights(0)), _dev(_inputs(1, 4, 8, 0))
    out = torch.empty(1, 4, 8, 256, device=DEV, dtype=torch.bfloat16)
    a = [ptr(inp["o1"]), ptr(wt["w2"]), ptr(wt["bn2"][0]), ptr(wt["bn2"][1]), ptr(wt["w3"]), ptr(wt["bn3"][0]), ptr(wt["bn3"][1])]
    none = ptr(None)
    both = a + [ptr(inp["residual"]), ptr(inp["x0"]), ptr(wt["wd"]), ptr(wt["bnd"][0]), ptr(wt["bnd"][1]), none, none, none, ptr(out), none]
    neither = a + [none] * 8 + [ptr(out), none]
    for args in (both, neither):
        assert L.cddmsl_bottleneck64_fwd(*args, 1, 4, 8, 0, stream_ptr()) == 1
    with pytest.raises((HipLibraryError, AssertionError)):
        hip.bottleneck64_fwd(inp["o1"].float(), wt["w2"], wt["bn2"], wt["w3"], wt["bn3"], residual=inp["residual"])


def test_against_float64_chain():
    """Independent anchor, 1 x 12 x 20: the chain restated on the CPU in float64 -- exact products and sums, FrozenBN, residual, ReLU
    -- with o2, out and o1n rounded to bf16 (ties to even) where the kernel rounds them.

    Tolerance, per output tensor: one bf16 ulp (the spacing 2^(e-7) at the tensor's largest exact magnitude) per rounded layer
    the value has passed through -- 2 for out (o2, out; 3 with the downsample result, itself a rounded layer), one more for o1n.
    Reasoning, as in tests/exact_gemm.py: the kernel's f32 accumulation differs from the exact sum by at most
    C_ACC * 2^-24 * sum|a*b|, about 2^-16 of a layer's magnitude at K <= 576 -- far below bf16's 2^-8 -- so a stored value equals
    the correctly rounded exact one except where the exact value lies that close to a rounding tie, and then it is the
    neighbouring bf16 number: at most one ulp of that layer.  The next layer sees such a flip through a weight of magnitude
    K^-1/2 <= 1/8 and |scale| <= 1.5, i.e. as less than one ulp of its own magnitude, and adds its own rounding."""
    from cddmsl_amd import hip
    N, H, W = 1, 12, 20
    wt, inp = _weights(7), _inputs(N, H, W, 107)
    f64 = lambda t: t.to(torch.float64)

    def conv(x, w, bn, pad=0):
        y = torch.nn.functional.conv2d(f64(x).permute(0, 3, 1, 2), f64(w).permute(0, 3, 1, 2), padding=pad).permute(0, 2, 3, 1)
        return y * f64(bn[0]) + f64(bn[1])
    o2 = round_bf16(conv(inp["o1"], wt["w2"], wt["bn2"], 1).clamp_min(0))
    for given in (True, False):
        idn = f64(inp["residual"]) if given else round_bf16(conv(inp["x0"], wt["wd"], wt["bnd"]))
        out = round_bf16((conv(o2, wt["w3"], wt["bn3"]) + idn).clamp_min(0))
        o1n = round_bf16(conv(out, wt["w1n"], wt["bn1n"]).clamp_min(0))
        got_out, got_o1n = _fused(hip, _dev(wt), _dev(inp), given, True)
        layers_out = 2 if given else 3
        for name, got, ref, nl in (("out", got_out, out, layers_out), ("o1n", got_o1n, o1n, layers_out + 1)):
            tol = nl * float(ulp_bf16(ref.abs().max()))
            err = float((f64(got.cpu()) - ref).abs().max())
            print(f"{name} given={given}: max|err| {err:.3e}, tolerance {tol:.3e}, max|ref| {float(ref.abs().max()):.3f}")
            assert err <= tol, (name, given, err, tol)
