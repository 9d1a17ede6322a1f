"""RoIAlign (cddmsl_amd/csrc/roi_align.hip) against float64 references of the operands each kernel was given (tests/exact_roi.py),
element by element, on the case tables of tests/roi_exact_cases.py: every entry point, called through the C-ABI with NaN-filled
outputs that are longer than the view; every dispatch threshold of k_roi_align_fwd_rows with a named box on each side; the tap
kernel's channel loop and its e4m3 second output; the NC = 1 / 2 / 4 instantiations of the gather backward, images holding 0, 1, 64,
65 and 130 RoIs, the pooled fold and a non-square grid; the NCHW any-order entry points.

Worst |err| / bound per kernel output, measured on one MI355X (the table this module prints at its end):
  bwd NC=1 bf16                                0.923
  bwd NC=1 f32                                 0.009
  bwd NC=2 bf16                                0.876
  bwd NC=2 f32                                 0.002
  bwd NC=4 bf16                                0.916
  bwd NC=4 f32                                 0.002
  bwd pooled NC=1 bf16                         0.897
  bwd pooled NC=1 f32                          0.009
  bwd pooled NC=2 bf16                         0.927
  bwd pooled NC=2 f32                          0.002
  bwd pooled NC=4 bf16                         0.931
  bwd pooled NC=4 f32                          0.002
  fwd_rows affine+relu bf16                    0.996
  fwd_rows crops bf16                          0.996
  fwd_rows pooled-only bf16                    0.996
  fwd_tap affine+relu f32                      0.371
  fwd_tap crops bf16                           0.996
  fwd_tap crops f32                            0.205
  fwd_tap emit8 crops bf16                     0.996
  fwd_tap emit8 y8 (e4m3)                      1.000
  fwd_tap<2> crops bf16                        0.996
  fwd_tap<2> crops f32                         0.192
  nchw_anyorder bwd bf16                       0.551
  nchw_anyorder bwd f32                        0.001
  nchw_anyorder fwd bf16                       0.996
  nchw_anyorder fwd f32                        0.153
The bf16 outputs sit near 1 because half an ulp of the store is most of their bound; their f32 twins show what the sums leave.
The f32 backward outputs are below 0.01: their bound is dominated by the coordinate term 2 delta per table entry (delta = C_GEO u M,
against sums that are in fact good to a few u), so on its own it would not see a small weight error there.  What still separates
them: the backward mutants of tests/test_roi_bound_host.py (RoIs 64.. skipped, the fold at weight 1, Ax read with the wrong stride, an
image left unwritten) are all rejected by the same bound, and the dyadic edge boxes have delta = 0, where the bound is the sums' alone.
The e4m3 copy reaches 1.000 at exact ties of the e4m3 rounding (either neighbour is accepted there).
"""
import ctypes

import pytest
import torch

import exact_roi as R
import roi_exact_cases as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
S = T.SCALE
EXTRA = 2                           # rows allocated behind the K crops (the wrappers' extra_rows): must stay untouched
WORST = {}
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    """the worst-ratio table starts empty; the cached operands and references are released after the module's last test"""
    WORST.clear()
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def _L():
    from cddmsl_amd import hip
    return hip._L()


def _stream():
    from cddmsl_amd import hip
    return hip.stream_ptr()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _dt(dtype):
    return 0 if dtype == torch.bfloat16 else 1


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, seed, dtype, s=1.0):
    return (torch.randn(shape, device=DEV, generator=_gen(seed)) * s).to(dtype)


def _nan_rows(K, rest, dtype):
    """a NaN-filled buffer of K + EXTRA leading rows -> (buffer, the view of the first K)"""
    buf = torch.full((K + EXTRA, *rest), float("nan"), device=DEV, dtype=dtype)
    return buf, buf[:K]


def _written(buf, K, what):
    assert bool(torch.isfinite(buf[:K].float()).all()), f"{what}: an element of the output view was not written (or is not finite)"
    assert bool(torch.isnan(buf[K:].float()).all()), f"{what}: an element past the output view was written"


def _judge(kernel, case, got, exact, bound, rows=None, bias=None):
    """``kernel``: the key of the worst-ratio table; ``rows``: the case table (names the RoI of a failing element)"""
    ok, r, w = R.check(got, exact, bound)
    WORST[kernel] = max(WORST.get(kernel, 0.0), r)
    msg = f"{kernel} [{case}]: worst |err|/bound {r:.3g}"
    if not ok:
        idx = R.locate(w, tuple(exact.shape))
        who = f"RoI {idx[0]} ({rows[idx[0]][0]})" if rows is not None else f"image {idx[0]}"
        g, e = R._f64(got).reshape(-1)[w], R._f64(exact).reshape(-1)[w]
        raise AssertionError(f"{msg}; {who}, bin / pixel {idx[1:3]}, channel {idx[3]}: got {float(g)!r}, exact {float(e)!r}, "
                             f"bound {float(R._f64(bound).reshape(-1)[w])!r}")
    if bias is not None:
        rb, n = R.store_bias(got, *bias)
        msg += f", store bias {rb:+.4f} over {n}"
        if n >= R.BIAS_MIN_ELEMENTS:
            assert abs(rb) <= R.BIAS_LIMIT, msg
    print(msg)


# ---------------------------------------------------------------------------------------------------------------- cached operands
def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _tab(name):
    """-> (rows, rois on the device, N, H, W)"""
    def make():
        if name == "bench":
            rows, N, H, W = T.table_bench(), 2, 50, 84
        elif name == "counts":
            rows, N, H, W = T.table_counts(13, 21, (64, 0, 130, 1, 65), 40), 5, 13, 21
        elif name == "wide":
            rows, N, H, W = T.table_counts(6, 7, (11, 9), 50), 2, 6, 7
        else:
            H, W = (13, 21) if name == "F13" else (40, 67)
            rows, N = T.table_F(H, W), 2
        return rows, T.rois_tensor(rows, DEV), N, H, W
    return _cached(("tab", name), make)


CMAX = {torch.bfloat16: 2560, torch.float32: 1280}


def _map(name, dtype, cmax=None):
    rows, rois, N, H, W = _tab(name)
    cmax = cmax or CMAX[dtype]
    return _cached(("map", name, dtype, cmax), lambda: _randn((N, H, W, cmax), 1 if dtype == torch.bfloat16 else 2, dtype))


def _fwd_ref(name, dtype, sr=0, aligned=True, pooled=False, cmax=None):
    """the float64 forward of the whole cached map (all CMAX channels): cases at fewer channels slice it"""
    rows, rois, N, H, W = _tab(name)
    cmax = cmax or CMAX[dtype]
    return _cached(("fwd", name, dtype, sr, aligned, pooled, cmax),
                   lambda: R.roi_fwd(_map(name, dtype, cmax), rois, T.PH, T.PW, S, sr, aligned, pooled=pooled, out_dtype=dtype))


def _launch_fwd(x, rois, ph, pw, sr, aligned, y=None, yp=None, esc=None, ebi=None, relu=False, y8=None, q8=None, amax8=None, plain=False):
    N, H, W, C = x.shape
    K = rois.shape[0]
    if plain:
        e = _L().cddmsl_roi_align_forward(_ptr(x), _ptr(rois), _ptr(y), _ptr(yp), None, N, C, H, W, K, ph, pw, S, sr, int(aligned), _dt(x.dtype), _stream())
    else:
        e = _L().cddmsl_roi_align_forward_affine(_ptr(x), _ptr(rois), _ptr(y), _ptr(yp), _ptr(esc), _ptr(ebi), int(relu), N, C, H, W, K, ph, pw, S,
                                                 sr, int(aligned), _dt(x.dtype), _ptr(y8), _ptr(q8), _ptr(amax8), _stream())
    assert e == 0, e


def _crops_case(kernel, name, dtype, C, sr=0, aligned=True, plain=True, cmax=None):
    rows, rois, N, H, W = _tab(name)
    x = _map(name, dtype, cmax)[..., :C].contiguous()
    f = R.affine(_fwd_ref(name, dtype, sr, aligned, cmax=cmax), out_dtype=dtype, channels=C)
    buf, y = _nan_rows(len(rows), (T.PH, T.PW, C), dtype)
    _launch_fwd(x, rois, T.PH, T.PW, sr, aligned, y=buf, plain=plain)
    _written(buf, len(rows), kernel)
    _judge(kernel, f"{name} C={C} sr={sr} aligned={aligned}", y, f["exact"], f["bound"], rows,
           (f["exact"], f["pre"]) if dtype == torch.bfloat16 else None)
    return y, f


MAPS = ["F13", "F40"]


# ================================================================================================== forward
@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("C", [64, 512, 1024, 2048])
def test_fwd_rows_kernel_bf16_crops(name, C):
    """8 / 64 / 128 / 256 channel chunks: one block of 64 .. 256 lanes per bin row, the row-sliding kernel"""
    _crops_case("fwd_rows crops bf16", name, torch.bfloat16, C)


@pytest.mark.parametrize("name", MAPS)
def test_fwd_tap_kernel_channel_loop(name):
    """320 chunks: more than one block's worth, so the tap kernel with its c += blockDim.x loop"""
    _crops_case("fwd_tap crops bf16", name, torch.bfloat16, 2560)


@pytest.mark.parametrize("name", MAPS)
def test_fwd_tap_kernel_on_the_same_boxes(name, monkeypatch):
    monkeypatch.setenv("CDDMSL_ROI_ROWS", "0")
    rows, rois, N, H, W = _tab(name)
    x = _map(name, torch.bfloat16)[..., :512].contiguous()
    f = R.affine(_fwd_ref(name, torch.bfloat16), out_dtype=torch.bfloat16, channels=512)
    buf, y = _nan_rows(len(rows), (14, 14, 512), torch.bfloat16)
    _launch_fwd(x, rois, 14, 14, 0, True, y=buf, plain=True)
    _written(buf, len(rows), "fwd_tap")
    _judge("fwd_tap crops bf16", f"{name} C=512 CDDMSL_ROI_ROWS=0", y, f["exact"], f["bound"], rows, (f["exact"], f["pre"]))


@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("C", [64, 1024, 1280])
def test_fwd_f32_crops(name, C):
    _crops_case("fwd_tap crops f32", name, torch.float32, C)


@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("dtype,C", [(torch.bfloat16, 512), (torch.float32, 64)], ids=["bf16", "f32"])
def test_fwd_affine_relu(name, dtype, C):
    """y = relu(scale * roi_align(x) + bias) with scales of both signs; an empty box and the RoI of image N give relu(bias)"""
    rows, rois, N, H, W = _tab(name)
    x = _map(name, dtype)[..., :C].contiguous()
    esc = (torch.rand(C, device=DEV, generator=_gen(11)) + 0.5) * torch.where(torch.arange(C, device=DEV) % 3 == 0, -1.0, 1.0)
    ebi = torch.randn(C, device=DEV, generator=_gen(12)) * 0.3
    f = R.affine(_fwd_ref(name, dtype), esc, ebi, True, dtype, C)
    buf, y = _nan_rows(len(rows), (14, 14, C), dtype)
    _launch_fwd(x, rois, 14, 14, 0, True, y=buf, esc=esc, ebi=ebi, relu=True)
    _written(buf, len(rows), "affine")
    kern = "fwd_rows affine+relu bf16" if dtype == torch.bfloat16 else "fwd_tap affine+relu f32"
    _judge(kern, f"{name} C={C}", y, f["exact"], f["bound"], rows, (f["exact"], f["pre"]) if dtype == torch.bfloat16 else None)
    k = T.names(rows).index("empty_adaptive")
    assert torch.equal(y[k].float(), ebi.clamp_min(0).to(dtype).float().expand(14, 14, C)) and torch.equal(y[-1], y[k])


@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("sr", [0, 2])
def test_fwd_pooled_only_output(name, C, sr):
    """k_roi_align_fwd_rows<2>: only the 2x2-average-pooled crops, the mean of four unrounded bins"""
    rows, rois, N, H, W = _tab(name)
    x = _map(name, torch.bfloat16, 512)[..., :C].contiguous()
    f = R.affine(_fwd_ref(name, torch.bfloat16, sr, True, pooled=True, cmax=512), out_dtype=torch.bfloat16, channels=C)
    buf, yp = _nan_rows(len(rows), (7, 7, C), torch.bfloat16)
    _launch_fwd(x, rois, 14, 14, sr, True, yp=buf)
    _written(buf, len(rows), "pooled-only")
    _judge("fwd_rows pooled-only bf16", f"{name} C={C} sr={sr}", yp, f["exact"], f["bound"], rows, (f["exact"], f["pre"]))


@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("dtype,C", [(torch.bfloat16, 512), (torch.float32, 64)], ids=["bf16", "f32"])
def test_fwd_crops_with_the_pooled_by_product(name, dtype, C):
    """with_pooled: the crops against the bound; the pooled map bit for bit T(((a0 + a1) + (a2 + a3)) * 0.25f) of the stored crops"""
    rows, rois, N, H, W = _tab(name)
    x = _map(name, dtype)[..., :C].contiguous()
    f = R.affine(_fwd_ref(name, dtype), out_dtype=dtype, channels=C)
    buf, y = _nan_rows(len(rows), (14, 14, C), dtype)
    bufp, yp = _nan_rows(len(rows), (7, 7, C), dtype)
    _launch_fwd(x, rois, 14, 14, 0, True, y=buf, yp=bufp, plain=True)
    _written(buf, len(rows), "with_pooled y")
    _written(bufp, len(rows), "with_pooled yp")
    _judge(f"fwd_tap<2> crops {'bf16' if dtype == torch.bfloat16 else 'f32'}", f"{name} C={C}", y, f["exact"], f["bound"], rows,
           (f["exact"], f["pre"]) if dtype == torch.bfloat16 else None)
    exp = R.pooled_of_stored(y)
    assert torch.equal(yp.view(torch.int16 if dtype == torch.bfloat16 else torch.int32), exp.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), \
        f"pooled by-product differs from the pooling of the stored crops in {int((yp != exp).sum())} elements"


@pytest.mark.parametrize("name", MAPS)
def test_fwd_e4m3_second_output(name):
    """emit8: y8 = e4m3(sat(y * q8)) of the unrounded y, max|y| in amax8; q8 = 200 saturates |y| > 2.24"""
    rows, rois, N, H, W = _tab(name)
    C, K, q8 = 512, len(rows), 200.0
    x = _map(name, torch.bfloat16)[..., :C].contiguous()
    esc = (torch.rand(C, device=DEV, generator=_gen(13)) + 0.5) * torch.where(torch.arange(C, device=DEV) % 2 == 0, -1.0, 1.0)
    ebi = torch.randn(C, device=DEV, generator=_gen(14)) * 0.3
    f = R.affine(_fwd_ref(name, torch.bfloat16), esc, ebi, True, torch.bfloat16, C)
    buf, y = _nan_rows(K, (14, 14, C), torch.bfloat16)
    b8 = torch.full((K + EXTRA, 14, 14, C), 0x7F, device=DEV, dtype=torch.uint8)          # (0x7f: e4m3's NaN)
    q = torch.tensor([q8], device=DEV)
    amax = torch.zeros(64, device=DEV)
    _launch_fwd(x, rois, 14, 14, 0, True, y=buf, esc=esc, ebi=ebi, relu=True, y8=b8, q8=q, amax8=amax)
    _written(buf, K, "emit8 y")
    assert bool((b8[K:] == 0x7F).all()) and bool(((b8[:K] & 0x7F) != 0x7F).all())
    _judge("fwd_tap emit8 crops bf16", f"{name} C={C}", y, f["exact"], f["bound"], rows, (f["exact"], f["pre"]))
    ok, r, w = R.check_e4m3(b8[:K], f["exact"], f["pre"], q8)
    WORST["fwd_tap emit8 y8 (e4m3)"] = max(WORST.get("fwd_tap emit8 y8 (e4m3)", 0.0), r)
    idx = R.locate(w, tuple(f["exact"].shape))
    assert ok, f"y8: |err|/bound {r:.3g} at RoI {idx[0]} ({rows[idx[0]][0]}) bin {idx[1:3]} channel {idx[3]}: code {int(b8[:K].reshape(-1)[w])}, exact*q8 {float(f['exact'].reshape(-1)[w]) * q8!r}"
    assert float(f["exact"].max()) * q8 > 448.0, "nothing saturates"
    ok, got, lo, hi = R.check_amax(amax, f["exact"], f["pre"] + R.U_F32 * f["exact"].abs())
    assert ok, f"amax8 {got!r} outside [{lo!r}, {hi!r}]"


@pytest.mark.parametrize("name", MAPS)
def test_fwd_sampling_ratio_2_and_unaligned(name):
    _crops_case("fwd_rows crops bf16", name, torch.bfloat16, 512, sr=2, cmax=512)
    _crops_case("fwd_rows crops bf16", name, torch.bfloat16, 512, aligned=False, cmax=512)
    _crops_case("fwd_tap crops f32", name, torch.float32, 64, sr=2, cmax=64)


def test_fwd_bench_geometry():
    """50 x 84 map, 96 + 70 boxes of ~9 feature pixels, 1024 channels: crops, affine + ReLU and the pooled-only output"""
    rows, rois, N, H, W = _tab("bench")
    C, dtype = 1024, torch.bfloat16
    _crops_case("fwd_rows crops bf16", "bench", dtype, C, plain=False, cmax=C)
    x = _map("bench", dtype, C)
    esc = torch.rand(C, device=DEV, generator=_gen(15)) + 0.5
    ebi = torch.randn(C, device=DEV, generator=_gen(16)) * 0.3
    f = R.affine(_fwd_ref("bench", dtype, cmax=C), esc, ebi, True, dtype)
    buf, y = _nan_rows(len(rows), (14, 14, C), dtype)
    _launch_fwd(x, rois, 14, 14, 0, True, y=buf, esc=esc, ebi=ebi, relu=True)
    _written(buf, len(rows), "bench affine")
    _judge("fwd_rows affine+relu bf16", "bench C=1024", y, f["exact"], f["bound"], rows, (f["exact"], f["pre"]))
    fp = R.roi_fwd(x, rois, 14, 14, S, 0, True, pooled=True, geo=f["geo"])
    buf, yp = _nan_rows(len(rows), (7, 7, C), dtype)
    _launch_fwd(x, rois, 14, 14, 0, True, yp=buf)
    _written(buf, len(rows), "bench pooled-only")
    _judge("fwd_rows pooled-only bf16", "bench C=1024", yp, fp["exact"], fp["bound"], rows, (fp["exact"], fp["pre"]))


# ================================================================================================== backward
def _launch_bwd(dy, rois, start, in_shape, sr, aligned, pooled=False):
    """-> (buffer of N + EXTRA images, NaN-filled before the launch)"""
    N, H, W, C = in_shape
    K, ph, pw, _ = dy.shape
    buf = torch.full((N + EXTRA, H, W, C), float("nan"), device=DEV, dtype=dy.dtype)
    ay = torch.full((max(K, 1) * H * ph,), float("nan"), device=DEV)
    ax = torch.full((max(K, 1) * W * pw,), float("nan"), device=DEV)
    fp = torch.zeros(max(K, 1) * 4, device=DEV, dtype=torch.int32)
    fn = _L().cddmsl_roi_align_backward_pooled if pooled else _L().cddmsl_roi_align_backward
    e = fn(_ptr(dy), _ptr(rois), _ptr(start), _ptr(buf), _ptr(ay), _ptr(ax), _ptr(fp), N, C, H, W, K, ph, pw, S, sr, int(aligned), _dt(dy.dtype), _stream())
    assert e == 0, e
    return buf


def _bwd_case(kernel, name, dtype, C, ph=14, pw=14, pooled=False, dy_scale=0.5):
    rows, rois, N, H, W = _tab(name)
    K = len(rows)
    cmax = max(C, 1024) if name in MAPS and dtype == torch.bfloat16 else C

    def make():
        dy = _randn((K, ph, pw, cmax), 21, dtype, dy_scale)
        dy[K // 2] = 0                                             # one RoI whose gradient is exactly zero
        return dy, R.roi_bwd(dy, rois, (N, H, W, cmax), S, 0, True, 2 if pooled else 1, dtype)
    dyf, ref = _cached(("bwd", name, dtype, cmax, ph, pw, pooled), make)
    dy = dyf[..., :C].contiguous()
    start = T.roi_start(rows, N, DEV)
    buf = _launch_bwd(dy, rois, start, (N, H, W, C), 0, True, pooled)
    _written(buf, N, kernel)
    exact, pre = ref["exact"][..., :C], ref["pre"][..., :C]
    _judge(kernel, f"{name} C={C} {ph}x{pw}{' pooled' if pooled else ''}", buf[:N], exact, R.store_bound(exact, pre, R.u_out(dtype)), None,
           (exact, pre) if dtype == torch.bfloat16 else None)
    return buf, dy, start


@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("pooled", [False, True], ids=["14x14", "pooled7x7"])
@pytest.mark.parametrize("dtype,C", [(torch.bfloat16, 64), (torch.bfloat16, 1024), (torch.float32, 64)], ids=["bf16-64", "bf16-1024", "f32-64"])
def test_bwd_one_chunk_per_thread(name, pooled, dtype, C):
    """NC = 1 on table F (an empty box, an inverted one, a RoI of image N past roi_start[N], one RoI with dy = 0)"""
    p = 7 if pooled else 14
    _bwd_case(f"bwd{' pooled' if pooled else ''} NC=1 {'bf16' if dtype == torch.bfloat16 else 'f32'}", name, dtype, C, p, p, pooled)


@pytest.mark.parametrize("pooled", [False, True], ids=["14x14", "pooled7x7"])
@pytest.mark.parametrize("dtype,C,nc", [(torch.bfloat16, 4096, 2), (torch.bfloat16, 8192, 4), (torch.float32, 2048, 2), (torch.float32, 4096, 4)],
                         ids=["bf16-NC2", "bf16-NC4", "f32-NC2", "f32-NC4"])
def test_bwd_two_and_four_chunks_per_thread(pooled, dtype, C, nc):
    """512 and 1024 chunks per pixel on a 6 x 7 map with 20 boxes"""
    p = 7 if pooled else 14
    _bwd_case(f"bwd{' pooled' if pooled else ''} NC={nc} {'bf16' if dtype == torch.bfloat16 else 'f32'}", "wide", dtype, C, p, p, pooled)


def test_bwd_non_square_grid():
    _bwd_case("bwd NC=1 bf16", "F13", torch.bfloat16, 64, 6, 14)
    _bwd_case("bwd NC=1 f32", "F40", torch.float32, 64, 6, 14)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_bwd_images_with_0_1_64_65_130_rois_and_determinism(dtype):
    """the ballot loop takes 64 RoIs at a time; an image without RoIs is still written, as zeros; odd H and W leave the 2x2 tiles hanging
    over the edge; two launches give the same bytes"""
    kern = f"bwd NC=1 {'bf16' if dtype == torch.bfloat16 else 'f32'}"
    buf, dy, start = _bwd_case(kern, "counts", dtype, 64)
    rows, rois, N, H, W = _tab("counts")
    assert start.tolist() == [0, 64, 64, 194, 195, 260]
    assert bool((buf[1] == 0).all()), "the image without RoIs is not zero"
    again = _launch_bwd(dy, rois, start, (N, H, W, 64), 0, True)
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert torch.equal(buf[:N].view(bits), again[:N].view(bits))


# ================================================================================================== NCHW, RoIs in any order
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_nchw_any_order_entry_points(dtype):
    """37 channels (not a whole 16-byte chunk), shuffled RoIs: forward and backward against the same references"""
    rows, rois0, N, H, W = _tab("F13")
    K, C = len(rows), 37
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(3)).to(DEV)
    rois = rois0[perm].contiguous()
    prow = [rows[i] for i in perm.tolist()]
    x = _randn((N, C, H, W), 31, dtype)
    xh = x.permute(0, 2, 3, 1)
    f = R.roi_fwd(xh, rois, 14, 14, S, 0, True, out_dtype=dtype)
    buf = torch.full((K + EXTRA, C, 14, 14), float("nan"), device=DEV, dtype=dtype)
    nbytes = ctypes.c_size_t(0)
    args = (N, C, H, W, K, 14, 14, S, 0, 1, _dt(dtype))
    assert _L().cddmsl_roi_align_nchw_anyorder(_ptr(x), _ptr(rois), _ptr(buf), *args, None, ctypes.byref(nbytes), _stream()) == 0
    ws = torch.empty(nbytes.value + 256, device=DEV, dtype=torch.uint8)
    assert _L().cddmsl_roi_align_nchw_anyorder(_ptr(x), _ptr(rois), _ptr(buf), *args, _ptr(ws), ctypes.byref(nbytes), _stream()) == 0
    _written(buf, K, "nchw forward")
    tag = "bf16" if dtype == torch.bfloat16 else "f32"
    _judge(f"nchw_anyorder fwd {tag}", "F13 shuffled C=37", buf[:K].permute(0, 2, 3, 1), f["exact"], f["bound"], prow,
           (f["exact"], f["pre"]) if dtype == torch.bfloat16 else None)
    dy = _randn((K, C, 14, 14), 32, dtype, 0.5)
    b = R.roi_bwd(dy.permute(0, 2, 3, 1), rois, (N, H, W, C), S, 0, True, 1, dtype)
    dbuf = torch.full((N + EXTRA, C, H, W), float("nan"), device=DEV, dtype=dtype)
    assert _L().cddmsl_roi_align_backward_nchw_anyorder(_ptr(dy), _ptr(rois), _ptr(dbuf), *args, None, ctypes.byref(nbytes), _stream()) == 0
    ws = torch.empty(nbytes.value + 256, device=DEV, dtype=torch.uint8)
    assert _L().cddmsl_roi_align_backward_nchw_anyorder(_ptr(dy), _ptr(rois), _ptr(dbuf), *args, _ptr(ws), ctypes.byref(nbytes), _stream()) == 0
    _written(dbuf, N, "nchw backward")
    _judge(f"nchw_anyorder bwd {tag}", "F13 shuffled C=37", dbuf[:N].permute(0, 2, 3, 1), b["exact"], b["bound"], None,
           (b["exact"], b["pre"]) if dtype == torch.bfloat16 else None)


# ================================================================================================== the table
def test_worst_ratio_table(capsys):
    """the module's last test: the worst |err| / bound of every kernel output checked above, one line each (shown without -s);
    every one of them is at most 1"""
    lines = ["", "worst |err| / bound per kernel output:"] + [f"  {k:44s} {WORST[k]:.3f}" for k in sorted(WORST)]
    with capsys.disabled():
        print("\n".join(lines))
    assert all(v <= 1.0 for v in WORST.values()), WORST
