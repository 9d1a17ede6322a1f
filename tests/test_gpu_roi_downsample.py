"""The RoI head's downsample conv evaluated on the feature map, in front of the pooling (layers.roi_downsample_on_map):

    bnd(convd(avgpool2(roi_align(x)))) = sd * avgpool2(roi_align(convd(x))) + bd

(a) the pooled-only RoIAlign forward carrying that affine AFTER the average, at 2048 and 64 channels, (b) its refusal of a ReLU,
(c) the pooled gather backward at 2048 channels, (d) the whole RoI head entry with CDDMSL_ROI_COMMUTE_DOWN=0 against =1."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE = 1.0 / 16


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------------------------------------ (a), (b): forward
N_A, H_A, W_A = 2, 13, 21


def _rois_a():
    """20 RoIs, ALL on image 1 (image 0 has none): random ones hanging over the borders plus the named edge boxes"""
    g = torch.Generator().manual_seed(71)
    K = 20
    x0, y0 = torch.rand(K, generator=g) * W_A * 16 * 0.9 - 30, torch.rand(K, generator=g) * H_A * 16 * 0.9 - 30
    b = torch.stack([x0, y0, x0 + 6 + torch.rand(K, generator=g) * 260, y0 + 6 + torch.rand(K, generator=g) * 170], dim=1)
    b[0] = torch.tensor([40.0, 50.0, 40.0, 50.0])                      # empty box: a 0 x 0 sampling grid
    b[1] = torch.tensor([5.0, 5.0, 9.0, 8.0])                          # smaller than one bin
    b[2] = torch.tensor([-400.0, -300.0, -200.0, -150.0])              # entirely outside the image
    b[3] = torch.tensor([W_A * 16 - 20.0, H_A * 16 - 30.0, W_A * 16 + 200.0, H_A * 16 + 150.0])   # hanging over the far corner
    b[4] = torch.tensor([200.0, 40.0, 90.0, 160.0])                    # inverted in x: the tap-by-tap fallback inside the rows kernel
    b[5] = torch.tensor([0.0, 0.0, W_A * 16.0, H_A * 16.0])            # the whole image
    return torch.cat([torch.ones(K, 1), b], dim=1).contiguous().cuda()


@pytest.mark.parametrize("C", [2048, 64])
def test_pooled_only_forward_carries_the_affine_after_the_average(C):
    """pooled-only with scale / bias against ``scale * pooled_only(x) + bias`` composed from the affine-free call.
    f32 (tap kernel, 512 / 16 chunks): 1e-5 of the tensor's max.
    bf16 (k_roi_align_fwd_rows<2>, 256 / 8 chunks, and its in-kernel fallback for the inverted box) against the f32 kernel's result
    on the same (bf16-representable) input: ONE bf16 rounding.  The kernel forms the value in f32 and rounds it once on the store:
    half an ulp, <= 2^-9 |ref|; the f32 sums of the two kernels run in different orders and may land on either side of a rounding
    boundary, so one ulp, 2^-8 |ref|, plus the f32 noise of the sums themselves, 1e-5 of the tensor's max (the f32 bound above)."""
    from cddmsl_amd import hip
    rois = _rois_a()
    K = rois.shape[0]
    x16 = _rand((N_A, H_A, W_A, C), 72).bfloat16().cuda()
    x32 = x16.float()
    g = torch.Generator().manual_seed(73)
    sc = ((torch.rand(C, generator=g) + 0.5) * torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0)).cuda()
    bs = (torch.randn(C, generator=g) * 0.3).cuda()
    plain32 = hip.roi_align_forward_affine(x32, rois, 14, 14, SCALE, 0, True, pooled_only=True)
    ref = plain32 * sc + bs
    mx = float(ref.abs().max())
    got32 = hip.roi_align_forward_affine(x32, rois, 14, 14, SCALE, 0, True, sc, bs, pooled_only=True)
    assert got32.shape == (K, 7, 7, C) and got32.dtype == torch.float32
    e32 = float((got32 - ref).abs().max())
    print(f"C={C} f32: max err {e32:.3g} of max {mx:.3g}")
    assert e32 <= 1e-5 * mx
    # the empty box and the box outside the image pool to zero: the bias alone
    for k in (0, 2):
        assert torch.equal(got32[k], bs.expand(7, 7, C))
    got16 = hip.roi_align_forward_affine(x16, rois, 14, 14, SCALE, 0, True, sc, bs, pooled_only=True)
    assert got16.shape == (K, 7, 7, C) and got16.dtype == torch.bfloat16
    err = (got16.float() - got32).abs()
    bound = 2.0 ** -8 * got32.abs() + 1e-5 * mx
    print(f"C={C} bf16: worst err / bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())
    # and the composition from the bf16 affine-free call: that one rounds the pooled value BEFORE the affine, so its error is
    # half an ulp of the pooled value times |scale|, plus the half ulp of the result
    plain16 = hip.roi_align_forward_affine(x16, rois, 14, 14, SCALE, 0, True, pooled_only=True).float()
    comp = plain16 * sc + bs
    bound2 = 2.0 ** -8 * (plain16.abs() * sc.abs() + comp.abs()) + 1e-5 * mx
    assert bool(((got16.float() - comp).abs() <= bound2).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pooled_only_forward_refuses_a_relu(dtype):
    """a ReLU does not commute with the 2x2 average, so the two kernels' orders would differ: CDDMSL_ERR_ARG (1), nothing launched"""
    import ctypes
    from cddmsl_amd import hip
    from cddmsl_amd._lib import HipLibraryError
    C = 64
    rois = _rois_a()
    K = rois.shape[0]
    x = _rand((N_A, H_A, W_A, C), 74).to(dtype).cuda()
    sc, bs = torch.ones(C).cuda(), torch.zeros(C).cuda()
    yp = torch.full((K, 7, 7, C), 7.0, device="cuda", dtype=dtype)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    for esc, ebi in ((sc, bs), (None, None)):
        st = hip._L().cddmsl_roi_align_forward_affine(p(x), p(rois), p(None), p(yp), p(esc), p(ebi), 1, N_A, C, H_A, W_A, K, 14, 14,
                                                      ctypes.c_float(SCALE), 0, 1, 0 if dtype == torch.bfloat16 else 1, p(None), p(None), p(None),
                                                      hip.stream_ptr())
        assert st == 1, st
    torch.cuda.synchronize()
    assert bool((yp == 7.0).all())
    with pytest.raises(HipLibraryError):
        hip.roi_align_forward_affine(x, rois, 14, 14, SCALE, 0, True, sc, bs, relu=True, pooled_only=True)


# ------------------------------------------------------------------------------------------------ (c): backward gather
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 1.5e-2)])
def test_pooled_gather_backward_at_2048_channels(dtype, tol):
    """roi_align_backward(pooled=True) at C = 2048 (bf16: one 16-byte chunk per thread at 256 threads; f32: two) against the plain
    backward of avgpool2_bwd(dy): the RoIs and tolerances of test_gpu_ops.test_roi_align_affine_and_pooled_entry_points"""
    from cddmsl_amd import hip
    N, C, H, W, K = 2, 2048, 11, 17, 23
    g = torch.Generator().manual_seed(9)
    bi = torch.sort(torch.randint(0, N, (K,), generator=g)).values.float()
    x0, y0 = torch.rand(K, generator=g) * W * 16 * 0.9 - 10, torch.rand(K, generator=g) * H * 16 * 0.9 - 10
    rois = torch.stack([bi, x0, y0, x0 + 4 + torch.rand(K, generator=g) * 200, y0 + 4 + torch.rand(K, generator=g) * 150], dim=1).cuda()
    start = torch.tensor([0, int((bi == 0).sum()), K], dtype=torch.int32).cuda()
    dy = _rand((K, 7, 7, C), 43).to(dtype).cuda()
    want = hip.roi_align_backward(hip.avgpool2_bwd(dy, (K, 14, 14, C)), rois, start, (N, H, W, C), SCALE, 0, True)
    got = hip.roi_align_backward(dy, rois, start, (N, H, W, C), SCALE, 0, True, pooled=True)
    assert got.shape == (N, H, W, C) and got.dtype == dtype
    err, mx = float((got.float() - want.float()).abs().max()), float(want.float().abs().max())
    print(f"{dtype}: max err {err:.3g} of max {mx:.3g}")
    assert mx > 0 and err <= tol * mx


# ------------------------------------------------------------------------------------------------ (d): the RoI head entry
def _entry_run(dtype, down, monkeypatch):
    from cddmsl_amd import synthetic
    from cddmsl_amd.config import get_cfg
    from cddmsl_amd.modeling import build_model
    from cddmsl_amd.structures import Boxes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(root, "configs", "VOC-Experiments", "faster_rcnn_CLIP_R_50_C4.yaml"))
    cfg.merge_from_list(["MODEL.COMPUTE_DTYPE", dtype])
    model = build_model(cfg)
    model.load_state_dict(synthetic.make_state_dict(0), strict=False)
    model.train()
    T = model.compute_dtype
    g = torch.Generator().manual_seed(6)
    N, H, W, E = 2, 13, 21, 3
    boxes = []
    for n in range(N):
        k = 8 + 5 * n
        x0, y0 = torch.rand(k, generator=g) * W * 16 * 0.8 - 20, torch.rand(k, generator=g) * H * 16 * 0.8 - 20
        b = torch.stack([x0, y0, x0 + 8 + torch.rand(k, generator=g) * 250, y0 + 8 + torch.rand(k, generator=g) * 180], dim=1)
        b[0] = torch.tensor([30.0, 30.0, 30.0, 30.0])            # empty box
        b[1] = torch.tensor([5.0, 5.0, 9.0, 8.0])                # smaller than one bin
        boxes.append(Boxes(b.cuda()))
    monkeypatch.delenv("CDDMSL_ROI_COMMUTE", raising=False)
    monkeypatch.setenv("CDDMSL_ROI_COMMUTE_DOWN", down)
    feat = (_rand((N, H, W, 1024), 81).relu()).bfloat16().to(T).cuda().requires_grad_(True)    # (bf16-representable inputs for both dtypes)
    extra = (_rand((E, 14, 14, 1024), 82).relu()).bfloat16().to(T).cuda().requires_grad_(True)
    out = model.roi_heads._pooled_embeddings(feat, boxes, model.backbone.layer4, model.backbone.attnpool, extra)
    assert tuple(out.shape) == (sum(len(b) for b in boxes) + E, 1024) and out.dtype == torch.float32
    (out * _rand(tuple(out.shape), 83).cuda()).sum().backward()
    torch.cuda.synchronize()
    res = {k: p.grad.detach().float().cpu().clone() for k, p in model.named_parameters()
           if p.grad is not None and (k.startswith("backbone.layer4.") or k.startswith("backbone.attnpool."))}
    res["(embeddings)"], res["(d feature map)"], res["(d appended maps)"] = out.detach().cpu(), feat.grad.float().cpu(), extra.grad.float().cpu()
    return res


def test_roi_head_entry_with_the_downsample_conv_on_the_map(monkeypatch):
    """RoIAlign -> layer4 -> attention pool with 3 appended maps, CDDMSL_ROI_COMMUTE_DOWN=0 (downsample conv on the pooled crops)
    against =1 (on the feature map, the affine behind the pooled RoIAlign, the pooled gather at 2048 channels in front of the
    conv's two gradient GEMMs): embeddings, the gradients wrt the feature map and the appended maps, every layer4 / attention-pool
    weight gradient.
    f32: the two orders agree to 2e-3 of each tensor's max.
    bf16: each setting against the f32 result; the map order has to be as close to f32 as the crop order, tensor by tensor
    (1.5 x its error + 1e-2: it rounds the 2048-channel map and the gathered gradient where the crop order rounds the pooled
    crops and their gradient -- the bound test_gpu_ops.test_roi_head_entry_with_conv1_in_front_of_the_pooling sets for this path)."""
    rel = lambda u, v: float((u - v).abs().max() / max(float(v.abs().max()), 1e-6))
    off = _entry_run("f32", "0", monkeypatch)
    on = _entry_run("f32", "1", monkeypatch)
    assert set(off) == set(on) and "backbone.layer4.0.downsample.0.weight" in off and "backbone.layer4.0.conv1.weight" in off
    assert any(not torch.equal(on[k], off[k]) for k in off), "the two settings ran the same launches"
    for k in off:
        if float(off[k].abs().max()) >= 1e-7:
            print(f"f32 {k}: {rel(on[k], off[k]):.3g}")
            assert rel(on[k], off[k]) < 2e-3, (k, rel(on[k], off[k]))
    off16 = _entry_run("bf16", "0", monkeypatch)
    on16 = _entry_run("bf16", "1", monkeypatch)
    for k in off:
        if float(off[k].abs().max()) < 1e-7:
            continue
        e_off, e_on = rel(off16[k], off[k]), rel(on16[k], off[k])
        print(f"bf16 vs f32 {k}: crops {e_off:.3g}, map {e_on:.3g}")
        assert e_on < 1.5 * e_off + 1e-2, (k, e_off, e_on)
