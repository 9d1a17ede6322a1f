"""Case table of tests/test_gpu_graph_exact.py and tests/test_graph_ref_host.py, plain data: every autograd node of
cddmsl_amd/layers.py and the stock ResNet's stage node (cddmsl_amd/modeling/resnet.py StockStageFn, kind ``stock_stage``), branch by
branch, at the smallest shapes at which the branch is still taken.

A case: ``kind`` (which node; tests/graph_ref.py ``reference`` and the GPU test's runner dispatch on it), ``branch`` (the name in
REQUIRED_BRANCHES it covers), ``selects`` (the condition in layers.py that takes the branch), ``why`` (what the shape is for, and
where it departs from the issue's starting point), the shapes, ``env`` (per-call switches, set through monkeypatch), which inputs want
a gradient, and ``seed``.  Every case runs in f32 and in bf16 on the same bf16-valued inputs."""

DTYPES = ("f32", "bf16")


def _case(name, kind, branch, selects, why, seed, env=None, **kw):
    return dict(name=name, kind=kind, branch=branch, selects=selects, why=why, seed=seed, env=dict(env or {}), dtypes=DTYPES, **kw)


def _conv(name, branch, selects, why, seed, x, w, bias=True, stride=1, pad=0, relu=False, residual=False, out_f32=False, train_w=True,
          x_grad=True, route=None):
    return _case(name, "conv", branch, selects, why, seed, x=x, w=w, bias=bias, stride=stride, pad=pad, relu=relu, residual=residual,
                 out_f32=out_f32, train_w=train_w, x_grad=x_grad, route=route)


def _stage(name, branch, selects, why, seed, x=(2, 10, 12, 32), planes=16, strides=(2,), x_grad=True, premasked=False, px="none",
           bits="1", pooled=None):
    return _case(name, "stage", branch, selects, why, seed, {"CDDMSL_POOL_MASK_BITS": bits}, x=x, planes=planes, strides=strides,
                 x_grad=x_grad, premasked=premasked, px=px, pooled=pooled)


def _stock(name, branch, selects, why, seed, x=(2, 10, 12, 32), planes=16, strides=(2,), x_grad=True, pool=False):
    # (32 channels in, 16 planes, 64 out: the first block has the shortcut convolution, the others the identity, as make_stage builds them)
    return _case(name, "stock_stage", branch, selects, why, seed, x=x, planes=planes, strides=strides, x_grad=x_grad, pool=pool)


def _roi(commute, extra, feat_grad, bits, seed):
    name = f"roi_commute{commute}_extra_{extra}_{'feat' if feat_grad else 'nofeat'}_bits{bits}"
    return _case(name, "roi", f"roi.on_map{commute}.extra_{extra}", "RoIStageFn.backward: `if on_map` / `if E` / `needs_input_grad[9]` / `needs_input_grad[0]`",
                 "six RoIs on image 1 (inside, over two borders each way, smaller than a bin, the whole map, over one border), none on "
                 "image 0; blocks (2, 1) of 32 planes on a 2 x 10 x 12 x 32 map, 14 x 14 crops", seed,
                 {"CDDMSL_ROI_COMMUTE_DOWN": str(commute), "CDDMSL_POOL_MASK_BITS": str(bits)}, feat=(2, 10, 12, 32), planes=32, strides=(2, 1),
                 extra=extra, feat_grad=feat_grad, on_map=bool(commute))


def _attn(name, branch, selects, why, seed, dx="1", premask=False, frozen=False, x_grad=True, stage=None):
    # mean_share: the frozen pool's k_proj draws 0.9 of the attention to the mean token (tests/graph_ref.py ``drop_dtypes`` says why; the
    # premasked one's map has a channel mean, and its rounded model then exceeds the cap)
    return _case(name, "attn", branch, selects, why, seed, {"CDDMSL_ATTNPOOL_DX": dx}, x=(3, 7, 7, 512), heads=8, out=64, premask=premask,
                 frozen=frozen, x_grad=x_grad, stage=stage, fused=(dx == "1" and x_grad), mean_share=0.9 if frozen and not premask else None)


_X = (2, 5, 7, 32)
_ATTN_WHY = ("the issue's 2 heads of D = 64 on 128 channels are refused: cddmsl_gemm_tn_batched takes rows of whole 16-byte chunks, and the "
             "softmax's transposed output has `heads` columns (8 in bf16, 4 in f32), and hip.attnpool_dx_ok wants 2 * heads % 8 == 0; 8 heads "
             "of D = 64 on 512 channels is the smallest shape that keeps D and is taken in both dtypes")

CASES = [
    # ---------------------------------------------------------------------------------------------------- ConvFn
    _conv("conv_1x1_bias_relu", "conv.relu_bias_dx", "ConvFn.backward: `if relu` (hip.relu_bwd), `if train_w`, `ctx.bias is not None`, the plain dgrad",
          "70 rows: one ragged tile; 24 output channels", 101, _X, (24, 32, 1, 1), relu=True),
    _conv("conv_3x3_residual", "conv.residual", "ConvFn.backward: `dy_in if ctx.needs_input_grad[9]`",
          "3x3 pad 1 with a residual of the compute dtype; its gradient is the incoming one, bit for bit", 102, _X, (24, 32, 3, 3), pad=1, residual=True),
    _conv("conv_3x3_residual_out_f32", "conv.residual_out_f32", "layers.conv `out_f32` with a residual: hip.conv_fwd `res_f32` on the bf16 path",
          "the f32 residual stream on the bf16 kernels (Cout a multiple of 8)", 103, _X, (24, 32, 3, 3), pad=1, residual=True, out_f32=True),
    _conv("conv_3x3_stride2_wgrad", "conv.strided_wgrad", "ConvFn.backward: `ctx.needs_input_grad[0]` False, hip.conv_wgrad with stride 2",
          "x wants no gradient (a strided input gradient is refused): the strided weight gradient alone", 104, _X, (24, 32, 3, 3), stride=2, pad=1, x_grad=False),
    _conv("conv_frozen_weights", "conv.train_w_false", "ConvFn.backward: `if train_w` False", "w.grad and b.grad stay None, dx is right", 105,
          _X, (24, 32, 1, 1), relu=True, train_w=False),
    _conv("linear_f32_gradient", "conv.bf16_of", "ConvFn.backward: `elif dy.dtype != T: bf16_of(dy)`",
          "a 2-D weight [N, K] through layers.linear with out_f32: the incoming gradient is f32 on the bf16 path", 106, (40, 64), (48, 64), out_f32=True),
    _conv("linear_sliced_dx", "conv.sliced_dx", "ConvFn.backward: `rows <= 1024 and Kd >= 8192 and Kd % (16 * 64) == 0`",
          "40 rows, Kd = 8192: the 16-slice batched input gradient", 107, (40, 64), (8192, 64), route="sliced"),
    _conv("linear_plain_dx_4096", "conv.plain_dx_below_8192", "ConvFn.backward: the same condition, False for Kd = 4096",
          "the sliced route's neighbour", 108, (40, 64), (4096, 64), route="plain"),
    # ---------------------------------------------------------------------------------------------------- FusedHeadsFn
    _case("heads_4d_out_f32", "heads", "heads.4d_out_f32", "FusedHeadsFn.backward: `_ohwi(_grad_buf(w)).add_` (4-D weights)",
          "widths 3 + 12 = 15 columns, padded to 16; the pad column's incoming gradient is not zero", 111, x=_X, widths=(3, 12), w4d=True, out_f32=True),
    _case("heads_2d_out_compute", "heads", "heads.2d_out_compute", "FusedHeadsFn.backward: `_grad_buf(w).view(n, -1).add_` (2-D weights)",
          "the same heads as [N, K] weights, output in the compute dtype", 112, x=_X, widths=(3, 12), w4d=False, out_f32=False),
    # ---------------------------------------------------------------------------------------------------- FrozenMlpFn
    _case("frozen_mlp", "mlp", "mlp.residual", "FrozenMlpFn.backward: relu_mask = h in fc2's input gradient; `dy if ctx.needs_input_grad[5]`",
          "[40, 64] -> 128 -> 64 with an f32 residual that wants a gradient", 121, rows=40, width=64, hidden=128),
    # ---------------------------------------------------------------------------------------------------- ResStageFn / _block_backward
    _stage("stage_pooled_residual", "stage.pooled_residual", "_block_backward: `pooled = x.shape[1] % 2 == 0 and x.shape[2] % 2 == 0 and hip.pooled_residual_ok(dxb)`",
           "stride 2 with a downsample convolution on 10 x 12: the quarter of the pooled gradient is added in conv1's dgrad epilogue", 131, pooled=True),
    _stage("stage_pool_fallback_odd", "stage.avgpool2_bwd_fallback", "_block_backward: `if not pooled: dxb = hip.avgpool2_bwd(dxb, x.shape)`",
           "9 x 11: the pooling floors, the last row and column get no gradient from either pooled path", 132, x=(2, 9, 11, 32), pooled=False),
    _stage("stage_two_blocks", "stage.mask_between_blocks", "_block_backward: `wdp is None: dxb = gs`, `relu_mask=x if mask_x`",
           "blocks (1, 1): the first with a downsample convolution and no pooling, the second with the identity", 133, strides=(1, 1)),
    _stage("stage_no_dx", "stage.need_dx_false", "_block_backward: `if not need_dx: return None`", "x wants no gradient: the four weight gradients alone", 134,
           x_grad=False),
    _stage("stage_premasked", "stage.out_grad_premasked", "ResStageFn.backward: `g.contiguous() if ctx.out_grad_premasked`",
           "the gradient passed in is that of the pre-ReLU sum", 135, premasked=True, pooled=True),
    _stage("stage_px_given", "stage.px_given_match", "_block_forward: `px_given is not None and tuple(px_given.shape) == (N, H // 2, W // 2, C)`",
           "x._pooled2 holds the right pooled map: one avgpool2_fwd launch fewer", 136, px="match", pooled=True),
    _stage("stage_px_given_other_shape", "stage.px_given_mismatch", "_block_forward: the same condition, False",
           "x._pooled2 of another shape, filled with NaN: ignored", 137, px="mismatch", pooled=True),
    _stage("stage_mask_bits_off", "stage.pool_mask_bits_off", "_pool_bits_wanted: CDDMSL_POOL_MASK_BITS=0 keeps o2 (every other stage case: 1, bits in bf16)",
           "hip.avgpool2_bwd with mask=o2 instead of hip.avgpool2_bwd_bits", 138, bits="0", pooled=True),
    # ---------------------------------------------------------------------------------------------------- RoIStageFn
    # pairwise over (CDDMSL_ROI_COMMUTE_DOWN, extra, feat.requires_grad, CDDMSL_POOL_MASK_BITS); every value of every switch meets extra present
    _roi(1, "grad", True, 1, 141),
    _roi(0, "grad", True, 0, 142),
    _roi(1, "nograd", False, 0, 143),
    _roi(0, "nograd", True, 1, 144),
    _roi(0, "none", True, 1, 145),
    _roi(1, "none", True, 0, 146),
    _roi(0, "grad", False, 1, 147),
    # ---------------------------------------------------------------------------------------------------- AttnPoolFn
    _attn("attn_fused_premask", "attn.fused_dx_premask", "AttnPoolFn.forward: `fused_dx and premask_input_grad` (attn_tokens_fwd_mask); backward: hip.attnpool_dx",
          _ATTN_WHY, 151, premask=True),
    _attn("attn_unfused_premask", "attn.unfused_premask", "CDDMSL_ATTNPOOL_DX=0: hip.attn_tokens_bwd with relu_mask = x", _ATTN_WHY, 152, dx="0", premask=True),
    _attn("attn_fused_plain", "attn.fused_dx_plain", "AttnPoolFn.backward: `if mbits is None: mbits = -1` (no mask)", _ATTN_WHY, 153),
    _attn("attn_unfused_plain", "attn.unfused_plain", "CDDMSL_ATTNPOOL_DX=0, `ctx.relu_src` None", _ATTN_WHY, 154, dx="0"),
    _attn("attn_frozen_fused", "attn.frozen_fused", "AttnPoolFn.backward: `train` False: gpos None, no parameter gradient", _ATTN_WHY, 155, frozen=True),
    _attn("attn_frozen_unfused_premask", "attn.frozen_unfused", "`train` False on the hip.attn_tokens_bwd route (gpos None, want_dx)", _ATTN_WHY, 156,
          dx="0", premask=True, frozen=True),
    _attn("attn_train_no_dx", "attn.trainable_no_dx", "AttnPoolFn.backward: `want_dx` False, `if want_dx or train` still produces gpos", _ATTN_WHY, 157,
          x_grad=False),
    _attn("attn_after_stage", "attn.res_stage_attnpool", "layers.res_stage_attnpool: `fuse`: out_grad_premasked stage + premask_input_grad pool",
          _ATTN_WHY + "; the stage in front is one stride-2 block of 128 planes (the issue's 32 give 128 channels) on 3 x 14 x 14 x 32", 158,
          stage=dict(x=(3, 14, 14, 32), planes=128, strides=(2,))),
    # ---------------------------------------------------------------------------------------------------- StackHalvesFn, MeanPoolFn
    _case("stack_halves", "halves", "halves.out_spec", "hip.conv_fwd: `out_spec.full is None` / `out_spec.used == 1`; StackHalvesFn.backward: two views",
          "two res_stage calls on the same block write the halves of one buffer", 161, {"CDDMSL_POOL_MASK_BITS": "1"}, x=(2, 10, 12, 32), planes=16, strides=(2,)),
    _case("mean_pool", "meanpool", "meanpool", "MeanPoolFn", "3 regions of 7 x 7 x 64", 162, x=(3, 7, 7, 64)),
    # ---------------------------------------------------------------------------------------------------- StockStageFn / _blk_backward (resnet.py)
    _stock("stock_s1_shortcut", "stock.stride1_shortcut", "_blk_backward: `if s == 1`, `blk.shortcut is not None`: dsc a dense dgrad, the residual of conv1's",
           "res2's first block: stride 1 with a shortcut convolution, 2 x 9 x 11", 171, x=(2, 9, 11, 32), strides=(1,)),
    _stock("stock_s1_two_blocks", "stock.identity_mask_between", "_blk_backward: `else gs` (identity), `mask = x if mask_x` (StockStageFn.backward: mask_x = i > 0)",
           "blocks (1, 1): the second has the identity and masks its input gradient by its input, the first block's output", 172, strides=(1, 1)),
    _stock("stock_s2_odd", "stock.stride2_odd", "_blk_backward: stride 2: `low = conv_fwd(dpre1, ..., residual=dsc)`, hip.upsample_zero2 with mask=None",
           "9 x 11 -> 5 x 6: (H - 1) // 2 + 1 does not floor; odd rows and columns of dx are exactly zero", 173, x=(2, 9, 11, 32)),
    _stock("stock_s2_even", "stock.stride2_even", "_blk_backward: the same, on a map whose last row and column no output pixel reads",
           "10 x 12 -> 5 x 6: the last row and column (every odd one) of dx are exactly zero, bit for bit", 174),
    _stock("stock_no_dx", "stock.need_dx_false", "_blk_backward: `if not need_dx: return None` (StockStageFn.backward: needs_input_grad[0])",
           "x wants no gradient: the four weight gradients alone, stride 2", 175, x_grad=False),
    _stock("stock_res5_crops", "stock.res5_mean_pool", "Res5ROIHeads.forward: layers.mean_pool(self.res5.forward_nhwc(x)); blocks (2, 1): upsample_zero2 below a masked block",
           "3 crops of 14 x 14 -> 7 x 7 through a stride-2 block and an identity block, then the mean over the map", 176, x=(3, 14, 14, 32),
           strides=(2, 1), pool=True),
]

REQUIRED_BRANCHES = [
    "conv.relu_bias_dx", "conv.residual", "conv.residual_out_f32", "conv.strided_wgrad", "conv.train_w_false", "conv.bf16_of", "conv.sliced_dx",
    "conv.plain_dx_below_8192", "heads.4d_out_f32", "heads.2d_out_compute", "mlp.residual", "stage.pooled_residual", "stage.avgpool2_bwd_fallback",
    "stage.mask_between_blocks", "stage.need_dx_false", "stage.out_grad_premasked", "stage.px_given_match", "stage.px_given_mismatch",
    "stage.pool_mask_bits_off", "roi.on_map1.extra_grad", "roi.on_map0.extra_grad", "roi.on_map1.extra_nograd", "roi.on_map0.extra_nograd",
    "roi.on_map0.extra_none", "roi.on_map1.extra_none", "attn.fused_dx_premask", "attn.unfused_premask", "attn.fused_dx_plain", "attn.unfused_plain",
    "attn.frozen_fused", "attn.frozen_unfused", "attn.trainable_no_dx", "attn.res_stage_attnpool", "halves.out_spec", "meanpool",
    "stock.stride1_shortcut", "stock.identity_mask_between", "stock.stride2_odd", "stock.stride2_even", "stock.need_dx_false", "stock.res5_mean_pool",
]

# the node families of the accumulation contract (two backward passes into the same .grad, f32): one case each
ACCUMULATE = ["conv_1x1_bias_relu", "heads_4d_out_f32", "stage_two_blocks", "roi_commute1_extra_grad_feat_bits1", "attn_fused_premask", "attn_after_stage",
              "stock_s1_two_blocks"]



def _natural(name):
    """the f32-only twin of a gated case: N(0, 0.3^2) FrozenBN biases, ReLU masks that vary from pixel to pixel (tests/graph_ref.py
    ``_make_blocks`` says why bf16 cannot be held on such data)"""
    c = dict(next(c for c in CASES if c["name"] == name))
    c.update(name=name + "_natural", masks="natural", dtypes=("f32",), seed=c["seed"] + 100, why=c["why"] + "; natural masks, f32 only")
    return c


CASES += [_natural(n) for n in ("conv_1x1_bias_relu", "frozen_mlp", "stage_pooled_residual", "stage_pool_fallback_odd", "stage_two_blocks",
                                "stage_premasked", "roi_commute1_extra_grad_feat_bits1", "roi_commute0_extra_grad_feat_bits0", "attn_after_stage",
                                    "stock_s1_two_blocks", "stock_s2_odd")]

BY_NAME = {c["name"]: c for c in CASES}
