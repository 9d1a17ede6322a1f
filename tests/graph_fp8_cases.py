"""Case table of tests/test_gpu_graph_fp8.py and tests/test_graph_fp8_ref_host.py, plain data: the e4m3 routes of ConvFn, ResStageFn,
RoIStageFn and CosineLogitsFn (cddmsl_amd/layers.py), branch by branch, at the smallest shapes at which each branch is still taken.

The forward e4m3 kernel wants Cin a multiple of 128 and Cout of 256, the e4m3 weight gradient both a multiple of 256: blocks have 256
planes on a 512-channel 2 x 10 x 12 map (240 rows).  ENV lowers the three size floors (tiles, reduction length, weight-gradient rows)
so that these shapes reach the kernels; they are set per call through monkeypatch.

A case: ``kind``, ``branch`` (its entry of REQUIRED_BRANCHES), ``selects`` (the condition in layers.py that takes the branch), ``plan``
({conv: (forward, input gradient, weight gradient) on e4m3 operands?} -- what hip.conv_fwd_fp8_ok, hip.conv_wgrad_fp8_ok,
_fp8_wgrad1x1_wanted and _fp8_dgrad_wanted decide under the case's switches), ``rows`` (per pass: launches of k_conv_fwd256_fp8,
k_wgrad256_fp8 and quantize_fp8 in hip.PROFILE; pass 1 calibrates, so no producer emits and every copy costs a quantisation pass;
the first pass also quantises the weights, which the second finds cached), ``gains`` (per block and layer, on the N(0, 1 / fan-in)
weights: the tensors a block quantises then differ in size, and so do their slots' scales)."""

ENV = {"CDDMSL_FP8_MIN_TILES": "1", "CDDMSL_FP8_MIN_K": "128", "CDDMSL_FP8_WGRAD_MIN_M": "1"}

E, P = True, False        # a GEMM on e4m3 operands / on the plain bf16 ones


def _case(name, kind, branch, selects, seed, env=None, **kw):
    return dict(name=name, kind=kind, branch=branch, selects=selects, seed=seed, env=dict(ENV, **(env or {})), **kw)


def _conv(name, branch, selects, seed, x, w, plan, rows, stride=1, pad=0, relu=False, bias=True, out_f32=False, train_w=True, x_grad=True, gain=1.0):
    return _case(name, "conv", branch, selects, seed, x=x, w=w, plan={"c": plan}, rows=rows, stride=stride, pad=pad, relu=relu, bias=bias,
                 residual=False, out_f32=out_f32, train_w=train_w, x_grad=x_grad, gain=gain, refused=not any(plan), deep=False)


# plans of a block: conv1's input gradient is never e4m3; the downsample conv's weight gradient never; a pooled block's conv3
# weight gradient reads p2, whose copy nobody keeps (`o2_8 is not None and not pool`)
_S1 = {"c1": (E, P, E), "c2": (E, E, E), "c3": (E, E, E), "cd": (E, E, P)}
_S2 = {"c1": (E, P, E), "c2": (E, E, E), "c3": (E, E, P), "cd": (E, E, P)}
_NEXT = {"c1": (E, P, E), "c2": (E, E, E), "c3": (E, E, E)}
_OFF = (P, P, P)


def _plan(*blocks):
    return {f"b{i}.{n}": p for i, b in enumerate(blocks) for n, p in b.items()}


# gains (conv1, conv2, conv3, downsample) on fan-in^-1/2.  A slot's scale follows its tensor's maximum, and the tensors of a block
# are chained: x -> o1 -> o2 (-> p2) forward, gs -> dpre2 -> dpre1 backward.  A gain of 1 moves the maximum by 0.8 (conv1), 1.5 (conv2:
# the gated biases add to it) forward and by 1.2 (conv3; 0.4 through a pooling), 0.7 (conv2) backward, so the issue's 0.5 / 1 / 2 leave
# neighbours within a factor of 2 of each other; a quarter per layer (an eighth for conv1 where the pooled px = x / 2 is a slot too)
# puts every tensor at most 0.4 times the one before it.  The downsample conv's 2 keeps the block's output of the size of its input.
_G1 = (0.25, 0.25, 0.25, 2.0)
_G2 = (0.125, 0.25, 0.25, 2.0)


def _stage(name, branch, selects, seed, strides, plan, rows, x_grad=True, bits="1", deep=False):
    return _case(name, "stage", branch, selects, seed, {"CDDMSL_POOL_MASK_BITS": bits}, x=(2, 10, 12, 512), planes=256, strides=strides,
                 plan=plan, rows=rows, x_grad=x_grad, gains=tuple(_G1 if st == 1 else _G2 for st in strides), refused=False, deep=deep)


def _roi(name, commute, extra, seed, rows, strides=(2, 1)):
    b0 = dict(_S2, c1=_OFF, cd=_OFF if commute else (E, E, P))
    two = len(strides) == 2
    return _case(name, "roi", f"roi.on_map{commute}.extra_{extra}" + ("" if two else ".one_block"), "_roi_block0_forward: `fp8_emit_for(...) if E == 0 else None`; RoIStageFn.backward: "
                 "the f8 branches (conv3's and conv2's input gradients, conv2's weight gradient, `dgrad_auto(gs, bp.pw[3], f8, gs_slot)` unless on_map)",
                 seed, {"CDDMSL_ROI_COMMUTE_DOWN": str(commute), "CDDMSL_POOL_MASK_BITS": "1"}, feat=(2, 10, 12, 512), planes=256, strides=strides,
                 rois=(0, 1, 3), extra=extra, feat_grad=True, on_map=bool(commute), plan=_plan(b0, _NEXT) if two else _plan(b0), rows=rows,
                 gains=(_G2, _G1) if two else (_G2,), refused=False, deep=two)


def _cos(name, branch, selects, seed, x, rows, fp8, wn8=False):
    return _case(name, "cosine", branch, selects, seed, x=x, rows=rows, T=0.01, fp8=fp8, wn8=wn8, refused=not fp8, deep=False)


# rows per pass: (k_conv_fwd256_fp8, k_wgrad256_fp8, quantize_fp8), counted from layers.py.  Every pass gets fresh input tensors, as
# a training step does; the weights' copies are made in pass 1 and found cached in pass 2 (no optimizer step in between).
# ConvFn: forward + input gradient = 2 launches of the forward kernel, one weight gradient; pass 1 quantises x, dy, the weights and
# the input-gradient weights, pass 2 x and dy.
# One stride-1 block with a downsample conv -- forward: 4 e4m3 convs; backward: conv3's, conv2's and the downsample conv's input
# gradients = 7 launches of the forward kernel; e4m3 weight gradients: conv2's and conv1's in pass 1, conv3's as well in pass 2
# (plan_for).  Quantisation passes, pass 1: x twice (conv1's slot, the downsample conv's), o1, o2, gs, dpre2, dpre1 = 7 tensors + 4
# forward weights + 3 input-gradient weights = 14; pass 2: conv1 emits o1, conv2 emits o2, conv3's input gradient emits dpre2,
# conv2's emits dpre1: x twice and gs are left = 3.
CASES = [
    # ---------------------------------------------------------------------------------------------------- ConvFn
    _conv("conv8_3x3_relu", "conv.fp8_all", "conv_fwd_auto: `_fp8_eligible`; ConvFn.backward: `f8 = ctx.fp8 and x8 is not None and stride == 1`, "
          "wgrad_auto(min_m=65536) under CDDMSL_FP8_WGRAD_MIN_M, dgrad_auto", 201, (2, 10, 12, 256), (256, 256, 3, 3), (E, E, E),
          ((2, 1, 4), (2, 1, 2)), pad=1, relu=True),
    _conv("conv8_3x3_frozen", "conv.fp8_train_w_false", "ConvFn.backward: `if train_w` False with f8: the input gradient alone", 202,
          (2, 10, 12, 256), (256, 256, 3, 3), (E, E, P), ((2, 0, 4), (2, 0, 2)), pad=1, relu=True, train_w=False),
    _conv("conv8_1x1_out_f32_refused", "conv.fp8_refused_out_f32", "conv_fwd_auto: `not kw.get('out_f32', False)`", 203, (2, 10, 12, 128), (256, 128, 1, 1),
          _OFF, ((0, 0, 0), (0, 0, 0)), out_f32=True),
    _conv("conv8_stride2_refused", "conv.fp8_refused_stride", "conv_fwd_auto: `kw.get('stride', 1) == 1`", 204, (2, 10, 12, 256), (256, 256, 3, 3),
          _OFF, ((0, 0, 0), (0, 0, 0)), stride=2, pad=1, x_grad=False),
    # ---------------------------------------------------------------------------------------------------- ResStageFn
    _stage("stage8_stride1_down", "stage.fp8_stride1", "_block_forward: `e8o2 = ... if save and not pool and _fp8_wgrad1x1_wanted`, fp8_emit_for(bp.pw[1]); "
           "_block_backward: `o2_8 is not None and not pool`, `d1_slot`, the `else` of `if pool` (conv3's input gradient emits dpre2's copy)", 211, (1,),
           _plan(_S1), ((7, 2, 14), (7, 3, 3))),
    # a pooled block: conv3's weight gradient is plain; p2 and px are quantised by passes; avgpool2_bwd emits dpre2's copy in pass 2.
    # pass 1: x, o1, p2, px, gs, dpre2, dpre1 + 4 + 3 weights = 14; pass 2: x, p2, px, gs = 4
    _stage("stage8_stride2_bits1", "stage.fp8_stride2_bits1", "_pool_bits_wanted: `not (bp.fp8 and _fp8_dgrad_wanted(bp.pw[1], ...))` -- with conv2's e4m3 "
           "input gradient wanted the block keeps o2 whole even at CDDMSL_POOL_MASK_BITS=1, and hip.avgpool2_bwd writes dpre2's copy", 212, (2,),
           _plan(_S2), ((7, 2, 14), (7, 2, 4))),
    _stage("stage8_stride2_bits0", "stage.fp8_stride2_bits0", "_block_backward: `hip.avgpool2_bwd(dp2, o2_shape, mask=o2, emit8=d2_slot.emit() ...)`", 213, (2,),
           _plan(_S2), ((7, 2, 14), (7, 2, 4)), bits="0"),
    # two blocks: 4 + 3 forward, 3 + 2 input gradients = 12; 2 + 2 weight gradients in pass 1, 3 + 3 in pass 2; pass 1: block 0's 7
    # tensors + block 1's x, o1, o2, gs, dpre2, dpre1 = 13 + 7 + 5 weights = 25; pass 2: block 0's x twice, block 1's gs (the stage's
    # incoming gradient) and block 0's gs = 4: block 1's last launch is a bf16 one below hip.conv_emit8_ok's 160 tiles, so it cannot
    # carry block 0's gs copy at this size (tests/test_gpu_graph_fp8.py reaches that producer in a case of its own)
    _stage("stage8_two_blocks", "stage.fp8_prev_next", "_block_forward: fp8_emit_for(next_pw, ...) (block 0's conv3 writes block 1's input copy); _block_backward: "
           "`prev_bp is not None ...` is taken, but dgrad_auto drops the emit8 below hip.conv_emit8_ok's 160 tiles: block 0's gs is quantised by a "
           "pass here, and test_last_launch_of_a_block_writes_the_previous_blocks_gs_copy reaches the emission on a larger map", 214, (1, 1), _plan(_S1, _NEXT), ((12, 4, 25), (12, 6, 4)), deep=True),
    # no input gradient: the downsample conv's is not computed: 6 launches of the forward kernel, one weight copy less
    _stage("stage8_no_dx", "stage.fp8_x_grad_false", "_block_backward: `if not need_dx: return None`", 215, (1,), _plan(_S1), ((6, 2, 13), (6, 3, 3)),
           x_grad=False),
    # ---------------------------------------------------------------------------------------------------- RoIStageFn
    # block 0 (stride 2, conv1 on the map in bf16): forward conv2, conv3 (+ the downsample conv on the crops) ; backward conv3's and
    # conv2's input gradients (+ the downsample conv's); weight gradient conv2's.  Block 1: 3 + 2 and 3.
    # commute 0: 3 + 3 forward, 2 + 3 backward = 11 launches of the forward kernel; weight gradients 2 + 1 in pass 1, 3 + 1 in pass 2;
    #            pass 1: o1, p2, px, gs, dpre2 + block 1's 6 = 11 tensors + 6 + 5 weights = 22; pass 2: RoIAlign emits o1, avgpool2_bwd
    #            dpre2, block 1's tensors are emitted except its gs: p2, px and the two gs = 4
    # commute 1: the downsample conv runs on the map in bf16: 2 launches, one tensor (px) and 2 weight copies less
    _roi("roi8_commute0", 0, "none", 221, ((11, 3, 22), (11, 4, 4))),
    _roi("roi8_commute1", 1, "none", 222, ((9, 3, 19), (9, 4, 3))),
    # appended rows are copied into o1 AFTER RoIAlign wrote it: no copy may be emitted there, conv2 quantises o1 itself
    _roi("roi8_commute0_extra", 0, "grad", 223, ((11, 3, 22), (11, 4, 5))),
    # the first block alone, a chain short enough for the issue's cap: RoIStageFn's own f8 branches held to the model.  commute 0: forward
    # conv2, the downsample conv, conv3; backward conv3's, conv2's and the downsample conv's input gradients = 6; conv2's weight gradient;
    # pass 1: o1, px, p2, gs, dpre2 + 3 + 3 weights = 11; pass 2: px, p2, gs = 3 (+ o1 with appended rows).  commute 1: 4 launches; o1, p2,
    # gs, dpre2 + 2 + 2 = 8, then p2 and gs
    _roi("roi8_one_block_commute0", 0, "none", 224, ((6, 1, 11), (6, 1, 3)), strides=(2,)),
    _roi("roi8_one_block_commute1", 1, "none", 225, ((4, 1, 8), (4, 1, 2)), strides=(2,)),
    _roi("roi8_one_block_commute0_extra", 0, "grad", 226, ((6, 1, 11), (6, 1, 4)), strides=(2,)),
    # ---------------------------------------------------------------------------------------------------- CosineLogitsFn
    _cos("cos8_20_rows", "cosine.fp8", "CosineLogitsFn.forward: `fp8 and x.shape[1] % 64 == 0 and wn.shape[0] <= 32`", 231, (40, 1024), 20, True),
    _cos("cos8_33_rows_refused", "cosine.refused_rows", "the same condition, False for 33 rows", 232, (40, 1024), 33, False),
    _cos("cos8_width_1000_refused", "cosine.refused_width", "the same condition, False for a width of 1000", 233, (40, 1000), 20, False),
    _cos("cos8_given_wn8", "cosine.given_wn8", "CosineLogitsFn.forward: `if wn8 is None` False", 234, (40, 1024), 20, True, wn8=True),
]

BY_NAME = {c["name"]: c for c in CASES}


def plan_for(case, calibrating):
    """the plan of pass 1 (``calibrating``) or pass 2.  Pass 1: conv3's slot has no scale of its own when conv2 runs, so conv2 writes
    no copy of o2 under it (`fp8_act_slot(bp.pw[2]).emit()` is None -> `o2_8` None) and conv3's weight gradient takes the plain kernel."""
    plan = case.get("plan", {})
    if not calibrating:
        return plan
    return {n: (p[0], p[1], p[2] and not n.endswith("c3")) for n, p in plan.items()}

REQUIRED_BRANCHES = [
    "conv.fp8_all", "conv.fp8_train_w_false", "conv.fp8_refused_out_f32", "conv.fp8_refused_stride",
    "stage.fp8_stride1", "stage.fp8_stride2_bits1", "stage.fp8_stride2_bits0", "stage.fp8_prev_next", "stage.fp8_x_grad_false",
    "roi.on_map0.extra_none", "roi.on_map1.extra_none", "roi.on_map0.extra_grad",
    "roi.on_map0.extra_none.one_block", "roi.on_map1.extra_none.one_block", "roi.on_map0.extra_grad.one_block",
    "cosine.fp8", "cosine.refused_rows", "cosine.refused_width", "cosine.given_wn8",
]
