"""GPU: the e4m3 routes of ConvFn, ResStageFn, RoIStageFn and CosineLogitsFn (cddmsl_amd/layers.py, ``--dtype fp8``), case by case
(tests/graph_fp8_cases.py), in bf16 with ``fp8`` on, on a fresh layers.Fp8Scales(), three passes each with FP8_SCALES.roll() and fresh
gradients in between: pass 1 calibrates the slots (no producer writes a copy); pass 2 is where producers write the e4m3 copies, on a
halved input and a halved gradient (graph_fp8_ref.pass_inputs) but, scaling being delayed, still under the scales of pass 1; pass 3
repeats it under the scales of pass 2's maxima, about twice those of pass 2 for the node's input and every gradient.

(a) the whole node against the quantisation-aware float64 model (tests/graph_fp8_ref.py) evaluated on that pass's inputs under the
    scales the product's slots held in that pass; metric max |got - ref| / max |ref| per tensor, limit max(4 x the error of the
    model's own round_bf16 run under the same scales, 2^-8): nothing of the limit comes from the product.  Every slot's scale is also
    within 2^-6 of 448 / max|the model's own tensor| of the pass whose maxima it was rolled from.  EVERY case is asserted; what the
    four ``deep`` cases' inputs are held to on the host is said in tests/test_graph_fp8_ref_host.py.
(b) link audit, every case: hip.quantize_fp8, hip.conv_fwd_fp8, hip.conv_wgrad_fp8, hip.fp8_dot_nt and the three emitters are
    wrapped; for every e4m3 GEMM launched each operand is a copy made once, in this pass (weights: since the last optimizer step),
    under the scale that the epilogue's factor inverts; the epilogue vector is deq_A * deq_B * bn_scale to 4 f32 ulps; the bytes of a
    quantisation pass are e4m3_encode(src * scale) exactly, those of an emitting epilogue at most one code from it (it converts the
    unrounded f32 value); no source tensor was written after its copy was made; the two operands' scales differ.
(c) routes from hip.PROFILE per pass: the counts of k_conv_fwd256_fp8, k_wgrad256_fp8 and quantize_fp8 the case table derives from
    layers.py; none at all for the refused cases, whose results are torch.equal to the ``fp8=False`` run.
(d) a raw-pointer optimizer step + layers.bump_weight_version() re-makes the e4m3 copies of the forward and the input-gradient
    weights from the new values; a frozen PreparedWeight keeps its copy.
(e) an Inf in the input raises the installed table's ``nonfinite`` flag and the slot keeps its scale through roll().
Two audit-only runs reach the bf16 producers, which need 160 tiles: a bf16 convolution writing its consumer's copy, and the last
launch of a block writing the previous block's gs copy.

Worst error / limit per case and the tensor it occurred on, measured on one MI355X (pass 1 | pass 2 | pass 3; test_worst_ratio_table
prints them; the limits are the model's, none was set from these figures).  A ratio of 0.250 is the final bf16 rounding of the
output, which the model's round_bf16 run makes at the same element:
  conv8_3x3_relu                 0.250 | 0.250 | 0.250 (y, dx)      stage8_two_blocks (deep)        0.250 | 0.257 | 0.271 (b0.w3, b0.w0)
  conv8_3x3_frozen               0.250 | 0.250 | 0.250 (dx)         roi8_commute0 (deep)            0.263 | 0.263 | 0.257 (b0.w3, b0.w1)
  conv8_1x1_out_f32_refused      0.250 | 0.250 | 0.250 (dx)         roi8_commute1 (deep)            0.755 | 0.670 | 0.736 (b0.w2: 1.2e-02 of 1.6e-02)
  conv8_stride2_refused          0.125 | 0.128 | 0.128 (y)          roi8_commute0_extra (deep)      0.281 | 0.268 | 0.259 (b0.w2, b0.w0)
  stage8_stride1_down            0.252 | 0.250 | 0.279 (b0.w1, y)   roi8_one_block_commute0         0.289 | 0.289 | 0.289 (dfeat)
  stage8_stride2_bits1           0.261 | 0.253 | 0.250 (b0.w2)      roi8_one_block_commute1         0.263 | 0.256 | 0.256 (b0.w1, dfeat)
  stage8_stride2_bits0           0.295 | 0.260 | 0.291 (y, b0.w0)   roi8_one_block_commute0_extra   0.383 | 0.383 | 0.383 (dfeat)
  stage8_no_dx                   0.290 | 0.250 | 0.250 (b0.w0, y)   cosine head, four cases         <= 0.005 (y)"""
import pytest
import torch

import exact_fp8 as X8
import graph_fp8_cases as GC
import graph_fp8_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
F64 = torch.float64
ROWS = ("k_conv_fwd256_fp8", "k_wgrad256_fp8", "quantize_fp8")
ULP4 = 4 * 2.0 ** -23


def _param(t):
    p = t.to(DEV)
    if p.dim() == 4:
        p = p.contiguous(memory_format=torch.channels_last)
    return torch.nn.Parameter(p, requires_grad=True)


# ---------------------------------------------------------------------------------------------------------------- the audit
class Audit:
    """records every e4m3 copy (buffer, source tensor and its version, a device-side clone of the scale, pass or emitter, pass number)
    and every e4m3 GEMM (operand buffers, epilogue vector, what identifies its convolution); everything recorded is kept alive, so
    an address names one buffer for the whole case"""

    EMITTERS = ("conv_fwd", "avgpool2_bwd", "roi_align_forward_affine")

    def __init__(self, mp):
        from cddmsl_amd import hip
        self.copies, self.gemms, self.by_ptr, self.pass_no, self.step, self.temperature = [], [], {}, 0, 0, None
        orig = {n: getattr(hip, n) for n in ("quantize_fp8", "conv_fwd_fp8", "conv_wgrad_fp8", "fp8_dot_nt") + self.EMITTERS}

        def quantize_fp8(x, scale=None, amax=None):
            y = orig["quantize_fp8"](x, scale, amax)
            self._copy(y, x, scale, "pass")
            return y

        def emitter(name):
            def f(*a, **kw):
                y = orig[name](*a, **kw)
                if kw.get("emit8") is not None:
                    assert getattr(y, "_fp8", None) is not None and y._fp8[1] == kw["emit8"][0].data_ptr(), (name, "emit8 given, no copy attached")
                    self._copy(y._fp8[0], y, kw["emit8"][0], "emit:" + name)
                return y
            return f

        def conv_fwd_fp8(x8, w8, scale=None, bias=None, residual=None, relu=False, relu_mask=None, pad=0, out_f32=False, emit8=None):
            y = orig["conv_fwd_fp8"](x8, w8, scale, bias, residual, relu, relu_mask, pad, out_f32, emit8)
            self.gemms.append(dict(kind="conv", a=x8, b=w8, eff=scale.clone(), out=None, pass_no=self.pass_no))
            if emit8 is not None:
                assert getattr(y, "_fp8", None) is not None and y._fp8[1] == emit8[0].data_ptr()
                self._copy(y._fp8[0], y, emit8[0], "emit:conv_fwd_fp8")
            return y

        def conv_wgrad_fp8(x8, dy8, w_shape, scale, pad=0, out=None):
            r = orig["conv_wgrad_fp8"](x8, dy8, w_shape, scale, pad, out)
            self.gemms.append(dict(kind="wgrad", a=x8, b=dy8, eff=scale.clone(), out=r.data_ptr(), pass_no=self.pass_no))
            return r

        def fp8_dot_nt(a8, b8, alpha=None):
            self.gemms.append(dict(kind="dot", a=a8, b=b8, eff=alpha.clone(), out=None, pass_no=self.pass_no))
            return orig["fp8_dot_nt"](a8, b8, alpha)
        mp.setattr(hip, "quantize_fp8", quantize_fp8)
        mp.setattr(hip, "conv_fwd_fp8", conv_fwd_fp8)
        mp.setattr(hip, "conv_wgrad_fp8", conv_wgrad_fp8)
        mp.setattr(hip, "fp8_dot_nt", fp8_dot_nt)
        for n in self.EMITTERS:
            mp.setattr(hip, n, emitter(n))

    def _copy(self, buf, src, scale, how):
        rec = dict(buf=buf, src=src, version=src._version, scale=scale.detach().clone(), scale_ptr=scale.data_ptr(), how=how,
                   pass_no=self.pass_no, step=self.step, checked=False)
        assert buf.data_ptr() not in self.by_ptr, "an e4m3 buffer was written twice"
        self.copies.append(rec)
        self.by_ptr[buf.data_ptr()] = rec

    def check_pass(self, weights, bn_of_param, wd_ptrs, grad_ptrs, frozen=()):
        """every GEMM of the current pass against its operands' records.  ``weights``: addresses of tensors whose copies live from
        one optimizer step to the next (parameters, prepared input-gradient weights, the unit-norm text rows); ``bn_of_param``:
        {parameter address: FrozenBN scale or None}; ``wd_ptrs``: addresses of prepared input-gradient weights; ``grad_ptrs``:
        {address of a parameter's gradient buffer: the parameter's address}; ``frozen``: addresses among ``weights`` whose copies are
        made once and kept (a frozen PreparedWeight)."""
        made = [c for c in self.copies if not c["checked"]]
        keys = [(c["src"].data_ptr(), tuple(c["src"].shape), c["scale_ptr"], c["src"].dtype, c["pass_no"]) for c in made]
        assert len(set(keys)) == len(keys), "a tensor was quantised twice under one slot in one pass"
        for c in made:                                   # the bytes, while the sources still hold what was quantised
            assert c["src"]._version == c["version"], (c["how"], "the source was written after its copy was made")
            want = R.codes(c["src"].detach().to(F64), float(c["scale"]))
            if c["how"] == "pass":
                assert X8.same_codes(c["buf"], want) == 0, (c["how"], tuple(c["src"].shape), X8.same_codes(c["buf"], want))
            else:
                g, w = c["buf"].reshape(-1).to(torch.int16), want.reshape(-1).to(torch.int16)
                zero = ((g & 0x7F) == 0) & ((w & 0x7F) == 0)
                ok = zero | (((g & 0x80) == (w & 0x80)) & (((g & 0x7F) - (w & 0x7F)).abs() <= 1)) | (((g & 0x7F) + (w & 0x7F)) <= 1)
                assert bool(ok.all()), (c["how"], tuple(c["src"].shape), int((~ok).sum()))
            c["checked"] = True
        n = 0
        for gm in (g for g in self.gemms if g["pass_no"] == self.pass_no):
            ra, rb = self.by_ptr.get(gm["a"].data_ptr()), self.by_ptr.get(gm["b"].data_ptr())
            assert ra is not None and rb is not None, (gm["kind"], "an operand that no audited launch produced")
            for r in (ra, rb):
                is_w = r["src"].data_ptr() in weights
                assert r["checked"] and r["src"]._version == r["version"], (gm["kind"], r["how"], "stale source")
                fresh = (r["step"] == self.step or r["src"].data_ptr() in frozen) if is_w else r["pass_no"] == self.pass_no
                assert fresh, (gm["kind"], r["how"], r["pass_no"], self.pass_no, r["step"], self.step, is_w)
            sa, sb = float(ra["scale"]), float(rb["scale"])
            # (the cosine head's two operands are both at the fixed scale 448: nothing to tell apart)
            assert sa != sb or gm["kind"] == "dot", (gm["kind"], sa, "the two operands' scales are equal: the factor check could not tell them apart")
            if gm["kind"] == "conv":
                wp = rb["src"].data_ptr()
                assert wp in bn_of_param or wp in wd_ptrs, "the second operand of a forward-kernel launch is no weight copy"
                bn = bn_of_param.get(wp)                  # (an input-gradient convolution: the FrozenBN scale is in its prepared weights)
            elif gm["kind"] == "wgrad":
                assert gm["out"] in grad_ptrs, "an e4m3 weight gradient was not written into a parameter's gradient"
                bn = bn_of_param[grad_ptrs[gm["out"]]]
            else:
                bn = None
            want = torch.full_like(gm["eff"], 1.0, dtype=F64) / sa / sb * (1.0 if bn is None else bn.to(F64))
            if gm["kind"] == "dot":
                want = want / self.temperature
            err = float(((gm["eff"].to(F64) - want).abs() / want.abs()).max())
            assert err <= ULP4, (gm["kind"], err, sa, sb)
            n += 1
        return n


# ---------------------------------------------------------------------------------------------------------------- running a case
class Node:
    """a case's parameters, built once; ``run`` makes one forward + backward pass on fresh input tensors"""

    def __init__(self, case, inp, fp8=True):
        from cddmsl_amd import layers
        self.case, self.inp, self.fp8, k = case, inp, fp8, case["kind"]
        self.params, self.bn_of_param, self.slots, self.pws, self.keep, self.kept = {}, {}, {}, [], False, {}
        if k == "conv":
            self.w = _param(inp["w"])
            self.b = _param(inp["b"]) if case["bias"] else None
            self.pw = layers.PreparedWeight(self.w, None, not case["train_w"])
            self.pws = [self.pw]
            self.bn_of_param[self.w.data_ptr()] = None
            if case["train_w"]:
                self.params.update({"w": self.w}, **({"b": self.b} if self.b is not None else {}))
        elif k in ("stage", "roi"):
            self.blocks = []
            for bi, b in enumerate(inp["blocks"]):
                w = [None if v is None else _param(v) for v in b["w"]]
                bn = [None if v is None else (v[0].to(DEV).contiguous(), v[1].to(DEV).contiguous()) for v in b["bn"]]
                bp = layers.BlockParams(*w, *bn, b["stride"], False, fp8=fp8)
                self.blocks.append(bp)
                for wi, v in enumerate(w):
                    if v is not None:
                        self.params[f"b{bi}.w{wi}"] = v
                        self.bn_of_param[v.data_ptr()] = bn[wi][0]
                        self.pws.append(bp.pw[wi])
        elif k == "cosine":
            self.wn = inp["wn"].to(DEV)
            self.wn8 = layers.fp8_unit_rows(self.wn) if case["wn8"] else None

    def slot_scales(self):
        """{model slot name: the scale the product's slot holds now}"""
        out = {}

        def put(name, owner, attr):
            sl = getattr(owner, attr, None)
            if sl is not None:
                out[name] = float(sl.scale)
        if self.case["kind"] == "conv":
            put("act", self.pw, "_fp8_slot")
            put("g", self.pw, "_fp8_g")
        elif self.case["kind"] in ("stage", "roi"):
            for bi, bp in enumerate(self.blocks):
                for j, n in enumerate(("c1", "c2", "c3", "cd")):
                    if bp.pw[j] is not None:
                        put(f"b{bi}.{n}.act", bp.pw[j], "_fp8_slot")
                put(f"b{bi}.gs", bp, "_fp8_gs")
                put(f"b{bi}.c2.g", bp.pw[1], "_fp8_g")
                put(f"b{bi}.c1.g", bp.pw[0], "_fp8_g")
        return out

    def run(self, poison=False, inp=None):
        """-> ({name: tensor} over graph_fp8_ref.compared, profiler rows); ``inp``: this pass's inputs (graph_fp8_ref.pass_inputs)"""
        from cddmsl_amd import hip, layers
        case, inp, k = self.case, (self.inp if inp is None else inp), self.case["kind"]
        def data(n, grad, dtype=BF):
            # fresh tensors every pass, as a training step has them (``keep``: the SAME tensor objects again, for the audit's control)
            if not (self.keep and n in self.kept):
                self.kept[n] = inp[n].to(DEV, dtype).requires_grad_(bool(grad))
            self.kept[n].grad = None
            return self.kept[n]
        for p in self.params.values():
            p.grad = None
        layers.take_touched()
        leaves = {}
        hip.PROFILE.enable()
        try:
            if k == "conv":
                leaves["dx"] = x = data("x", case["x_grad"])
                if poison:
                    with torch.no_grad():
                        x.view(-1)[5] = float("inf")
                y = layers.conv(x, self.pw, self.b, case["stride"], case["pad"], case["relu"], case["out_f32"], case["train_w"], None, self.fp8)
            elif k == "stage":
                leaves["dx"] = data("x", case["x_grad"])
                y = layers.res_stage(leaves["dx"], self.blocks, False)
            elif k == "roi":
                leaves["dfeat"] = data("feat", case["feat_grad"])
                if "extra" in inp:
                    leaves["dextra"] = data("extra", case["extra"] == "grad")
                rois = inp["rois"].to(DEV)
                roi_start = torch.tensor([0, 0, rois.shape[0]], device=DEV, dtype=torch.int32)
                y = layers.roi_stage(leaves["dfeat"], rois, roi_start, self.blocks, False, 14, 1.0 / 16, 0, leaves.get("dextra"))
                assert y.grad_fn.meta[4] == case["on_map"]
            else:
                leaves["dx"] = data("x", True, torch.float32)
                y = layers.cosine_logits(leaves["dx"], self.wn, case["T"], case["fp8"] and self.fp8, self.wn8)
            y.backward(inp["gy"].to(DEV, y.dtype))
            rows = [e[0] for e in hip.PROFILE.events]
            hip.PROFILE.collect()
        finally:
            hip.PROFILE.on = False
        torch.cuda.synchronize()
        out = {"y": y.detach()}
        for n in R.compared(case)[1:]:
            t = leaves[n] if n in leaves else self.params[n]
            assert t.grad is not None, (case["name"], n, "received no gradient")
            out[n] = t.grad.detach().clone()
        return out, tuple(rows.count(r) for r in ROWS)

    def audit_args(self):
        weights = {p.data_ptr() for p in self.bn_of_param_tensors()} | {pw._wd.data_ptr() for pw in self.pws if pw._wd is not None}
        if self.case["kind"] == "cosine":
            weights.add(self.wn.data_ptr())
        wd_ptrs = {pw._wd.data_ptr() for pw in self.pws if pw._wd is not None}
        grad_ptrs = {p.grad.data_ptr(): p.data_ptr() for p in self.params.values() if p.grad is not None}
        return weights, self.bn_of_param, wd_ptrs, grad_ptrs

    def bn_of_param_tensors(self):
        return [pw.param for pw in self.pws]

    def frozen_ptrs(self):
        return {t.data_ptr() for pw in self.pws if pw.frozen for t in (pw.param, pw._wd) if t is not None}


class fresh_scales:
    """a new layers.Fp8Scales() installed for the case, the old one restored afterwards"""

    def __enter__(self):
        from cddmsl_amd import layers
        self.old, layers.FP8_SCALES = layers.FP8_SCALES, layers.Fp8Scales()
        return layers.FP8_SCALES

    def __exit__(self, *a):
        from cddmsl_amd import layers
        layers.FP8_SCALES = self.old


def _bias_only_max(case, inp, slot):
    """the largest value relu(bias) of the convolution whose epilogue writes ``slot``'s copy in pass 2 (0 where none does): conv1's bias
    for conv2's input, conv2's for conv3's in a stride-1 block, the previous block's conv3's for conv1's; RoIAlign and the pooling
    passes have no padded rows, an input-gradient convolution no bias"""
    if case["kind"] not in ("stage", "roi") or not slot.endswith(".act"):
        return 0.0
    bi, conv = int(slot[1]), slot.split(".")[1]
    blocks = inp["blocks"]
    if conv == "c2" and not (case["kind"] == "roi" and bi == 0):
        b = blocks[bi]["bn"][0][1]
    elif conv == "c3" and blocks[bi]["stride"] == 1:
        b = blocks[bi]["bn"][1][1]
    elif conv == "c1" and bi > 0:
        b = blocks[bi - 1]["bn"][2][1]
    else:
        return 0.0
    return float(b.clamp_min(0).max())


_results = {}


def _evaluate(name):
    """one case, run once: three passes with the audit on -> per pass (rows of (tensor, error, limit), profiler counts, GEMMs audited)"""
    if isinstance(_results.get(name), Exception):
        raise RuntimeError(f"{name} failed before: {_results[name]!r}")            # (never run a failed case a second time)
    if name in _results:
        return _results[name]
    from cddmsl_amd import layers
    case = GC.BY_NAME[name]
    inp, _, sc0, _ = R.prepared(case)
    try:
        with pytest.MonkeyPatch.context() as mp, fresh_scales() as table:
            for key, v in case["env"].items():
                mp.setenv(key, v)
            audit = Audit(mp)
            audit.temperature = case.get("T")
            node = Node(case, inp)
            passes, own, own_r = [], None, None
            for pass_no in (1, 2, 3):
                audit.pass_no = pass_no
                inp_p = R.pass_inputs(inp, pass_no)
                before = node.slot_scales()
                got, counts = node.run(inp=inp_p)
                held = before if pass_no > 1 else node.slot_scales()         # (pass 1 calibrates inside the pass)
                audited = audit.check_pass(*node.audit_args())
                rows = []
                if case["kind"] != "cosine" and not case["refused"]:
                    assert set(sc0.used) <= set(held), (name, "slots the model names that the product never made", set(sc0.used) - set(held))
                    assert pass_no == 1 or held == node.slot_scales(), "a slot's scale changed inside a pass"
                given = {n: held[n] for n in sc0.used}
                ref, sc, lim = R.limits(case, inp_p, given, calibrating=pass_no == 1)
                # delayed scaling: a pass runs under 448 / the maxima of the pass before it (pass 1: its own, calibrated); every case,
                # every slot, against the model's own tensors
                # 2^-6 in the two passes the scheme needs (a maximum moves by a few bf16 roundings).  Pass 3 runs under maxima that
                # PRODUCERS recorded in pass 2: as far as the model's own rounded run moves a maximum, times 4, floor 2^-6 -- and from
                # above an emitting convolution may record more than its tensor holds: the rows of its last 256-row tile past M carry
                # the bias alone (csrc/conv_fwd256.hip: "an over-estimate at worst"), and 240 or 588 rows leave such rows.  Measured:
                # stage8_two_blocks b0.c3.act, recorded 0.56640625 = the largest relu(bias), the tensor's maximum 0.5547: a scale 2.1 %
                # smaller than the model's
                own, own_r = (sc.own, sc.own_rounded) if own is None else (own, own_r)
                for n, s in sc.used.items():
                    tol = 2.0 ** -6 if pass_no < 3 else max(2.0 ** -6, R.BF16_FACTOR * abs(own_r[n] / own[n] - 1.0))
                    top = max(448.0 / own[n], _bias_only_max(case, inp, n) if pass_no == 3 else 0.0)
                    assert (448.0 / own[n]) * (1.0 - tol) <= 448.0 / s <= top * (1.0 + tol), (name, pass_no, n, s, own[n], tol, top)
                if pass_no == 3:
                    # (the node's own input and every gradient halved: their slots' scales about doubled; an inner activation is
                    # mostly its bias and may keep its scale to the bit)
                    moved = [n for n in sc.used if not n.endswith(".act") or n in ("b0.c1.act", "b0.cd.act")]
                    assert all(1.5 <= held[n] / passes[1][4][n] <= 3.0 for n in moved), "a slot kept its scale although its tensor halved"
                own, own_r = sc.own, sc.own_rounded
                for n, r in ref.items():
                    assert bool(torch.isfinite(got[n].float()).all()), (name, pass_no, n)
                    rows.append((n, R.rel_err(got[n], r), lim[n]))
                passes.append((rows, counts, audited, got, held))
                table.roll()
            assert table.nonfinite is None or not bool(table.nonfinite.item())
            if case["refused"]:
                plain, _ = Node(case, inp, fp8=False).run(inp=R.pass_inputs(inp, 3))
                for n, v in plain.items():
                    assert torch.equal(v, passes[2][3][n]), (name, n, "a refused case differs from the fp8=False run")
    except Exception as e:
        _results[name] = e
        raise
    _results[name] = passes
    return passes


NAMES = [c["name"] for c in GC.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_node_against_quantised_model_and_link_audit(name):
    case = GC.BY_NAME[name]
    passes = _evaluate(name)
    bad = []
    for i, (rows, counts, audited, _, _) in enumerate(passes, start=1):
        for n, err, limit in rows:
            print(f"{name} pass {i} {n}: error {err:.3e} limit {limit:.3e} ratio {err / limit:.3f}")
            if not err <= limit:
                bad.append((i, n, err, limit))
        print(f"{name} pass {i}: launches {dict(zip(ROWS, counts))}, {audited} e4m3 GEMMs audited")
    assert not bad, bad


@pytest.mark.parametrize("name", NAMES)
def test_routes(name):
    """the profiler's rows per pass are exactly the ones the case table derives from layers.py (pass 3 repeats pass 2: which tensors a
    producer writes and which a quantisation pass is in those counts); a refused case launches nothing in e4m3"""
    case = GC.BY_NAME[name]
    passes = _evaluate(name)
    counts = [p[1] for p in passes]
    if case["kind"] == "cosine":
        want = (0, 0, 0 if case["refused"] else (1 if case["wn8"] else 2))
        assert counts == [want] * 3, counts
        assert [p[2] for p in passes] == [0 if case["refused"] else 1] * 3
        return
    assert counts == [tuple(r) for r in case["rows"]] + [tuple(case["rows"][1])], (counts, case["rows"])
    assert [p[2] for p in passes] == [c[0] + c[1] for c in counts]               # every e4m3 GEMM went through the audit


@pytest.mark.parametrize("name", ["conv8_3x3_relu", "conv8_3x3_frozen", "stage8_stride1_down"])
def test_weight_copies_follow_a_raw_pointer_step(name):
    """(d): after pass 2 the trainable weights move through hip.sgd_clip_step (raw pointers: no tensor version changes) and
    layers.bump_weight_version(); pass 3 must read e4m3 copies of the forward AND of the input-gradient weights made in pass 3 from
    the NEW values (the audit compares the bytes with the sources as they are after the pass); a frozen PreparedWeight keeps its copy"""
    from cddmsl_amd import hip, layers
    case = GC.BY_NAME[name]
    inp = R.prepared(case)[0]
    with pytest.MonkeyPatch.context() as mp, fresh_scales() as table:
        for key, v in case["env"].items():
            mp.setenv(key, v)
        audit = Audit(mp)
        node = Node(case, inp)
        for pass_no in (1, 2):
            audit.pass_no = pass_no
            node.run()
            audit.check_pass(*node.audit_args())
            table.roll()
        ws = [p for n, p in node.params.items() if p.dim() == 4]
        old = [p.detach().clone() for p in ws]
        if ws:
            lr = 0.25 * min(float(p.detach().abs().max() / p.grad.abs().max()) for p in ws)
            hip.sgd_clip_step([p.data for p in ws], [p.grad for p in ws], [torch.zeros_like(p) for p in ws],
                              torch.zeros(len(ws), device=DEV), lr, 0.0, 0.0, 1e30, True)
            torch.cuda.synchronize()
            assert all(not torch.equal(o, p.detach()) for o, p in zip(old, ws))
        layers.bump_weight_version()
        audit.step, audit.pass_no = 1, 3
        node.run()
        n = audit.check_pass(*node.audit_args(), frozen=node.frozen_ptrs())
        assert n > 0
        made3 = [c for c in audit.copies if c["pass_no"] == 3]
        w_ptrs = {p.data_ptr() for p in ws}
        wd_ptrs = {pw._wd.data_ptr() for pw in node.pws if pw._wd is not None}
        fwd3 = {c["src"].data_ptr() for c in made3 if c["src"].data_ptr() in w_ptrs}
        wd3 = {c["src"].data_ptr() for c in made3 if c["src"].data_ptr() in wd_ptrs}
        plan = case["plan"]
        if case["kind"] == "conv" and not case["train_w"]:
            assert not fwd3 and not wd3, "a frozen weight's e4m3 copies were made again"
            used = {audit.by_ptr[g["b"].data_ptr()]["pass_no"] for g in audit.gemms if g["pass_no"] == 3 and g["kind"] == "conv"}
            assert used == {1}, used
        else:
            want_f = sum(1 for p in plan.values() if p[0])
            want_d = sum(1 for p in plan.values() if p[1])
            assert len(fwd3) == want_f and len(wd3) == want_d, (len(fwd3), want_f, len(wd3), want_d)
            for c in made3:
                if c["src"].data_ptr() in w_ptrs:       # the bytes are those of the new values, not of the old ones
                    i = [p.data_ptr() for p in ws].index(c["src"].data_ptr())
                    assert X8.same_codes(c["buf"], R.codes(old[i].permute(0, 2, 3, 1).to(F64), float(c["scale"]))) > 0


def test_audit_sees_a_copy_that_outlives_its_pass():
    """control of (b): the same input TENSOR OBJECT fed to two passes keeps the copy attached to it in pass 1 (``t._fp8``, made under
    the slot's pass-1 scale; fp8_copy compares the slot, not the step), and pass 2's convolution reads it: the audit must refuse that
    GEMM.  A training step makes its activations anew, so the product never meets this; the audit has to."""
    case = GC.BY_NAME["conv8_3x3_relu"]
    inp = R.prepared(case)[0]
    with pytest.MonkeyPatch.context() as mp, fresh_scales() as table:
        for key, v in case["env"].items():
            mp.setenv(key, v)
        audit = Audit(mp)
        node = Node(case, inp)
        node.keep = True
        audit.pass_no = 1
        node.run()
        assert audit.check_pass(*node.audit_args()) == 3
        table.roll()
        audit.pass_no = 2
        _, counts = node.run()
        assert counts == (2, 1, 1), counts                # (x was not quantised again)
        with pytest.raises(AssertionError, match="conv"):
            audit.check_pass(*node.audit_args())


def test_non_finite_input_raises_the_flag_and_keeps_the_scale():
    """(e): the graph-level counterpart of test_fp8_quantisation_records_non_finite_inputs: an Inf in ConvFn's input in pass 2"""
    case = GC.BY_NAME["conv8_3x3_relu"]
    inp = R.prepared(case)[0]
    with pytest.MonkeyPatch.context() as mp, fresh_scales() as table:
        for key, v in case["env"].items():
            mp.setenv(key, v)
        node = Node(case, inp)
        node.run()
        table.roll()
        assert table.nonfinite is None or not bool(table.nonfinite.item())
        before = node.slot_scales()
        node.run(poison=True)
        table.roll()
        assert table.nonfinite is not None and bool(table.nonfinite.item())
        after = node.slot_scales()
        assert after["act"] == before["act"] and after["act"] != 1.0


def test_bf16_producer_writes_its_consumers_copy(monkeypatch):
    """audit only: hip.conv_emit8_ok has a 160-tile floor, which no stage case reaches: a 1x1 128 -> 256 bf16 convolution over
    40 960 rows through conv_fwd_auto with ``emit8`` from its consumer's calibrated slot, then the consuming e4m3 1x1 convolution"""
    from cddmsl_amd import hip, layers
    for key, v in GC.ENV.items():
        monkeypatch.setenv(key, v)
    g = torch.Generator().manual_seed(241)
    x = (torch.randn(4, 80, 128, 128, generator=g)).to(DEV, BF)
    w1, w2 = _param(torch.randn(256, 128, 1, 1, generator=g) * 128 ** -0.5), _param(torch.randn(256, 256, 1, 1, generator=g) * 0.25 * 256 ** -0.5)
    with fresh_scales() as table:
        audit = Audit(monkeypatch)
        pw1, pw2 = layers.PreparedWeight(w1, None, True), layers.PreparedWeight(w2, None, True)
        counts = []
        for pass_no in (1, 2):
            audit.pass_no = pass_no
            hip.PROFILE.enable()
            e8 = layers.fp8_emit_for(pw2, (4, 80, 128, 256), 0, True, producer_cout=256)
            assert (e8 is None) == (pass_no == 1)
            y1 = layers.conv_fwd_auto(x, pw1, None, None, False, emit8=e8, relu=True)      # (fp8 False: the bf16 kernel is the producer)
            y2 = layers.conv_fwd_auto(y1, pw2, None, None, True)
            rows = [e[0] for e in hip.PROFILE.events]
            hip.PROFILE.collect()
            torch.cuda.synchronize()
            counts.append(tuple(rows.count(r) for r in ROWS))
            weights = {w1.data_ptr(), w2.data_ptr()}
            assert audit.check_pass(weights, {w1.data_ptr(): None, w2.data_ptr(): None}, set(), {}) == 1
            table.roll()
        # pass 1 quantises y1 and the consumer's weights, pass 2 nothing: the bf16 launch wrote y1's copy
        assert counts == [(1, 0, 2), (1, 0, 0)], counts
        assert [c["how"] for c in audit.copies if c["pass_no"] == 2 and c["src"] is y1] == ["emit:conv_fwd"]


def test_last_launch_of_a_block_writes_the_previous_blocks_gs_copy(monkeypatch):
    """audit only, no float64 model: two stride-1 blocks on a 4 x 52 x 52 x 512 map.  Block 1's last launch (conv1's input gradient with
    the residual and block 0's output mask, a bf16 launch of 43 x 4 = 172 tiles) is over hip.conv_emit8_ok's floor, so in passes 2 and 3
    it writes the e4m3 copy of ITS result under block 0's gs slot (_block_backward: ``fp8_slot_of(prev_bp, "_fp8_gs").emit()``), and
    block 0's conv3 and downsample input gradients and conv3's weight gradient read that copy: one quantisation pass less than the
    240-row case (x twice and block 1's gs are left)."""
    from cddmsl_amd import hip, layers
    for key, v in GC.ENV.items():
        monkeypatch.setenv(key, v)
    g = torch.Generator().manual_seed(251)
    rn = lambda *s: torch.randn(*s, generator=g)
    blocks, cin = [], 512
    for bi in range(2):
        w = [_param(rn(256, cin, 1, 1) * cin ** -0.5), _param(rn(256, 256, 3, 3) * 2304 ** -0.5), _param(rn(1024, 256, 1, 1) * 256 ** -0.5),
             _param(rn(1024, cin, 1, 1) * cin ** -0.5) if bi == 0 else None]
        bn = [None if v is None else ((torch.rand(v.shape[0], generator=g) + 0.5).to(DEV), (rn(v.shape[0]) * 0.3).to(DEV)) for v in w]
        blocks.append(layers.BlockParams(*w, *bn, 1, False, fp8=True))
        cin = 1024
    params = [v for bp in blocks for v in bp.w if v is not None]
    pws = [pw for bp in blocks for pw in bp.pw if pw is not None]
    bn_of = {pw.param.data_ptr(): pw.scale for pw in pws}
    x0 = rn(4, 52, 52, 512).clamp_min(0)
    gy = rn(4, 52, 52, 1024) * R.GRAD_SIZE
    with fresh_scales() as table:
        audit = Audit(monkeypatch)
        for pass_no in (1, 2, 3):
            audit.pass_no = pass_no
            for p in params:
                p.grad = None
            x = x0.to(DEV, BF).requires_grad_(True)
            hip.PROFILE.enable()
            y = layers.res_stage(x, blocks, False)
            y.backward(gy.to(DEV, BF))
            rows = [e[0] for e in hip.PROFILE.events]
            hip.PROFILE.collect()
            torch.cuda.synchronize()
            wd = {pw._wd.data_ptr() for pw in pws if pw._wd is not None}
            n = audit.check_pass({p.data_ptr() for p in params} | wd, bn_of, wd, {p.grad.data_ptr(): p.data_ptr() for p in params})
            gs_slot = blocks[0]._fp8_gs
            mine = [c for c in audit.copies if c["pass_no"] == pass_no and c["scale_ptr"] == gs_slot.scale.data_ptr()]
            assert len(mine) == 1 and tuple(mine[0]["src"].shape) == (4, 52, 52, 1024)
            readers = [gm["kind"] for gm in audit.gemms if gm["pass_no"] == pass_no and mine[0]["buf"].data_ptr() in (gm["a"].data_ptr(), gm["b"].data_ptr())]
            if pass_no == 1:
                assert mine[0]["how"] == "pass" and n == 16 and sorted(readers) == ["conv", "conv"], (mine[0]["how"], n, readers)
            else:
                assert mine[0]["how"] == "emit:conv_fwd" and n == 18 and sorted(readers) == ["conv", "conv", "wgrad"], (mine[0]["how"], n, readers)
                assert rows.count("quantize_fp8") == 3, rows.count("quantize_fp8")
            table.roll()


def test_worst_ratio_table(capsys):
    """one row per case: the worst error / limit of each pass and the tensor it occurred on; every REQUIRED_BRANCHES entry was run"""
    lines, seen = [], set()
    for name in NAMES:
        if isinstance(_results.get(name), Exception):
            lines.append(f"{name:30s} not evaluated: {_results[name]!r:.120}")
            continue
        case = GC.BY_NAME[name]
        cells = []
        for rows, _, _, _, _ in _evaluate(name):
            n, err, limit = max(rows, key=lambda r: r[1] / r[2])
            cells.append(f"{err / limit:6.3f} ({n}: {err:.2e} of {limit:.2e})")
        seen.add(case["branch"])
        lines.append(f"{name:30s} {'deep' if case['deep'] else '    '}  " + "  |  ".join(cells))
    with capsys.disabled():
        print("\ne4m3 routes against the quantised float64 model: worst error / limit per case, pass 1 | pass 2 | pass 3\n" + "\n".join(lines))
    assert seen >= set(GC.REQUIRED_BRANCHES)
