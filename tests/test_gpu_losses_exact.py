"""The loss-side kernels against float64 references of the operands they were given (tests/exact_losses.py): every extern "C" entry
point of cddmsl_amd/csrc/losses.hip and cddmsl_sgd_clip_step, called through the C-ABI at the case list the host test shares
(tests/test_losses_bound_host.py runs the same drivers on an f32 emulation and on its mutants).  Outputs are NaN-filled with at
least four guard rows (or elements) past them, which must come back untouched bit for bit; the worst |err| / bound of every output
is printed by the module's last test.

Entry points and the case that reaches each branch (every one also in test_argument_errors_and_empty_launches_write_nothing for its
CDDMSL_ERR_ARG return and, where it has one, its R == 0 / count == 0 return):
  cddmsl_l2norm_fwd / _bwd          test_l2norm: D = 1, 63 (part of one 256-thread pass), 256, 257 and 1024 (the stride loop wraps);
                                    eps = 0 (plain division) and 1e-12 with a row below it (the fmaxf takes eps)
  cddmsl_cosine_logits_fwd          test_cosine_logits: R = 1, 5, 6 (a partly filled block: r >= R returns), D % 64 != 0 (200, 1030)
  cddmsl_cosine_logits_bwd          the register branch D = 64, 200, 1024; the two-pass branch D = 1030, 1088; accumulate 0 and 1 in both
  cddmsl_contrastive_fwd / _bwd     test_contrastive: k_lse_rows plain and transposed, k_contrastive_loss, k_contrastive_grad at
                                    ld = n and ld = n + 5; n = 1, 3, 48 (one pass), 257, 300 (the 256-thread loops wrap, 2 grad blocks+)
  cddmsl_layernorm_fwd / _bwd       test_layernorm: k_layernorm_*_v<T, 1..4> at D = 256, 512, 768, 1024 for T = bf16 and f32; the generic
                                    kernels at D = 1, 65, 200 and at D = 768 with x, y / dy, gamma or beta / dx one element off
                                    16-byte alignment (aligned16 fails); accumulate 0 and 1 on both; R = 1, 5, 37
  cddmsl_focal_ce_fwd / _bwd        test_focal_ce: gamma = 0 (mod = 1, dmod = 0) and > 0; C = 64 (no padding lane), 1, 9, 21; t == bg_class
                                    and not; omp == 0 (dmod's guard) on the saturated rows and C = 1; pt below 1e-38 (the clamp of ce)
  cddmsl_rpn_losses                 test_rpn_losses: forward (gout2 null) and backward; npos + nneg = 0 (no loop pass) .. 1000 (the loop
                                    wraps); is_pos and not; sgn at e > 0, < 0 and == 0
  cddmsl_box_l1                     test_box_l1: forward and backward; cls null (column 0) and given; ld = 4, 4 Kc, 4 Kc + 4; nfg = 0, 1, 300
  cddmsl_sgd_clip_step              test_sgd_clip_step: 1, 2 and 3 batches of SGD_MAX (count = 1, 4, 97, 193); k_sqnorm's vector path and
                                    its scalar path (g misaligned); k_sgd's vector path and its scalar path for each of p, g, m
                                    misaligned; the n % 4 tail; four tensors of about 2^20 elements (n % 4 = 3, 2, 1, 0), one per
                                    alignment pattern, so each of those loops wraps; first_step 1 and 0; coef clamped
                                    to 1 and below 1

Measured on one MI355X, worst |err| / bound over all cases (none below 0.05, the mark of a loose bound; the two lowest are
cosine_logits_fwd scores, dominated by the (wave_depth + 2) u sum|x w| accumulation term, and rpn_losses out2, dominated by the
block_depth u sum of the terms):
  box_l1 out1 0.104                 contrastive_bwd dS 0.411          contrastive_fwd clse 0.566        contrastive_fwd loss 0.115
  contrastive_fwd rlse 0.554        cosine_logits_bwd dx 0.237        ... (accumulate) 0.356            cosine_logits_fwd inv 0.218
  cosine_logits_fwd scores 0.058    focal_ce_bwd dlogits 0.371        focal_ce_fwd probs 0.219          focal_ce_fwd row_loss 0.457
  l2norm_bwd dx 0.800               l2norm_fwd inv 0.168              l2norm_fwd y 0.243                layernorm_bwd dx 0.335
  ... (accumulate) 0.343            layernorm_fwd mean 0.149          layernorm_fwd rstd 0.363          layernorm_fwd y bf16 0.995
  layernorm_fwd y f32 0.248         rpn_losses dlogits 0.607          rpn_losses out2 0.082             sgd_clip_step m 0.916
  sgd_clip_step norm_ws 0.119       sgd_clip_step p 0.990
The pooled signed store error of layernorm_fwd y bf16 is +0.0013 ulp over 229292 elements.
(0.99 is a correctly rounded store of a value just above a power of two: half an ulp is u |value| there.)"""
import ctypes

import pytest
import torch

import exact_losses as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4
WORST = {}
POOL = E.Report()                   # the signed bf16 store error, pooled over the module's cases (judged by the last test)
LIVE = []                           # the device operands of the running test: a pointer handed to a launch stays allocated


def _L():
    from cddmsl_amd import hip
    return hip._L()


def _stream():
    from cddmsl_amd import hip
    return hip.stream_ptr()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _dev(t, shift=False):
    """the tensor on the GPU; ``shift``: as a view one element into a larger buffer, so that its base is not 16-byte aligned"""
    if t is None:
        return None
    if not shift:
        v = t.to(DEV).contiguous()
    else:
        buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 != 0
    LIVE.append(v)
    return v


class _Out:
    """an output of ``rows`` x ``cols`` elements with GUARD rows (at least GUARD elements) past it and, when ``shift``, one element
    before it; NaN-filled, or ``init`` in the data and NaN around it.  get() checks the surroundings bit for bit"""

    def __init__(self, rows, cols=None, dtype=torch.float32, init=None, shift=False, fill=float("nan")):
        self.shape = (rows,) if cols is None else (rows, cols)
        cols = cols or 1
        self.n, self.lead = rows * cols, 1 if shift else 0
        self.buf = torch.full((self.lead + self.n + GUARD * cols,), float("nan"), dtype=dtype, device=DEV)
        self.data = self.buf[self.lead:self.lead + self.n]
        if init is not None:
            self.data.copy_(init.reshape(-1))
        elif fill == fill:
            self.data.fill_(fill)
        self.before = self.buf.clone()

    @property
    def ptr(self):
        return ctypes.c_void_p(self.data.data_ptr())

    def get(self, written=True):
        torch.cuda.synchronize()
        a, b = self.buf.cpu(), self.before.cpu()
        assert E.bits_equal(a[:self.lead], b[:self.lead]) and E.bits_equal(a[self.lead + self.n:], b[self.lead + self.n:]), \
            "an element outside the output was written"
        if not written:
            assert E.bits_equal(a, b), "the output was written"
        return a[self.lead:self.lead + self.n].view(self.shape).clone()


def _ok(status):
    assert status == 0, f"status {status}"


class Gpu:
    """exact_losses' implementation interface on the C-ABI: CPU tensors in, CPU tensors out"""

    def l2_fwd(self, x, eps):
        R, D = x.shape
        y, inv = _Out(R, D), _Out(R)
        _ok(_L().cddmsl_l2norm_fwd(_p(_dev(x)), y.ptr, inv.ptr, R, D, eps, _stream()))
        return y.get(), inv.get()

    def l2_bwd(self, dy, y, inv):
        R, D = y.shape
        dx = _Out(R, D)
        _ok(_L().cddmsl_l2norm_bwd(_p(_dev(dy)), _p(_dev(y)), _p(_dev(inv)), dx.ptr, R, D, _stream()))
        return dx.get()

    def cos_fwd(self, x, wn, T, eps):
        R, D = x.shape
        Kc = wn.shape[0]
        sc, inv = _Out(R, Kc + 1), _Out(R)
        _ok(_L().cddmsl_cosine_logits_fwd(_p(_dev(x)), _p(_dev(wn)), sc.ptr, inv.ptr, R, D, Kc, T, eps, _stream()))
        return sc.get(), inv.get()

    def cos_bwd(self, ds, x, wn, inv, T, dx0):
        R, D = x.shape
        dx = _Out(R, D, init=dx0)
        _ok(_L().cddmsl_cosine_logits_bwd(_p(_dev(ds)), _p(_dev(x)), _p(_dev(wn)), _p(_dev(inv)), dx.ptr, R, D, wn.shape[0], T,
                                          int(dx0 is not None), _stream()))
        return dx.get()

    def con_fwd(self, S, n):
        rl, cl, loss = _Out(n), _Out(n), _Out(1)
        _ok(_L().cddmsl_contrastive_fwd(_p(_dev(S)), rl.ptr, cl.ptr, loss.ptr, n, S.shape[1], _stream()))
        return rl.get(), cl.get(), loss.get()

    def con_bwd(self, S, rl, cl, gloss, n):
        dS = _Out(n, n)
        _ok(_L().cddmsl_contrastive_bwd(_p(_dev(S)), _p(_dev(rl)), _p(_dev(cl)), _p(_dev(gloss)), dS.ptr, n, S.shape[1], _stream()))
        return dS.get()

    def ln_fwd(self, x, ga, be, eps, dt, mis=None):
        R, D = x.shape
        y, mean, rstd = _Out(R, D, dt, shift=mis == "y"), _Out(R), _Out(R)
        _ok(_L().cddmsl_layernorm_fwd(_p(_dev(x, mis == "x")), _p(_dev(ga, mis == "gamma")), _p(_dev(be, mis == "dx")), y.ptr, mean.ptr,
                                      rstd.ptr, R, D, eps, 0 if dt == torch.bfloat16 else 1, _stream()))
        return y.get(), mean.get(), rstd.get()

    def ln_bwd(self, dy, x, ga, mean, rstd, dx0, mis=None):
        R, D = x.shape
        dx = _Out(R, D, init=dx0, shift=mis == "dx")
        _ok(_L().cddmsl_layernorm_bwd(_p(_dev(dy, mis == "y")), _p(_dev(x, mis == "x")), _p(_dev(ga, mis == "gamma")), _p(_dev(mean)),
                                      _p(_dev(rstd)), dx.ptr, R, D, int(dx0 is not None), 0 if dy.dtype == torch.bfloat16 else 1, _stream()))
        return dx.get()

    def focal_fwd(self, z, t, gamma, bg, bgw):
        R, C = z.shape
        row, probs = _Out(R), _Out(R, C)
        _ok(_L().cddmsl_focal_ce_fwd(_p(_dev(z)), _p(_dev(t)), row.ptr, probs.ptr, R, C, gamma, bg, bgw, _stream()))
        return row.get(), probs.get()

    def focal_bwd(self, z, t, probs, gs, gamma, bg, bgw):
        R, C = z.shape
        dl = _Out(R, C)
        _ok(_L().cddmsl_focal_ce_bwd(_p(_dev(z)), _p(_dev(t)), _p(_dev(probs)), _p(_dev(gs)), dl.ptr, R, C, gamma, bg, bgw, _stream()))
        return dl.get()

    def rpn(self, logits, deltas, pos, neg, midx, gt, gt_off, anchors, A, w, inv_norm, gout=None):
        args = (_p(_dev(logits)), _p(_dev(deltas)), _p(_dev(pos)), pos.numel(), _p(_dev(neg)), neg.numel(), _p(_dev(midx)), _p(_dev(gt)),
                _p(_dev(gt_off)), _p(_dev(anchors)), A, *w, inv_norm)
        if gout is None:
            out = _Out(2)
            _ok(_L().cddmsl_rpn_losses(*args, out.ptr, None, None, None, _stream()))
            return out.get()
        dl, dd = _Out(logits.numel(), fill=0.0), _Out(logits.numel(), 4, fill=0.0)      # zero-filled by the caller: the contract
        _ok(_L().cddmsl_rpn_losses(*args, None, _p(_dev(gout)), dl.ptr, dd.ptr, _stream()))
        return dl.get(), dd.get()

    def box(self, deltas, fg, cls, src, tgt, w, inv_norm, gout=None):
        R, ld = deltas.shape
        args = (_p(_dev(deltas)), ld, _p(_dev(fg)), fg.numel(), _p(_dev(cls)), _p(_dev(src)), _p(_dev(tgt)), *w, inv_norm)
        if gout is None:
            out = _Out(1)
            _ok(_L().cddmsl_box_l1(*args, out.ptr, None, None, _stream()))
            return out.get()
        dd = _Out(R, ld, fill=0.0)
        _ok(_L().cddmsl_box_l1(*args, None, _p(_dev(gout)), dd.ptr, _stream()))
        return dd.get()

    def sgd(self, lay, p, g, m, ws, lr, mo, wd, clip, first):
        pd, gd, md, wsd = _dev(p), _dev(g), _dev(m), _dev(ws)
        n = len(lay)
        at = lambda buf, k: (ctypes.c_void_p * n)(*[buf.data_ptr() + 4 * l[k] for l in lay])
        sizes = (ctypes.c_long * n)(*[l[0] for l in lay])
        _ok(_L().cddmsl_sgd_clip_step(at(pd, 1), at(gd, 2), at(md, 3), sizes, n, _p(wsd), lr, mo, wd, clip, int(first), _stream()))
        torch.cuda.synchronize()
        assert E.bits_equal(gd.cpu(), g), "the gradient buffer was written"
        return pd.cpu(), md.cpu(), wsd.cpu()


def _run(run, case):
    rep = E.Report()
    run(case, Gpu(), rep)
    torch.cuda.synchronize()
    LIVE.clear()
    for k, v in rep.worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
    for k, (sm, n) in rep.pool.items():
        acc = POOL.pool.setdefault(k, [0.0, 0])
        acc[0] += sm
        acc[1] += n
    for k, v in rep.worst.items():
        print(f"{k} [{E.tag(case)}]: worst |err|/bound {v:.3g}")
    assert not rep.fail, "\n".join(rep.fail)


def _cases(fn):
    return dict(argvalues=fn(), ids=[E.tag(c).replace(" ", ",") for c in fn()])


@pytest.mark.parametrize("case", **_cases(E.l2_cases))
def test_l2norm(case):
    """cddmsl_l2norm_fwd / _bwd: D below, at and past the 256-thread stride, eps = 0 and 1e-12, a row of norm below eps"""
    _run(E.run_l2, case)


@pytest.mark.parametrize("case", **_cases(E.cos_cases))
def test_cosine_logits(case):
    """cddmsl_cosine_logits_fwd / _bwd: the register path (D <= 1024) and the two-pass path (1030, 1088), D % 64 != 0, R % 4 != 0,
    accumulate into a random dx, a non-zero background column in ds"""
    _run(E.run_cos, case)


@pytest.mark.parametrize("case", **_cases(E.con_cases))
def test_contrastive(case):
    """cddmsl_contrastive_fwd / _bwd: ld = n and ld = n + 5 with NaN in the padding, n past the 256-thread stride, S in [-1, 1] and
    times 100, gloss != 1"""
    _run(E.run_con, case)


@pytest.mark.parametrize("case", **_cases(E.ln_cases))
def test_layernorm(case):
    """cddmsl_layernorm_fwd / _bwd: the register kernels (D = 256 .. 1024), the generic ones (D = 1, 65, 200, and D = 768 with one
    operand off 16-byte alignment), both dtypes, accumulate, a constant row, a row of mean 1e3"""
    _run(E.run_ln, case)


@pytest.mark.parametrize("case", **_cases(E.focal_cases))
def test_focal_ce(case):
    """cddmsl_focal_ce_fwd / _bwd: C = 1, 9, 21, 64, gamma = 0 / 0.5 / 2, both background conventions, logits of spread 1 and 100,
    rows of all-negative logits, saturated rows (1 - pt == 0) and rows whose pt underflows"""
    _run(E.run_focal, case)


@pytest.mark.parametrize("case", **_cases(E.rpn_cases))
def test_rpn_losses(case):
    """cddmsl_rpn_losses forward and backward: 0 .. 1000 sampled anchors around the 256-thread stride, no positives, no negatives,
    an image without boxes, weights != 1, positives whose delta equals its target"""
    _run(E.run_rpn, case)


@pytest.mark.parametrize("case", **_cases(E.box_cases))
def test_box_l1(case):
    """cddmsl_box_l1 forward and backward: class-specific at ld = 4 Kc and 4 Kc + 4, class-agnostic at ld = 4, 0 / 1 / 300 rows"""
    _run(E.run_box, case)


@pytest.mark.parametrize("case", **_cases(E.sgd_cases))
def test_sgd_clip_step(case):
    """cddmsl_sgd_clip_step: views at element offsets 0..3 into flat buffers (the vector path, the scalar path for each of p, g, m
    misaligned, the n % 4 tail), 1 .. 3 batches of 96, four tensors of about 2^20 elements, one per alignment pattern (every
    grid-stride loop wraps), a first step on a
    NaN momentum and a second one, norms above, around and below the clip and zero, norm_ws pre-filled"""
    _run(E.run_sgd, case)


def test_argument_errors_and_empty_launches_write_nothing():
    """the branches of the host dispatch that return before any launch: CDDMSL_ERR_ARG (1), and R == 0 / count == 0 (0)"""
    L, st = _L(), _stream()
    x = _dev(torch.randn(8, 65))
    lng = _dev(torch.zeros(8, dtype=torch.int64))
    o = [_Out(8, 65) for _ in range(4)]
    calls = [
        (1, lambda: L.cddmsl_focal_ce_fwd(_p(x), _p(lng), o[0].ptr, o[1].ptr, 8, 65, 0.5, 64, 0.2, st)),      # C = 65
        (1, lambda: L.cddmsl_focal_ce_bwd(_p(x), _p(lng), _p(x), _p(x), o[0].ptr, 8, 65, 0.5, 64, 0.2, st)),
        (0, lambda: L.cddmsl_focal_ce_fwd(_p(x), _p(lng), o[0].ptr, o[1].ptr, 0, 21, 0.5, 20, 0.2, st)),
        (0, lambda: L.cddmsl_focal_ce_bwd(_p(x), _p(lng), _p(x), _p(x), o[0].ptr, 0, 21, 0.5, 20, 0.2, st)),
        (1, lambda: L.cddmsl_l2norm_fwd(_p(x), o[0].ptr, o[1].ptr, 8, 0, 0.0, st)),
        (0, lambda: L.cddmsl_l2norm_fwd(_p(x), o[0].ptr, o[1].ptr, 0, 65, 0.0, st)),
        (1, lambda: L.cddmsl_l2norm_bwd(_p(x), _p(x), _p(x), o[0].ptr, -1, 65, st)),
        (0, lambda: L.cddmsl_l2norm_bwd(_p(x), _p(x), _p(x), o[0].ptr, 0, 65, st)),
        (1, lambda: L.cddmsl_cosine_logits_fwd(_p(x), _p(x), o[0].ptr, o[1].ptr, 8, 65, 4, 0.0, 1e-12, st)),  # temperature 0
        (1, lambda: L.cddmsl_cosine_logits_fwd(_p(x), _p(x), o[0].ptr, o[1].ptr, 8, 65, 0, 0.01, 1e-12, st)),
        (0, lambda: L.cddmsl_cosine_logits_fwd(_p(x), _p(x), o[0].ptr, o[1].ptr, 0, 65, 4, 0.01, 1e-12, st)),
        (1, lambda: L.cddmsl_cosine_logits_bwd(_p(x), _p(x), _p(x), _p(x), o[0].ptr, 8, 65, 4, -1.0, 0, st)),
        (0, lambda: L.cddmsl_cosine_logits_bwd(_p(x), _p(x), _p(x), _p(x), o[0].ptr, 0, 65, 4, 0.01, 0, st)),
        (1, lambda: L.cddmsl_contrastive_fwd(_p(x), o[0].ptr, o[1].ptr, o[2].ptr, 8, 7, st)),                 # ld < n
        (1, lambda: L.cddmsl_contrastive_fwd(_p(x), o[0].ptr, o[1].ptr, o[2].ptr, 0, 8, st)),
        (1, lambda: L.cddmsl_contrastive_bwd(_p(x), _p(x), _p(x), _p(x), o[0].ptr, 8, 7, st)),
        (1, lambda: L.cddmsl_layernorm_fwd(_p(x), _p(x), _p(x), o[0].ptr, o[1].ptr, o[2].ptr, 8, 65, 1e-5, 2, st)),   # dtype
        (0, lambda: L.cddmsl_layernorm_fwd(_p(x), _p(x), _p(x), o[0].ptr, o[1].ptr, o[2].ptr, 0, 65, 1e-5, 1, st)),
        (1, lambda: L.cddmsl_layernorm_bwd(_p(x), _p(x), _p(x), _p(x), _p(x), o[0].ptr, 8, 0, 0, 1, st)),
        (0, lambda: L.cddmsl_layernorm_bwd(_p(x), _p(x), _p(x), _p(x), _p(x), o[0].ptr, 0, 65, 0, 1, st)),
        (1, lambda: L.cddmsl_rpn_losses(_p(x), _p(x), _p(lng), 1, _p(lng), 1, _p(lng), _p(x), _p(lng), _p(x), 4, 1.0, 1.0, 1.0, 1.0, 1.0,
                                        None, None, None, None, st)),                                         # forward without out2
        (1, lambda: L.cddmsl_rpn_losses(_p(x), _p(x), _p(lng), 1, _p(lng), 1, _p(lng), _p(x), _p(lng), _p(x), 4, 1.0, 1.0, 1.0, 1.0, 1.0,
                                        None, _p(x), o[0].ptr, None, st)),                                    # backward without ddeltas
        (1, lambda: L.cddmsl_rpn_losses(_p(x), _p(x), _p(lng), -1, _p(lng), 1, _p(lng), _p(x), _p(lng), _p(x), 4, 1.0, 1.0, 1.0, 1.0, 1.0,
                                        o[0].ptr, None, None, None, st)),
        (1, lambda: L.cddmsl_box_l1(_p(x), 3, _p(lng), 1, None, _p(x), _p(x), 1.0, 1.0, 1.0, 1.0, 1.0, o[0].ptr, None, None, st)),   # ld < 4
        (1, lambda: L.cddmsl_box_l1(_p(x), 4, _p(lng), 1, None, _p(x), _p(x), 1.0, 1.0, 1.0, 1.0, 1.0, None, _p(x), None, st)),
        (1, lambda: L.cddmsl_sgd_clip_step(None, None, None, None, -1, o[0].ptr, 0.1, 0.9, 0.0, 1.0, 1, st)),
        (0, lambda: L.cddmsl_sgd_clip_step(None, None, None, None, 0, o[0].ptr, 0.1, 0.9, 0.0, 1.0, 1, st)),
    ]
    for i, (want, call) in enumerate(calls):
        assert call() == want, f"call {i}"
    for b in o:
        b.get(written=False)


def test_wrappers_refuse_non_contiguous_operands():
    """cddmsl_amd.hip passes raw pointers: a transposed (non-contiguous) operand would be read as if it were contiguous.  Every
    wrapper of this family refuses it, and sgd_clip_step refuses a norm workspace shorter than the tensor list"""
    from cddmsl_amd import hip
    n = 8
    sq = torch.randn(n, n, device=DEV)
    tr = sq.t()
    assert not tr.is_contiguous()
    vec = torch.rand(n, device=DEV) + 0.5
    tgt = torch.zeros(n, dtype=torch.int64, device=DEV)
    one = torch.ones(1, device=DEV)
    wn = torch.randn(n - 1, n, device=DEV)
    bad = [
        lambda: hip.l2norm_fwd(tr, 0.0),
        lambda: hip.l2norm_bwd(sq, tr, vec),
        lambda: hip.l2norm_bwd(sq, sq, torch.rand(2 * n, device=DEV)[::2]),
        lambda: hip.cosine_logits_fwd(tr, wn, 0.01),
        lambda: hip.cosine_logits_bwd(sq, tr, wn, vec, 0.01),
        lambda: hip.cosine_logits_bwd(sq, sq, torch.randn(n, n - 1, device=DEV).t(), vec, 0.01),
        lambda: hip.cosine_logits_bwd(sq, sq, wn, vec, 0.01, dx=torch.zeros(n, n, device=DEV).t()),
        lambda: hip.cosine_logits_bwd(sq, sq, wn, vec, 0.01, dx=torch.zeros(n, n, device=DEV, dtype=torch.bfloat16)),
        lambda: hip.contrastive_fwd(tr),
        lambda: hip.contrastive_bwd(tr, vec, vec, one),
        lambda: hip.contrastive_bwd(sq, torch.rand(2 * n, device=DEV)[::2], vec, one),
        lambda: hip.focal_ce_fwd(tr, tgt, 0.5, n - 1, 0.2),
        lambda: hip.focal_ce_bwd(tr, tgt, sq, one, 0.5, n - 1, 0.2),
        lambda: hip.focal_ce_bwd(sq, tgt, tr, one, 0.5, n - 1, 0.2),
        lambda: hip.focal_ce_bwd(sq, torch.zeros(2 * n, dtype=torch.int64, device=DEV)[::2], sq, one, 0.5, n - 1, 0.2),
        lambda: hip.layernorm_fwd(tr, vec, vec, torch.float32),
        lambda: hip.layernorm_fwd(sq, torch.rand(2 * n, device=DEV)[::2], vec, torch.float32),
        lambda: hip.layernorm_bwd(sq, tr, vec, vec, vec),
        lambda: hip.layernorm_bwd(sq, sq, vec, torch.rand(2 * n, device=DEV)[::2], vec),
        lambda: hip.sgd_clip_step([sq.clone(), sq.clone()], [sq, sq], [sq.clone(), sq.clone()], torch.zeros(1, device=DEV), 0.1, 0.9, 0.0, 1.0, True),
    ]
    for call in bad:
        with pytest.raises(AssertionError):
            call()
    # the same calls with contiguous operands go through
    y, inv = hip.l2norm_fwd(sq, 0.0)
    hip.l2norm_bwd(sq, y, inv)
    hip.cosine_logits_bwd(sq, sq, wn, vec, 0.01, dx=torch.zeros(n, n, device=DEV))
    loss, rl, cl = hip.contrastive_fwd(sq)
    hip.contrastive_bwd(sq, rl, cl, one)
    yl, mean, rstd = hip.layernorm_fwd(sq, vec, vec, torch.float32)
    hip.layernorm_bwd(sq, sq, vec, mean, rstd)
    row, probs = hip.focal_ce_fwd(sq, tgt, 0.5, n - 1, 0.2)
    hip.focal_ce_bwd(sq, tgt, probs, one, 0.5, n - 1, 0.2)
    hip.sgd_clip_step([sq.clone()], [sq], [sq.clone()], torch.zeros(1, device=DEV), 0.1, 0.9, 0.0, 1.0, True)
    torch.cuda.synchronize()


def test_worst_ratio_table(capsys):
    """the module's last test: the worst |err| / bound of every kernel output the tests before it checked, one line each (shown
    without -s); every ratio is at most 1"""
    lines = ["", "worst |err| / bound per kernel output:"] + [f"  {k:44s} {WORST[k]:.3f}" for k in sorted(WORST)]
    with capsys.disabled():
        print("\n".join(lines))
    assert all(v <= 1.0 for v in WORST.values())
    POOL.finish()
    with capsys.disabled():
        print("\n".join(f"  store bias of {k}: {sm / max(n, 1):+.4f} ulp over {n} elements" for k, (sm, n) in POOL.pool.items()))
    assert not POOL.fail, POOL.fail
