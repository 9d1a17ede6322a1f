"""CPU: the pooled stem convolution's entry point in plan-only mode (validate, plan, return; no GPU): kernel id 8 for the layer it is
built for, CDDMSL_ERR_ARG for everything else; the mask-bit pooling entry points refuse f32."""
import ctypes

import pytest

ERR_ARG = 1
PTR = ctypes.c_void_p(4096)      # a non-null argument; plan-only mode dereferences nothing
NULL = ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from cddmsl_amd import hip
    return hip._L()


def _plan(L, N=16, H=400, W=667, Cin=32, Cout=64, stride=1, dtype=0, mask=NULL, scale=PTR, bias=PTR):
    was = L.cddmsl_plan_only(1)
    try:
        st = L.cddmsl_conv3x3_pool_fwd(PTR, PTR, PTR, scale, bias, mask, N, H, W, Cin, Cout, stride, dtype, NULL)
        return st, L.cddmsl_last_kernel()
    finally:
        L.cddmsl_plan_only(was)


@pytest.mark.parametrize("shape", [(16, 400, 667), (16, 112, 112), (1, 2, 2), (1, 7, 9)])
def test_pooled_stem_conv_plans_the_small_kernel(L, shape):
    assert _plan(L, *shape) == (0, 8)


@pytest.mark.parametrize("kw", [dict(dtype=1), dict(Cout=32), dict(Cin=64), dict(stride=2), dict(mask=PTR), dict(scale=NULL), dict(bias=NULL),
                                dict(H=1), dict(N=64, H=800, W=1336)],
                         ids=["f32", "cout32", "cin64", "stride2", "mask", "no_scale", "no_bias", "one_row", "input_past_2GiB"])
def test_pooled_stem_conv_refusals(L, kw):
    assert _plan(L, **kw)[0] == ERR_ARG


def test_pool_bits_refuse_f32_and_odd_channels(L):
    for dtype, C in ((1, 8), (0, 12)):
        assert L.cddmsl_avgpool2_fwd_bits(PTR, PTR, PTR, 1, 4, 4, C, dtype, NULL) == ERR_ARG
        assert L.cddmsl_avgpool2_bwd_bits(PTR, PTR, PTR, 1, 4, 4, C, dtype, NULL) == ERR_ARG
    assert L.cddmsl_avgpool2_fwd_bits(PTR, PTR, NULL, 1, 4, 4, 8, 0, NULL) == ERR_ARG
