"""The pooling / streaming kernels of cddmsl_amd/csrc/elementwise.hip, each called directly through the C-ABI and compared bit for bit
with torch f32 elementwise arithmetic on the stored operands (tests/pool_exact.py): avgpool2_fwd / _bwd / _bwd_q8, maxpool3s2_fwd,
upsample_zero2, meanpool_fwd / _bwd and relu_bwd, in bf16 and f32, at odd sizes and with every optional operand present and absent;
and once more in a fresh process whose grid is capped at 3 blocks, so that every grid-stride loop iterates several times."""
import os
import subprocess
import sys

import pytest
import torch

import pool_exact as P

pytestmark = pytest.mark.gpu
DT = pytest.mark.parametrize("dtype", P.DTYPES, ids=["bf16", "f32"])


def _c(dtype, chunks):
    return chunks * (8 if dtype == torch.bfloat16 else 4)


@DT
@pytest.mark.parametrize("H,W", [(2, 2), (7, 9), (8, 6)])
def test_avgpool2_fwd(dtype, H, W):
    P.avgpool2_fwd(3, H, W, _c(dtype, 5), dtype)


@DT
@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("add", [False, True])
def test_avgpool2_bwd(dtype, mask, add):
    """even sizes, and odd H / W: the floor-dropped row and column receive ``add`` or 0"""
    for (H, W) in ((4, 6), (7, 9), (2, 3)):
        P.avgpool2_bwd(3, H, W, _c(dtype, 5), dtype, mask, add)


@pytest.mark.parametrize("mask,add", [(False, False), (True, True), (True, False)])
def test_avgpool2_bwd_q8(mask, add):
    P.avgpool2_bwd_q8(3, 7, 9, 40, mask, add)


def test_avgpool2_bwd_q8_grid_stride_loop():
    """its grid is capped at 8192 blocks whatever the environment says: 2 * 66 * 64 * 256 chunks make every thread loop twice"""
    P.avgpool2_bwd_q8(2, 66, 64, 2048, True, True)


@DT
@pytest.mark.parametrize("H", [1, 2, 7, 8])
@pytest.mark.parametrize("W", [1, 2, 7, 8])
def test_maxpool3s2_fwd(dtype, H, W):
    P.maxpool3s2_fwd(3, H, W, _c(dtype, 3), dtype)


@DT
@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("add", [False, True])
def test_upsample_zero2(dtype, mask, add):
    for (H, W) in ((4, 6), (7, 9), (1, 1), (2, 5)):
        P.upsample_zero2(3, H, W, _c(dtype, 5), dtype, mask, add)


@DT
@pytest.mark.parametrize("Pn", [1, 49])
def test_meanpool_fwd_and_bwd(dtype, Pn):
    P.meanpool_fwd(37, Pn, 100, dtype)
    P.meanpool_bwd(37, Pn, 100, dtype)


@pytest.mark.parametrize("dtype,g_f32", [(torch.bfloat16, False), (torch.bfloat16, True), (torch.float32, False)], ids=["bf16", "bf16_f32grad", "f32"])
def test_relu_bwd(dtype, g_f32):
    P.relu_bwd(4000, dtype, g_f32)


def test_grid_stride_loops_iterate_in_a_process_with_a_capped_grid():
    """one fresh child (the cap is read once per process): python -m pool_exact with CDDMSL_GRID_CAP=3"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, CDDMSL_GRID_CAP="3")
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    try:
        r = subprocess.run([sys.executable, "-m", "pool_exact"], cwd=here, env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"the child did not finish in 120 s:\n{e.stdout}\n{e.stderr}")
    print(r.stdout)
    assert r.returncode == 0, f"child exit {r.returncode}\n{r.stdout}\n{r.stderr[-4000:]}"
    assert r.stdout.count(": ok (CDDMSL_GRID_CAP=3)") == 8, r.stdout
