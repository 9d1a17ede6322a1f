"""layers.roi_downsample_on_map: when the RoI head's downsample conv runs on the feature map instead of on the pooled crops."""
import pytest

BENCH_SUPERVISED = (8192, 14, 16, 50, 83)      # 8192 sampled RoIs on the 16 res4 maps of 800 x 1333: 401 408 crop rows, 66 400 pixels
BENCH_REGIONS = (512, 14, 32, 50, 83)          # the region-level branch: 25 088 crop rows, 132 800 pixels


@pytest.fixture
def rule(monkeypatch):
    from cddmsl_amd import layers
    monkeypatch.delenv("CDDMSL_ROI_COMMUTE", raising=False)
    monkeypatch.delenv("CDDMSL_ROI_COMMUTE_DOWN", raising=False)
    return layers.roi_downsample_on_map


def test_the_rule_at_the_two_calls_of_the_bench(rule):
    assert rule(*BENCH_SUPERVISED) is True
    assert rule(*BENCH_REGIONS) is False


def test_the_rule_compares_pooled_crop_rows_with_map_pixels(rule):
    # 25 crops x 49 rows against 2 x 13 x 21 = 546 pixels (the RoI head entry tests); equality stays on the crops
    assert rule(25, 14, 2, 13, 21) is True
    assert rule(4, 14, 1, 14, 14) is False and rule(5, 14, 1, 14, 14) is True
    assert rule(0, 14, 2, 13, 21) is False


@pytest.mark.parametrize("value,want", [("0", (False, False)), ("1", (True, True)), (None, (True, False))])
def test_the_override(rule, monkeypatch, value, want):
    if value is not None:
        monkeypatch.setenv("CDDMSL_ROI_COMMUTE_DOWN", value)
    assert (rule(*BENCH_SUPERVISED), rule(*BENCH_REGIONS)) == want


@pytest.mark.parametrize("down", [None, "0", "1"])
def test_the_literal_order_wins(rule, monkeypatch, down):
    """CDDMSL_ROI_COMMUTE=0 keeps the pooler in front of the whole of layer4: nothing of it runs on the map"""
    monkeypatch.setenv("CDDMSL_ROI_COMMUTE", "0")
    if down is not None:
        monkeypatch.setenv("CDDMSL_ROI_COMMUTE_DOWN", down)
    assert rule(*BENCH_SUPERVISED) is False and rule(*BENCH_REGIONS) is False
    monkeypatch.setenv("CDDMSL_ROI_COMMUTE", "1")
    assert rule(*BENCH_SUPERVISED) is (down != "0")
