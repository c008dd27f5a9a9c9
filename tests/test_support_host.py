"""tests/support.py's launch counting on literal profiles: no library, no GPU."""
import pytest

import support


def test_launch_counts_sums_a_name_over_its_sizes():
    prof = {"conv_u8|2x16x8x8": (2, 0.1), "conv_u8|2x16x4x4": (1, 0.2), "avgpool_u8_nhwc|2x16x8x8": (1, 0.3)}
    assert support.launch_counts(prof) == {"conv_u8": 3, "avgpool_u8_nhwc": 1}
    assert support.launch_counts({}) == {}


def test_glue_check_raises_on_a_layout_launch_and_passes_without_one():
    clean = {"conv_u8|a": (2,), "lut_u8_nhwc|a": (1,), "lut_u8_nhwc|b": (1,)}
    support.assert_no_glue_launches(support.launch_counts(clean))
    assert support.split_launches(support.launch_counts(clean), "lut_u8") == (2, 2, {"conv_u8": 2, "lut_u8_nhwc": 2})
    dirty = dict(clean, **{"layout_nchw_to_nhwc|a": (1,)})
    assert support.launch_counts(dirty)["layout_nchw_to_nhwc"] == 1  # counting alone asserts nothing
    with pytest.raises(AssertionError):
        support.assert_no_glue_launches(support.launch_counts(dirty))
    with pytest.raises(AssertionError):
        support.split_launches(support.launch_counts(dirty), "lut_u8")
    for name in support.GLUE_KERNELS:
        with pytest.raises(AssertionError):
            support.assert_no_glue_launches({name + "x": 1})
