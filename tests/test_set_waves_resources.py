"""The three kernels block sets on the wave-per-component route add (k_wset<batched>, k_wset<bit-serial>, k_wsetd), read from
the gfx950 code object's metadata (no GPU): they exist, under names the counts of tests/test_kernel_resources.py do not see,
and within the register and scratch limits of their plain twins k_gpipe / k_gdec."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from kernel_stats import kernel_table  # noqa: E402

OTHERS = ("k_gpipe", "k_gdec", "k_chain", "k_pipe", "k_dpipe", "k_lanes")


@pytest.fixture(scope="module")
def table(zpq):
    zpq.lib()
    return kernel_table()


def test_exactly_three_new_kernels_within_their_limits(table):
    new = {k: v for k, v in table.items() if "k_wset" in k}
    assert len(new) == 3, sorted(new)
    for name in new:
        assert not any(o in name for o in OTHERS), name
    dec = [k for k in new if "k_wsetd" in k]
    enc = [k for k in new if "k_wsetd" not in k]
    assert len(dec) == 1 and len(enc) == 2
    assert sorted("Lb1E" in k for k in enc) == [False, True]     # both BATCH forms
    for k in enc:
        assert new[k]["vgpr"] <= 128 and new[k]["scratch"] <= 16, (k, new[k])
    assert new[dec[0]]["vgpr"] <= 128 and new[dec[0]]["scratch"] == 0, new[dec[0]]


def test_the_pinned_counts_are_unchanged(table):
    assert sum("k_gpipe" in k for k in table) == 2
    assert sum("k_gdec" in k for k in table) == 1
    assert sum("k_vpipe" in k for k in table) == 2 and sum("k_vdec" in k for k in table) == 1
    for k, v in table.items():
        if "k_gpipe" in k:
            assert v["vgpr"] <= 128 and v["scratch"] <= 16, (k, v)
        if "k_gdec" in k:
            assert v["vgpr"] <= 128 and v["scratch"] == 0, (k, v)
