"""The three kernels block sets on the interpreter-wave route add (k_vset<batched>, k_vset<bit-serial>, k_vsetd), read from the
gfx950 code object's metadata (no GPU): they exist, under names the counts of the other resource tests do not see, and within
the register limit of a 1024-thread workgroup and the scratch of their plain twins k_vpipe<same BATCH> / k_vdec."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from kernel_stats import kernel_table  # noqa: E402

OTHERS = ("k_wset", "k_vpipe", "k_vdec", "k_gpipe", "k_gdec", "k_chain", "k_pipe", "k_dpipe", "k_lanes")


@pytest.fixture(scope="module")
def table(zpq):
    zpq.lib()
    return kernel_table()


def only(table, part, batch=None):
    hits = [k for k in table if part in k and (batch is None or ("Lb1E" if batch else "Lb0E") in k)]
    assert len(hits) == 1, (part, batch, hits)
    return table[hits[0]]


def test_exactly_three_new_kernels_within_their_limits(table):
    new = {k: v for k, v in table.items() if "k_vset" in k}
    assert len(new) == 3, sorted(new)
    for name in new:
        assert not any(o in name for o in OTHERS), name
    dec = [k for k in new if "k_vsetd" in k]
    enc = [k for k in new if "k_vsetd" not in k]
    assert len(dec) == 1 and len(enc) == 2
    assert sorted("Lb1E" in k for k in enc) == [False, True]     # both BATCH forms
    for k in enc:                                                # (at n = 14 a workgroup is 16 waves: 128 VGPRs is a hard limit)
        twin = only(table, "k_vpipe", "Lb1E" in k)
        assert new[k]["vgpr"] <= 128 and new[k]["scratch"] <= twin["scratch"], (k, new[k], twin)
    twin = only(table, "k_vdec")
    assert new[dec[0]]["vgpr"] <= 128 and new[dec[0]]["scratch"] <= twin["scratch"], (new[dec[0]], twin)


def test_the_pinned_counts_are_unchanged(table):
    assert sum("k_gpipe" in k for k in table) == 2
    assert sum("k_gdec" in k for k in table) == 1
    assert sum("k_vpipe" in k for k in table) == 2
    assert sum("k_vdec" in k for k in table) == 1
    assert sum("k_wset" in k for k in table) == 3
