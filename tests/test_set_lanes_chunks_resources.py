"""What the pause (ZPQ_SET_CHUNKS) cost the eight state hand-over forms of k_rows / k_lanes, read from the gfx950 code object's
metadata (no GPU): no new form, every one within its launch bound, none with more scratch than it had before the pause, the
hash-chain forms of k_lanes still with none.  Template arguments in the names: <DEC, KEEP, SP, VMH>."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from kernel_stats import kernel_table  # noqa: E402

TAIL = "EEv6DBatchNS_4LCfgE"
# scratch bytes (private_segment_fixed_size) of the KEEP forms as tools/kernel_stats.py printed them for a build of the commit
# before the pause went in ("State the hash-row lookup, the store probe and hash programs once"), same compiler, same flags:
# (kernel, DEC, VMH) -> bytes.  Their VGPRs then: k_rows 144 / 124 / 148 / 127, k_lanes 127 / 109 / 127 / 109.
SCRATCH_BEFORE = {("k_rows", 0, 0): 0, ("k_rows", 0, 1): 0, ("k_rows", 1, 0): 0, ("k_rows", 1, 1): 0,
                  ("k_lanes", 0, 0): 12, ("k_lanes", 0, 1): 0, ("k_lanes", 1, 0): 12, ("k_lanes", 1, 1): 0}


@pytest.fixture(scope="module")
def table(zpq):
    zpq.lib()
    return kernel_table()


def form(table, kernel, dec, keep, sp, vmh):
    key = "%sI%s%s" % (kernel, "".join("Lb%dE" % int(x) for x in (dec, keep, sp, vmh)), TAIL)
    found = [k for k in table if key in k]
    assert len(found) == 1, (key, found)
    return table[found[0]]


def test_still_twenty_four_forms(table):
    lanes = [k for k in table if "k_lanesI" in k or "k_rowsI" in k]
    assert len(lanes) == 24, sorted(lanes)
    keep = [k for k in lanes if k.split("I", 1)[1][4:8] == "Lb1E"]
    assert len(keep) == 8 and all(k.split("I", 1)[1].count("Lb") == 4 for k in lanes), sorted(keep)   # four template arguments


@pytest.mark.parametrize("kernel,dec,vmh", sorted(SCRATCH_BEFORE))
def test_a_keep_form_within_its_bounds(table, kernel, dec, vmh):
    f = form(table, kernel, dec, True, False, vmh)
    # __launch_bounds__(256, VMH ? 4 : 2) for k_rows, (256, 4) for k_lanes: 128 or 256 registers a lane
    bound = 256 if kernel == "k_rows" and not vmh else 128
    assert f["vgpr"] <= bound, (kernel, dec, vmh, f)
    assert f["scratch"] <= SCRATCH_BEFORE[(kernel, dec, vmh)], (kernel, dec, vmh, f)
    if kernel == "k_lanes" and vmh:
        assert f["scratch"] == 0, f
