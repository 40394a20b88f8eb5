"""The eight line-store forms of k_rows / k_lanes (ZPQ_FLAG_LINESTORE), read from the gfx950 code object's metadata (no GPU):
they exist -- both directions, hash chain in registers (VMH) and interpreter, no state hand-over form --, the probe has cost
them no spill beyond their dense twins', and no pinned count of another kernel name has moved.  Template arguments in the
names: <DEC, KEEP, SP, VMH>."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from kernel_stats import kernel_table  # noqa: E402

TAIL = "EEEv6DBatchNS_4LCfgE"


@pytest.fixture(scope="module")
def table(zpq):
    zpq.lib()
    return kernel_table()


def form(table, kernel, dec, keep, sp, vmh):
    key = "%sI%s%s" % (kernel, "".join("Lb%dE" % int(x) for x in (dec, keep, sp, vmh)), TAIL[1:])
    found = [k for k in table if key in k]
    assert len(found) == 1, (key, found)
    return table[found[0]]


def test_eight_store_forms_within_their_dense_twins_limits(table):
    lanes = [k for k in table if "k_lanesI" in k or "k_rowsI" in k]
    assert len(lanes) == 24, sorted(lanes)                       # 16 dense (plain and state hand-over) and 8 on the store
    store = [k for k in lanes if k.split("I", 1)[1][8:12] == "Lb1E"]
    assert len(store) == 8, sorted(store)
    assert not any(k.split("I", 1)[1][4:8] == "Lb1E" for k in store), store      # no KEEP form on the store
    for kernel, bound in (("k_rows", {True: 128, False: 256}), ("k_lanes", {True: 128, False: 128})):
        for dec in (False, True):
            vmh = form(table, kernel, dec, False, True, True)
            assert vmh["scratch"] == 0 and vmh["vgpr"] <= bound[True], (kernel, dec, vmh)
            vm, twin = form(table, kernel, dec, False, True, False), form(table, kernel, dec, False, False, False)
            # (__launch_bounds__(256, VMH ? 4 : 2) for k_rows, (256, 4) for k_lanes: 128 or 256 registers a lane)
            assert vm["scratch"] <= twin["scratch"] and vm["vgpr"] <= bound[False], (kernel, dec, vm, twin)


def test_the_pinned_counts_are_unchanged(table):
    for name, count in (("k_gpipe", 2), ("k_gdec", 1), ("k_vpipe", 2), ("k_vdec", 1), ("k_wset", 3), ("k_vset", 3),
                        ("k_chain", 50), ("k_pipeI", 22), ("k_pipe2", 4), ("k_dpipe", 3), ("k_generic", 2)):
        assert sum(name in k for k in table) == count, (name, sorted(k for k in table if name in k))
    # the hash-chain forms of k_lanes that tests/test_kernel_resources.py finds by their last template argument: now six
    vmh = [k for k in table if "k_lanes" in k and k.endswith("Lb1" + TAIL)]
    assert len(vmh) == 6 and all(table[k]["scratch"] == 0 for k in vmh), vmh
