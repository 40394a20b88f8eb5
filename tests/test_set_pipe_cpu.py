"""ZPQ_SET_PIPE on the host (no GPU): the request that sends a chain-model set's encode calls to the wave-pipelined encoder.
The predicate looks at the model's shape alone (one of the five chains k_pipe codes), the two requests of a set are resolved
independently, the environment variable is read like ZPQ_SET_LANES, and every answer without the request is the one the
library gave before it existed."""
import ctypes as C
import os
import sys

import pytest

import chain_models as CM
import general_models as GM

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from inputs import C4B  # noqa: E402

E_ARG = -2
SET_LANES, SET_PIPE = 1, 4
PIPE_NAMED = ("l2_mixed", "l2_hh2_hm1", "l1_sizes", "l3_mixed", "l4_rate255", "l4_rate0", "l5_small")


@pytest.fixture
def no_knobs(monkeypatch):
    for k in ("ZPQ_SET_PIPE", "ZPQ_SET_LANES", "ZPQ_ENC_PIPE", "ZPQ_ENC_SPLIT", "ZPQ_CHAIN_G", "ZPQ_LANES_ROWS"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_symbols(zpq):
    L = zpq.lib()
    assert L.zpq_blockset_pipe_applies
    assert zpq.SET_PIPE == SET_PIPE and zpq.SET_LANES == SET_LANES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zpaq_hip.h")).read()
    assert "#define ZPQ_SET_PIPE 4u" in header and "zpq_blockset_pipe_applies(" in header
    assert L.zpq_blockset_pipe_applies(None) == 0


def test_predicate_on_shipped_levels_and_c4b(zpq, no_knobs):
    L = zpq.lib()
    for level in (1, 2, 3, 4, 5):
        m = zpq.Model(level=level)
        assert L.zpq_blockset_pipe_applies(m.h) == 1, level
        assert L.zpq_blockset_resolve_flags(m.h, SET_PIPE) == SET_PIPE, level
        assert L.zpq_blockset_resolve_flags(m.h, SET_PIPE | SET_LANES) == SET_PIPE, level
        m.close()
    m = zpq.Model(header=C4B)
    assert L.zpq_blockset_pipe_applies(m.h) == 0
    assert L.zpq_blockset_resolve_flags(m.h, SET_PIPE) == 0
    assert L.zpq_blockset_resolve_flags(m.h, SET_PIPE | SET_LANES) == SET_LANES
    m.close()


@pytest.mark.parametrize("name", sorted(CM.NAMED))
def test_predicate_on_named_chain_models(zpq, no_knobs, name):
    """1 exactly for the routes whose nch_spec is 2, 3 or 5 without a MIX2, or 6 or 8 with one."""
    L = zpq.lib()
    hdr, want = CM.NAMED[name]
    m = zpq.Model(header=hdr)
    shape = want is not None and ((want[0] in (2, 3, 5) and not want[3]) or (want[0] in (6, 8) and want[3] == 1))
    assert shape == (name in PIPE_NAMED), (name, want)
    rt = CM.route(zpq, m)
    assert CM.route_key(rt) == want                           # (the route the predicate is derived from is the expected one)
    assert L.zpq_blockset_pipe_applies(m.h) == (1 if shape else 0), (name, want)
    assert L.zpq_blockset_resolve_flags(m.h, SET_PIPE) == (SET_PIPE if shape else 0), name
    assert L.zpq_blockset_resolve_flags(m.h, 0) == 0, name
    if shape:
        assert L.zpq_blockset_lanes_applies(m.h) == 0, name   # no model can have both
    m.close()


def test_runtime_loop_routes_are_not_taken(zpq, no_knobs):
    L = zpq.lib()
    for name in ("l2_hm0", "chain7", "l4_mask15", "mix2_chain3", "chain16", "chain17", "isse_j_skip"):
        m = zpq.Model(header=CM.NAMED[name][0])
        assert L.zpq_blockset_pipe_applies(m.h) == 0, name
        m.close()


@pytest.mark.parametrize("name", sorted(GM.NAMED))
def test_predicate_on_general_models(zpq, no_knobs, name):
    """A general model never gets the pipeline; its ZPQ_SET_LANES answer is not touched by the other request."""
    L = zpq.lib()
    m = zpq.Model(header=GM.NAMED[name][0])
    lanes = L.zpq_blockset_resolve_flags(m.h, SET_LANES)
    if not L.zpq_blockset_pipe_applies(m.h):
        assert L.zpq_blockset_resolve_flags(m.h, SET_PIPE) == 0
        assert L.zpq_blockset_resolve_flags(m.h, SET_PIPE | SET_LANES) == lanes
    else:                                                    # (a chain-shaped entry of that table)
        assert lanes == 0 and L.zpq_blockset_resolve_flags(m.h, SET_PIPE | SET_LANES) == SET_PIPE
    m.close()


def test_environment(zpq, no_knobs):
    """ZPQ_SET_PIPE=1 makes the request, =0 withdraws it, anything but a leading 0 / 1 decides nothing."""
    L = zpq.lib()
    general, chain = zpq.Model(header=C4B), zpq.Model(level=2)
    table = ((None, 0, 0), (None, 4, 4), ("1", 0, 4), ("1", 4, 4), ("0", 0, 0), ("0", 4, 0), ("x", 0, 0), ("x", 4, 4), ("", 4, 4),
             ("", 0, 0), ("10", 0, 4), ("01", 4, 0), ("yes", 0, 0))
    for env, flags, want in table:
        if env is None:
            no_knobs.delenv("ZPQ_SET_PIPE", raising=False)
        else:
            no_knobs.setenv("ZPQ_SET_PIPE", env)
        assert L.zpq_blockset_resolve_flags(chain.h, flags) == want, (env, flags)
        assert L.zpq_blockset_resolve_flags(general.h, flags) == 0, (env, flags)       # no chain model: it decides nothing
        assert L.zpq_blockset_resolve_flags(general.h, flags | SET_LANES) == SET_LANES, (env, flags)
        assert L.zpq_blockset_resolve_flags(chain.h, 2) == E_ARG
    # the two variables are independent
    no_knobs.setenv("ZPQ_SET_PIPE", "1")
    no_knobs.setenv("ZPQ_SET_LANES", "1")
    assert L.zpq_blockset_resolve_flags(chain.h, 0) == SET_PIPE and L.zpq_blockset_resolve_flags(general.h, 0) == SET_LANES
    no_knobs.setenv("ZPQ_SET_LANES", "0")
    assert L.zpq_blockset_resolve_flags(chain.h, 0) == SET_PIPE and L.zpq_blockset_resolve_flags(general.h, 5) == 0
    general.close()
    chain.close()


def test_unknown_bits_are_still_refused(zpq, no_knobs):
    L = zpq.lib()
    m = zpq.Model(level=2)
    for flags in (2, 6, 8, 0x100, 3, 7, 0x80000000, 0x80000004):
        assert L.zpq_blockset_resolve_flags(m.h, flags) == E_ARG, flags
        out = C.c_void_p(0x1234)
        assert L.zpq_blockset_create_ex(None, m.h, 3, 0, flags, C.byref(out)) == E_ARG and out.value is None, flags
        assert L.zpq_blockset_capacity_ex(None, m.h, 0, flags) == E_ARG, flags
    for flags in (0, 1, 4, 5):                               # known bits: the NULL ctx is what is refused, not the flags
        assert L.zpq_blockset_resolve_flags(m.h, flags) >= 0, flags
    m.close()


def test_answers_without_the_request_are_unchanged(zpq, no_knobs):
    """Without the variable and without bit 2: 0 for every chain model, ZPQ_SET_LANES where the lane kernels apply."""
    L = zpq.lib()
    for name in sorted(CM.NAMED):
        m = zpq.Model(header=CM.NAMED[name][0])
        applies = L.zpq_blockset_lanes_applies(m.h)
        assert L.zpq_blockset_resolve_flags(m.h, 0) == 0, name
        assert L.zpq_blockset_resolve_flags(m.h, SET_LANES) == (SET_LANES if applies else 0), name
        m.close()
    for name in sorted(GM.NAMED):
        m = zpq.Model(header=GM.NAMED[name][0])
        applies = L.zpq_blockset_lanes_applies(m.h)
        assert L.zpq_blockset_resolve_flags(m.h, 0) == 0, name
        assert L.zpq_blockset_resolve_flags(m.h, SET_LANES) == (SET_LANES if applies else 0), name
        m.close()
