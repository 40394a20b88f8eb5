"""ZPQ_SET_LANES on the host (no GPU): the entry points exist and check their arguments, the predicate that tells whether a
set of a model is coded on the lane-per-component kernels (no chain kernel takes it, at most 64 components), and how the
ZPQ_SET_LANES environment variable is read."""
import ctypes as C
import os
import sys

import pytest

import general_models as GM

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from inputs import C4B  # noqa: E402

E_ARG = -2
SET_LANES = 1


@pytest.fixture
def no_knobs(monkeypatch):
    for k in ("ZPQ_SET_LANES", "ZPQ_LANES_ROWS", "ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _lib(zpq):
    L = zpq.lib()
    L.zpq_chain_blocks_per_wg.argtypes = [C.c_void_p]
    L.zpq_chain_blocks_per_wg.restype = C.c_int
    return L


def test_symbols(zpq):
    L = zpq.lib()
    for name in ("zpq_blockset_create_ex", "zpq_blockset_capacity_ex", "zpq_blockset_flags", "zpq_blockset_lanes_applies",
                 "zpq_blockset_resolve_flags", "zpq_blockset_create", "zpq_blockset_capacity"):
        assert getattr(L, name)
    assert zpq.SET_LANES == SET_LANES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zpaq_hip.h")).read()
    assert "#define ZPQ_SET_LANES 1u" in header
    for name in ("zpq_blockset_create_ex", "zpq_blockset_capacity_ex", "zpq_blockset_flags", "zpq_blockset_lanes_applies"):
        assert name + "(" in header, name


def test_argument_checks_need_no_device(zpq, no_knobs):
    L = zpq.lib()
    m = zpq.Model(header=C4B)
    for ctx, flags in ((None, 0), (None, SET_LANES), (None, 2), (None, 0x80000001)):
        out = C.c_void_p(0x1234)                             # must come back NULL
        assert L.zpq_blockset_create_ex(ctx, m.h, 3, 0, flags, C.byref(out)) == E_ARG
        assert out.value is None
        assert L.zpq_blockset_capacity_ex(ctx, m.h, 0, flags) == E_ARG
    assert L.zpq_blockset_create_ex(None, m.h, 3, 0, 0, None) == E_ARG
    assert L.zpq_blockset_flags(None) == 0
    assert L.zpq_blockset_lanes_applies(None) == 0
    # unknown flag bits are refused by the host-only form too
    for flags in (2, 3, 0x100, 0x80000000):
        assert L.zpq_blockset_resolve_flags(m.h, flags) == E_ARG, flags
    assert L.zpq_blockset_resolve_flags(None, 0) == E_ARG
    m.close()


@pytest.mark.parametrize("name", sorted(GM.NAMED))
def test_predicate_on_named_models(zpq, no_knobs, name):
    """True exactly where the lane kernels take the model (the route's `lanes` entry) and no chain kernel does."""
    L = _lib(zpq)
    hdr, want = GM.NAMED[name]
    m = zpq.Model(header=hdr)
    chain = L.zpq_chain_blocks_per_wg(m.h) > 0
    assert L.zpq_blockset_lanes_applies(m.h) == (1 if want[2] == 1 and not chain else 0), (name, want, chain)
    assert L.zpq_blockset_resolve_flags(m.h, SET_LANES) == (SET_LANES if want[2] == 1 and not chain else 0)
    assert L.zpq_blockset_resolve_flags(m.h, 0) == 0
    if name == "n65":
        assert L.zpq_blockset_lanes_applies(m.h) == 0
    if name in ("n17", "n64", "rates", "hm0", "fwd_n20"):
        assert L.zpq_blockset_lanes_applies(m.h) == 1
    m.close()


def test_predicate_on_shipped_levels_and_c4b(zpq, no_knobs):
    L = _lib(zpq)
    for level in (1, 2, 3, 4, 5):
        m = zpq.Model(level=level)
        assert L.zpq_chain_blocks_per_wg(m.h) > 0
        assert L.zpq_blockset_lanes_applies(m.h) == 0, level
        assert L.zpq_blockset_resolve_flags(m.h, SET_LANES) == 0, level
        m.close()
    m = zpq.Model(header=C4B)
    assert L.zpq_blockset_lanes_applies(m.h) == 1 and L.zpq_blockset_resolve_flags(m.h, SET_LANES) == SET_LANES
    m.close()


def test_environment(zpq, no_knobs):
    """ZPQ_SET_LANES=1 makes the request, =0 withdraws it, anything but a leading 0 / 1 decides nothing."""
    L = zpq.lib()
    general, chain = zpq.Model(header=C4B), zpq.Model(level=2)
    table = ((None, 0, 0), (None, 1, 1), ("1", 0, 1), ("1", 1, 1), ("0", 0, 0), ("0", 1, 0), ("x", 0, 0), ("x", 1, 1), ("", 1, 1),
             ("", 0, 0), ("10", 0, 1), ("01", 1, 0), ("yes", 0, 0))
    for env, flags, want in table:
        if env is None:
            no_knobs.delenv("ZPQ_SET_LANES", raising=False)
        else:
            no_knobs.setenv("ZPQ_SET_LANES", env)
        assert L.zpq_blockset_resolve_flags(general.h, flags) == want, (env, flags)
        assert L.zpq_blockset_resolve_flags(chain.h, flags) == 0, (env, flags)      # a chain model: it decides nothing
        assert L.zpq_blockset_resolve_flags(general.h, 2) == E_ARG
    general.close()
    chain.close()


@pytest.mark.parametrize("what", ["fwd_isse", "fwd_avg"])
def test_the_gpu_cases_tell_a_kept_p_from_a_zeroed_one(no_knobs, what):
    """The reference keeps p[], the last bit's predictions, across segments (Predictor.reset does not touch it), and so does
    the oracle.  In fwd_isse and fwd_avg a component reads a LATER component's prediction and feeds the coded one: the
    first bit of a segment is coded with what was predicted for the last bit of the segment before.  On members that
    test_gpu_set_lanes.py::test_parity codes for these models, the Python reference with p[] zeroed between segments
    writes other bytes than the oracle does: a set that dropped p[] would fail those cases."""
    import oracle_lib as O
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "pyref"))
    import zpaq_pyref as P
    from test_gpu_lanes import MODELS, hdr as lanes_hdr
    from test_gpu_set_lanes import parity_members
    hdr = lanes_hdr(MODELS[what])
    assert GM.has_forward_reference(hdr)
    members = [segs for segs in parity_members(what) if len(segs) >= 2 and sum(map(len, segs)) <= 700]
    assert len(members) >= 3
    differ = 0
    for segs in members[:4]:
        codec, kept, zeroed = O.Codec(hdr), P.new_model(hdr), P.new_model(hdr)
        want = [codec.encode(s, pp=True) for s in segs]
        assert [P.encode_segment(kept, s) for s in segs] == want
        other = []
        for s in segs:
            zeroed.p = [0] * len(zeroed.p)
            other.append(P.encode_segment(zeroed, s))
        assert other[0] == want[0]
        differ += other != want
    assert differ >= 1
