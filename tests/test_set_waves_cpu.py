"""ZPQ_SET_WAVES on the host (no GPU): the flag and its predicate exist, the predicate is the lanes predicate and the envelope of
BOTH wave-per-component kernels taken from the model's shape alone, the request is resolved on its own and honoured only on
top of ZPQ_SET_LANES, unknown bits stay refused -- and the input of the GPU test's MATCH case can tell a MATCH state that was
handed from segment to segment from one that was dropped."""
import ctypes as C
import itertools
import os
import sys

import pytest

import general_models as GM

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from inputs import C4B  # noqa: E402

E_ARG = -2
SET_LANES, SET_PIPE, SET_WAVES = 1, 4, 16
KNOBS = ("ZPQ_SET_LANES", "ZPQ_SET_PIPE", "ZPQ_SET_WAVES", "ZPQ_LANES_ROWS", "ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE", "ZPQ_ENC_PIPE")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _lib(zpq):
    L = zpq.lib()
    L.zpq_blockset_waves_applies.argtypes = [C.c_void_p]
    L.zpq_blockset_waves_applies.restype = C.c_int
    return L


def test_header_and_symbols(zpq):
    L = _lib(zpq)
    assert L.zpq_blockset_waves_applies
    assert zpq.SET_WAVES == SET_WAVES and zpq.SET_LANES == SET_LANES and zpq.SET_PIPE == SET_PIPE
    header = open(os.path.join(ROOT, "include", "zpaq_hip.h")).read()
    assert "#define ZPQ_SET_WAVES 16u" in header
    assert "int zpq_blockset_waves_applies(const zpq_model *);" in header
    assert "ZPQ_GDEC_BPW is ignored" in header
    assert L.zpq_blockset_waves_applies(None) == 0


def _models(zpq):
    for name in sorted(GM.NAMED):
        yield name, zpq.Model(header=GM.NAMED[name][0]), GM.NAMED[name][1]
    yield "C4B", zpq.Model(header=C4B), GM.PIPE
    for level in (1, 2, 3, 4, 5):
        yield "level%d" % level, zpq.Model(level=level), None


def test_predicate_is_lanes_and_both_envelopes(zpq, no_knobs):
    """waves_applies == lanes_applies and gpipe_applies and gdec_applies with the environment clean: 1 for the PIPE class
    (but for ht_bits0, which a chain kernel takes), 0 for ROWS_ONLY, LANES_ONLY, GENERIC_ONLY and the shipped levels.  The
    per-call knobs ZPQ_ENC_GPIPE / ZPQ_DEC_GPIPE, which switch the route predicates off, do not move it."""
    L = _lib(zpq)
    seen = {0: 0, 1: 0}
    for name, m, cls in _models(zpq):
        for k in ("ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE"):
            no_knobs.delenv(k, raising=False)
        route = GM.route(zpq, m)
        lanes = L.zpq_blockset_lanes_applies(m.h)
        want = 1 if lanes and route[0] and route[1] else 0
        assert L.zpq_blockset_waves_applies(m.h) == want, (name, route, lanes)
        if cls is None:
            assert want == 0 and lanes == 0, name                 # a chain model
        elif cls == GM.PIPE:
            assert route[:2] == (1, 1) and want == lanes, name    # (lanes == 0 only for a PIPE model a chain kernel takes)
        else:
            assert want == 0, name
        for k in ("ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE"):
            no_knobs.setenv(k, "0")
            assert GM.route(zpq, m)[0 if "ENC" in k else 1] == 0, (name, k)
            assert L.zpq_blockset_waves_applies(m.h) == want, (name, k)
        seen[want] += 1
        m.close()
    assert seen[1] >= 20 and seen[0] >= 20, seen
    for name in ("n16", "mix9", "ring138", "match_buf0", "hh_small", "n17", "n64", "n65", "perturbed_rows"):
        m = zpq.Model(header=GM.NAMED[name][0])
        assert L.zpq_blockset_waves_applies(m.h) == 0, name
        m.close()


ENV_WAVES = (None, "1", "0", "x", "")
ENV_LANES = (None, "1", "0")
FLAGS = (0, 1, 16, 17, 4, 5, 20, 21)


def _request(env, flags, bit):
    """set_request: a leading 0 / 1 in the environment decides, anything else leaves it to the flag."""
    if env is not None and env[:1] in ("0", "1"):
        return env[0] == "1"
    return bool(flags & bit)


def _table(zpq, no_knobs, model, lanes_ok, waves_ok, pipe_ok):
    L = _lib(zpq)
    got = set()
    for flags, ew, el in itertools.product(FLAGS, ENV_WAVES, ENV_LANES):
        for var, val in (("ZPQ_SET_WAVES", ew), ("ZPQ_SET_LANES", el)):
            if val is None:
                no_knobs.delenv(var, raising=False)
            else:
                no_knobs.setenv(var, val)
        lanes = lanes_ok and _request(el, flags, SET_LANES)
        waves = lanes and waves_ok and _request(ew, flags, SET_WAVES)
        pipe = pipe_ok and bool(flags & SET_PIPE)
        want = (SET_LANES if lanes else 0) | (SET_WAVES if waves else 0) | (SET_PIPE if pipe else 0)
        res = L.zpq_blockset_resolve_flags(model.h, flags)
        assert res == want, (flags, ew, el, res, want)
        got.add(res)
    return got


def test_resolve_flags_on_a_pipe_class_model(zpq, no_knobs):
    """17 only where both requests are in force, else 1 or 0: ZPQ_SET_WAVES alone decides nothing."""
    for header in (C4B, GM.NAMED["mix_x4"][0]):
        m = zpq.Model(header=header)
        assert _table(zpq, no_knobs, m, True, True, False) == {0, 1, 17}
        for k in ("ZPQ_SET_WAVES", "ZPQ_SET_LANES"):
            no_knobs.delenv(k, raising=False)
        L = _lib(zpq)
        assert [L.zpq_blockset_resolve_flags(m.h, f) for f in FLAGS] == [0, 1, 0, 17, 0, 1, 0, 17]
        no_knobs.setenv("ZPQ_SET_WAVES", "1")                   # the variable alone: still nothing without ZPQ_SET_LANES
        assert [L.zpq_blockset_resolve_flags(m.h, f) for f in FLAGS] == [0, 17, 0, 17, 0, 17, 0, 17]
        no_knobs.setenv("ZPQ_SET_LANES", "1")
        assert [L.zpq_blockset_resolve_flags(m.h, f) for f in FLAGS] == [17] * 8
        no_knobs.setenv("ZPQ_SET_WAVES", "0")
        assert [L.zpq_blockset_resolve_flags(m.h, f) for f in FLAGS] == [1] * 8
        m.close()


def test_resolve_flags_on_a_rows_only_model(zpq, no_knobs):
    for name in ("n16", "n17", "hh_small"):
        m = zpq.Model(header=GM.NAMED[name][0])
        assert _table(zpq, no_knobs, m, True, False, False) == {0, 1}      # never 16
        m.close()


def test_resolve_flags_on_level_2(zpq, no_knobs):
    m = zpq.Model(level=2)
    assert _table(zpq, no_knobs, m, False, False, True) == {0, 4}          # only ZPQ_SET_PIPE can come back
    m.close()


def test_unknown_bits_stay_refused(zpq, no_knobs):
    L = _lib(zpq)
    m = zpq.Model(header=C4B)
    for flags in (2, 8, 32, 0x100, 18, 24, 0x80000010):
        out = C.c_void_p(0x1234)
        assert L.zpq_blockset_create_ex(None, m.h, 3, 0, flags, C.byref(out)) == E_ARG and out.value is None, flags
        assert L.zpq_blockset_capacity_ex(None, m.h, 0, flags) == E_ARG, flags
        assert L.zpq_blockset_resolve_flags(m.h, flags) == E_ARG, flags
    for flags in (16, 17):                                       # not refused for the flags themselves
        assert L.zpq_blockset_resolve_flags(m.h, flags) in (0, 17), flags
        out = C.c_void_p(0x1234)
        assert L.zpq_blockset_create_ex(None, m.h, 3, 0, flags, C.byref(out)) == E_ARG and out.value is None   # (the NULL ctx)
        assert L.zpq_blockset_create_ex(None, m.h, 3, 0, flags, None) == E_ARG
    m.close()


def test_the_binding_surfaces_the_library_error(zpq, no_knobs):
    """Without a device: BlockSet(..., waves=True) and blockset_capacity(..., waves=True) reach the library, which refuses the
    closed context -- a ZpqError, not an AttributeError from a binding that does not know the argument."""
    import inspect
    assert "waves" in inspect.signature(zpq.BlockSet.__init__).parameters
    assert "waves" in inspect.signature(zpq.Context.blockset_capacity).parameters
    assert isinstance(zpq.BlockSet.waves, property) and zpq.BlockSet.waves.fset is None

    class NoCtx:
        h = None
        _children = set()
    m = zpq.Model(header=C4B)
    with pytest.raises(zpq.ZpqError) as e:
        zpq.BlockSet(NoCtx(), m, 2, waves=True)
    assert e.value.code == E_ARG
    with pytest.raises(zpq.ZpqError) as e:
        zpq.Context.blockset_capacity(NoCtx(), m, waves=True)
    assert e.value.code == E_ARG
    m.close()


@pytest.mark.parametrize("what", ["match_idx_gt_buf"])
def test_the_gpu_case_tells_a_kept_match_state_from_a_dropped_one(no_knobs, what):
    """MATCH's a (length), b (offset), c (predicted bit), limit (buffer position) and cxt outlive a segment in the reference.
    On members that test_gpu_set_waves.py::test_match_across_segments codes -- later segments repeat the earlier ones'
    content -- the Python reference with those five zeroed between segments writes other bytes than the oracle for a later
    segment (rounds 0-2 of the members short enough for it): a hand-over that lost them would fail that case.
    (The GPU case's other model, bits0_all, cannot show it on any input: its last component is an SSE whose row lies beyond
    its 32-entry table from a block's second byte on, so it predicts 0 whatever MATCH says -- quirk Q10, general_models.py.
    It is there for the smallest MATCH the wave kernels take: a two-byte buffer and a one-entry index.)"""
    import oracle_lib as O
    sys.path.insert(0, os.path.join(ROOT, "oracle", "pyref"))
    import zpaq_pyref as P
    from test_gpu_set_waves import match_members
    hdr = GM.NAMED[what][0]
    match_at = [i for i, c in enumerate(GM.components(hdr)) if c[0] == GM.MATCH]
    assert match_at
    members = [segs[:3] for segs in match_members(what) if sum(map(len, segs[:3])) <= 1300][:3]    # (the Python reference is slow)
    assert len(members) >= 2
    differ = 0
    for segs in members:
        codec, kept, dropped = O.Codec(hdr), P.new_model(hdr), P.new_model(hdr)
        want = [codec.encode(s, pp=True) for s in segs]
        assert [P.encode_segment(kept, s) for s in segs] == want
        other = []
        for k, s in enumerate(segs):
            for i in match_at if k else ():                     # (between segments: the first one starts from Predictor.init)
                c = dropped.comp[i]
                c.a = c.b = c.c = c.limit = c.cxt = 0
            other.append(P.encode_segment(dropped, s))
        assert other[0] == want[0]
        differ += other != want
    assert differ >= 1
