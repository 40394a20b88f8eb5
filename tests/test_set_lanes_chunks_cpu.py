"""ZPQ_SET_CHUNKS (128) on the host (no GPU): a request on top of ZPQ_SET_LANES that lets the chunk calls code such a set.  It
is honoured exactly where ZPQ_SET_LANES is in force, decides nothing anywhere else, changes no result for flags without it, and
has no environment variable; the bits that were refused stay refused; the binding passes it on."""
import ctypes as C
import os
import sys

import pytest

import general_models as GM
import vpipe_models as VM

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from inputs import C4B  # noqa: E402

E_ARG = -2
SET_LANES, SET_PIPE, SET_WAVES, SET_VMWAVES, SET_CHUNKS = 1, 4, 16, 64, 128
FLAGS = (128, 129, 145, 193, 209, 132)


@pytest.fixture
def no_knobs(monkeypatch):
    for k in ("ZPQ_SET_LANES", "ZPQ_SET_PIPE", "ZPQ_SET_WAVES", "ZPQ_SET_VMWAVES", "ZPQ_SET_CHUNKS", "ZPQ_LANES_ROWS",
              "ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_the_flag_is_declared(zpq):
    assert zpq.SET_CHUNKS == SET_CHUNKS
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zpaq_hip.h")).read()
    assert "#define ZPQ_SET_CHUNKS 128u" in header


def test_resolve_flags(zpq, no_knobs):
    L = zpq.lib()
    models = {"C4B": zpq.Model(header=C4B), "C4B_VM": zpq.Model(header=VM.C4B_VM), "level2": zpq.Model(level=2),
              "n65": zpq.Model(header=GM.NAMED["n65"][0])}
    want = {"C4B": [0, 129, 145, 129, 145, 0],                # the hash chain: ZPQ_SET_WAVES applies, ZPQ_SET_VMWAVES does not
            "C4B_VM": [0, 129, 129, 193, 193, 0],             # any other program: the other way round
            "level2": [0, 0, 0, 0, 0, 4],                     # a chain model: only ZPQ_SET_PIPE can come back
            "n65": [0] * 6}                                   # 65 components: no lane kernel takes it
    try:
        for name, m in models.items():
            got = [L.zpq_blockset_resolve_flags(m.h, f) for f in FLAGS]
            assert got == want[name], (name, got)
            for f in FLAGS:                                   # without bit 128: what it was, and what bit 128 is added to
                plain = L.zpq_blockset_resolve_flags(m.h, f & ~SET_CHUNKS)
                assert plain >= 0 and not plain & SET_CHUNKS
                with_it = L.zpq_blockset_resolve_flags(m.h, f)
                assert with_it == (plain | SET_CHUNKS if plain & SET_LANES else plain), (name, f, plain, with_it)
        assert L.zpq_blockset_resolve_flags(models["C4B"].h, SET_CHUNKS) == 0     # alone it decides nothing
    finally:
        for m in models.values():
            m.close()


def test_the_environment_makes_no_such_request(zpq, no_knobs):
    """ZPQ_SET_LANES=1 in the environment puts ZPQ_SET_LANES in force, and bit 128 of the flags is then honoured; no variable
    makes the request itself"""
    L = zpq.lib()
    m = zpq.Model(header=C4B)
    try:
        no_knobs.setenv("ZPQ_SET_CHUNKS", "1")
        assert [L.zpq_blockset_resolve_flags(m.h, f) for f in (0, 1, 17, 128)] == [0, 1, 17, 0]
        no_knobs.setenv("ZPQ_SET_LANES", "1")
        assert [L.zpq_blockset_resolve_flags(m.h, f) for f in (0, 1, 128, 144)] == [1, 1, 129, 145]
        no_knobs.setenv("ZPQ_SET_LANES", "0")
        assert [L.zpq_blockset_resolve_flags(m.h, f) for f in (129, 145)] == [0, 0]
    finally:
        m.close()


def test_the_refused_bits_stay_refused(zpq, no_knobs):
    L = zpq.lib()
    m = zpq.Model(header=C4B)
    try:
        for flags in (2, 8, 32, 0x100, 0x80000080, 130, 136, 160, 0x180):
            out = C.c_void_p(0x1234)
            assert L.zpq_blockset_create_ex(None, m.h, 3, 0, flags, C.byref(out)) == E_ARG and out.value is None, flags
            assert L.zpq_blockset_capacity_ex(None, m.h, 0, flags) == E_ARG, flags
            assert L.zpq_blockset_resolve_flags(m.h, flags) == E_ARG, flags
        for flags in (128, 129, 145, 193):                    # not refused for the flags themselves
            assert L.zpq_blockset_resolve_flags(m.h, flags) >= 0, flags
    finally:
        m.close()


def test_the_binding_passes_the_request_on(zpq, no_knobs, monkeypatch):
    """BlockSet(..., chunks=True) reaches zpq_blockset_create_ex with ZPQ_SET_LANES | ZPQ_SET_CHUNKS"""
    seen = []

    class Lib:
        def zpq_blockset_create_ex(self, ctx, model, n, promise, flags, out):
            seen.append((n, promise, flags))
            return 0

        def zpq_blockset_flags(self, h):
            return seen[-1][2]

    class Ctx:
        h = None
        _children = set()

    class Model:
        h = None

    import zpaq_v_amd.binding as B
    monkeypatch.setattr(B, "lib", lambda: Lib())
    for kw, want in (({"chunks": True}, 129), ({"lanes": True, "chunks": True}, 129), ({"waves": True, "chunks": True}, 145),
                     ({"vmwaves": True, "chunks": True}, 193), ({"lanes": True}, 1), ({}, 0)):
        st = B.BlockSet(Ctx(), Model(), 3, **kw)
        assert seen[-1] == (3, 0, want), (kw, seen[-1])
        assert st.chunks == bool(want & SET_CHUNKS) and st.lanes == bool(want & SET_LANES)
        st.h = None                                           # (nothing to destroy)
    assert B._set_flags(False, False, False) == 0 and B._set_flags(True, False, True, False) == 17
