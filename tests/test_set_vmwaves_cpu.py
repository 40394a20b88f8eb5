"""ZPQ_SET_VMWAVES on the host (no GPU): the flag and its predicate exist; the predicate is the lanes predicate and the envelope
of k_vpipe / k_vdec taken from the model's shape alone; the request is resolved on its own and honoured only on top of
ZPQ_SET_LANES; no model gets it together with ZPQ_SET_WAVES; flags without bit 64 resolve as they did; unknown bits stay
refused -- and the inputs of the GPU tests can tell a ZPAQL state (a b c d f, H, R, M) that was handed from segment to segment
from one that was dropped."""
import ctypes as C
import inspect
import itertools
import os
import random
import sys

import pytest

import general_models as GM
import oracle_lib as O
import vpipe_models as VM
import zpaql_programs as ZP

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from inputs import C4B  # noqa: E402

E_ARG = -2
SET_LANES, SET_PIPE, SET_WAVES, SET_VMWAVES = 1, 4, 16, 64
KNOBS = ("ZPQ_SET_LANES", "ZPQ_SET_PIPE", "ZPQ_SET_WAVES", "ZPQ_SET_VMWAVES", "ZPQ_LANES_ROWS", "ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE",
         "ZPQ_ENC_PIPE", "ZPQ_VM_PIPE")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("zpq_blockset_vmwaves_applies", "zpq_blockset_waves_applies", "zpq_blockset_lanes_applies", "zpq_blockset_resolve_flags",
           "zpq_blockset_create_ex", "zpq_blockset_capacity_ex", "zpq_blockset_flags", "zpq_launch_vset")


@pytest.fixture
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _lib(zpq):
    L = zpq.lib()
    for f in (L.zpq_blockset_vmwaves_applies, L.zpq_blockset_waves_applies):
        f.argtypes = [C.c_void_p]
        f.restype = C.c_int
    return L


def _model(zpq, header, offsets=None):
    return zpq.Model(header=header, offsets=offsets) if offsets else zpq.Model(header=header)


# ---------------------------------------------------------------- 1. header and exports
def test_header_and_exports(zpq):
    L = zpq.lib()
    for name in EXPORTS:
        assert getattr(L, name), name
    assert zpq.SET_VMWAVES == SET_VMWAVES and zpq.SET_WAVES == SET_WAVES and zpq.SET_LANES == SET_LANES and zpq.SET_PIPE == SET_PIPE
    header = open(os.path.join(ROOT, "include", "zpaq_hip.h")).read()
    assert "#define ZPQ_SET_VMWAVES 64u" in header
    assert "zpq_blockset_vmwaves_applies(" in header
    assert "k_vset<encode>" in header and "k_vsetd<decode>" in header


# ---------------------------------------------------------------- 2. the predicate
def test_predicate_inside_the_envelope(zpq, no_knobs):
    L = _lib(zpq)
    cases = [("C4B_VM", VM.C4B_VM, None), ("n14", *VM.lds_edge(0)), ("hh_small", GM.NAMED["hh_small"][0], None),
             ("hm0", GM.NAMED["hm0"][0], None)]
    assert VM.lds_edge(0)[0][4] == 14                              # n + 2 waves = 1024 threads
    cases += [(name, *ZP.embed(ZP.NAMED[name], "rows")) for name in sorted(ZP.NAMED)]
    assert len(cases) == 4 + len(ZP.NAMED)
    for name, hdr, offs in cases:
        m = _model(zpq, hdr, offs)
        assert L.zpq_blockset_vmwaves_applies(m.h) == 1, name
        assert L.zpq_blockset_waves_applies(m.h) == 0, name          # never both
        assert L.zpq_blockset_lanes_applies(m.h) == 1, name
        for k in ("ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE", "ZPQ_VM_PIPE", "ZPQ_SET_VMWAVES", "ZPQ_SET_LANES"):   # its shape alone
            no_knobs.setenv(k, "0")
            assert L.zpq_blockset_vmwaves_applies(m.h) == 1, (name, k)
            no_knobs.delenv(k)
        m.close()


def n15():
    """Fifteen components no chain kernel takes (fourteen CMs and a MIX) behind a program that is not the hash chain."""
    from chain_models import perturbed_hashchain
    return GM.H(GM.cms(14, 4, 9) + [[GM.MIX, 4, 0, 4, 24, 255]], 4, 8, perturbed_hashchain(15, random.Random(6)))


def test_predicate_outside_the_envelope(zpq, no_knobs):
    """The hash chain (C4B), the chain models, fifteen components, the 19 components of the `lanes` shape, NULL.
    VM.chain(14) and VM.chain(15) are ISSE chains: a chain kernel codes their sets (zpq_blockset_lanes_applies is 0), so
    ZPQ_SET_LANES is never in force for them and neither request decides anything, whatever zpq_vpipe_applies says."""
    L = _lib(zpq)
    assert L.zpq_blockset_vmwaves_applies(None) == 0
    for n, vpipe in ((14, 1), (15, 0)):
        m = zpq.Model(header=VM.chain(n))
        assert VM.applies(zpq, m) == (vpipe, vpipe) and L.zpq_blockset_lanes_applies(m.h) == 0
        assert L.zpq_blockset_vmwaves_applies(m.h) == 0 and L.zpq_blockset_resolve_flags(m.h, 65) == 0, n
        m.close()
    m = zpq.Model(header=n15())
    assert L.zpq_blockset_lanes_applies(m.h) == 1 and VM.applies(zpq, m) == (0, 0)
    assert L.zpq_blockset_vmwaves_applies(m.h) == 0 and L.zpq_blockset_resolve_flags(m.h, 65) == 1
    m.close()
    lanes19 = ZP.embed(ZP.NAMED["loop_count"], "lanes")
    assert lanes19[0][4] == 19
    outside = [("C4B", zpq.Model(header=C4B)), ("lanes19", _model(zpq, *lanes19)),
               ("mix3_sse3_n22_vm", zpq.Model(header=GM.NAMED["mix3_sse3_n22_vm"][0]))]
    outside += [("level%d" % lv, zpq.Model(level=lv)) for lv in (1, 2, 3, 4, 5)]
    for name, m in outside:
        assert L.zpq_blockset_vmwaves_applies(m.h) == 0, name
        m.close()
    m = zpq.Model(header=C4B)
    assert L.zpq_blockset_waves_applies(m.h) == 1                     # (the hash chain has its own request)
    m.close()


def test_predicate_follows_the_lds_formula(zpq, no_knobs):
    L = _lib(zpq)
    seen = set()
    for pad in (60, 68, 69, 70, 71, 78):
        hdr, offs = VM.lds_edge(pad)
        fits = max(VM.lds_bytes(hdr)) <= VM.LDS_MAX
        m = _model(zpq, hdr, offs)
        assert L.zpq_blockset_vmwaves_applies(m.h) == (1 if fits else 0), (pad, VM.lds_bytes(hdr))
        assert L.zpq_blockset_resolve_flags(m.h, 65) == (65 if fits else 1), pad
        seen.add(fits)
        m.close()
    assert seen == {True, False}
    assert VM.lds_bytes(VM.lds_edge(69)[0])[0] == VM.LDS_MAX and VM.lds_bytes(VM.lds_edge(70)[0])[0] == VM.LDS_MAX + 16


# ---------------------------------------------------------------- 3. resolve_flags
FLAGS = (0, 1, 16, 64, 65, 17, 81)
ENV_VMWAVES = (None, "1", "0", "x")
ENV_LANES = (None, "1", "0")


def _request(env, flags, bit):
    """set_request: a leading 0 / 1 in the environment decides, anything else leaves it to the flag."""
    if env is not None and env[:1] in ("0", "1"):
        return env[0] == "1"
    return bool(flags & bit)


def _table(zpq, no_knobs, model, lanes_ok, waves_ok, vmwaves_ok):
    L = _lib(zpq)
    got = set()
    for flags, ev, el in itertools.product(FLAGS, ENV_VMWAVES, ENV_LANES):
        for var, val in (("ZPQ_SET_VMWAVES", ev), ("ZPQ_SET_LANES", el)):
            if val is None:
                no_knobs.delenv(var, raising=False)
            else:
                no_knobs.setenv(var, val)
        lanes = lanes_ok and _request(el, flags, SET_LANES)
        waves = lanes and waves_ok and bool(flags & SET_WAVES)
        vmwaves = lanes and vmwaves_ok and _request(ev, flags, SET_VMWAVES)
        want = (SET_LANES if lanes else 0) | (SET_WAVES if waves else 0) | (SET_VMWAVES if vmwaves else 0)
        res = L.zpq_blockset_resolve_flags(model.h, flags)
        assert res == want, (flags, ev, el, res, want)
        got.add(res)
    for var in ("ZPQ_SET_VMWAVES", "ZPQ_SET_LANES"):
        no_knobs.delenv(var, raising=False)
    return got


def test_resolve_flags_on_an_interpreter_model(zpq, no_knobs):
    """65 only where both requests are in force, else 1 or 0: ZPQ_SET_VMWAVES alone decides nothing, ZPQ_SET_WAVES nothing at all."""
    L = _lib(zpq)
    for hdr, offs in ((VM.C4B_VM, None), ZP.embed(ZP.NAMED["loop_count"], "rows")):
        m = _model(zpq, hdr, offs)
        assert _table(zpq, no_knobs, m, True, False, True) == {0, 1, 65}
        assert [L.zpq_blockset_resolve_flags(m.h, f) for f in FLAGS] == [0, 1, 0, 0, 65, 1, 65]
        no_knobs.setenv("ZPQ_SET_VMWAVES", "1")                 # the variable alone: still nothing without ZPQ_SET_LANES
        assert [L.zpq_blockset_resolve_flags(m.h, f) for f in FLAGS] == [0, 65, 0, 0, 65, 65, 65]
        no_knobs.setenv("ZPQ_SET_LANES", "1")
        assert [L.zpq_blockset_resolve_flags(m.h, f) for f in FLAGS] == [65] * 7
        no_knobs.setenv("ZPQ_SET_VMWAVES", "0")
        assert [L.zpq_blockset_resolve_flags(m.h, f) for f in FLAGS] == [1] * 7
        no_knobs.delenv("ZPQ_SET_VMWAVES")
        no_knobs.delenv("ZPQ_SET_LANES")
        m.close()


def test_resolve_flags_on_c4b_and_level_2(zpq, no_knobs):
    L = _lib(zpq)
    m = zpq.Model(header=C4B)
    got = _table(zpq, no_knobs, m, True, True, False)
    assert got == {0, 1, 17} and not any(g & 64 for g in got)
    assert [L.zpq_blockset_resolve_flags(m.h, f) for f in FLAGS] == [0, 1, 0, 0, 1, 17, 17]
    m.close()
    m = zpq.Model(level=2)
    assert _table(zpq, no_knobs, m, False, False, False) == {0}
    for flags, ev in itertools.product((0, 4, 5, 68, 69, 85), ENV_VMWAVES):
        if ev is None:
            no_knobs.delenv("ZPQ_SET_VMWAVES", raising=False)
        else:
            no_knobs.setenv("ZPQ_SET_VMWAVES", ev)
        assert L.zpq_blockset_resolve_flags(m.h, flags) == (4 if flags & 4 else 0), (flags, ev)     # only ever 0 or 4
    m.close()


# ---------------------------------------------------------------- 4. flags without bit 64 resolve as they did
OLD_FLAGS = (0, 1, 16, 17, 4, 5, 20, 21)


def test_flags_without_the_bit_resolve_as_before(zpq, no_knobs):
    """The literal tables of test_set_waves_cpu.py, and the same on an interpreter model (where bit 16 decides nothing)."""
    L = _lib(zpq)
    for header in (C4B, GM.NAMED["mix_x4"][0]):
        m = zpq.Model(header=header)
        assert [L.zpq_blockset_resolve_flags(m.h, f) for f in OLD_FLAGS] == [0, 1, 0, 17, 0, 1, 0, 17]
        no_knobs.setenv("ZPQ_SET_WAVES", "1")
        assert [L.zpq_blockset_resolve_flags(m.h, f) for f in OLD_FLAGS] == [0, 17, 0, 17, 0, 17, 0, 17]
        no_knobs.setenv("ZPQ_SET_LANES", "1")
        assert [L.zpq_blockset_resolve_flags(m.h, f) for f in OLD_FLAGS] == [17] * 8
        no_knobs.setenv("ZPQ_SET_WAVES", "0")
        assert [L.zpq_blockset_resolve_flags(m.h, f) for f in OLD_FLAGS] == [1] * 8
        no_knobs.delenv("ZPQ_SET_WAVES")
        no_knobs.delenv("ZPQ_SET_LANES")
        m.close()
    for name in ("n16", "n17", "hh_small"):
        m = zpq.Model(header=GM.NAMED[name][0])
        assert [L.zpq_blockset_resolve_flags(m.h, f) for f in OLD_FLAGS] == [0, 1, 0, 1, 0, 1, 0, 1], name
        m.close()
    m = zpq.Model(level=2)
    assert [L.zpq_blockset_resolve_flags(m.h, f) for f in OLD_FLAGS] == [0, 0, 0, 0, 4, 4, 4, 4]
    m.close()


# ---------------------------------------------------------------- 5. refused flags
def test_unknown_bits_stay_refused(zpq, no_knobs):
    L = _lib(zpq)
    for m in (zpq.Model(header=C4B), zpq.Model(header=VM.C4B_VM)):
        for flags in (2, 8, 32, 0x100, 66, 72, 0x80000040):
            out = C.c_void_p(0x1234)
            assert L.zpq_blockset_create_ex(None, m.h, 3, 0, flags, C.byref(out)) == E_ARG and out.value is None, flags
            assert L.zpq_blockset_capacity_ex(None, m.h, 0, flags) == E_ARG, flags
            assert L.zpq_blockset_resolve_flags(m.h, flags) == E_ARG, flags
        for flags in (64, 65, 81):                                  # not refused for the flags themselves
            assert L.zpq_blockset_resolve_flags(m.h, flags) in (0, 1, 17, 65), flags
            out = C.c_void_p(0x1234)
            assert L.zpq_blockset_create_ex(None, m.h, 3, 0, flags, C.byref(out)) == E_ARG and out.value is None   # (the NULL ctx)
        m.close()


# ---------------------------------------------------------------- 6. the binding
def test_the_binding_surfaces_the_library_error(zpq, no_knobs):
    assert "vmwaves" in inspect.signature(zpq.BlockSet.__init__).parameters
    assert "vmwaves" in inspect.signature(zpq.Context.blockset_capacity).parameters
    assert isinstance(zpq.BlockSet.vmwaves, property) and zpq.BlockSet.vmwaves.fset is None

    class NoCtx:
        h = None
        _children = set()
    m = zpq.Model(header=VM.C4B_VM)
    with pytest.raises(zpq.ZpqError) as e:
        zpq.BlockSet(NoCtx(), m, 2, vmwaves=True)
    assert e.value.code == E_ARG
    with pytest.raises(zpq.ZpqError) as e:
        zpq.Context.blockset_capacity(NoCtx(), m, vmwaves=True)
    assert e.value.code == E_ARG
    m.close()


# ---------------------------------------------------------------- 7. the GPU inputs tell a kept VM state from a dropped one
def _zero_regs(z):
    z.a = z.b = z.c = z.d = 0
    z.f = 0


def _zero_h(z):
    z.h = [0] * len(z.h)


def _zero_r(z):
    z.r = [0] * 256


def _zero_m(z):
    z.m = bytearray(len(z.m))


PARTS = {"regs": (_zero_regs, ("f_sticks", "d_walks_h", "loop_on_old_f")),
         "H": (_zero_h, ("f_sticks", "d_walks_h", "loop_on_old_f", "loop_hh9_hm16")),
         "R": (_zero_r, ("r_delay",)),
         "M": (_zero_m, ("loop_scan_m",))}


def small_members(name):
    """Three members of three segments of 40-150 random bytes (f_sticks flips on a byte with (byte & 31) == 5, loop_on_old_f
    on one above 100: random bytes meet both at once)."""
    r = random.Random(100 + sum(name.encode()))
    return [[bytes(r.getrandbits(8) for _ in range(r.choice([40, 90, 150]))) for _ in range(3)] for _ in range(3)]


@pytest.mark.parametrize("part,name", [(p, n) for p in sorted(PARTS) for n in PARTS[p][1]])
def test_the_gpu_inputs_tell_a_kept_vm_state_from_a_dropped_one(no_knobs, part, name):
    """ZPAQL's a b c d f, H, R and M outlive a segment in the reference (Predictor.reset clears only the contexts h[i]).  With
    one of them zeroed between segments the Python reference writes other bytes for a later segment than the oracle does: a
    hand-over that lost that part fails the GPU test of the program."""
    sys.path.insert(0, os.path.join(ROOT, "oracle", "pyref"))
    import zpaq_pyref as P
    hdr, offs = ZP.embed(ZP.NAMED[name], "rows")
    assert tuple(O.scan_header(hdr)) == tuple(offs)
    zero = PARTS[part][0]
    differ = 0
    for segs in small_members(name):
        assert len(segs) == 3 and all(len(s) <= 150 for s in segs)
        codec, kept, dropped = O.Codec(hdr), P.new_model(hdr, offs), P.new_model(hdr, offs)
        want = [codec.encode(s, pp=True) for s in segs]
        assert [P.encode_segment(kept, s) for s in segs] == want
        other = []
        for k, s in enumerate(segs):
            if k:                                               # (between segments: the first one starts from ZPAQL.clear)
                zero(dropped.z)
            other.append(P.encode_segment(dropped, s))
        assert other[0] == want[0]
        differ += other != want
    print("\n%s zeroed under %s: %d of 3 members differ" % (part, name, differ))
    assert differ >= 1
