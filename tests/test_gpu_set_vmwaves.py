"""Block sets of general models whose HCOMP program is not the shipped hash chain on the interpreter-wave kernels
(ZPQ_SET_LANES | ZPQ_SET_VMWAVES, BlockSet(..., vmwaves=True)): one launch of k_vset<batched / bit-serial> or k_vsetd per call, a
wave per component, one for the coder and one that runs the ZPAQL interpreter, a lane per member; every member's state -- the
interpreter's a b c d f pc, M, H and R with the components' tables -- handed from launch to launch through its slot in the
format k_rows / k_lanes<..., KEEP> keep, so calls on one set may alternate between the families.  Expected bytes, lengths and
consumed come from oracle_lib.Codec, one codec per member and direction, one call per segment."""
import ctypes as C
import os
import random
import sys

import pytest

import general_models as GM
import oracle_lib as O
import vpipe_models as VM
import zpaql_programs as ZP
from test_gpu_blockset import make_members
from test_gpu_set_waves import cut, members_of
from test_set_vmwaves_cpu import n15

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from inputs import C4B  # noqa: E402

pytestmark = pytest.mark.gpu

KNOBS = ("ZPQ_SET_LANES", "ZPQ_SET_WAVES", "ZPQ_SET_VMWAVES", "ZPQ_SET_PIPE", "ZPQ_LANES_ROWS", "ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE",
         "ZPQ_GPIPE_BATCH", "ZPQ_GDEC_BPW", "ZPQ_VM_PIPE", "ZPQ_ENC_PIPE", "ZPQ_DEC_PIPE")
E_ARG, E_NOMEM, E_OVERFLOW, E_VMSTEPS, E_CLOSED = -2, -6, -7, -8, -10
VSET = ("k_vset<encode>", "k_vsetd<decode>")
WSET = ("k_wset<encode>", "k_wsetd<decode>")
ROWS, LANES = ("k_rows<encode>", "k_rows<decode>"), ("k_lanes<encode>", "k_lanes<decode>")
CHAIN, GENERIC = ("k_chain<encode>", "k_chain<decode>"), ("k_generic<encode>", "k_generic<decode>")
MAXLEN = 3000
FLAG_PP = 1
NOFIRST = 0xFFFFFFFF


@pytest.fixture()
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def model_of(zpq, header, offs=None):
    return zpq.Model(header=header, offsets=offs) if offs else zpq.Model(header=header)


_ORACLE = {}


def oracle_history(key, header, members, offs=None, pp=True):
    """coded[m][s]: what the sequential coder writes for segment s of member m; computed once per key, never changed."""
    if key not in _ORACLE:
        out = []
        for segs in members:
            codec = O.Codec(header, offs)
            out.append([codec.encode(seg, pp=pp) for seg in segs])
        _ORACLE[key] = out
    return _ORACLE[key]


def run_members(zpq, ctx, header, members, want, names=VSET, flags=65, offs=None, kw=None, before_call=None):
    """Two sets made with `kw` (the request: vmwaves=True), which must come back with `flags` in force.  Round r codes segment r
    of every member that has one on one set and decodes it on the other: coded bytes, out_len, decoded bytes, consumed and
    first_byte against the oracle, the kernel's name after every call.  before_call(r, decode) may set the environment and
    returns the name that call must report."""
    kw = {"vmwaves": True} if kw is None else kw
    n = len(members)
    model = model_of(zpq, header, offs)
    enc, dec = zpq.BlockSet(ctx, model, n, **kw), zpq.BlockSet(ctx, model, n, **kw)
    try:
        assert zpq.lib().zpq_blockset_flags(enc.h) == flags == zpq.lib().zpq_blockset_flags(dec.h)
        assert enc.vmwaves is bool(flags & 64) and enc.lanes is bool(flags & 1) and enc.waves is bool(flags & 16)
        for r in range(max(len(segs) for segs in members)):
            idx = [m for m in range(n) if len(members[m]) > r]
            name = before_call(r, 0) if before_call else names[0]
            coded, status, out_len = enc.encode_segments([members[m][r] for m in idx], members=idx)
            assert ctx.last_kernel_name == name, (r, ctx.last_kernel_name)
            assert [int(s) for s in status] == [0] * len(idx), (r, list(status))
            assert [int(x) for x in out_len] == [len(want[m][r]) for m in idx], r
            for j, m in enumerate(idx):
                assert coded[j] == want[m][r], ("coded bytes", r, m, len(members[m][r]))
            name = before_call(r, 1) if before_call else names[1]
            back, status, consumed, _, first = dec.decode_segments([want[m][r] for m in idx], cap=MAXLEN + 8, members=idx)
            assert ctx.last_kernel_name == name, (r, ctx.last_kernel_name)
            assert [int(s) for s in status] == [0] * len(idx), (r, list(status))
            for j, m in enumerate(idx):
                assert back[j] == members[m][r], ("decoded bytes", r, m, len(members[m][r]), len(back[j]))
            assert [int(c) for c in consumed] == [len(want[m][r]) for m in idx], r
            assert all(int(f) == 0 for f in first), r
    finally:
        enc.close()
        dec.close()
        model.close()


# ---------------------------------------------------------------- 1. the VM goes from launch to launch
@pytest.mark.parametrize("batch", ["batched", "bit_serial"])
@pytest.mark.parametrize("name", ZP.SEGMENT_PROGRAMS + ("loop_scan_m", "loop_hh9_hm16"))
def test_the_vm_goes_from_launch_to_launch(zpq, gpu_ctx, clean_env, name, batch):
    """a b c d f pc, M, H and R of 21 members of 1-4 segments (empty ones among them) through the set's slots.
    tests/test_set_vmwaves_cpu.py shows on the host that segments of these programs tell each part kept from dropped."""
    if batch == "bit_serial":
        clean_env.setenv("ZPQ_GPIPE_BATCH", "0")
    header, offs = ZP.embed(ZP.NAMED[name], "rows")
    members = make_members(700 + len(name) + len("rows"))
    assert len(members) == 21 and {len(s) for s in members} == {1, 2, 3, 4}
    assert any(len(s) == 0 for segs in members for s in segs)
    run_members(zpq, gpu_ctx, header, members, oracle_history(("vm", name), header, members, offs), offs=offs)


# ---------------------------------------------------------------- 2. all nine types
@pytest.mark.parametrize("batch", ["batched", "bit_serial"])
def test_all_nine_types(zpq, gpu_ctx, clean_env, batch):
    """C4b's components behind `a=a` and its own hash chain: the interpreter computes the contexts the hash-chain kernels keep in
    registers, so the streams equal the oracle's for that header, the oracle's for C4B, and what a waves=True set of C4B writes."""
    if batch == "bit_serial":
        clean_env.setenv("ZPQ_GPIPE_BATCH", "0")
    members = members_of(41, 7)
    assert all(len(segs) == 4 and all(1 <= len(s) <= MAXLEN for s in segs) for segs in members)
    want = oracle_history(("nine", "C4B_VM"), VM.C4B_VM, members)
    assert want == oracle_history(("nine", "C4B"), C4B, members)
    run_members(zpq, gpu_ctx, VM.C4B_VM, members, want)
    model = zpq.Model(header=C4B)
    st = zpq.BlockSet(gpu_ctx, model, len(members), waves=True)
    assert st.waves and not st.vmwaves
    for r in range(4):
        coded, status, _ = st.encode_segments([segs[r] for segs in members])
        assert gpu_ctx.last_kernel_name == WSET[0] and (status == 0).all()
        assert coded == [want[m][r] for m in range(len(members))], r
    st.close()
    model.close()


# ---------------------------------------------------------------- 3. one slot format for both families
@pytest.mark.parametrize("what", ["d_walks_h", "r_delay", "loop_scan_m", "C4B_VM"])
def test_the_families_alternate_on_one_set(zpq, gpu_ctx, clean_env, what):
    """Rounds 0 and 2 on k_vset / k_vsetd, round 1 on k_rows (ZPQ_ENC_GPIPE=0 / ZPQ_DEC_GPIPE=0 at the call), round 3 on k_lanes
    (the same, and ZPQ_LANES_ROWS=0): each family goes on from what the other left in the slot."""
    header, offs = (VM.C4B_VM, None) if what == "C4B_VM" else ZP.embed(ZP.NAMED[what], "rows")
    members = members_of(57 + len(what), 5, lengths=[1, 2, 17, 64, 65, 300, 1500])
    family = [VSET, ROWS, VSET, LANES]

    def before_call(r, decode):
        for k in ("ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE", "ZPQ_LANES_ROWS"):
            clean_env.delenv(k, raising=False)
        if family[r] is not VSET:
            clean_env.setenv("ZPQ_DEC_GPIPE" if decode else "ZPQ_ENC_GPIPE", "0")
        if family[r] is LANES:
            clean_env.setenv("ZPQ_LANES_ROWS", "0")
        return family[r][decode]

    run_members(zpq, gpu_ctx, header, members, oracle_history(("alt", what), header, members, offs), offs=offs,
                before_call=before_call)


# ---------------------------------------------------------------- 4. lane mapping
def test_lane_mapping(zpq, gpu_ctx, clean_env):
    """67 members of loop_count: two workgroups, three lanes in the second.  Subsets in shuffled member[] order, fresh members
    joining in later rounds, segments of 0, 1 and 3000 bytes side by side, and ZP.divergence_batch() as one round (neighbouring
    lanes run 1 against 16 interpreter iterations per byte)."""
    n = 67
    header, offs = ZP.embed(ZP.NAMED["loop_count"], "rows")
    model = model_of(zpq, header, offs)
    r = random.Random(n)
    enc_o, dec_o = [O.Codec(header, offs) for _ in range(n)], [O.Codec(header, offs) for _ in range(n)]
    enc, dec = zpq.BlockSet(gpu_ctx, model, n, vmwaves=True), zpq.BlockSet(gpu_ctx, model, n, vmwaves=True)
    assert enc.vmwaves and dec.vmwaves and enc.lanes
    calls = [0]

    def call(idx, segs):
        calls[0] += 1
        coded, status, out_len = enc.encode_segments(segs, members=idx)
        assert gpu_ctx.last_kernel_name == VSET[0]
        assert [int(s) for s in status] == [0] * len(idx)
        want = [enc_o[m].encode(s, pp=True) for m, s in zip(idx, segs)]
        assert [int(x) for x in out_len] == [len(w) for w in want]
        for j, m in enumerate(idx):
            assert coded[j] == want[j], ("coded", calls[0], m, len(segs[j]))
        back, status, consumed, code, first = dec.decode_segments(want, cap=MAXLEN + 8, members=idx)
        assert gpu_ctx.last_kernel_name == VSET[1]
        assert [int(s) for s in status] == [0] * len(idx)
        for j, m in enumerate(idx):
            data, _, cons, fcode, _ = dec_o[m].decode_prefix(want[j], MAXLEN + 9)
            assert back[j] == segs[j] and b"\0" + segs[j] == data, ("decoded", calls[0], m, len(segs[j]))
            assert int(consumed[j]) == cons == len(want[j]) and int(code[j]) == fcode, (calls[0], m)
            assert int(first[j]) == 0

    def some(idx, lengths):
        return [cut(n * 1000 + calls[0] * 131 + m, r.choice(lengths)) for m in idx]

    first = list(range(40))
    r.shuffle(first)
    call(first, some(first, [1, 17, 65, 300]))                                   # 40 lanes of one workgroup, shuffled
    div = ZP.divergence_batch()
    call(list(range(len(div))), div)                                             # members 0 .. 22 in lane order
    everyone = list(range(n))
    r.shuffle(everyone)
    edge = {0: 0, 1: 1, 2: MAXLEN, 63: 0, 64: MAXLEN, 65: 1, 66: 0}
    call(everyone, [cut(9000 + m, edge.get(m, r.choice([2, 64, 300]))) for m in everyone])   # 40 .. 66 are fresh
    call([66, 1, 64], some([66, 1, 64], [300]))                                  # a subset of 3: one workgroup, 61 idle lanes
    r.shuffle(everyone)
    call(everyone, some(everyone, [0, 1, 17, 65]))
    enc.close()
    dec.close()
    model.close()


# ---------------------------------------------------------------- 5. without ZPQ_FLAG_PP
def test_without_the_pp_flag(zpq, gpu_ctx, clean_env):
    """Three rounds with flags = 0.  The encoder codes no PP byte (the oracle's pp=False); the decoder, fed streams that hold one,
    stores it as the first output byte and reports first_byte 0xFFFFFFFF."""
    header, offs = ZP.embed(ZP.NAMED["r_delay"], "rows")
    members = [segs[:3] for segs in members_of(77, 6, lengths=[1, 17, 65, 300])]
    raw, with_pp = oracle_history(("nopp", 0), header, members, offs, pp=False), oracle_history(("nopp", 1), header, members, offs)
    model = model_of(zpq, header, offs)
    enc, dec = zpq.BlockSet(gpu_ctx, model, 6, vmwaves=True), zpq.BlockSet(gpu_ctx, model, 6, vmwaves=True)
    assert enc.vmwaves and dec.vmwaves
    for r in range(3):
        coded, status, _ = enc.encode_segments([segs[r] for segs in members], flags=0)
        assert gpu_ctx.last_kernel_name == VSET[0] and (status == 0).all()
        assert coded == [raw[m][r] for m in range(6)], r
        back, status, consumed, _, first = dec.decode_segments([with_pp[m][r] for m in range(6)], cap=MAXLEN + 8, flags=0)
        assert gpu_ctx.last_kernel_name == VSET[1] and (status == 0).all()
        assert back == [b"\0" + segs[r] for segs in members], r
        assert [int(c) for c in consumed] == [len(with_pp[m][r]) for m in range(6)]
        assert all(int(f) == NOFIRST for f in first), r
    enc.close()
    dec.close()
    model.close()


# ---------------------------------------------------------------- 6. the step cap
def test_the_step_cap_is_sticky(zpq, gpu_ctx, clean_env):
    """The rounds of test_gpu_set_lanes.py::test_the_step_cap_is_sticky: members 1, 6 and 7 of 12 meet a byte on which the
    program never ends in round 0: ZPQ_E_VMSTEPS then and in every later call, from the encoder set and from the decoder set; the
    nine others, lanes of the same waves, equal the oracle throughout."""
    header, offs = ZP.embed(ZP.STEP_CAP, "rows")
    model = zpq.Model(header=header, offsets=offs)
    first = ZP.step_cap_batch()
    r = random.Random(13)
    rounds = [first, [bytes(r.randrange(255) for _ in range(n)) for n in (17, 3, 40, 0, 1, 65, 2, 30, 9, 33, 40, 5)],
              [bytes(r.randrange(255) for _ in range(20)) for _ in range(12)]]
    capped, good = (1, 6, 7), (0, 2, 3, 4, 5, 8, 9, 10, 11)
    codecs = [O.Codec(header, offs) for _ in range(12)]
    want = [[codecs[m].encode(rounds[k][m]) if m in good else None for m in range(12)] for k in range(3)]
    enc, dec = zpq.BlockSet(gpu_ctx, model, 12, vmwaves=True), zpq.BlockSet(gpu_ctx, model, 12, vmwaves=True)
    assert enc.vmwaves and dec.vmwaves
    streams0 = [O.Codec(header, offs).encode(b) for b in first]    # (the oracle has the same cap: its streams of the capped members are only an input)
    for k in range(3):
        coded, status, out_len = enc.encode_segments(rounds[k])
        assert gpu_ctx.last_kernel_name == VSET[0]
        assert [int(s) for s in status] == [E_VMSTEPS if m in capped else 0 for m in range(12)], (k, list(status))
        assert [coded[m] for m in good] == [want[k][m] for m in good], k
        if k:
            assert all(int(out_len[m]) == 0 for m in capped)
        feed = [want[k][m] if m in good else (streams0[m] if k == 0 else b"\0\0\0\0") for m in range(12)]
        back, status, _, _, _ = dec.decode_segments(feed, cap=72)
        assert gpu_ctx.last_kernel_name == VSET[1]
        assert [int(s) for s in status] == [E_VMSTEPS if m in capped else 0 for m in range(12)], (k, list(status))
        assert [back[m] for m in good] == [rounds[k][m] for m in good], k
    enc.close()
    dec.close()
    model.close()


# ---------------------------------------------------------------- 7. overflow is sticky
def test_encoder_overflow_is_sticky(zpq, gpu_ctx, clean_env):
    header = VM.C4B_VM
    model = zpq.Model(header=header)
    n = 6
    codecs = [O.Codec(header) for _ in range(n)]
    enc = zpq.BlockSet(gpu_ctx, model, n, vmwaves=True)
    assert enc.vmwaves
    good = (0, 2, 3, 4, 5)
    segs = [cut(2, 64), cut(1, 300), cut(6, 64), cut(3, 65), cut(4, 17), cut(5, 3)]
    coded, status, out_len = enc.encode_segments(segs, cap=[4096, 16, 4096, 4096, 4096, 4096])   # 300 random bytes do not fit 16
    assert gpu_ctx.last_kernel_name == VSET[0]
    assert [int(s) for s in status] == [0, E_OVERFLOW, 0, 0, 0, 0]
    assert int(out_len[1]) == len(O.Codec(header).encode(segs[1]))           # the encoder keeps counting
    assert [coded[m] for m in good] == [codecs[m].encode(segs[m]) for m in good]
    for k in range(2):
        segs = [cut(10 + 6 * k + m, 17 + 100 * m) for m in range(n)]
        coded, status, out_len = enc.encode_segments(segs)
        assert gpu_ctx.last_kernel_name == VSET[0]
        assert [int(s) for s in status] == [0, E_OVERFLOW, 0, 0, 0, 0] and int(out_len[1]) == 0
        assert [coded[m] for m in good] == [codecs[m].encode(segs[m]) for m in good]
    coded, status, _ = enc.encode_segments([b"abc"], members=[1])
    assert [int(s) for s in status] == [E_OVERFLOW]
    enc.close()
    model.close()


def test_decoder_overflow_touches_no_other_member(zpq, gpu_ctx, clean_env):
    """Round 0: member 1's slab is too small for its segment.  It keeps ZPQ_E_OVERFLOW with nothing decoded; a later call that
    lists it copies only the live members' stored bytes; every other member follows its oracle codec through all rounds."""
    header, offs = ZP.embed(ZP.NAMED["d_walks_h"], "rows")
    n = 7
    members = members_of(91, n, lengths=[65, 300, 700])
    coded = oracle_history(("dover", 0), header, members, offs)
    model = model_of(zpq, header, offs)
    dec = zpq.BlockSet(gpu_ctx, model, n, vmwaves=True)
    assert dec.vmwaves
    mirror = [O.Codec(header, offs) for _ in range(n)]
    full = MAXLEN + 8
    for k in range(3):
        calls = [([m for m in range(n) if m != 1], full), ([1], 16)] if k == 0 else [(list(range(n)), full)]
        for idx, cap in calls:
            back, status, consumed, code, _ = dec.decode_segments([coded[m][k] for m in idx], cap=cap, members=idx, flags=0)
            if k == 0 or idx != [1]:
                assert gpu_ctx.last_kernel_name == VSET[1]
            for j, m in enumerate(idx):
                if m == 1 and k:
                    assert int(status[j]) == E_OVERFLOW and back[j] == b"", k
                    continue
                data, out_len, cons, fcode, _ = mirror[m].decode_prefix(coded[m][k], cap)
                assert int(status[j]) == (E_OVERFLOW if out_len > cap else 0), (k, m)
                assert back[j] == data and len(back[j]) <= cap, (k, m)
                assert int(consumed[j]) == cons and int(code[j]) == fcode, (k, m)
                if m != 1:
                    assert int(status[j]) == 0 and back[j] == b"\0" + members[m][k], (k, m)
                else:
                    assert int(status[j]) == E_OVERFLOW
    dec.close()
    model.close()


# ---------------------------------------------------------------- 8. damaged segments
@pytest.mark.parametrize("pp", [True, False], ids=["pp", "raw"])
def test_sets_follow_damaged_segments(zpq, gpu_ctx, clean_env, pp):
    """The 360 mutated members of tests/offnominal_sets.py for hm0 (a program that is not the hash chain): a good, a damaged and a
    good segment on one set, every slab policy, all outputs the oracle's."""
    from test_gpu_offnominal_sets import general_sets
    seen = set()
    general_sets(zpq, gpu_ctx, "hm0", pp, lambda which, rnd: VSET[1], seen, {"vmwaves": True}, 65)
    print("\nkernels hm0 pp=%d flags 65: %s" % (pp, sorted(seen)))
    assert seen == {"k_vsetd<decode>", "k_vsetd<decode> some failed"}


@pytest.mark.parametrize("order", ["vmwaves_then_rows", "rows_then_vmwaves"])
def test_the_other_family_reads_what_a_damaged_segment_left(zpq, gpu_ctx, clean_env, order):
    """hm0 under tight slabs: rounds 0 and 1 on k_vsetd and round 2 on k_rows (ZPQ_DEC_GPIPE=0 at the call), and the reverse."""
    from test_gpu_offnominal_sets import general_sets, set_env
    seen = set()

    def kernel_of(which, rnd):
        on_waves = (rnd < 2) == (order == "vmwaves_then_rows")
        set_env(clean_env, {} if on_waves else {"ZPQ_DEC_GPIPE": "0"})
        return VSET[1] if on_waves else ROWS[1]

    general_sets(zpq, gpu_ctx, "hm0", True, kernel_of, seen, {"vmwaves": True}, 65, policies=("tight",), tag=" " + order)
    print("\nkernels hm0 %s flags 65: %s" % (order, sorted(seen)))
    assert seen == ({"k_vsetd<decode>", "k_rows<decode> some failed"} if order == "vmwaves_then_rows"
                    else {"k_rows<decode>", "k_vsetd<decode> some failed"})


# ---------------------------------------------------------------- 9. the edges of the envelope
def small_members(seed):
    return [[s[:300] for s in segs[:2]] for segs in make_members(seed, nmembers=3)]


@pytest.mark.parametrize("what", ["n14", "lds_160k", "hh_small", "hm0"])
def test_inside_the_envelope(zpq, gpu_ctx, clean_env, what):
    """Fourteen components (16 waves, 1024 threads); the same fourteen with the encoder's LDS at 160 KiB exactly; an H smaller
    than the number of components; no M."""
    header, offs = {"n14": VM.lds_edge(0), "lds_160k": VM.lds_edge(69)}.get(what) or (GM.NAMED[what][0], None)
    if what == "lds_160k":
        assert VM.lds_bytes(header)[0] == VM.LDS_MAX
    members = small_members(5)
    run_members(zpq, gpu_ctx, header, members, oracle_history(("edge", what), header, members, offs), offs=offs)


@pytest.mark.parametrize("what", ["n15", "lds_beyond", "mix3_sse3_n22_vm", "chain14", "chain15"])
def test_a_request_that_decides_nothing(zpq, gpu_ctx, clean_env, what):
    """Fifteen components, LDS 16 bytes beyond 160 KiB, 22 components: flags 1 and k_rows / k_lanes as without the request.
    VM.chain(14) / VM.chain(15): ISSE chains, whose sets a chain kernel codes -- ZPQ_SET_LANES is not in force, flags 0, k_chain."""
    header, offs, names, flags = {
        "n15": (n15(), None, ROWS, 1), "lds_beyond": VM.lds_edge(70) + (ROWS, 1),
        "mix3_sse3_n22_vm": (GM.NAMED["mix3_sse3_n22_vm"][0], None, LANES, 1),
        "chain14": (VM.chain(14), None, CHAIN, 0), "chain15": (VM.chain(15), None, CHAIN, 0)}[what]
    model = model_of(zpq, header, offs)
    assert gpu_ctx.blockset_capacity(model, vmwaves=True) == gpu_ctx.blockset_capacity(model, lanes=True)
    model.close()
    members = small_members(3)
    run_members(zpq, gpu_ctx, header, members, oracle_history(("nothing", what), header, members, offs), names=names,
                flags=flags, offs=offs, kw={"vmwaves": True, "max_member_bytes": 700})


def test_both_wave_requests_on_c4b(zpq, gpu_ctx, clean_env):
    """81 = lanes | waves | vmwaves: on the hash chain's model it resolves to 17 and the set runs on k_wset / k_wsetd."""
    members = small_members(4)
    run_members(zpq, gpu_ctx, C4B, members, oracle_history(("81", "C4B"), C4B, members), names=WSET, flags=17,
                kw={"waves": True, "vmwaves": True})
    run_members(zpq, gpu_ctx, VM.C4B_VM, members, oracle_history(("81", "C4B_VM"), VM.C4B_VM, members), names=VSET, flags=65,
                kw={"waves": True, "vmwaves": True})


# ---------------------------------------------------------------- 10. flags, capacity, lifetime
def test_the_environment_makes_and_withdraws_the_request(zpq, gpu_ctx, clean_env):
    header, offs = ZP.embed(ZP.NAMED["loop_count"], "rows")
    model = model_of(zpq, header, offs)
    seg = [cut(2, 108)]
    want = O.Codec(header, offs).encode(seg[0])
    table = ((("1", "1"), {}, 65), (("1", None), {}, 0), (("1", None), {"lanes": True}, 65), ((None, "1"), {}, 1),
             ((None, "1"), {"vmwaves": True}, 65), (("0", "1"), {"vmwaves": True}, 1), (("0", None), {"vmwaves": True}, 1),
             (("1", "0"), {"vmwaves": True}, 0), (("x", None), {"vmwaves": True}, 65), ((None, None), {"vmwaves": True}, 65),
             ((None, None), {"waves": True}, 1), ((None, None), {"lanes": True}, 1), ((None, None), {}, 0))
    for (ev, el), kw, flags in table:
        for var, val in (("ZPQ_SET_VMWAVES", ev), ("ZPQ_SET_LANES", el)):
            if val is None:
                clean_env.delenv(var, raising=False)
            else:
                clean_env.setenv(var, val)
        st = zpq.BlockSet(gpu_ctx, model, 2, **kw)
        assert zpq.lib().zpq_blockset_flags(st.h) == flags, (ev, el, kw)
        assert (st.vmwaves, st.lanes, st.waves) == (bool(flags & 64), bool(flags & 1), False)
        assert st.encode_segments(seg, members=[1])[0][0] == want
        assert gpu_ctx.last_kernel_name == {65: VSET[0], 1: ROWS[0], 0: GENERIC[0]}[flags], (ev, el, kw)
        st.close()
    model.close()


def test_capacity_and_a_batch_between_two_rounds(zpq, gpu_ctx, clean_env):
    L = zpq.lib()
    header = VM.C4B_VM
    model = zpq.Model(header=header)
    plain, lanes, vm = gpu_ctx.blockset_capacity(model), gpu_ctx.blockset_capacity(model, lanes=True), gpu_ctx.blockset_capacity(model, vmwaves=True)
    assert 1 <= plain <= lanes == vm <= 1 << 20
    assert L.zpq_blockset_capacity_ex(gpu_ctx.h, model.h, 0, 65) == L.zpq_blockset_capacity_ex(gpu_ctx.h, model.h, 0, 1) == lanes
    assert L.zpq_blockset_capacity_ex(gpu_ctx.h, model.h, 0, 64) == plain        # alone: decides nothing
    out = C.c_void_p(0x1234)
    assert L.zpq_blockset_create_ex(gpu_ctx.h, model.h, vm + 1, 0, 65, C.byref(out)) == E_NOMEM and out.value is None
    for bad in (66, 72, 32):
        assert L.zpq_blockset_capacity_ex(gpu_ctx.h, model.h, 0, bad) == E_ARG
        assert L.zpq_blockset_create_ex(gpu_ctx.h, model.h, 1, 0, bad, C.byref(out)) == E_ARG and out.value is None
    codecs = [O.Codec(header) for _ in range(4)]
    st = zpq.BlockSet(gpu_ctx, model, 4, vmwaves=True)
    assert st.vmwaves
    segs = [cut(20 + m, 150) for m in range(4)]
    assert st.encode_segments(segs)[0] == [codecs[m].encode(segs[m]) for m in range(4)]
    blocks = [cut(7 + k, 200) for k in range(14)]                                # the ctx's slot pool, never the set's slots
    coded, status, _ = gpu_ctx.encode_blocks(model, blocks, flags=zpq.FLAG_PP | zpq.FLAG_VMPIPE)
    assert gpu_ctx.last_kernel_name == "k_vpipe<encode>"
    assert (status == 0).all() and coded == O.encode_blocks(header, blocks)
    segs = [cut(30 + m, 151) for m in range(4)]
    assert st.encode_segments(segs)[0] == [codecs[m].encode(segs[m]) for m in range(4)]
    assert gpu_ctx.last_kernel_name == VSET[0]
    st.close()
    model.close()


def test_lifetime_orders(zpq):
    """On a context of the test's own: the ctx destroyed before its set (orphaned: ZPQ_E_CLOSED from both directions, destroy
    still fine), and the binding's order."""
    header, offs = ZP.embed(ZP.NAMED["f_sticks"], "rows")
    seg = cut(2, 150)
    want = O.Codec(header, offs).encode(seg)
    ctx = zpq.Context(0)
    model = model_of(zpq, header, offs)
    a = zpq.BlockSet(ctx, model, 2, vmwaves=True)
    b = zpq.BlockSet(ctx, model, 3, vmwaves=True)
    assert a.vmwaves and b.vmwaves
    assert a.encode_segments([seg], members=[1])[0][0] == want
    assert ctx.last_kernel_name == VSET[0]
    a.close()
    assert b.decode_segments([want], cap=200, members=[2])[0][0] == seg
    assert ctx.last_kernel_name == VSET[1]
    zpq.lib().zpq_ctx_destroy(ctx.h)                       # the ctx before the set, through the raw call
    ctx.h = None
    with pytest.raises(zpq.ZpqError) as e:
        b.encode_segments([b"abc"], members=[0])
    assert e.value.code == E_CLOSED
    with pytest.raises(zpq.ZpqError) as e:
        b.decode_segments([want], cap=200, members=[0])
    assert e.value.code == E_CLOSED
    b.close()
    model.close()
    ctx2 = zpq.Context(0)
    m2 = model_of(zpq, header, offs)
    c = zpq.BlockSet(ctx2, m2, 2, vmwaves=True)
    ctx2.close()                                           # the binding's order: children first
    assert c.h is None
