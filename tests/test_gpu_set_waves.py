"""Block sets of general models on the wave-per-component kernels (ZPQ_SET_LANES | ZPQ_SET_WAVES, BlockSet(..., waves=True)):
one launch of k_wset<batched / bit-serial> or k_wsetd per call, a wave per component and a lane per member, every member's
state handed from launch to launch through its slot in the format k_rows / k_lanes<..., KEEP> keep -- so calls on one set may
alternate between the families.  Expected bytes, lengths, consumed and the decoder's final code come from oracle_lib.Codec,
one codec per member and direction, one call per segment.  Segments are cut from tests/workload.py's blocks."""
import ctypes as C
import os
import random
import sys
import types

import pytest

import general_models as GM
import oracle_lib as O
import workload as W
from test_gpu_blockset import check_parity, make_members, oracle_history

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from inputs import C4B  # noqa: E402

pytestmark = pytest.mark.gpu

KNOBS = ("ZPQ_SET_LANES", "ZPQ_SET_WAVES", "ZPQ_SET_PIPE", "ZPQ_LANES_ROWS", "ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE", "ZPQ_GPIPE_BATCH",
         "ZPQ_GDEC_BPW", "ZPQ_VM_PIPE")
E_ARG, E_NOMEM, E_OVERFLOW, E_CLOSED = -2, -6, -7, -10
WAVES = ("k_wset<encode>", "k_wsetd<decode>")
ROWS, LANES = ("k_rows<encode>", "k_rows<decode>"), ("k_lanes<encode>", "k_lanes<decode>")
CHAIN, GENERIC = ("k_chain<encode>", "k_chain<decode>"), ("k_generic<encode>", "k_generic<decode>")
ROUNDS, MAXLEN = 4, 3000
LENGTHS = [1, 2, 3, 17, 64, 65, 300, 1500, 3000]
PIPE_CLASS = sorted(k for k, (_, rt) in GM.NAMED.items() if rt == GM.PIPE)
FLAG_PP = 1


@pytest.fixture()
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def header_of(what):
    return C4B if what == "C4B" else GM.NAMED[what][0]


def seed_of(what):
    return 3000 + len(what) * 7 + sum(what.encode())


def cut(block, n, at=0):
    """n bytes of workload block `block` (class block mod 4: zeros, random, text, periodic) from offset `at`."""
    return W.make_block(block, at + n)[at:at + n].tobytes() if n else b""


def members_of(seed, nmembers, lengths=LENGTHS):
    """members[m][r]: ROUNDS segments of 1-3000 bytes per member, each from a workload block of its own."""
    r = random.Random(seed)
    return [[cut(seed * 131 + m * ROUNDS + k, r.choice(lengths)) for k in range(ROUNDS)] for m in range(nmembers)]


def match_members(what, nmembers=5):
    """Later segments repeat the earlier ones' content: member m codes a growing prefix of ONE workload block round after round
    (a MATCH with a two-byte buffer lives on runs of one byte: the zeros; the others on the periodic blocks), so a MATCH that kept its buffer, hash index, length and offset
    from the segment before predicts the next one's bytes.  tests/test_set_waves_cpu.py shows on the host that these
    members tell a kept MATCH state from a dropped one."""
    r = random.Random(seed_of(what))
    out = []
    for m in range(nmembers):
        block = 4 * (seed_of(what) + m) + (m + 3) % 4           # classes periodic, zeros, random, text, periodic
        lens = [r.choice([40, 100, 200]), r.choice([150, 300]), r.choice([300, 700, 1500]), r.choice([64, 3000])]
        out.append([cut(block, n) for n in lens])
    return out


_ORACLE = {}


def oracle_rounds(key, header, members, pp=True):
    """(coded[m][r], final_code[m][r], consumed[m][r]) of every segment, computed once per key and shared, never changed."""
    if key not in _ORACLE:
        coded, codes, cons = [], [], []
        for segs in members:
            enc, dec = O.Codec(header), O.Codec(header)
            cs = [enc.encode(s, pp=pp) for s in segs]
            back = [dec.decode_prefix(c, len(s) + 8) for c, s in zip(cs, segs)]
            assert [b[0] for b in back] == [(b"\0" if pp else b"") + s for s in segs]
            coded.append(cs); codes.append([b[3] for b in back]); cons.append([b[2] for b in back])
        _ORACLE[key] = (coded, codes, cons)
    return _ORACLE[key]


def run_rounds(zpq, ctx, header, members, want, names=WAVES, before_call=None, flags=17):
    """Two sets made with waves=True, which must come back with `flags` in force.  Round r codes segment r of every member on one set and decodes it on another: coded bytes, out_len, decoded bytes,
    consumed and final_code against the oracle, the kernel's name after every call.  before_call(r, decode) may set the
    environment and returns the name that call must report."""
    coded_w, code_w, cons_w = want
    n = len(members)
    model = zpq.Model(header=header)
    enc, dec = zpq.BlockSet(ctx, model, n, waves=True), zpq.BlockSet(ctx, model, n, waves=True)      # the request, always
    try:
        assert zpq.lib().zpq_blockset_flags(enc.h) == flags == zpq.lib().zpq_blockset_flags(dec.h)
        assert enc.waves is bool(flags & 16) and dec.lanes is bool(flags & 1)
        for r in range(ROUNDS):
            name = before_call(r, 0) if before_call else names[0]
            coded, status, out_len = enc.encode_segments([members[m][r] for m in range(n)])
            assert ctx.last_kernel_name == name, (r, ctx.last_kernel_name)
            assert [int(s) for s in status] == [0] * n, (r, list(status))
            assert [int(x) for x in out_len] == [len(coded_w[m][r]) for m in range(n)], r
            for m in range(n):
                assert coded[m] == coded_w[m][r], ("coded bytes", r, m, len(members[m][r]))
            name = before_call(r, 1) if before_call else names[1]
            back, status, consumed, code, first = dec.decode_segments([coded_w[m][r] for m in range(n)], cap=MAXLEN + 8)
            assert ctx.last_kernel_name == name, (r, ctx.last_kernel_name)
            assert [int(s) for s in status] == [0] * n, (r, list(status))
            for m in range(n):
                assert back[m] == members[m][r], ("decoded bytes", r, m, len(members[m][r]), len(back[m]))
            assert [int(c) for c in consumed] == [cons_w[m][r] for m in range(n)] == [len(coded_w[m][r]) for m in range(n)], r
            assert [int(c) for c in code] == [code_w[m][r] for m in range(n)], r
            assert all(int(f) == 0 for f in first), r
    finally:
        enc.close()
        dec.close()
        model.close()


def waves_honoured(zpq, header):
    L = zpq.lib()
    L.zpq_blockset_waves_applies.argtypes = [C.c_void_p]
    m = zpq.Model(header=header)
    try:
        return L.zpq_blockset_waves_applies(m.h) == 1
    finally:
        m.close()


# ---------------------------------------------------------------- parity, both directions, both encoder forms
@pytest.mark.parametrize("batch", ["batched", "bit_serial"])
@pytest.mark.parametrize("what", ["C4B"] + PIPE_CLASS)
def test_parity(zpq, gpu_ctx, clean_env, what, batch):
    """Five members, four rounds.  (ht_bits0 is of the PIPE class by its shape, but a chain kernel takes it: the request decides
    nothing there and the set runs on k_chain as it did -- the case stays, with the names of the parent.)"""
    header = header_of(what)
    if batch == "bit_serial":
        clean_env.setenv("ZPQ_GPIPE_BATCH", "0")
    members = members_of(seed_of(what), 5)
    assert {len(segs) for segs in members} == {ROUNDS} and all(1 <= len(s) <= MAXLEN for segs in members for s in segs)
    want = oracle_rounds(("parity", what), header, members)
    if what == "ht_bits0":
        assert not waves_honoured(zpq, header)
        run_rounds(zpq, gpu_ctx, header, members, want, names=CHAIN, flags=0)
        return
    assert waves_honoured(zpq, header)
    run_rounds(zpq, gpu_ctx, header, members, want)


@pytest.mark.parametrize("batch", ["batched", "bit_serial"])
@pytest.mark.parametrize("what", ["match_idx_gt_buf", "bits0_all"])
def test_match_across_segments(zpq, gpu_ctx, clean_env, what, batch):
    header = header_of(what)
    if batch == "bit_serial":
        clean_env.setenv("ZPQ_GPIPE_BATCH", "0")
    members = match_members(what)
    run_rounds(zpq, gpu_ctx, header, members, oracle_rounds(("match", what), header, members))


# ---------------------------------------------------------------- workgroup edges: 64 lanes, one more workgroup, a third
@pytest.mark.parametrize("n", [64, 70, 130])
def test_workgroup_edges(zpq, gpu_ctx, clean_env, n):
    """Members of one workgroup with segments of 0, 1 and 3000 bytes (the pipeline's drain and the decoder's per-lane end must
    leave the short ones' state at THEIR end); member[] a permutation, then a subset of 3 (61 or more lanes of the one
    workgroup idle, the other workgroups not launched); a plain batch of the model on the ctx's slot pool in between; the
    last member coded in calls of its own with ZPQ_FLAG_PP while every other call runs without it."""
    header = C4B
    model = zpq.Model(header=header)
    r = random.Random(n)
    enc_o, dec_o = [O.Codec(header) for _ in range(n)], [O.Codec(header) for _ in range(n)]
    enc, dec = zpq.BlockSet(gpu_ctx, model, n, waves=True), zpq.BlockSet(gpu_ctx, model, n, waves=True)
    assert enc.waves and dec.waves and enc.lanes
    pp_member = n - 1
    edge = {0: 0, 1: 1, 2: MAXLEN, 63: 0, n - 2: MAXLEN, n - 3: 1, 64 % n: 0}
    calls = [0]

    def call(idx, lens, flags):
        calls[0] += 1
        pp = bool(flags & FLAG_PP)
        segs = [cut(n * 1000 + calls[0] * 131 + m, ln) for m, ln in zip(idx, lens)]
        coded, status, out_len = enc.encode_segments(segs, members=idx, flags=flags)
        assert gpu_ctx.last_kernel_name == WAVES[0]
        assert [int(s) for s in status] == [0] * len(idx)
        want = [enc_o[m].encode(s, pp=pp) for m, s in zip(idx, segs)]
        assert [int(x) for x in out_len] == [len(w) for w in want]
        for j, m in enumerate(idx):
            assert coded[j] == want[j], ("coded", calls[0], m, len(segs[j]))
        back, status, consumed, code, first = dec.decode_segments(want, cap=MAXLEN + 8, members=idx, flags=flags)
        assert gpu_ctx.last_kernel_name == WAVES[1]
        assert [int(s) for s in status] == [0] * len(idx)
        for j, m in enumerate(idx):
            data, _, cons, fcode, _ = dec_o[m].decode_prefix(want[j], MAXLEN + 9)
            assert back[j] == segs[j] and (b"\0" if pp else b"") + segs[j] == data, ("decoded", calls[0], m, len(segs[j]))
            assert int(consumed[j]) == cons == len(want[j]) and int(code[j]) == fcode, (calls[0], m)
            assert int(first[j]) == (0 if pp else 0xFFFFFFFF)

    rest = list(range(n - 1))
    perm = rest[:]
    r.shuffle(perm)
    call(perm, [edge.get(m, r.choice(LENGTHS)) for m in perm], 0)               # a permutation; 0, 1 and 3000 side by side
    call([pp_member], [300], FLAG_PP)
    call([next(m for m in perm if m not in (1, n - 2)), 1, n - 2], [MAXLEN, 0, 1], 0)   # a subset of 3
    blocks = [cut(7 + k, 200) for k in range(14)]                               # the ctx's slot pool, never the set's slots
    coded, status, _ = gpu_ctx.encode_blocks(model, blocks)
    assert gpu_ctx.last_kernel_name == "k_gpipe<encode>"
    assert (status == 0).all() and coded == O.encode_blocks(header, blocks)
    call([pp_member], [0], FLAG_PP)
    call(rest, [r.choice([0, 1, 17, 65, 300]) if m != 62 else MAXLEN for m in rest], 0)
    call([pp_member], [MAXLEN], FLAG_PP)
    r.shuffle(perm)
    call(perm, [r.choice([1, 2, 64]) for _ in perm], 0)
    call([pp_member], [1], FLAG_PP)
    enc.close()
    dec.close()
    model.close()


# ---------------------------------------------------------------- one format in the slot for both families
FAMILY = {"W": WAVES, "R": ROWS, "L": LANES}
ORDERS = {"waves_first": [("W", "W"), ("R", "W"), ("W", "L"), ("L", "R")],
          "lanes_first": [("R", "L"), ("W", "R"), ("L", "W"), ("W", "W")]}


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("what", ["C4B", "mix_masks", "match_idx_gt_buf"])
def test_the_families_alternate_on_one_set(zpq, gpu_ctx, clean_env, what, order):
    """Per round (encoder's family, decoder's family): W = the wave kernels, R = k_rows (ZPQ_ENC_GPIPE=0 / ZPQ_DEC_GPIPE=0 at the
    call), L = k_lanes (and ZPQ_LANES_ROWS=0).  Both orders; rounds that encode on one family and decode on the other; a
    round on k_rows / k_lanes reads the p[] the wave kernels did not write (dead for these models)."""
    header = header_of(what)
    members = match_members(what) if what == "match_idx_gt_buf" else members_of(seed_of(what) + 1, 5)

    def before_call(r, decode):
        fam = ORDERS[order][r][decode]
        var = "ZPQ_DEC_GPIPE" if decode else "ZPQ_ENC_GPIPE"
        for k in ("ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE", "ZPQ_LANES_ROWS"):
            clean_env.delenv(k, raising=False)
        if fam != "W":
            clean_env.setenv(var, "0")
        if fam == "L":
            clean_env.setenv("ZPQ_LANES_ROWS", "0")
        return FAMILY[fam][decode]

    run_rounds(zpq, gpu_ctx, header, members, oracle_rounds(("alt", what), header, members), before_call=before_call)


# ---------------------------------------------------------------- sticky failures
def test_encoder_overflow_is_sticky(zpq, gpu_ctx, clean_env):
    header = C4B
    model = zpq.Model(header=header)
    n = 6
    codecs = [O.Codec(header) for _ in range(n)]
    enc = zpq.BlockSet(gpu_ctx, model, n, waves=True)
    assert enc.waves
    good = (0, 2, 3, 4, 5)
    segs = [cut(2, 64), cut(1, 300), cut(6, 64), cut(3, 65), cut(4, 17), cut(5, 3)]
    coded, status, out_len = enc.encode_segments(segs, cap=[4096, 16, 4096, 4096, 4096, 4096])   # 300 random bytes do not fit 16
    assert gpu_ctx.last_kernel_name == WAVES[0]
    assert [int(s) for s in status] == [0, E_OVERFLOW, 0, 0, 0, 0]
    assert int(out_len[1]) == len(O.Codec(header).encode(segs[1]))           # the encoder keeps counting
    assert [coded[m] for m in good] == [codecs[m].encode(segs[m]) for m in good]
    for k in range(2):
        segs = [cut(10 + 6 * k + m, 17 + 100 * m) for m in range(n)]
        coded, status, out_len = enc.encode_segments(segs)
        assert gpu_ctx.last_kernel_name == WAVES[0]
        assert [int(s) for s in status] == [0, E_OVERFLOW, 0, 0, 0, 0] and int(out_len[1]) == 0
        assert [coded[m] for m in good] == [codecs[m].encode(segs[m]) for m in good]
    coded, status, _ = enc.encode_segments([b"abc"], members=[1])
    assert [int(s) for s in status] == [E_OVERFLOW]
    enc.close()
    model.close()


def test_decoder_failures_touch_no_other_member(zpq, gpu_ctx, clean_env):
    """Round 1 of four: member 1's slab is too small for its segment, member 3's coded segment is cut to half (truncated),
    member 4's has 24 of its bytes replaced (damaged).  The decoder set follows one oracle codec per member through
    Codec.decode_prefix (the kernels' stop rule: EOF, or right after byte cap + 1) fed the same bytes: status, the stored bytes,
    consumed and the final code are the oracle's for every member in every round; a member that overflowed keeps that status
    with nothing decoded; every other member is untouched.  Decoded without ZPQ_FLAG_PP as decode_prefix does."""
    header, n = C4B, 7
    members = members_of(91, n, lengths=[65, 300, 700, 1500])
    coded = [list(c) for c in oracle_rounds(("dfail", "C4B"), header, members)[0]]
    r = random.Random(5)
    half = coded[3][1][:len(coded[3][1]) // 2]
    coded[3][1] = half
    bad = bytearray(coded[4][1])
    for k in range(8, min(32, len(bad))):
        bad[k] = r.getrandbits(8)
    coded[4][1] = bytes(bad)
    model = zpq.Model(header=header)
    dec = zpq.BlockSet(gpu_ctx, model, n, waves=True)
    assert dec.waves
    mirror = [O.Codec(header) for _ in range(n)]
    failed = {}
    full = MAXLEN + 8
    for k in range(ROUNDS):
        live = [m for m in range(n) if not (k == 1 and m == 1)]
        calls = [(live, full)] + ([([1], 16)] if k == 1 else [])                # (one cap per call: member 1's small slab apart)
        for idx, cap in calls:
            back, status, consumed, code, _ = dec.decode_segments([coded[m][k] for m in idx], cap=cap, members=idx, flags=0)
            if any(m not in failed for m in idx):
                assert gpu_ctx.last_kernel_name == WAVES[1]
            for j, m in enumerate(idx):
                if m in failed:
                    assert int(status[j]) == failed[m] and back[j] == b"", (k, m)
                    continue
                data, out_len, cons, fcode, _ = mirror[m].decode_prefix(coded[m][k], cap)
                want_status = E_OVERFLOW if out_len > cap else 0
                assert int(status[j]) == want_status, (k, m, int(status[j]), out_len)
                assert len(back[j]) <= cap and back[j] == data, (k, m, len(back[j]), len(data))
                assert int(consumed[j]) == cons and int(code[j]) == fcode, (k, m)
                if m not in (1, 3, 4) or k == 0:
                    assert want_status == 0 and back[j] == b"\0" + members[m][k], (k, m)
                if want_status:
                    failed[m] = want_status
    assert failed.get(1) == E_OVERFLOW
    dec.close()
    model.close()


# ---------------------------------------------------------------- the request, honoured or not
def requesting(zpq):
    return types.SimpleNamespace(Model=zpq.Model, BlockSet=lambda *a, **k: zpq.BlockSet(*a, waves=True, **k))


@pytest.mark.parametrize("what", ["n16", "mix9", "ring138", "match_buf0", "hh_small", "n17", "level2"])
def test_a_request_that_decides_nothing(zpq, gpu_ctx, clean_env, what):
    """Outside the envelope of the wave kernels (16 components, a MIX of 9 inputs, rings beyond the LDS, a one-byte MATCH
    buffer, a program that is not the hash chain, 17 components) and on a chain model: the flags come back without 16 and the
    kernels are those of the parent."""
    header = zpq.level_header(2) if what == "level2" else GM.NAMED[what][0]
    names = CHAIN if what == "level2" else (LANES if GM.NAMED[what][1][3] == GM.LANES else ROWS)
    assert not waves_honoured(zpq, header)
    model = zpq.Model(header=header)
    st = zpq.BlockSet(gpu_ctx, model, 3, waves=True)
    assert st.waves is False and st.lanes is (what != "level2")
    assert zpq.lib().zpq_blockset_flags(st.h) == (0 if what == "level2" else 1)
    assert gpu_ctx.blockset_capacity(model, waves=True) == gpu_ctx.blockset_capacity(model, lanes=True)
    st.close()
    model.close()
    members = [[s[:300] for s in segs[:2]] for segs in make_members(3, nmembers=3)]
    check_parity(requesting(zpq), gpu_ctx, header, members, oracle_history(header, members), *names)


def test_the_environment_makes_and_withdraws_the_request(zpq, gpu_ctx, clean_env):
    model = zpq.Model(header=C4B)
    seg = [cut(2, 108)]
    want = O.Codec(C4B).encode(seg[0])
    table = ((("1", "1"), {}, 17), (("1", "1"), {"lanes": True}, 17), (("1", None), {}, 0), (("1", None), {"lanes": True}, 17),
             ((None, "1"), {}, 1), ((None, "1"), {"waves": True}, 17), (("0", "1"), {"waves": True}, 1),
             (("0", None), {"waves": True}, 1), (("1", "0"), {"waves": True}, 0), (("x", None), {"waves": True}, 17),
             (("x", "1"), {}, 1), ((None, None), {"waves": True}, 17), ((None, None), {"lanes": True}, 1), ((None, None), {}, 0))
    for (ew, el), kw, flags in table:
        for var, val in (("ZPQ_SET_WAVES", ew), ("ZPQ_SET_LANES", el)):
            if val is None:
                clean_env.delenv(var, raising=False)
            else:
                clean_env.setenv(var, val)
        st = zpq.BlockSet(gpu_ctx, model, 2, **kw)
        assert zpq.lib().zpq_blockset_flags(st.h) == flags, (ew, el, kw)
        assert (st.waves, st.lanes) == (bool(flags & 16), bool(flags & 1))
        assert st.encode_segments(seg, members=[1])[0][0] == want
        assert gpu_ctx.last_kernel_name == {17: WAVES[0], 1: ROWS[0], 0: GENERIC[0]}[flags], (ew, el, kw)
        st.close()
    model.close()


def test_the_plain_entry_point_and_the_capacity_are_unchanged(zpq, gpu_ctx, clean_env):
    L = zpq.lib()
    model = zpq.Model(header=C4B)
    out = C.c_void_p()
    assert L.zpq_blockset_create(gpu_ctx.h, model.h, 3, 0, C.byref(out)) == 0
    assert L.zpq_blockset_flags(out) == 0
    L.zpq_blockset_destroy(out)
    st = zpq.BlockSet(gpu_ctx, model, 3)
    assert (st.waves, st.lanes, st.pipe) == (False, False, False)
    seg = cut(6, 200)
    assert st.encode_segments([seg], members=[2])[0][0] == O.Codec(C4B).encode(seg)
    assert gpu_ctx.last_kernel_name == GENERIC[0]
    st.close()
    for header in (C4B, GM.NAMED["match_min"][0], GM.NAMED["mix_x4"][0]):
        m = zpq.Model(header=header)
        lanes, waves = gpu_ctx.blockset_capacity(m, lanes=True), gpu_ctx.blockset_capacity(m, waves=True)
        assert 1 <= gpu_ctx.blockset_capacity(m) <= lanes == waves <= 1 << 20
        assert L.zpq_blockset_capacity_ex(gpu_ctx.h, m.h, 0, 17) == lanes
        assert L.zpq_blockset_capacity_ex(gpu_ctx.h, m.h, 0, 16) == gpu_ctx.blockset_capacity(m)      # alone: decides nothing
        out = C.c_void_p(0x1234)
        assert L.zpq_blockset_create_ex(gpu_ctx.h, m.h, waves + 1, 0, 17, C.byref(out)) == E_NOMEM and out.value is None
        for bad in (18, 24, 32):
            assert L.zpq_blockset_capacity_ex(gpu_ctx.h, m.h, 0, bad) == E_ARG
            assert L.zpq_blockset_create_ex(gpu_ctx.h, m.h, 1, 0, bad, C.byref(out)) == E_ARG and out.value is None
        m.close()
    model.close()


def test_lifetime_orders(zpq):
    """On a context of the test's own: the set first; the model dropped before the set built on it; the ctx before the set
    (orphaned: ZPQ_E_CLOSED from both directions, destroy still fine)."""
    header = C4B
    seg = cut(2, 150)
    want = O.Codec(header).encode(seg)
    ctx = zpq.Context(0)
    model = zpq.Model(header=header)
    a = zpq.BlockSet(ctx, model, 2, waves=True)
    b = zpq.BlockSet(ctx, model, 3, waves=True)
    assert a.waves and b.waves
    assert a.encode_segments([seg], members=[1])[0][0] == want
    assert ctx.last_kernel_name == WAVES[0]
    a.close()
    zpq.lib().zpq_model_destroy(model.h)
    model.h = None
    assert b.decode_segments([want], cap=200, members=[2])[0][0] == seg
    assert ctx.last_kernel_name == WAVES[1]
    zpq.lib().zpq_ctx_destroy(ctx.h)                       # the ctx before the set, through the raw call
    ctx.h = None
    with pytest.raises(zpq.ZpqError) as e:
        b.encode_segments([b"abc"], members=[0])
    assert e.value.code == E_CLOSED
    with pytest.raises(zpq.ZpqError) as e:
        b.decode_segments([want], cap=200, members=[0])
    assert e.value.code == E_CLOSED
    b.close()
    ctx2 = zpq.Context(0)
    m2 = zpq.Model(header=header)
    c = zpq.BlockSet(ctx2, m2, 2, waves=True)
    ctx2.close()                                           # the binding's order: children first
    assert c.h is None
