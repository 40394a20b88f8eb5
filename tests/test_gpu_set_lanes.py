"""Block sets of general models on the lane-per-component kernels (ZPQ_SET_LANES, BlockSet(..., lanes=True)): one launch
of k_rows / k_lanes<..., KEEP> per round, the state of every member handed from launch to launch through its slot --
tables, the ZPAQL machine (a b c d f pc, M, H, R), MATCH's scalars, and p[], the last bit's predictions, which the
reference keeps across segments (a component whose input index is not below its own reads them at the next segment's
first bit).  Expected bytes come from oracle_lib.Codec, one codec per member and one encode per segment."""
import os
import random
import sys
import types

import pytest

import general_models as GM
import oracle_lib as O
import zpaql_programs as ZP
from test_gpu_blockset import LENGTHS, NMEMBERS, _data, check_parity, make_members, oracle_history

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from inputs import C4B  # noqa: E402
from test_gpu_lanes import MODELS, hdr as lanes_hdr  # noqa: E402

pytestmark = pytest.mark.gpu

KNOBS = ("ZPQ_SET_LANES", "ZPQ_LANES_ROWS", "ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE", "ZPQ_VM_PIPE")
E_ARG, E_NOMEM, E_OVERFLOW, E_VMSTEPS, E_CLOSED = -2, -6, -7, -8, -10
ROWS, LANES = ("k_rows<encode>", "k_rows<decode>"), ("k_lanes<encode>", "k_lanes<decode>")

NAMED = ["bits0_all", "ht_edge", "match_idx_gt_buf", "rates",      # rows, hash chain
         "hm0", "perturbed_rows",                                  # rows, interpreter
         "n17", "n64", "mix_wave64",                               # lanes, hash chain
         "perturbed_lanes", "mix3_sse3_n22_vm",                    # lanes, interpreter
         "fwd_n20"]                                                # forward references: p[] across segments


@pytest.fixture()
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def requesting(zpq):
    """The two names check_parity uses, every set made with lanes=True."""
    return types.SimpleNamespace(Model=zpq.Model, BlockSet=lambda *a, **k: zpq.BlockSet(*a, lanes=True, **k))


def model_case(zpq, what):
    """(header, (encode kernel, decode kernel)) of a case of the parity test."""
    if what == "C4B":
        return C4B, ROWS
    if what in MODELS:
        return lanes_hdr(MODELS[what]), ROWS
    header, route = GM.NAMED[what]
    return header, (ROWS if route[3] == GM.ROWS else LANES)


def honoured(zpq, header):
    m = zpq.Model(header=header)
    try:
        return zpq.lib().zpq_blockset_lanes_applies(m.h) == 1
    finally:
        m.close()


def four_segments(seed, nmembers=NMEMBERS):
    r = random.Random(seed)
    return [[_data(r, (m + s) % 4, r.choice(LENGTHS)) for s in range(4)] for m in range(nmembers)]


def parity_members(what):
    """The members of test_parity's case `what` (test_set_lanes_cpu.py shows on the host that those of fwd_isse and fwd_avg tell
    a kept p[] from a zeroed one)."""
    return make_members(2000 + len(what) * 7 + sum(what.encode()))


# ---------------------------------------------------------------- parity, both directions, kernel names asserted
@pytest.mark.parametrize("what", ["C4B"] + NAMED + ["isse_stale_input", "fwd_isse", "fwd_avg"])
def test_parity(zpq, gpu_ctx, clean_env, what):
    """(fwd_isse, fwd_avg: forward references that reach the coded prediction.  fwd_n20's last component is a MIX over
    itself whose prediction stays 0, isse_stale_input's ISSE feeds nothing: their streams do not depend on p[].)"""
    header, names = model_case(zpq, what)
    assert honoured(zpq, header)
    members = parity_members(what)
    assert len(members) == 21 and {len(s) for s in members} == {1, 2, 3, 4}
    check_parity(requesting(zpq), gpu_ctx, header, members, oracle_history(header, members), *names)


@pytest.mark.parametrize("shape", ["rows", "lanes"])
@pytest.mark.parametrize("name", ZP.SEGMENT_PROGRAMS + ("loop_hh9_hm16",))
def test_the_vm_goes_from_launch_to_launch(zpq, gpu_ctx, clean_env, name, shape):
    """a b c d f pc, M, H and R of 21 members through the set's slots (loop_hh9_hm16: an H of 512 words, which k_lanes
    leaves in the slot; the others' H of 16 or 32 words it keeps in LDS and copies in and out)."""
    header, _ = ZP.embed(ZP.NAMED[name], shape)
    assert honoured(zpq, header)
    members = make_members(700 + len(name) + len(shape))
    assert any(len(s) == 0 for segs in members for s in segs)
    check_parity(requesting(zpq), gpu_ctx, header, members, oracle_history(header, members), *(ROWS if shape == "rows" else LANES))


# ---------------------------------------------------------------- one format in the slot for both kernels
@pytest.mark.parametrize("what", ["C4B", "perturbed_rows", "match_idx_gt_buf", "d_walks_h"])
def test_rows_and_lanes_alternate_on_one_set(zpq, gpu_ctx, clean_env, what):
    """Rounds 0 and 2 on k_rows, rounds 1 and 3 on k_lanes (ZPQ_LANES_ROWS=0): the bytes still equal the oracle's."""
    header = ZP.embed(ZP.NAMED[what], "rows")[0] if what == "d_walks_h" else model_case(zpq, what)[0]
    assert header[4] <= 16
    members = four_segments(31 + len(what))
    want = oracle_history(header, members)
    model = zpq.Model(header=header)
    enc, dec = zpq.BlockSet(gpu_ctx, model, NMEMBERS, lanes=True), zpq.BlockSet(gpu_ctx, model, NMEMBERS, lanes=True)
    assert enc.lanes and dec.lanes
    for r in range(4):
        if r % 2:
            clean_env.setenv("ZPQ_LANES_ROWS", "0")
        else:
            clean_env.delenv("ZPQ_LANES_ROWS", raising=False)
        names = LANES if r % 2 else ROWS
        coded, status, _ = enc.encode_segments([members[m][r] for m in range(NMEMBERS)])
        assert gpu_ctx.last_kernel_name == names[0]
        assert (status == 0).all() and coded == [want[m][r] for m in range(NMEMBERS)], r
        back, status, consumed, _, first = dec.decode_segments(coded, cap=1500 + 8)
        assert gpu_ctx.last_kernel_name == names[1]
        assert (status == 0).all() and back == [members[m][r] for m in range(NMEMBERS)], r
        assert [int(c) for c in consumed] == [len(c) for c in coded] and all(int(f) == 0 for f in first)
    enc.close()
    dec.close()
    model.close()


# ---------------------------------------------------------------- subsets, and a batch on the pool between two rounds
def test_subsets_and_a_batch_between(zpq, gpu_ctx, clean_env):
    header = C4B
    model = zpq.Model(header=header)
    r = random.Random(9)
    codecs = [O.Codec(header) for _ in range(8)]
    enc = zpq.BlockSet(gpu_ctx, model, 8, lanes=True)
    assert enc.lanes

    def call(idx):
        segs = [_data(r, (m + len(idx)) % 4, r.choice([1, 17, 65, 300])) for m in idx]
        coded, status, _ = enc.encode_segments(segs, members=idx)
        assert gpu_ctx.last_kernel_name == "k_rows<encode>"
        assert [int(s) for s in status] == [0] * len(idx)
        for j, m in enumerate(idx):
            assert coded[j] == codecs[m].encode(segs[j], pp=True), (idx, m)

    call([5, 2, 7])
    call([2, 0, 5, 1])                                    # 0 and 1 are fresh, 2 and 5 are not
    blocks = [_data(r, k % 4, 200) for k in range(14)]    # the ctx's slot pool, never the set's slots
    coded, status, _ = gpu_ctx.encode_blocks(model, blocks)
    assert (status == 0).all() and coded == O.encode_blocks(header, blocks)
    call([7, 1, 3, 0])
    call([6, 4, 2])
    call(list(range(8)))
    enc.close()
    model.close()


# ---------------------------------------------------------------- sticky failures
@pytest.mark.parametrize("what", ["C4B", "n17"])
def test_overflow_is_sticky(zpq, gpu_ctx, clean_env, what):
    header, names = model_case(zpq, what)
    model = zpq.Model(header=header)
    r = random.Random(11)
    n = 6
    codecs = [O.Codec(header) for _ in range(n)]
    enc = zpq.BlockSet(gpu_ctx, model, n, lanes=True)
    assert enc.lanes
    segs = [_data(r, 2, 64), _data(r, 1, 300), _data(r, 2, 64), _data(r, 3, 65), _data(r, 0, 17), _data(r, 1, 3)]
    coded, status, out_len = enc.encode_segments(segs, cap=[4096, 16, 4096, 4096, 4096, 4096])   # 300 random bytes do not fit 16
    assert gpu_ctx.last_kernel_name == names[0]
    assert [int(s) for s in status] == [0, E_OVERFLOW, 0, 0, 0, 0]
    assert [coded[m] for m in (0, 2, 3, 4, 5)] == [codecs[m].encode(segs[m]) for m in (0, 2, 3, 4, 5)]
    for _ in range(2):
        segs = [_data(r, 2, 17) for _ in range(n)]
        coded, status, out_len = enc.encode_segments(segs)
        assert [int(s) for s in status] == [0, E_OVERFLOW, 0, 0, 0, 0] and int(out_len[1]) == 0
        assert [coded[m] for m in (0, 2, 3, 4, 5)] == [codecs[m].encode(segs[m]) for m in (0, 2, 3, 4, 5)]
    coded, status, _ = enc.encode_segments([b"abc"], members=[1])
    assert [int(s) for s in status] == [E_OVERFLOW]
    enc.close()
    model.close()


@pytest.mark.parametrize("shape", ["rows", "lanes"])
def test_the_step_cap_is_sticky(zpq, gpu_ctx, clean_env, shape):
    """a== 255; jf; jmp self before the hash chain: a run never ends on byte 0xFF.  Members 1, 6 and 7 of 12 meet such a
    byte in round 0: ZPQ_E_VMSTEPS then and in every later call, from the encoder and from the decoder; the nine others,
    in the same rows and waves, equal the oracle throughout."""
    header, offs = ZP.embed(ZP.STEP_CAP, shape)
    model = zpq.Model(header=header, offsets=offs)
    names = ROWS if shape == "rows" else LANES
    first = ZP.step_cap_batch()
    r = random.Random(13)
    rounds = [first, [bytes(r.randrange(255) for _ in range(n)) for n in (17, 3, 40, 0, 1, 65, 2, 30, 9, 33, 40, 5)],
              [bytes(r.randrange(255) for _ in range(20)) for _ in range(12)]]
    capped, good = (1, 6, 7), (0, 2, 3, 4, 5, 8, 9, 10, 11)
    codecs = [O.Codec(header, offs) for _ in range(12)]
    want = [[codecs[m].encode(rounds[k][m]) if m in good else None for m in range(12)] for k in range(3)]
    enc, dec = zpq.BlockSet(gpu_ctx, model, 12, lanes=True), zpq.BlockSet(gpu_ctx, model, 12, lanes=True)
    assert enc.lanes and dec.lanes
    streams0 = [O.Codec(header, offs).encode(b) for b in first]    # (the oracle has the same cap: its streams of the capped members are only an input)
    for k in range(3):
        coded, status, out_len = enc.encode_segments(rounds[k])
        assert gpu_ctx.last_kernel_name == names[0]
        assert [int(s) for s in status] == [E_VMSTEPS if m in capped else 0 for m in range(12)], (k, list(status))
        assert [coded[m] for m in good] == [want[k][m] for m in good], k
        if k:
            assert all(int(out_len[m]) == 0 for m in capped)
        feed = [want[k][m] if m in good else (streams0[m] if k == 0 else b"\0\0\0\0") for m in range(12)]
        back, status, _, _, _ = dec.decode_segments(feed, cap=72)
        assert gpu_ctx.last_kernel_name == names[1]
        assert [int(s) for s in status] == [E_VMSTEPS if m in capped else 0 for m in range(12)], (k, list(status))
        assert [back[m] for m in good] == [rounds[k][m] for m in good], k
    enc.close()
    dec.close()
    model.close()


# ---------------------------------------------------------------- damaged input
def test_damaged_segments_touch_no_other_member(zpq, gpu_ctx, clean_env):
    """Round 1 of three: member 3's coded segment cut to half, member 8's replaced by 64 random bytes.  The decoder set
    follows one oracle codec per member through Codec.decode_prefix (the kernels' stop rule), fed the same bytes: status
    (0, or ZPQ_E_OVERFLOW with out_len = cap + 1 as for batches), out_len, the stored bytes and consumed are the
    oracle's for every member in every round, the damaged ones included; a stored prefix never exceeds the slab.
    Decoded without ZPQ_FLAG_PP: the PP byte is then the first output byte, as in decode_prefix."""
    header, cap = C4B, 1500 + 8
    members = four_segments(77)
    members = [segs[:3] for segs in members]
    coded = oracle_history(header, members)
    r = random.Random(5)
    coded[3][1] = coded[3][1][:len(coded[3][1]) // 2]
    coded[8][1] = bytes(r.getrandbits(8) for _ in range(64))
    model = zpq.Model(header=header)
    dec = zpq.BlockSet(gpu_ctx, model, NMEMBERS, lanes=True)
    assert dec.lanes
    mirror = [O.Codec(header) for _ in range(NMEMBERS)]
    failed = {}
    for k in range(3):
        back, status, consumed, code, _ = dec.decode_segments([coded[m][k] for m in range(NMEMBERS)], cap=cap, flags=0)
        assert gpu_ctx.last_kernel_name == "k_rows<decode>"
        for m in range(NMEMBERS):
            if m in failed:
                assert int(status[m]) == failed[m] and back[m] == b"", (k, m)
                continue
            data, out_len, cons, fcode, _ = mirror[m].decode_prefix(coded[m][k], cap)
            want_status = E_OVERFLOW if out_len > cap else 0
            assert int(status[m]) == want_status, (k, m, int(status[m]), out_len)
            assert len(back[m]) <= cap and back[m] == data, (k, m, len(back[m]), len(data))
            assert int(consumed[m]) == cons and int(code[m]) == fcode, (k, m)
            if m not in (3, 8):
                assert want_status == 0 and back[m] == b"\0" + members[m][k], (k, m)
            if want_status:
                failed[m] = want_status
    dec.close()
    model.close()


# ---------------------------------------------------------------- the request, honoured or not
def test_a_request_that_decides_nothing(zpq, gpu_ctx, clean_env):
    for header, names in ((zpq.level_header(2), ("k_chain<encode>", "k_chain<decode>")),
                          (GM.NAMED["n65"][0], ("k_generic<encode>", "k_generic<decode>"))):
        assert not honoured(zpq, header)
        model = zpq.Model(header=header)
        st = zpq.BlockSet(gpu_ctx, model, 3, lanes=True)
        assert st.lanes is False
        assert gpu_ctx.blockset_capacity(model, lanes=True) == gpu_ctx.blockset_capacity(model)
        st.close()
        model.close()
        members = [[s[:64] for s in segs[:2]] for segs in make_members(3, nmembers=3)]
        check_parity(requesting(zpq), gpu_ctx, header, members, oracle_history(header, members), *names)


def test_the_old_entry_point_is_unchanged(zpq, gpu_ctx, clean_env):
    assert "ZPQ_SET_LANES" not in os.environ
    members = [segs[:2] + [b"x" * 17] * (2 - len(segs[:2])) for segs in make_members(3, nmembers=3)]
    check_parity(zpq, gpu_ctx, C4B, members, oracle_history(C4B, members), "k_generic<encode>", "k_generic<decode>")
    model = zpq.Model(header=C4B)
    st = zpq.BlockSet(gpu_ctx, model, 3, lanes=False)
    assert st.lanes is False and zpq.lib().zpq_blockset_flags(st.h) == 0
    st.close()
    model.close()


def test_the_environment_makes_and_withdraws_the_request(zpq, gpu_ctx, clean_env):
    model = zpq.Model(header=C4B)
    seg = [b"environment " * 9]
    want = O.Codec(C4B).encode(seg[0])
    for env, lanes, is_lanes in (("1", False, True), ("0", True, False), ("x", True, True), ("x", False, False)):
        clean_env.setenv("ZPQ_SET_LANES", env)
        st = zpq.BlockSet(gpu_ctx, model, 2, lanes=lanes)
        assert st.lanes is is_lanes, (env, lanes)
        assert st.encode_segments(seg, members=[1])[0][0] == want
        assert gpu_ctx.last_kernel_name == ("k_rows<encode>" if is_lanes else "k_generic<encode>")
        st.close()
    model.close()


def test_capacity_is_bounded_by_memory(zpq, gpu_ctx, clean_env):
    """No allocation of any size: one member beyond the capacity is refused by arithmetic, before any memory is asked for."""
    L = zpq.lib()
    import ctypes as C
    for header in (C4B, GM.NAMED["match_min"][0], GM.NAMED["n64"][0]):
        model = zpq.Model(header=header)
        default, lanes = gpu_ctx.blockset_capacity(model), gpu_ctx.blockset_capacity(model, lanes=True)
        assert 1 <= default <= lanes <= 1 << 20, (default, lanes)
        out = C.c_void_p(0x1234)
        assert L.zpq_blockset_create_ex(gpu_ctx.h, model.h, lanes + 1, 0, zpq.SET_LANES, C.byref(out)) == E_NOMEM
        assert out.value is None
        assert L.zpq_blockset_capacity_ex(gpu_ctx.h, model.h, 0, 2) == E_ARG
        assert L.zpq_blockset_create_ex(gpu_ctx.h, model.h, 1, 0, 2, C.byref(out)) == E_ARG and out.value is None
        model.close()
    # a slot of a few KiB: the cap of 2^20 members, not memory, is the bound -- and far beyond what is resident at once
    model = zpq.Model(header=GM.NAMED["match_min"][0])
    assert gpu_ctx.blockset_capacity(model, lanes=True) == 1 << 20 > gpu_ctx.blockset_capacity(model)
    model.close()


def test_lifetime_orders(zpq):
    """On a context of the test's own: the set first; the ctx first (the set is orphaned: ZPQ_E_CLOSED, destroy still
    fine); the model dropped before the set that was built on it."""
    header = C4B
    want = O.Codec(header).encode(b"abc" * 50)
    ctx = zpq.Context(0)
    model = zpq.Model(header=header)
    a = zpq.BlockSet(ctx, model, 2, lanes=True)
    b = zpq.BlockSet(ctx, model, 3, lanes=True)
    assert a.lanes and b.lanes
    assert a.encode_segments([b"abc" * 50], members=[1])[0][0] == want
    a.close()                                              # the set before its ctx
    zpq.lib().zpq_model_destroy(model.h)                   # the model before the set: the set holds a reference
    model.h = None
    assert b.encode_segments([b"abc" * 50], members=[2])[0][0] == want
    assert ctx.last_kernel_name == "k_rows<encode>"
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
    c = zpq.BlockSet(ctx2, m2, 2, lanes=True)
    ctx2.close()                                           # the binding's order: children first
    assert c.h is None
