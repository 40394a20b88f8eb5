"""Chunked coding on block sets (zpq_blockset_{encode,decode}_chunks, binding.BlockSet.encode_chunks / decode_chunks): a
member's segment a piece at a time, the coder and the predictor carried from launch to launch through the set's slots.
Expected values come from oracle_lib.Codec used as test_gpu_blockset.oracle_history uses it -- one Codec per member, one
encode per WHOLE segment: a segment's chunks, one behind the other, must be exactly that.  The plan of members, chunks
and calls is tests/set_chunks.py (checked on its own by test_set_chunks_cpu.py)."""
import os
import random
import sys

import numpy as np
import pytest

import chain_models as CM
import general_models as GM
import oracle_lib as O
import set_chunks as SC
import zpaql_programs as ZP

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

pytestmark = pytest.mark.gpu

# the models and knob settings of test_gpu_blockset.py (test_every_route, test_other_routes)
KNOBS = ("ZPQ_ENC_PIPE", "ZPQ_ENC_SPLIT", "ZPQ_DEC_PIPE", "ZPQ_DEC_HYP16", "ZPQ_SPARSE_MODE", "ZPQ_SPARSE_FORCE_LOG2",
         "ZPQ_CHAIN_G", "ZPQ_CHAIN_BPW", "ZPQ_SET_LANES", "ZPQ_SET_PIPE", "ZPQ_SET_WAVES", "ZPQ_SET_VMWAVES")
NAMES = ["l1_sizes", "l2_hh2_hm1", "l2_hm0", "l3_mixed", "chain7", "l4_rate255", "l5_small", "mix2_chain3", "chain16"]
ROUTES = [(w, {}) for w in [1, 2, 3, 4, 5] + NAMES] + [
    (3, {"ZPQ_SPARSE_FORCE_LOG2": "10"}), ("l3_mixed", {"ZPQ_SPARSE_FORCE_LOG2": "10"}),
    (3, {"ZPQ_DEC_HYP16": "0"}), (4, {"ZPQ_DEC_HYP16": "0"}),
    (2, {"ZPQ_SPARSE_MODE": "never"}), (3, {"ZPQ_SPARSE_MODE": "never"}),
    (3, {"ZPQ_SPARSE_MODE": "never", "ZPQ_DEC_HYP16": "0"})]
E_OVERFLOW, E_TOOBIG, E_ARG = -7, -4, -2
NO_BYTE = 0xFFFFFFFF
FILL = 0xEE
CHAIN = ("k_chain<encode>", "k_chain<decode>")
GENERIC = ("k_generic<encode>", "k_generic<decode>")


@pytest.fixture()
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def header_of(zpq, what):
    return zpq.level_header(what) if isinstance(what, int) else CM.NAMED[what][0]


_PLANS, _WANT = {}, {}


def plan_of(env=None, nmembers=SC.NMEMBERS):
    """the plan (computed once, never changed); the short-chunk form where a line store is forced small (set_chunks.make_plan)"""
    short = bool(env) and "ZPQ_SPARSE_FORCE_LOG2" in env
    key = (short, nmembers)
    if key not in _PLANS:
        _PLANS[key] = SC.make_plan(nmembers=nmembers, lengths=SC.SHORT_LENGTHS if short else SC.CHUNK_LENGTHS)
    return _PLANS[key]


def oracle_history(header, plan, key):
    """coded[m][s]: what the sequential coder writes for the WHOLE segment s of member m (computed once per model and plan)"""
    if key not in _WANT:
        out = []
        for segs in plan.members:
            codec = O.Codec(header)
            out.append([codec.encode(seg, pp=True) for seg in segs])
        _WANT[key] = out
    return _WANT[key]


def promise(plan):
    return max(sum(len(s) for s in segs) for segs in plan.members)


def encode_plan(zpq, ctx, st, plan, want, name):
    """Every round of the plan through encode_chunks: status, out_len, the bytes so far against the oracle's stream, and
    every member's open mark after every call.  Returns coded[m][s], the chunks joined."""
    acc = [[b"" for _ in segs] for segs in plan.members]
    is_open = [False] * len(plan.members)
    for t, rnd in enumerate(plan.rounds):
        for ch in rnd:
            assert is_open[ch.member] == (not ch.opens), (t, ch.member)
        coded, status, out_len = st.encode_chunks([ch.data for ch in rnd], [ch.more for ch in rnd],
                                                  members=[ch.member for ch in rnd])
        assert ctx.last_kernel_name == name, (t, ctx.last_kernel_name)
        assert [int(s) for s in status] == [0] * len(rnd), (t, list(status))
        for j, ch in enumerate(rnd):
            assert int(out_len[j]) == len(coded[j]), (t, ch.member)
            acc[ch.member][ch.seg] += coded[j]
            w = want[ch.member][ch.seg]
            got = acc[ch.member][ch.seg]
            if ch.more:
                assert w[:len(got)] == got and len(got) < len(w), ("chunk", t, ch.member, ch.seg, ch.idx, len(ch.data))
            else:
                assert got == w, ("segment", t, ch.member, ch.seg, ch.idx, len(got), len(w))
            is_open[ch.member] = ch.more
        assert [st.member_open(m) for m in range(len(plan.members))] == is_open, t
    assert not any(is_open)
    return acc


def decode_plan(zpq, ctx, st, plan, want, name):
    """The oracle's streams through decode_chunks, the caps cycling per call (set_chunks.simulate_decode): bytes, out_len,
    open, first_byte and the member's open mark of every call; a segment's consumed[] add up to its stream."""
    pos = [0] * len(plan.members)                           # where member m's decoder stands in its current stream
    exact = closing = 0
    after_exact = set()
    for t, call in enumerate(SC.simulate_decode(plan.members)):
        back, status, consumed, _, first, opened = st.decode_chunks(
            [want[s.member][s.seg][pos[s.member]:] for s in call], [s.cap for s in call], members=[s.member for s in call])
        assert ctx.last_kernel_name == name, (t, ctx.last_kernel_name)
        assert [int(x) for x in status] == [0] * len(call), (t, list(status))        # (never ZPQ_E_OVERFLOW)
        for j, s in enumerate(call):
            what = (t, s.member, s.seg, s.cap, s.begin)
            assert back[j] == plan.members[s.member][s.seg][s.begin:s.begin + s.take], ("bytes",) + what
            assert int(opened[j]) == (1 if s.open else 0), ("open",) + what           # 1 while bytes remain, or the slab is just full
            assert int(first[j]) == (0 if s.opening else NO_BYTE), ("first_byte",) + what
            assert st.member_open(s.member) == s.open, what
            pos[s.member] += int(consumed[j])
            if s.member in after_exact:
                after_exact.discard(s.member)
                if s.cap:                                   # the call behind an exact fit finds nothing but the EOF
                    assert (len(back[j]), int(opened[j])) == (0, 0), what
                    closing += 1
                else:
                    after_exact.add(s.member)               # (no room to look: still open)
            if s.exact:
                exact += 1
                after_exact.add(s.member)
            if not s.open:
                assert pos[s.member] == len(want[s.member][s.seg]), ("consumed",) + what
                pos[s.member] = 0
    return exact, closing


# ---------------------------------------------------------------- 1, 2: the chain kernels
@pytest.mark.parametrize("what,env", ROUTES, ids=str)
def test_chain_encode(zpq, gpu_ctx, clean_env, what, env):
    for k, v in env.items():
        clean_env.setenv(k, v)
    header, plan = header_of(zpq, what), plan_of(env)
    want = oracle_history(header, plan, (what, "ZPQ_SPARSE_FORCE_LOG2" in env))
    model = zpq.Model(header=header)
    st = zpq.BlockSet(gpu_ctx, model, len(plan.members), max_member_bytes=promise(plan))
    try:
        encode_plan(zpq, gpu_ctx, st, plan, want, CHAIN[0])
        if "ZPQ_SPARSE_FORCE_LOG2" in env:
            assert gpu_ctx.last_line_store == 1024
        if env.get("ZPQ_SPARSE_MODE") == "never":
            assert gpu_ctx.last_line_store == 0
    finally:
        st.close()
        model.close()


@pytest.mark.parametrize("level", [1, 2, 3, 5])
def test_a_pipe_set_codes_chunks_on_the_chain_encoder(zpq, gpu_ctx, clean_env, level):
    header, plan = zpq.level_header(level), plan_of()
    want = oracle_history(header, plan, (level, False))
    model = zpq.Model(header=header)
    st = zpq.BlockSet(gpu_ctx, model, len(plan.members), max_member_bytes=promise(plan), pipe=True)
    try:
        assert st.pipe and any(len(rnd) >= 12 for rnd in plan.rounds)
        encode_plan(zpq, gpu_ctx, st, plan, want, CHAIN[0])
        # ... and whole segments on the same set still take the pipeline (12 closed members)
        segs = [bytes([65 + m]) * 40 for m in range(12)]
        ref = [O.Codec(header) for _ in range(12)]
        for m in range(12):
            for seg in plan.members[m]:
                ref[m].encode(seg, pp=True)
        coded, status, _ = st.encode_segments(segs, members=list(range(12)))
        assert gpu_ctx.last_kernel_name == "k_pipe<encode>" and (status == 0).all()
        assert coded == [ref[m].encode(segs[m], pp=True) for m in range(12)]
    finally:
        st.close()
        model.close()


@pytest.mark.parametrize("what,env", ROUTES, ids=str)
def test_chain_decode(zpq, gpu_ctx, clean_env, what, env):
    """levels 1-2 and their named kin: the eight-lane two-hypothesis decoders; levels 3-4: the sixteen-lane ones, and the
    one-copy decoders under ZPQ_DEC_HYP16=0; level 5, chain7, chain16, mix2_chain3: one copy, runtime loops among them"""
    for k, v in env.items():
        clean_env.setenv(k, v)
    header, plan = header_of(zpq, what), plan_of(env)
    want = oracle_history(header, plan, (what, "ZPQ_SPARSE_FORCE_LOG2" in env))
    model = zpq.Model(header=header)
    st = zpq.BlockSet(gpu_ctx, model, len(plan.members), max_member_bytes=promise(plan))
    try:
        exact, closing = decode_plan(zpq, gpu_ctx, st, plan, want, CHAIN[1])
        assert exact >= 3 and closing >= 1, (exact, closing)
    finally:
        st.close()
        model.close()


# ---------------------------------------------------------------- 3: the same bytes as the existing calls
@pytest.mark.parametrize("level", [2, 4])
def test_chunks_and_segments_give_the_same_bytes(zpq, gpu_ctx, clean_env, level):
    header, plan = zpq.level_header(level), plan_of()
    want = oracle_history(header, plan, (level, False))
    model = zpq.Model(header=header)
    n = len(plan.members)
    a, b = (zpq.BlockSet(gpu_ctx, model, n, max_member_bytes=promise(plan)) for _ in range(2))
    c, d = (zpq.BlockSet(gpu_ctx, model, n, max_member_bytes=promise(plan)) for _ in range(2))
    try:
        chunked = encode_plan(zpq, gpu_ctx, a, plan, want, CHAIN[0])
        decode_plan(zpq, gpu_ctx, c, plan, chunked, CHAIN[1])
        for r in range(3):
            idx = [m for m in range(n) if len(plan.members[m]) > r]
            coded, status, _ = b.encode_segments([plan.members[m][r] for m in idx], members=idx)
            assert (status == 0).all() and coded == [chunked[m][r] for m in idx], r
            back, status, consumed, _, first = d.decode_segments(coded, cap=700, members=idx)
            assert (status == 0).all() and back == [plan.members[m][r] for m in idx], r
            assert [int(x) for x in consumed] == [len(x) for x in coded] and (first == 0).all()
    finally:
        for s in (a, b, c, d):
            s.close()
        model.close()


# ---------------------------------------------------------------- 4: the lane-0 kernel
def _generic_models():
    from inputs import C4B
    return {"C4B": C4B,                                                    # all nine component types, a MATCH among them
            "fwd_n20": GM.NAMED["fwd_n20"][0],                             # forward references: p[] must cross a pause
            "d_walks_h": ZP.embed(ZP.NAMED["d_walks_h"], "rows")[0]}       # d is never reset: VM state from run to run


@pytest.mark.parametrize("name", ["C4B", "fwd_n20", "d_walks_h"])
def test_generic(zpq, gpu_ctx, clean_env, name):
    header = _generic_models()[name]
    if name == "fwd_n20":
        assert GM.has_forward_reference(header)
    plan = plan_of(nmembers=5)
    want = oracle_history(header, plan, (name, 5))
    model = zpq.Model(header=header)
    enc, dec = (zpq.BlockSet(gpu_ctx, model, 5) for _ in range(2))
    try:
        assert not enc.lanes
        encode_plan(zpq, gpu_ctx, enc, plan, want, GENERIC[0])
        decode_plan(zpq, gpu_ctx, dec, plan, want, GENERIC[1])
    finally:
        enc.close()
        dec.close()
        model.close()


@pytest.mark.parametrize("name", ["level2", "level4", "C4B"])
def test_an_empty_opening_chunk_without_the_pp_byte(zpq, gpu_ctx, clean_env, name):
    """reset() zeroes h[] and leaves the VM's H alone: a second segment opened by an empty chunk, with no PP byte, has coded
    no byte when it goes on and must do so with h[] = 0, not with what H holds from the first segment."""
    from inputs import C4B
    header = C4B if name == "C4B" else zpq.level_header(int(name[-1]))
    names = GENERIC if name == "C4B" else CHAIN
    r = random.Random(41)
    segs = [[SC._data(r, 2, 90), SC._data(r, 2 + m % 2, 70)] for m in range(5)]
    ref = [O.Codec(header) for _ in range(5)]
    want = [[ref[m].encode(seg, pp=False) for seg in segs[m]] for m in range(5)]
    model = zpq.Model(header=header)
    enc, dec = zpq.BlockSet(gpu_ctx, model, 5), zpq.BlockSet(gpu_ctx, model, 5)
    try:
        coded, status, _ = enc.encode_chunks([x[0] for x in segs], None, flags=0)           # with more == NULL: encode_segments
        assert (status == 0).all() and coded == [w[0] for w in want]
        got = [b""] * 5
        for k, (lo, hi) in enumerate(((0, 0), (0, 20), (20, 70))):
            coded, status, out_len = enc.encode_chunks([x[1][lo:hi] for x in segs], [k < 2] * 5, flags=0)
            assert (status == 0).all() and gpu_ctx.last_kernel_name == names[0]
            if k == 0:
                assert [int(x) for x in out_len] == [0] * 5                                    # nothing coded, nothing put
            got = [g + c for g, c in zip(got, coded)]
        assert got == [w[1] for w in want]
        back, status, consumed, _, first, opened = dec.decode_chunks([w[0] for w in want], 200, flags=0)
        assert (status == 0).all() and back == [x[0] for x in segs] and list(opened) == [0] * 5
        back, status, consumed, _, first, opened = dec.decode_chunks([w[1] for w in want], 0, flags=0)     # opens, decodes nothing
        assert (status == 0).all() and list(opened) == [1] * 5 and all(int(f) == NO_BYTE for f in first)
        assert gpu_ctx.last_kernel_name == names[1]
        back, status, c2, _, first, opened = dec.decode_chunks([w[1][int(c):] for w, c in zip(want, consumed)], 200, flags=0)
        assert (status == 0).all() and back == [x[1] for x in segs] and list(opened) == [0] * 5
        assert [int(a) + int(b) for a, b in zip(consumed, c2)] == [len(w[1]) for w in want]
    finally:
        enc.close()
        dec.close()
        model.close()


# ---------------------------------------------------------------- 5: refusals and failures
def test_an_open_member_is_refused_by_the_segment_calls(zpq, gpu_ctx, clean_env):
    header = zpq.level_header(2)
    model = zpq.Model(header=header)
    r = random.Random(3)
    data = [SC._data(r, 2, 200) for _ in range(3)]
    want = [O.Codec(header).encode(x, pp=True) for x in data]
    enc, dec = zpq.BlockSet(gpu_ctx, model, 3), zpq.BlockSet(gpu_ctx, model, 3)
    try:
        first, status, _ = enc.encode_chunks([x[:70] for x in data], [1, 0, 1])
        assert (status == 0).all() and [enc.member_open(m) for m in range(3)] == [True, False, True]
        for call in (lambda: enc.encode_segments([b"abc"], members=[0]), lambda: enc.encode_segments([b"a", b"b"], members=[1, 2]),
                     lambda: enc.decode_segments([want[0]], cap=300, members=[2]),
                     lambda: enc.decode_chunks([want[0]], 300, members=[0])):     # opened by the encoder: no decode call
            with pytest.raises(zpq.ZpqError) as e:
                call()
            assert e.value.code == E_ARG
        rest, status, _ = enc.encode_chunks([data[0][70:], data[2][70:]], None, members=[0, 2])
        assert (status == 0).all() and first[0] + rest[0] == want[0] and first[2] + rest[1] == want[2]
        assert not any(enc.member_open(m) for m in range(3))
        back, status, consumed, _, _, opened = dec.decode_chunks(want, 50)
        assert (status == 0).all() and list(opened) == [1, 1, 1] and back == [x[:50] for x in data]
        for call in (lambda: dec.decode_segments([want[1]], cap=300, members=[1]),
                     lambda: dec.encode_chunks([b"abc"], None, members=[1]), lambda: dec.encode_segments([b"abc"], members=[1])):
            with pytest.raises(zpq.ZpqError) as e:
                call()
            assert e.value.code == E_ARG
        more, status, c2, _, fb, opened = dec.decode_chunks([w[int(c):] for w, c in zip(want, consumed)], 300)
        assert (status == 0).all() and list(opened) == [0, 0, 0] and more == [x[50:] for x in data]
        assert [int(a) + int(b) for a, b in zip(consumed, c2)] == [len(w) for w in want] and all(int(f) == NO_BYTE for f in fb)
    finally:
        enc.close()
        dec.close()
        model.close()


def test_lanes_sets_and_noeof_are_refused(zpq, gpu_ctx, clean_env):
    from inputs import C4B
    model = zpq.Model(header=C4B)
    st = zpq.BlockSet(gpu_ctx, model, 2, lanes=True)
    plain = zpq.BlockSet(gpu_ctx, model, 2)
    try:
        assert st.lanes
        with pytest.raises(zpq.ZpqError) as e:
            st.encode_chunks([b"abc", b"def"], [1, 0])
        assert e.value.code == E_ARG
        with pytest.raises(zpq.ZpqError) as e:
            st.decode_chunks([b"\0" * 8, b"\0" * 8], 4)
        assert e.value.code == E_ARG
        assert not st.member_open(0)
        coded, status, _ = st.encode_segments([b"abc", b"def"])               # the set itself is as good as before
        assert (status == 0).all() and coded[0] == O.Codec(C4B).encode(b"abc", pp=True)
        for call in (lambda: plain.encode_chunks([b"abc"], [1], flags=zpq.FLAG_PP | 4), lambda: plain.decode_chunks([b"\0" * 8], 4, flags=4)):
            with pytest.raises(zpq.ZpqError) as e:
                call()
            assert e.value.code == E_ARG                                       # ZPQ_FLAG_NOEOF
        assert not plain.member_open(0)
    finally:
        st.close()
        plain.close()
        model.close()


def test_a_chunk_that_does_not_fit_fails_the_member(zpq, gpu_ctx, clean_env):
    header = zpq.level_header(2)
    model = zpq.Model(header=header)
    r = random.Random(11)
    data = [SC._data(r, 1, 300) for _ in range(3)]                              # random bytes: the coded stream is longer than they are
    want = [O.Codec(header).encode(x, pp=True) for x in data]
    st, roomy = zpq.BlockSet(gpu_ctx, model, 3), zpq.BlockSet(gpu_ctx, model, 3)
    try:
        # how many bytes the second chunk puts: from a set with room, whose three chunks joined are the oracle's stream
        parts = [roomy.encode_chunks([x[k:k + 100] for x in data], [k < 200] * 3)[0] for k in (0, 100, 200)]
        assert [parts[0][m] + parts[1][m] + parts[2][m] for m in range(3)] == want
        need = len(parts[1][1])
        assert need > 1
        a, status, out_len = st.encode_chunks([x[:100] for x in data], [1, 1, 1])
        assert (status == 0).all() and a == parts[0]
        b, status, out_len = st.encode_chunks([x[100:200] for x in data], [1, 1, 1], cap=[4096, need - 1, 4096])   # one byte short
        assert [int(s) for s in status] == [0, E_OVERFLOW, 0] and int(out_len[1]) == need
        assert [st.member_open(m) for m in range(3)] == [True, False, True]
        c, status, out_len = st.encode_chunks([x[200:] for x in data], None)
        assert [int(s) for s in status] == [0, E_OVERFLOW, 0] and int(out_len[1]) == 0
        assert a[0] + b[0] + c[0] == want[0] and a[2] + b[2] + c[2] == want[2]
        assert not any(st.member_open(m) for m in range(3))
    finally:
        st.close()
        roomy.close()
        model.close()


def test_a_full_line_store_fails_the_member_in_its_third_chunk(zpq, gpu_ctx, clean_env):
    """A 1024-line store refuses beyond 960 claimed lines per table.  Member 1: two chunks of 150 random bytes claim at most
    2 (300 + 2) = 604; the third, 300 more, takes the member beyond its promise.  Its neighbours never notice."""
    clean_env.setenv("ZPQ_SPARSE_FORCE_LOG2", "10")
    header = zpq.level_header(3)
    model = zpq.Model(header=header)
    r = random.Random(5)
    data = [SC._data(r, 2, 230), SC._data(r, 1, 600), SC._data(r, 3, 230)]
    cuts = [(0, 80, 160, 230), (0, 150, 300, 600), (0, 80, 160, 230)]
    want = [O.Codec(header).encode(x, pp=True) for x in data]
    st = zpq.BlockSet(gpu_ctx, model, 3)
    try:
        got = [b"", b"", b""]
        for k in range(3):
            coded, status, _ = st.encode_chunks([data[m][cuts[m][k]:cuts[m][k + 1]] for m in range(3)], [k < 2] * 3)
            assert gpu_ctx.last_line_store == 1024 and gpu_ctx.last_kernel_name == CHAIN[0]
            assert [int(s) for s in status] == [0, E_TOOBIG if k == 2 else 0, 0], (k, list(status))
            for m in range(3):
                got[m] += coded[m]
            if k < 2:
                assert want[1][:len(got[1])] == got[1]
        assert got[0] == want[0] and got[2] == want[2]
        assert not any(st.member_open(m) for m in range(3))
        coded, status, out_len = st.encode_chunks([b"abc"], [1], members=[1])
        assert int(status[0]) == E_TOOBIG and int(out_len[0]) == 0 and not st.member_open(1)
    finally:
        st.close()
        model.close()


# ---------------------------------------------------------------- 6: buffers
def test_nothing_outside_the_windows_is_touched(zpq, gpu_ctx, clean_env):
    """the sentinel check of tests/abi_windows.py at one small shape: first offsets other than 0, 0xEE around the window"""
    header = zpq.level_header(1)
    model = zpq.Model(header=header)
    r = random.Random(21)
    data = [SC._data(r, 2, 150), b"", SC._data(r, 1, 90)]
    want = [O.Codec(header).encode(x, pp=True) for x in data]
    enc, dec = zpq.BlockSet(gpu_ctx, model, 3), zpq.BlockSet(gpu_ctx, model, 3)

    def layout(lengths, shift):
        off = np.zeros(len(lengths) + 1, dtype=np.uint64)
        off[0] = shift
        off[1:] = shift + np.cumsum(np.asarray(lengths, dtype=np.uint64))
        return off

    def untouched(a, lo, hi):
        assert (a[lo:hi] == FILL).all(), (lo, hi)

    try:
        acc = [b"", b"", b""]
        for k, more in ((0, 1), (1, 0)):
            parts = [x[:60] if k == 0 else x[60:] for x in data]
            caps = [400, 64, 400]
            in_off, out_off = layout([len(p) for p in parts], 40), layout(caps, 72)
            src = np.full(int(in_off[-1]) + 16, 0x55, dtype=np.uint8)
            for i, p in enumerate(parts):
                src[int(in_off[i]):int(in_off[i]) + len(p)] = np.frombuffer(p, dtype=np.uint8)
            out = np.full(int(out_off[-1]) + 64, FILL, dtype=np.uint8)
            rc, olen, status = enc.encode_chunks_raw(None, src.ctypes.data, in_off, zpq.FLAG_PP, [more] * 3, out.ctypes.data, out_off)
            assert rc == 0 and (status == 0).all()
            untouched(out, 0, 72)
            untouched(out, int(out_off[-1]), len(out))
            for i in range(3):
                acc[i] += out[int(out_off[i]):int(out_off[i]) + int(olen[i])].tobytes()
        assert acc == want
        pos = [0, 0, 0]
        back = [b"", b"", b""]
        for k, caps in enumerate(([60, 0, 90], [100, 8, 8])):
            parts = [w[p:] for w, p in zip(want, pos)]
            in_off, out_off = layout([len(p) for p in parts], 40), layout(caps, 72)
            src = np.full(int(in_off[-1]) + 16, 0x55, dtype=np.uint8)
            for i, p in enumerate(parts):
                src[int(in_off[i]):int(in_off[i]) + len(p)] = np.frombuffer(p, dtype=np.uint8)
            out = np.full(int(out_off[-1]) + 64, FILL, dtype=np.uint8)
            rc, olen, cons, code, fb, status, opened = dec.decode_chunks_raw(None, src.ctypes.data, in_off, zpq.FLAG_PP, out.ctypes.data, out_off)
            assert rc == 0 and (status == 0).all()
            assert list(opened) == ([1, 1, 1] if k == 0 else [0, 0, 0])       # (member 2: 90 of 90, an exact fit)
            untouched(out, 0, 72)
            untouched(out, int(out_off[-1]), len(out))
            for i in range(3):
                back[i] += out[int(out_off[i]):int(out_off[i]) + int(olen[i])].tobytes()
                pos[i] += int(cons[i])
        assert back == data and pos == [len(w) for w in want]
    finally:
        enc.close()
        dec.close()
        model.close()
