"""Chunked coding on ZPQ_SET_LANES | ZPQ_SET_CHUNKS block sets: zpq_blockset_{encode,decode}_chunks on the state hand-over
forms of k_rows / k_lanes, one launch per call.  Everything is held to the oracle (oracle_lib.Codec, one encode per WHOLE
segment: a segment's chunks, one behind the other, must be exactly that), and every call's kernel is asserted from
gpu_ctx.last_kernel_name.  The plan of members, segments, chunks and calls is tests/set_chunks.py: 21 members (a multiple of
neither four blocks per wave nor four waves per workgroup) of at most 3 segments x 5 chunks x 300 bytes; the helpers that
walk it are test_gpu_set_chunks.py's."""
import os
import random
import sys

import numpy as np
import pytest

import general_models as GM
import oracle_lib as O
import set_chunks as SC
import vpipe_models as VM
import zpaql_programs as ZP
from abi_windows import FILL
from test_gpu_set_chunks import decode_plan, encode_plan, oracle_history, plan_of

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

pytestmark = pytest.mark.gpu

KNOBS = ("ZPQ_SET_LANES", "ZPQ_SET_PIPE", "ZPQ_SET_WAVES", "ZPQ_SET_VMWAVES", "ZPQ_LANES_ROWS", "ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE",
         "ZPQ_GPIPE_BATCH", "ZPQ_LANES_STORE")
E_OVERFLOW, E_ARG = -7, -2
NO_BYTE = 0xFFFFFFFF
ROWS = ("k_rows<encode>", "k_rows<decode>")
LANES = ("k_lanes<encode>", "k_lanes<decode>")


@pytest.fixture()
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _models():
    from inputs import C4B
    return {
        "C4B": (C4B, ROWS),                                                         # nine types, a MATCH
        "n17": (GM.NAMED["n17"][0], LANES),                                         # the hash chain in registers, k_lanes
        "fwd_n20": (GM.NAMED["fwd_n20"][0], LANES),                                 # p[] across a pause
        "match_min": (GM.NAMED["match_min"][0], ROWS),                              # coder, MATCH and h[] around ONE component
        "match_buf0": (GM.NAMED["match_buf0"][0], ROWS),
        "d_walks_h_rows": (ZP.embed(ZP.NAMED["d_walks_h"], "rows")[0], ROWS),       # VM registers across a pause, interpreter forms
        "d_walks_h_lanes": (ZP.embed(ZP.NAMED["d_walks_h"], "lanes")[0], LANES),
        "loop_hh9_hm16_lanes": (ZP.embed(ZP.NAMED["loop_hh9_hm16"], "lanes")[0], LANES),   # H of 512 words: in the slot, not in LDS
    }


def _set(zpq, ctx, model, n, want_flags=129, **kw):
    st = zpq.BlockSet(ctx, model, n, lanes=True, chunks=True, **kw)
    assert zpq.lib().zpq_blockset_flags(st.h) == want_flags and st.lanes and st.chunks
    return st


# ---------------------------------------------------------------- 1: the full plan on a 129 set
@pytest.mark.parametrize("name", sorted(_models()))
def test_the_plan_on_a_129_set(zpq, gpu_ctx, clean_env, name):
    header, names = _models()[name]
    ncomp = len(GM.components(header))
    assert names == (ROWS if ncomp <= 16 else LANES), ncomp
    if name == "fwd_n20":
        assert GM.has_forward_reference(header)
    if name == "loop_hh9_hm16_lanes":
        assert header[0] == 9                                                       # 512 words of H, beyond the 256 kept in LDS
    if name.startswith("match_"):
        assert ncomp == 1 and GM.is_hashchain(header)
    plan = plan_of()
    assert len(plan.members) == 21
    want = oracle_history(header, plan, ("set_lanes_chunks", name))
    model = zpq.Model(header=header)
    enc, dec = _set(zpq, gpu_ctx, model, 21), _set(zpq, gpu_ctx, model, 21)
    try:
        encode_plan(zpq, gpu_ctx, enc, plan, want, names[0])
        exact, closing = decode_plan(zpq, gpu_ctx, dec, plan, want, names[1])
        assert exact >= 3 and closing >= 1, (exact, closing)
    finally:
        enc.close()
        dec.close()
        model.close()


# ---------------------------------------------------------------- 2: h[] = 0 behind an empty opening chunk
@pytest.mark.parametrize("name", ["C4B", "d_walks_h_rows"])
def test_an_empty_opening_chunk_without_the_pp_byte(zpq, gpu_ctx, clean_env, name):
    """reset() zeroes h[] and leaves the VM's H alone: a second segment opened by an empty chunk, with no PP byte, has coded
    no byte when it goes on and must do so with h[] = 0, not with what H holds from the first segment."""
    header, names = _models()[name]
    r = random.Random(41)
    segs = [[SC._data(r, 2, 90), SC._data(r, 2 + m % 2, 70)] for m in range(5)]
    ref = [O.Codec(header) for _ in range(5)]
    want = [[ref[m].encode(seg, pp=False) for seg in segs[m]] for m in range(5)]
    model = zpq.Model(header=header)
    enc, dec = _set(zpq, gpu_ctx, model, 5), _set(zpq, gpu_ctx, model, 5)
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
        assert gpu_ctx.last_kernel_name == names[1] and back == [b""] * 5
        back, status, c2, _, first, opened = dec.decode_chunks([w[1][int(c):] for w, c in zip(want, consumed)], 200, flags=0)
        assert (status == 0).all() and back == [x[1] for x in segs] and list(opened) == [0] * 5
        assert [int(a) + int(b) for a, b in zip(consumed, c2)] == [len(w[1]) for w in want]
    finally:
        enc.close()
        dec.close()
        model.close()


# ---------------------------------------------------------------- 3: k_rows and k_lanes read each other's pauses
def test_lanes_rows_flipped_between_the_calls_of_open_segments(zpq, gpu_ctx, clean_env):
    """ZPQ_LANES_ROWS is read at every call: k_rows pauses, k_lanes goes on and pauses, k_rows ends -- same bytes"""
    header, _ = _models()["C4B"]
    r = random.Random(77)
    data = [SC._data(r, 1 + m % 3, 200 + 17 * m) for m in range(6)]
    want = [O.Codec(header).encode(x, pp=True) for x in data]
    cuts = (0, 64, 130, 400)
    model = zpq.Model(header=header)
    enc, dec = _set(zpq, gpu_ctx, model, 6), _set(zpq, gpu_ctx, model, 6)
    try:
        got = [b""] * 6
        for k, names in enumerate((ROWS, LANES, ROWS)):
            if names is LANES:
                clean_env.setenv("ZPQ_LANES_ROWS", "0")
            else:
                clean_env.delenv("ZPQ_LANES_ROWS", raising=False)
            coded, status, _ = enc.encode_chunks([x[cuts[k]:cuts[k + 1]] for x in data], [k < 2] * 6)
            assert (status == 0).all() and gpu_ctx.last_kernel_name == names[0], (k, gpu_ctx.last_kernel_name)
            got = [g + c for g, c in zip(got, coded)]
            assert all(w[:len(g)] == g for w, g in zip(want, got)), k
        assert got == want
        pos, back = [0] * 6, [b""] * 6
        for k, (names, cap) in enumerate(((ROWS, 65), (LANES, 64), (ROWS, 17), (LANES, 400))):
            if names is LANES:
                clean_env.setenv("ZPQ_LANES_ROWS", "0")
            else:
                clean_env.delenv("ZPQ_LANES_ROWS", raising=False)
            out, status, consumed, _, first, opened = dec.decode_chunks([w[p:] for w, p in zip(want, pos)], cap)
            assert (status == 0).all() and gpu_ctx.last_kernel_name == names[1], (k, gpu_ctx.last_kernel_name)
            assert list(opened) == [1 if k < 3 else 0] * 6 and all(int(f) == (0 if k == 0 else NO_BYTE) for f in first)
            back = [b + o for b, o in zip(back, out)]
            pos = [p + int(c) for p, c in zip(pos, consumed)]
        assert back == data and pos == [len(w) for w in want]
    finally:
        enc.close()
        dec.close()
        model.close()


# ---------------------------------------------------------------- 4: the wave kernels' sets chunk on k_rows / k_lanes
@pytest.mark.parametrize("which", ["waves", "vmwaves"])
def test_a_wave_set_chunks_on_the_lane_kernels(zpq, gpu_ctx, clean_env, which):
    """a 145 set (C4B) and a 193 set (C4B_VM): every chunk call on k_rows, a whole-segment call before and after the chunked
    segment on the wave kernels -- one slot format --, every segment's bytes the oracle's"""
    from inputs import C4B
    header = C4B if which == "waves" else VM.C4B_VM
    wave = ("k_wset<encode>", "k_wsetd<decode>") if which == "waves" else ("k_vset<encode>", "k_vsetd<decode>")
    flags = 145 if which == "waves" else 193
    r = random.Random(5)
    segs = [[SC._data(r, 1 + (m + s) % 3, 150 + 31 * s + m) for s in range(3)] for m in range(5)]
    ref = [O.Codec(header) for _ in range(5)]
    want = [[ref[m].encode(seg, pp=True) for seg in segs[m]] for m in range(5)]
    model = zpq.Model(header=header)
    enc, dec = (_set(zpq, gpu_ctx, model, 5, want_flags=flags, **{which: True}) for _ in range(2))
    try:
        for s in (0, 1, 2):
            if s != 1:
                coded, status, _ = enc.encode_segments([x[s] for x in segs])
                assert (status == 0).all() and gpu_ctx.last_kernel_name == wave[0], gpu_ctx.last_kernel_name
            else:
                coded = [b""] * 5
                for k, (lo, hi) in enumerate(((0, 0), (0, 65), (65, 400))):
                    part, status, _ = enc.encode_chunks([x[s][lo:hi] for x in segs], [k < 2] * 5)
                    assert (status == 0).all() and gpu_ctx.last_kernel_name == ROWS[0], gpu_ctx.last_kernel_name
                    coded = [c + p for c, p in zip(coded, part)]
            assert coded == [w[s] for w in want], s
        for s in (0, 1, 2):
            if s != 1:
                back, status, consumed, _, first = dec.decode_segments([w[s] for w in want], cap=400)
                assert (status == 0).all() and gpu_ctx.last_kernel_name == wave[1], gpu_ctx.last_kernel_name
            else:
                back, pos = [b""] * 5, [0] * 5
                for k, cap in enumerate((0, 64, 400)):
                    out, status, consumed, _, first, opened = dec.decode_chunks([w[s][p:] for w, p in zip(want, pos)], cap)
                    assert (status == 0).all() and gpu_ctx.last_kernel_name == ROWS[1], gpu_ctx.last_kernel_name
                    assert list(opened) == [1 if k < 2 else 0] * 5
                    back = [b + o for b, o in zip(back, out)]
                    pos = [p + int(c) for p, c in zip(pos, consumed)]
                assert pos == [len(w[s]) for w in want]
            assert back == [x[s] for x in segs], s
    finally:
        enc.close()
        dec.close()
        model.close()


# ---------------------------------------------------------------- 5: the same bytes as the whole-segment calls
def test_chunks_and_segments_give_the_same_bytes(zpq, gpu_ctx, clean_env):
    """one 129 set per direction: its members coded by the segment calls in one round and by chunks in the next"""
    header, names = _models()["C4B"]
    plan = plan_of()
    want = oracle_history(header, plan, ("set_lanes_chunks", "C4B"))
    n = len(plan.members)
    model = zpq.Model(header=header)
    enc, dec = _set(zpq, gpu_ctx, model, n), _set(zpq, gpu_ctx, model, n)
    try:
        for rnd in range(3):
            idx = [m for m in range(n) if len(plan.members[m]) > rnd]
            segs = [plan.members[m][rnd] for m in idx]
            if rnd != 1:
                coded, status, _ = enc.encode_segments(segs, members=idx)
                assert (status == 0).all()
                back, status, consumed, _, first = dec.decode_segments(coded, cap=1600, members=idx)
                assert (status == 0).all() and (first == 0).all()
            else:
                coded, back, pos = [b""] * len(idx), [b""] * len(idx), [0] * len(idx)
                for k in range(3):
                    part, status, _ = enc.encode_chunks([x[100 * k:100 * k + 100] if k < 2 else x[200:] for x in segs], [k < 2] * len(idx), members=idx)
                    assert (status == 0).all() and gpu_ctx.last_kernel_name == names[0]
                    coded = [c + p for c, p in zip(coded, part)]
                todo = list(range(len(idx)))                   # (a member whose decoder has met its EOF takes no further call)
                for cap in (100, 100, 1600):
                    out, status, consumed, _, first, opened = dec.decode_chunks(
                        [want[idx[j]][rnd][pos[j]:] for j in todo], cap, members=[idx[j] for j in todo])
                    assert (status == 0).all() and gpu_ctx.last_kernel_name == names[1]
                    for j, o, c in zip(todo, out, consumed):
                        back[j] += o
                        pos[j] += int(c)
                    todo = [j for j, op in zip(todo, opened) if op]
                assert todo == [] and not any(dec.member_open(m) or enc.member_open(m) for m in idx)
            assert coded == [want[m][rnd] for m in idx], rnd
            assert back == segs, rnd
    finally:
        enc.close()
        dec.close()
        model.close()


# ---------------------------------------------------------------- 6: refusals and failures
def test_an_open_member_is_refused_by_the_segment_calls(zpq, gpu_ctx, clean_env):
    header, _ = _models()["C4B"]
    model = zpq.Model(header=header)
    r = random.Random(3)
    data = [SC._data(r, 2, 200) for _ in range(3)]
    want = [O.Codec(header).encode(x, pp=True) for x in data]
    enc, dec = _set(zpq, gpu_ctx, model, 3), _set(zpq, gpu_ctx, model, 3)
    try:
        first, status, _ = enc.encode_chunks([x[:70] for x in data], [1, 0, 1])
        assert (status == 0).all() and [enc.member_open(m) for m in range(3)] == [True, False, True]
        for call in (lambda: enc.encode_segments([b"abc"], members=[0]), lambda: enc.encode_segments([b"a", b"b"], members=[1, 2]),
                     lambda: enc.decode_segments([want[0]], cap=300, members=[2]),
                     lambda: enc.decode_chunks([want[0]], 300, members=[0])):     # opened by the encoder: no decode call
            with pytest.raises(zpq.ZpqError) as e:
                call()
            assert e.value.code == E_ARG
        rest, status, _ = enc.encode_chunks([data[0][70:], data[2][70:]], None, members=[0, 2])     # nothing was coded meanwhile
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


def test_noeof_is_refused(zpq, gpu_ctx, clean_env):
    header, _ = _models()["C4B"]
    model = zpq.Model(header=header)
    st = _set(zpq, gpu_ctx, model, 2)
    try:
        for call in (lambda: st.encode_chunks([b"abc"], [1], members=[0], flags=zpq.FLAG_PP | 4),
                     lambda: st.decode_chunks([b"\0" * 8], 4, members=[0], flags=4)):
            with pytest.raises(zpq.ZpqError) as e:
                call()
            assert e.value.code == E_ARG                                       # ZPQ_FLAG_NOEOF
        assert not st.member_open(0)
        coded, status, _ = st.encode_chunks([b"abc", b"def"], None)            # the set itself is as good as before
        assert (status == 0).all() and coded[0] == O.Codec(header).encode(b"abc", pp=True)
    finally:
        st.close()
        model.close()


def test_a_chunk_that_does_not_fit_fails_the_member(zpq, gpu_ctx, clean_env):
    header, _ = _models()["C4B"]
    model = zpq.Model(header=header)
    r = random.Random(11)
    data = [SC._data(r, 1, 300) for _ in range(3)]                              # random bytes: the coded stream is longer than they are
    want = [O.Codec(header).encode(x, pp=True) for x in data]
    st, roomy = _set(zpq, gpu_ctx, model, 3), _set(zpq, gpu_ctx, model, 3)
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
        assert [int(s) for s in status] == [0, E_OVERFLOW, 0] and int(out_len[1]) == 0          # sticky
        assert a[0] + b[0] + c[0] == want[0] and a[2] + b[2] + c[2] == want[2]                  # the neighbours never notice
        assert not any(st.member_open(m) for m in range(3))
    finally:
        st.close()
        roomy.close()
        model.close()


def test_nothing_outside_the_windows_is_touched(zpq, gpu_ctx, clean_env):
    """the sentinel check of tests/abi_windows.py at one small shape: first offsets other than 0, 0xEE around the window"""
    header, _ = _models()["C4B"]
    model = zpq.Model(header=header)
    r = random.Random(21)
    data = [SC._data(r, 2, 150), b"", SC._data(r, 1, 90)]
    want = [O.Codec(header).encode(x, pp=True) for x in data]
    enc, dec = _set(zpq, gpu_ctx, model, 3), _set(zpq, gpu_ctx, model, 3)

    def layout(lengths, shift):
        off = np.zeros(len(lengths) + 1, dtype=np.uint64)
        off[0] = shift
        off[1:] = shift + np.cumsum(np.asarray(lengths, dtype=np.uint64))
        return off

    def untouched(a, lo, hi):
        assert (a[lo:hi] == FILL).all(), (lo, hi)

    def source(parts, in_off):
        src = np.full(int(in_off[-1]) + 16, 0x55, dtype=np.uint8)
        for i, p in enumerate(parts):
            src[int(in_off[i]):int(in_off[i]) + len(p)] = np.frombuffer(p, dtype=np.uint8)
        return src

    try:
        acc = [b"", b"", b""]
        for k, more in ((0, 1), (1, 0)):
            parts = [x[:60] if k == 0 else x[60:] for x in data]
            in_off, out_off = layout([len(p) for p in parts], 40), layout([1200, 64, 1200], 72)   # (C4B expands these bytes sixfold)
            src = source(parts, in_off)
            out = np.full(int(out_off[-1]) + 64, FILL, dtype=np.uint8)
            rc, olen, status = enc.encode_chunks_raw(None, src.ctypes.data, in_off, zpq.FLAG_PP, [more] * 3, out.ctypes.data, out_off)
            assert rc == 0 and (status == 0).all()
            untouched(out, 0, 72)
            untouched(out, int(out_off[-1]), len(out))
            for i in range(3):
                acc[i] += out[int(out_off[i]):int(out_off[i]) + int(olen[i])].tobytes()
        assert acc == want
        pos, back = [0, 0, 0], [b"", b"", b""]
        for k, caps in enumerate(([60, 0, 90], [100, 8, 8])):
            parts = [w[p:] for w, p in zip(want, pos)]
            in_off, out_off = layout([len(p) for p in parts], 40), layout(caps, 72)
            src = source(parts, in_off)
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
