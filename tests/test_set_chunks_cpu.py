"""Chunked coding on block sets, the part that needs no GPU: the plan test_gpu_set_chunks.py runs (tests/set_chunks.py)
holds what it promises, the three entry points exist in the built library and refuse a NULL set, and the binding has
its methods."""
import ctypes as C

import set_chunks as SC

E_ARG = -2


def test_the_plan_holds_every_shape():
    plan = SC.make_plan()
    c = SC.counts(plan)
    assert len(plan.members) == 21 and all(1 <= len(segs) <= 3 for segs in plan.members)
    for k in ("opened_by_empty", "ended_by_empty", "one_chunk", "second_after_chunked", "mixed_rounds"):
        assert c[k] >= 3, (k, c[k])
    used = {n for segs in plan.cuts for cut in segs for n in cut}
    assert used == set(SC.CHUNK_LENGTHS), sorted(set(SC.CHUNK_LENGTHS) - used)
    # every chunk once, in order, a member at most once per call; `more` and `opens` as the cuts say
    seen = {}
    for rnd in plan.rounds:
        assert len({ch.member for ch in rnd}) == len(rnd)
        for ch in rnd:
            before = (ch.seg, ch.idx - 1) if ch.idx or not ch.seg else (ch.seg - 1, len(plan.cuts[ch.member][ch.seg - 1]) - 1)
            assert seen.get(ch.member, (0, -1)) == before, (ch.member, ch.seg, ch.idx)
            seen[ch.member] = (ch.seg, ch.idx)
            assert ch.more == (ch.idx + 1 < len(plan.cuts[ch.member][ch.seg])) and ch.opens == (ch.idx == 0)
            assert len(ch.data) == plan.cuts[ch.member][ch.seg][ch.idx]
    for m, segs in enumerate(plan.cuts):
        assert seen[m] == (len(segs) - 1, len(segs[-1]) - 1)
        for s, cut in enumerate(segs):
            assert sum(cut) == len(plan.members[m][s])
    assert any(len(rnd) >= 12 for rnd in plan.rounds)       # the wave-pipelined encoder's floor: a ZPQ_SET_PIPE set would take it
    assert SC.make_plan().rounds == plan.rounds             # deterministic


def test_the_decode_schedule_holds_every_case():
    plan = SC.make_plan()
    calls = SC.simulate_decode(plan.members)
    steps = [st for call in calls for st in call]
    assert {st.cap for st in steps} == set(SC.DECODE_CAPS)
    assert sum(st.exact for st in steps) >= 3                               # a stream that ends exactly with a full slab ...
    follow = 0
    for t, call in enumerate(calls[:-1]):
        for st in call:
            if st.exact:
                nxt = [x for x in calls[t + 1] if x.member == st.member][0]
                assert nxt.seg == st.seg and nxt.take == 0 and not nxt.opening
                follow += (not nxt.open)                                    # ... and the empty call that closes it
    assert follow >= 1
    assert sum(1 for st in steps if st.opening and st.cap == 0) >= 3        # an opening call that decodes the PP byte alone
    assert any(len({(st.opening, st.open) for st in call}) == 4 for call in calls)
    for m, segs in enumerate(plan.members):
        for s, seg in enumerate(segs):
            assert sum(st.take for st in steps if (st.member, st.seg) == (m, s)) == len(seg)


def test_the_entry_points_exist_and_refuse_a_null_set(zpq):
    L = zpq.lib()
    for name in ("zpq_blockset_encode_chunks", "zpq_blockset_decode_chunks", "zpq_blockset_member_open"):
        assert hasattr(L, name), name
    off = (C.c_uint64 * 2)(0, 0)
    u = (C.c_uint32 * 1)()
    st = (C.c_int32 * 1)()
    op = (C.c_uint8 * 1)()
    assert L.zpq_blockset_encode_chunks(None, 1, None, None, off, 1, None, None, off, u, st) == E_ARG
    assert L.zpq_blockset_decode_chunks(None, 1, None, None, off, 1, None, off, u, u, u, u, op, st) == E_ARG
    assert L.zpq_blockset_member_open(None, 0) == E_ARG


def test_the_binding_has_the_methods(zpq):
    for name in ("encode_chunks", "decode_chunks", "member_open", "encode_chunks_raw", "decode_chunks_raw"):
        assert callable(getattr(zpq.BlockSet, name, None)), name
