"""The block-set kernels (the state hand-over forms k_chain<..., KEEP>, k_pipe<..., KEEP>, k_rows / k_lanes<..., KEEP>, k_wset /
k_wsetd, and the default route of one k_generic launch per member) held to the oracle off the nominal path.

Decoders: every member of tests/offnominal_sets.py decodes a good segment, a damaged one and a good one again on ONE set;
all six outputs and the stored bytes of every member and round are the oracle's, which followed the member with a codec of
its own (Codec.decode_prefix).  A member that survives its damaged segment must have left in its slot the state of the byte
boundary where IT stopped: the follow-on segment shows it (test_offnominal_sets_cpu.py: for at least 100 members of every
model).  Encoders: 42 members meet slabs of 0, 1, 3, 4, len - 1 and len bytes in their second round.
Every call's kernel name is asserted; every test prints and asserts what it saw."""
import concurrent.futures
import random

import numpy as np
import pytest

import general_models as GM
import offnominal_corpus as OC
import offnominal_sets as OS
import oracle_lib as O
from test_gpu_chain_models import _block
from test_gpu_offnominal import ENC_SIZES, PAD, SENTINEL, _offsets, _source, check_decode, check_encode, raw_set_decode

pytestmark = pytest.mark.gpu

KNOBS = ("ZPQ_SET_LANES", "ZPQ_SET_WAVES", "ZPQ_SET_PIPE", "ZPQ_LANES_ROWS", "ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE", "ZPQ_GPIPE_BATCH",
         "ZPQ_GDEC_BPW", "ZPQ_VM_PIPE", "ZPQ_ENC_PIPE", "ZPQ_ENC_SPLIT", "ZPQ_PIPE_PER", "ZPQ_PIPE_SHARE", "ZPQ_DEC_PIPE",
         "ZPQ_DEC_HYP16", "ZPQ_SPARSE_MODE", "ZPQ_SPARSE_FORCE_LOG2", "ZPQ_CHAIN_G", "ZPQ_CHAIN_BPW")
PP = pytest.mark.parametrize("pp", [True, False], ids=["pp", "raw"])
WORKERS = 4                                            # (a process opens four hardware queues by default)


@pytest.fixture()
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def set_env(mp, env, only=("ZPQ_DEC_GPIPE", "ZPQ_ENC_GPIPE", "ZPQ_LANES_ROWS")):
    """The knobs read at the call, set to `env` (a knob it does not name is cleared)."""
    for k in only:
        if k in env:
            mp.setenv(k, env[k])
        else:
            mp.delenv(k, raising=False)


def pad_untouched(got):
    out, out_off = got[0], got[1]
    return bool((out[int(out_off[-1]):] == SENTINEL).all()) and len(out) == int(out_off[-1]) + PAD


# ---------------------------------------------------------------- decoders
def follow_members(zpq, ctx, name, pp, make_set, capacity, kernel_of, seen, policies=OS.POLICIES, pick=None, tag="", stores=None):
    """Every slab policy on a NEW set (state moves): the three rounds through the raw call, everything checked after every
    round.  A set that holds fewer members than there are takes them in consecutive groups, one set after the other.
    kernel_of(policy, round) prepares the call's environment and returns the kernel it must run.  A round in which a member
    of the call has failed before copies only the live members' stored bytes: no other byte of the output may change."""
    batch = OS.layout(name, pp)
    idx = list(range(len(batch))) if pick is None else pick
    F = zpq.FLAG_PP if pp else 0
    assert capacity >= 1
    for which in policies:
        want, caps = OS.expectations(name, pp, which), OS.caps_of(batch, which)
        for lo in range(0, len(idx), capacity):
            group = idx[lo:lo + capacity]
            bs = make_set(len(group))
            try:
                for rnd in range(OS.ROUNDS):
                    kernel = kernel_of(which, rnd)
                    exp = [want[rnd][i] for i in group]
                    gcaps = [caps[rnd][i] for i in group]
                    got = raw_set_decode(zpq, bs, [batch[i].streams[rnd] for i in group], gcaps, F)
                    assert ctx.last_kernel_name == kernel, (which, rnd, ctx.last_kernel_name, kernel)
                    if stores is not None:
                        stores.add(ctx.last_line_store)
                    some_failed = any(want[r][i].status != 0 for r in range(rnd) for i in group)
                    assert any(e.status == 0 for e in exp)                   # (somebody was coded: the name is this call's)
                    check_decode("%s%s pp=%d %s round %d %s" % (name, tag, pp, which, rnd, kernel), [OS.as_case(batch[i], rnd) for i in group],
                                 gcaps, exp, got, whole=some_failed)
                    assert pad_untouched(got), (which, rnd)
                    seen.add("%s%s" % (kernel, " some failed" if some_failed else ""))
            finally:
                bs.close()


def member_total(name, pp):
    """The most bytes a member decodes over its three rounds (PP bytes and the byte past a full slab included): what a set's
    line store must be sized for."""
    want = OS.expectations(name, pp, "roomy")
    return max(sum(want[r][i].out_len + 2 for r in range(OS.ROUNDS)) for i in range(len(want[0])))


CHAIN_CASES = ([(m, "default") for m in OC.MODELS[:5] + OS.CHAIN_EXTRA] + [("level%d" % i, "dense") for i in (1, 2, 3)]
               + [("level%d" % i, "hyp16off") for i in (3, 4)])
CHAIN_ENV = {"default": {}, "dense": {"ZPQ_SPARSE_MODE": "never"}, "hyp16off": {"ZPQ_DEC_HYP16": "0"}}


@PP
@pytest.mark.parametrize("name,variant", CHAIN_CASES, ids=["%s-%s" % c for c in CHAIN_CASES])
def test_chain_sets_follow_damaged_segments(zpq, gpu_ctx, clean_env, name, variant, pp):
    """k_chain<decode, KEEP>: every level with the line store sized for the largest member, levels 1-3 on dense tables,
    levels 3 and 4 on the eight-lane form, the unspecialised chains at 8 and 16 lanes per block."""
    for k, v in CHAIN_ENV[variant].items():
        clean_env.setenv(k, v)
    total = member_total(name, pp)
    model = zpq.Model(header=OS.header_of(name))
    seen, stores = set(), set()

    def kernel_of(which, rnd):
        return "k_chain<decode>"

    def make_set(n):
        return zpq.BlockSet(gpu_ctx, model, n, max_member_bytes=total)

    try:
        follow_members(zpq, gpu_ctx, name, pp, make_set, gpu_ctx.blockset_capacity(model, total), kernel_of, seen, tag=" " + variant,
                       stores=stores)
    finally:
        model.close()
    print("\nkernels %s %s pp=%d: %s, line store %s" % (name, variant, pp, sorted(seen), sorted(stores)))
    assert seen == {"k_chain<decode>", "k_chain<decode> some failed"}
    assert stores and all((s == 0) == (variant == "dense") for s in stores), stores


def general_sets(zpq, ctx, name, pp, kernel_of, seen, set_kw, flags, **more):
    model = zpq.Model(header=OS.header_of(name))

    def make_set(n):
        bs = zpq.BlockSet(ctx, model, n, **set_kw)
        assert zpq.lib().zpq_blockset_flags(bs.h) == flags
        return bs

    try:
        follow_members(zpq, ctx, name, pp, make_set, ctx.blockset_capacity(model, **set_kw), kernel_of, seen, **more)
    finally:
        model.close()


@PP
@pytest.mark.parametrize("name", ["cm_alias", "match_idx_gt_buf", "mix9", "hm0"])
def test_rows_sets_follow_damaged_segments(zpq, gpu_ctx, clean_env, name, pp):
    assert GM.NAMED[name][1][3] == GM.ROWS
    seen = set()
    general_sets(zpq, gpu_ctx, name, pp, lambda which, rnd: "k_rows<decode>", seen, {"lanes": True}, 1)
    print("\nkernels %s pp=%d: %s" % (name, pp, sorted(seen)))
    assert seen == {"k_rows<decode>", "k_rows<decode> some failed"}


@PP
@pytest.mark.parametrize("name", ["n17", "mix3_sse3_n22_vm", "cm_alias", "hm0"])
def test_lanes_sets_follow_damaged_segments(zpq, gpu_ctx, clean_env, name, pp):
    """k_lanes<decode, KEEP>: the two models only it takes (the second runs the ZPAQL interpreter, as hm0 does), and two of
    k_rows' under ZPQ_LANES_ROWS=0."""
    rows = GM.NAMED[name][1][3] == GM.ROWS
    assert rows == (name in ("cm_alias", "hm0"))
    if rows:
        clean_env.setenv("ZPQ_LANES_ROWS", "0")
    seen = set()
    general_sets(zpq, gpu_ctx, name, pp, lambda which, rnd: "k_lanes<decode>", seen, {"lanes": True}, 1)
    print("\nkernels %s pp=%d%s: %s" % (name, pp, " ZPQ_LANES_ROWS=0" if rows else "", sorted(seen)))
    assert seen == {"k_lanes<decode>", "k_lanes<decode> some failed"}


@PP
@pytest.mark.parametrize("name", ["cm_alias", "match_idx_gt_buf", "mix_x4"])
def test_wave_sets_follow_damaged_segments(zpq, gpu_ctx, clean_env, name, pp):
    seen = set()
    general_sets(zpq, gpu_ctx, name, pp, lambda which, rnd: "k_wsetd<decode>", seen, {"waves": True}, 17)
    print("\nkernels %s pp=%d flags 17: %s" % (name, pp, sorted(seen)))
    assert seen == {"k_wsetd<decode>", "k_wsetd<decode> some failed"}


@PP
@pytest.mark.parametrize("order", ["waves_then_rows", "rows_then_waves"])
def test_the_other_family_reads_what_a_damaged_segment_left(zpq, gpu_ctx, clean_env, order, pp):
    """cm_alias under tight slabs: rounds 0 and 1 on k_wsetd and round 2 on k_rows (ZPQ_DEC_GPIPE=0 at the call), and the
    reverse -- the slot holds one format for both families, after a damaged segment too."""
    seen = set()

    def kernel_of(which, rnd):
        on_waves = (rnd < 2) == (order == "waves_then_rows")
        set_env(clean_env, {} if on_waves else {"ZPQ_DEC_GPIPE": "0"})
        return "k_wsetd<decode>" if on_waves else "k_rows<decode>"

    general_sets(zpq, gpu_ctx, "cm_alias", pp, kernel_of, seen, {"waves": True}, 17, policies=("tight",), tag=" " + order)
    print("\nkernels cm_alias pp=%d %s flags 17: %s" % (pp, order, sorted(seen)))
    assert seen == ({"k_wsetd<decode>", "k_rows<decode> some failed"} if order == "waves_then_rows"
                    else {"k_rows<decode>", "k_wsetd<decode> some failed"})


@PP
@pytest.mark.parametrize("name", ["cm_alias", "n65"])
def test_default_route_sets_follow_damaged_segments(zpq, clean_env, name, pp):
    """A set nobody asked the lane kernels for: one k_generic launch per member, ZB_KEEP_STATE from its second segment on.
    Every fourth member of the layout and all junk; the subset still holds every mutation, and members that leave their
    damaged segment somewhere else than the original.  (n65: of the originals of at most 17 bytes.  One lane works through
    65 components, half a millisecond a byte, and a decode that runs on to the end of a roomy slab is 4033 bytes: with all
    originals and one launch after the other the case took 85 s, as it is 24 s; the slowest case of test_gpu_offnominal.py
    takes 10 s.)"""
    batch = OS.layout(name, pp)
    of = [i for i, m in enumerate(batch) if m.kind == "junk" or name != "n65" or m.nominal <= 17]
    pick = [i for k, i in enumerate(of) if k % 4 == 0 or batch[i].kind == "junk"]
    labels = {m.what.split(" ", 1)[1] for m in batch if m.kind not in ("junk", "filler")}
    assert len(labels) == 15 and {batch[i].what.split(" ", 1)[1] for i in pick if batch[i].kind not in ("junk", "filler")} == labels
    assert sum(1 for i in pick if batch[i].kind == "junk") == 15
    roomy = OS.expectations(name, pp, "roomy")[1]
    assert sum(1 for i in pick if batch[i].kind not in ("junk", "filler") and roomy[i].status == 0 and roomy[i].data != batch[i].data) >= 10
    for which in OS.POLICIES:
        OS.expectations(name, pp, which)                    # (computed once, before the workers read them)

    def worker(share):
        """A launch is one wave: four contexts on four host threads code four shares of the members side by side (measured:
        half the time of one context; shares of equal decoded bytes change nothing)."""
        ctx, seen = zpq.Context(0), set()
        try:
            general_sets(zpq, ctx, name, pp, lambda which, rnd: "k_generic<decode>", seen, {}, 0, pick=share)
        finally:
            ctx.close()
        return seen

    with concurrent.futures.ThreadPoolExecutor(WORKERS) as pool:
        seen = set().union(*pool.map(worker, [pick[w::WORKERS] for w in range(WORKERS)]))
    print("\nkernels %s pp=%d (%d members): %s" % (name, pp, len(pick), sorted(seen)))
    assert seen == {"k_generic<decode>", "k_generic<decode> some failed"}


# ---------------------------------------------------------------- encoders on short slabs
WARM_SIZES, NEXT_SIZES = (17, 64, 300, 1), (64, 17, 120, 2)
_ENC = {}


def encoder_members(name, pp):
    """42 members of three rounds: a warm-up, a segment of every length of ENC_SIZES that meets every slab of 0, 1, 3, 4,
    len - 1 and len bytes (len = the oracle's coded length in that member's state), a follow-on.  Returns (data[round][m],
    the oracle's streams [round][m], round 1's slabs); one oracle codec per member, which goes on whatever the slab."""
    key = (name, pp)
    if key not in _ENC:
        r = random.Random(313)
        sizes = [n for n in ENC_SIZES if n <= 300 or name not in OC.SMALL_ONLY]
        hdr = OS.header_of(name)
        data, coded = [[], [], []], [[], [], []]
        for i in range(6 * len(sizes)):
            segs = (_block(r, (i + 1) % 4, WARM_SIZES[i % 4]), _block(r, i % 4, sizes[i % len(sizes)]), _block(r, (i + 2) % 4, NEXT_SIZES[i % 4]))
            enc = O.Codec(hdr)
            for rnd in range(3):
                data[rnd].append(segs[rnd])
                coded[rnd].append(enc.encode(segs[rnd], pp=pp))
            del enc
        caps = [(0, 1, 3, 4, len(w) - 1, len(w))[i % 6] for i, w in enumerate(coded[1])]
        _ENC[key] = (data, coded, caps)
    return _ENC[key]


def raw_set_encode(zpq, bs, blocks, caps, flags):
    n = len(blocks)
    src, in_off, out_off = _source(blocks), _offsets([len(b) for b in blocks]), _offsets(caps)
    out = np.full(int(out_off[-1]) + PAD, SENTINEL, dtype=np.uint8)
    out_len = np.zeros(n, dtype=np.uint32)
    status = np.full(n, -99, dtype=np.int32)
    rc = zpq.lib().zpq_blockset_encode_segments(bs.h, n, None, src.ctypes.data, in_off.ctypes.data, flags, out.ctypes.data,
                                                out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data)
    assert rc == 0, "library call failed: %d" % rc
    return out, out_off, out_len, status


def encoders_on_short_slabs(zpq, ctx, name, pp, set_kw, flags, kernel_of, seen, tag="", stores=None):
    """Round 0 roomy and the oracle's; round 1 on the short slabs: out_len the full coded length of every member, -7 exactly
    where the slab is shorter, the slab holds the oracle's first cap bytes, the pad untouched; round 2: every member that
    overflowed reports -7 and 0 bytes, every other member's bytes are its oracle codec's, which went on -- and no other byte
    of the output changes (the call copies the live members' bytes only)."""
    data, coded, short = encoder_members(name, pp)
    n = len(short)
    assert n == (42 if name not in OC.SMALL_ONLY else 36)
    F = zpq.FLAG_PP if pp else 0
    model = zpq.Model(header=OS.header_of(name))
    total = sum(max(len(d) for d in data[rnd]) + 1 for rnd in range(3))
    bs = zpq.BlockSet(ctx, model, n, max_member_bytes=total, **set_kw)
    try:
        assert zpq.lib().zpq_blockset_flags(bs.h) == flags
        over = [cap < len(w) for cap, w in zip(short, coded[1])]
        assert sum(over) >= 12 and over.count(False) >= 6
        for rnd in range(3):
            live = n - (sum(over) if rnd == 2 else 0)
            kernel = kernel_of(rnd, live)
            caps = short if rnd == 1 else [len(d) * 17 + 4096 for d in data[rnd]]
            got = raw_set_encode(zpq, bs, data[rnd], caps, F)
            assert ctx.last_kernel_name == kernel, (rnd, live, ctx.last_kernel_name, kernel)
            if stores is not None:
                stores.add(ctx.last_line_store)
            what = "%s%s pp=%d round %d %s" % (name, tag, pp, rnd, kernel)
            out, out_off, out_len, status = got
            if rnd == 1:
                check_encode(what, data[rnd], coded[rnd], caps, got)
            if rnd < 2:
                assert [int(x) for x in out_len] == [len(w) for w in coded[rnd]], what
                assert [int(s) for s in status] == [0 if cap >= len(w) else -7 for w, cap in zip(coded[rnd], caps)], (what, list(status))
                for i, (w, cap) in enumerate(zip(coded[rnd], caps)):
                    o = int(out_off[i])
                    assert out[o:o + min(cap, len(w))].tobytes() == w[:cap], (what, "stored bytes of member", i, len(data[rnd][i]), cap)
            else:
                assert [int(s) for s in status] == [-7 if f else 0 for f in over], (what, list(status))
                assert [int(x) for x in out_len] == [0 if f else len(w) for f, w in zip(over, coded[2])], what
                image = np.full(len(out), SENTINEL, dtype=np.uint8)
                for i, w in enumerate(coded[2]):
                    if not over[i]:
                        image[int(out_off[i]):int(out_off[i]) + len(w)] = np.frombuffer(w, dtype=np.uint8)
                bad = np.nonzero(out != image)[0]
                assert not len(bad), (what, "byte", int(bad[0]), "member", int(np.searchsorted(out_off, bad[0], side="right")) - 1, len(bad))
            assert pad_untouched(got), what
            seen.add("%s round %d" % (kernel, rnd))
    finally:
        bs.close()
        model.close()


@PP
@pytest.mark.parametrize("level", OC.CHAIN_LEVELS)
def test_chain_set_encoders_on_slabs_too_small(zpq, gpu_ctx, clean_env, level, pp):
    seen = set()
    encoders_on_short_slabs(zpq, gpu_ctx, "level%d" % level, pp, {}, 0, lambda rnd, live: "k_chain<encode>", seen)
    print("\nkernels level%d pp=%d: %s" % (level, pp, sorted(seen)))
    assert seen == {"k_chain<encode> round %d" % r for r in range(3)}


PIPE_CASES = [(i, "store") for i in OC.CHAIN_LEVELS] + [(i, "dense") for i in (1, 2, 3)]


@PP
@pytest.mark.parametrize("level,tables", PIPE_CASES, ids=["level%d-%s" % c for c in PIPE_CASES])
def test_pipe_set_encoders_on_slabs_too_small(zpq, gpu_ctx, clean_env, level, tables, pp):
    """k_pipe<encode, KEEP> while the call has the pipeline's floor of 12 live members (rounds 0 and 1), whichever encoder
    that floor implies in round 2."""
    if tables == "dense":
        clean_env.setenv("ZPQ_SPARSE_MODE", "never")
    seen, stores = set(), set()

    def kernel_of(rnd, live):
        assert rnd == 2 or live >= 12
        return "k_pipe<encode>" if live >= 12 else "k_chain<encode>"

    encoders_on_short_slabs(zpq, gpu_ctx, "level%d" % level, pp, {"pipe": True}, 4, kernel_of, seen, tag=" " + tables, stores=stores)
    print("\nkernels level%d %s pp=%d flags 4: %s, line store %s" % (level, tables, pp, sorted(seen), sorted(stores)))
    assert {s.rsplit(" round", 1)[0] for s in seen if not s.endswith("2")} == {"k_pipe<encode>"} and len(seen) == 3
    assert stores and all((s == 0) == (tables == "dense") for s in stores), stores


@PP
@pytest.mark.parametrize("name", ["cm_alias", "n17", "hm0"])
def test_lane_set_encoders_on_slabs_too_small(zpq, gpu_ctx, clean_env, name, pp):
    kernel = "k_rows<encode>" if GM.NAMED[name][1][3] == GM.ROWS else "k_lanes<encode>"
    assert (kernel == "k_lanes<encode>") == (name == "n17")
    seen = set()
    encoders_on_short_slabs(zpq, gpu_ctx, name, pp, {"lanes": True}, 1, lambda rnd, live: kernel, seen)
    print("\nkernels %s pp=%d flags 1: %s" % (name, pp, sorted(seen)))
    assert seen == {"%s round %d" % (kernel, r) for r in range(3)}


@PP
@pytest.mark.parametrize("batch", ["batched", "bit_serial"])
@pytest.mark.parametrize("name", ["cm_alias", "match_idx_gt_buf"])
def test_wave_set_encoders_on_slabs_too_small(zpq, gpu_ctx, clean_env, name, batch, pp):
    if batch == "bit_serial":
        clean_env.setenv("ZPQ_GPIPE_BATCH", "0")
    seen = set()
    encoders_on_short_slabs(zpq, gpu_ctx, name, pp, {"waves": True}, 17, lambda rnd, live: "k_wset<encode>", seen, tag=" " + batch)
    print("\nkernels %s %s pp=%d flags 17: %s" % (name, batch, pp, sorted(seen)))
    assert seen == {"k_wset<encode> round %d" % r for r in range(3)}


@PP
def test_default_route_set_encoder_on_slabs_too_small(zpq, gpu_ctx, clean_env, pp):
    seen = set()
    encoders_on_short_slabs(zpq, gpu_ctx, "n65", pp, {}, 0, lambda rnd, live: "k_generic<encode>", seen)
    print("\nkernels n65 pp=%d: %s" % (pp, sorted(seen)))
    assert seen == {"k_generic<encode> round %d" % r for r in range(3)}
