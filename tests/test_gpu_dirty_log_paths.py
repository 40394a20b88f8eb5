"""The dirty-line logs (tests/dirty_log.py) on the paths test_gpu_dirty_log.py leaves out: slots that code several blocks in
one launch, host batches in rounds, other kernels on the same model between two log-keeping launches, own-slot launches
that must leave the logs alone, damaged streams, the device-pointer entry points, two contexts, two threads, models that
come and go, and the edges of ZPQ_DIRTY_LOG_CAP.  Every launch is compared with the C oracle stream for stream with a status
per block; every sequence runs twice on one ctx: once with the logs' counts read back after each launch that keeps them
(conditions on every count, and the overflow regime the sequence names), once with zpq_debug_pool_residue (= 0) instead.
After a launch that keeps no log both calls must fail."""
import threading

import pytest

import dirty_log as DL
import segment_path as SP
from dirty_log import BUDGET, MAX_BLOCK, Run, oracle
from test_gpu_host_stripes import EARLY, KNOBS, STRIPED, EncBufs, cap_of, decode_raw, knobs
from test_gpu_offnominal import check_decode, raw_decode

pytestmark = pytest.mark.gpu

CAPS = [None, "64", "8", "13", "1"]
# what a batch with 2 KiB uniform blocks beside one-byte blocks must reach: 2 * (2048 + 2) < 16384; a one-byte block logs
# at least one line and at most 2 * (1 + 2) = 6 < 8; any coded byte makes a line of every table non-zero
REGIME = {None: "never", "64": "mixed", "8": "mixed", "13": "mixed", "1": "always"}


@pytest.fixture
def env(monkeypatch, zpq, gpu_ctx):
    """Kernel-selecting knobs and the capacity cleared before, budget and max_block back at the defaults afterwards."""
    for k in KNOBS + ("ZPQ_DIRTY_LOG_CAP",):
        monkeypatch.delenv(k, raising=False)
    try:
        yield monkeypatch
    finally:
        zpq.lib().zpq_ctx_set_state_budget(gpu_ctx.h, BUDGET)
        zpq.lib().zpq_ctx_set_max_block_bytes(gpu_ctx.h, MAX_BLOCK)


def set_cap(mp, cap_env):
    if cap_env is None:
        mp.delenv("ZPQ_DIRTY_LOG_CAP", raising=False)
    else:
        mp.setenv("ZPQ_DIRTY_LOG_CAP", cap_env)


def twice(zpq, ctx, name, cap_env, seq, **kw):
    """the sequence with the counts read back, then with the residue pass"""
    for residue in (False, True):
        r = Run(zpq, ctx, name, cap_env, residue, **kw)
        try:
            seq(r)
            r.finish()
        finally:
            r.model.close()


# ---------------------------------------------------------------- rounds inside a launch
def seq_rounds(r):
    """83 blocks (four rounds and a partial one), 19, 45, 83, encode and decode in turn, then the same with the directions
    swapped; the plans (dirty_log.round_plan) put clean-table data behind dirty data on every slot count."""
    r.enc("rounds", 83, 1)
    r.dec("rounds", 19, 2, pp=False)
    r.enc("rounds", 45, 3)
    r.dec("rounds", 83, 1)
    r.dec("rounds", 83, 4, pp=False)
    r.enc("rounds", 19, 2, pp=False)
    r.dec("rounds", 45, 3)
    r.enc("rounds", 83, 4, pp=False)
    r.dec("rounds", 19, 2, pp=False)


@pytest.mark.parametrize("cap_env", CAPS)
@pytest.mark.parametrize("slots", [19, 13, 5])
@pytest.mark.parametrize("name", ["level2", "small"])
def test_rounds_inside_a_launch(zpq, gpu_ctx, env, name, slots, cap_env):
    set_cap(env, cap_env)
    env.setenv("ZPQ_SPARSE_MODE", "never")
    model = zpq.Model(header=DL.HEADERS[name])
    zpq.lib().zpq_ctx_set_state_budget(gpu_ctx.h, slots * model.state_bytes + 1000)    # (once: the call drops the logs)
    model.close()

    def seq(r):
        seq_rounds(r)
        assert gpu_ctx.last_line_store == 0
    twice(zpq, gpu_ctx, name, cap_env, seq, slots=slots, regime=REGIME[cap_env])


# ---------------------------------------------------------------- host batches in rounds
def host_rounds(r, decode, kind, nb, seed, pp, rounds, last_kernel, keeps):
    """one host-pointer call that host_pipeline launches once per round of r.slots blocks"""
    blocks, want = oracle(r.name, kind, nb, seed, pp)
    flags = r.zpq.FLAG_PP if pp else 0
    if decode:
        got, status, *_ = r.ctx.decode_blocks(r.model, want, cap=2100, flags=flags)
        expect = blocks
    else:
        got, status, _ = r.ctx.encode_blocks(r.model, blocks, flags=flags)
        expect = want
    assert r.ctx.last_host_transfer == rounds << 8 and r.ctx.last_kernel_name == last_kernel
    assert r.ctx.last_slots == (nb - 1) % r.slots + 1
    r.after(keeps, [(len(b), pp) for b in blocks], nslots=min(nb, r.slots))
    assert (status == 0).all() and got == expect, (kind, nb, decode)


@pytest.mark.parametrize("cap_env", [None, "64", "8"])
@pytest.mark.parametrize("name", ["level2", "small"])
def test_host_batches_in_rounds(zpq, gpu_ctx, env, name, cap_env):
    """83 blocks on 16 slots: five rounds of 16 and one of 3, whose encoder is k_chain<encode> -- the call ends without a
    valid log; the decoder keeps it through all six."""
    set_cap(env, cap_env)
    env.setenv("ZPQ_SPARSE_MODE", "never")
    env.setenv("ZPQ_PIPE_MIN_BYTES", "1")
    model = zpq.Model(header=DL.HEADERS[name])
    zpq.lib().zpq_ctx_set_state_budget(gpu_ctx.h, 16 * model.state_bytes + 1000)
    model.close()

    def seq(r):
        r.both("uniform2k", 16, 1)
        host_rounds(r, False, "rounds16", 83, 5, True, 6, "k_chain<encode>", False)
        r.both("zeros", 16, 1)
        host_rounds(r, True, "rounds16", 83, 5, True, 6, "k_chain<decode>", True)
        r.both("zeros", 16, 1)
        host_rounds(r, True, "rounds16", 83, 6, False, 6, "k_chain<decode>", True)
        host_rounds(r, False, "rounds16", 83, 6, False, 6, "k_chain<encode>", False)
        host_rounds(r, True, "rounds16", 83, 5, True, 6, "k_chain<decode>", True)
        r.both("periodic", 16, 3)
    twice(zpq, gpu_ctx, name, cap_env, seq, slots=16, regime=REGIME[cap_env])


# ---------------------------------------------------------------- another kernel on the same model
# knobs, the directions they change, (encoder, decoder) that must run, does the launch still keep the log, a line store?
# ZPQ_CHAIN_G: level 2's specialised kernels exist for eight lanes per block only and build_cfg says so whatever the knob
# asks for -- the launch is the default one and keeps its log.  ZPQ_CHAIN_BPW regroups the slots over the workgroups.
VARIANTS = {
    "enc_chain": ({"ZPQ_ENC_PIPE": "0"}, "e", ("k_chain<encode>", None), False, False),
    "enc_split": ({"ZPQ_ENC_SPLIT": "60cd1"}, "e", ("k_pipe2<encode>", None), False, False),
    "dec_pipe": ({"ZPQ_DEC_PIPE": "1"}, "d", (None, "k_dpipe<decode>"), False, False),
    "line_store": ({"ZPQ_SPARSE_FORCE_LOG2": "13"}, "ed", ("k_pipe<encode>", "k_chain<decode>"), False, True),
    "chain_g": ({"ZPQ_CHAIN_G": "16"}, "ed", ("k_pipe<encode>", "k_chain<decode>"), True, False),
    "chain_bpw": ({"ZPQ_CHAIN_BPW": "16"}, "ed", ("k_pipe<encode>", "k_chain<decode>"), True, False),
    "enc_few": ({}, "e", ("k_chain<encode>", None), False, False),          # 11 blocks: below the pipeline's floor
}


def variant_launch(r, mp, which, decode):
    kv, _, names, keeps, store = VARIANTS[which]
    nb = 11 if which == "enc_few" else 40
    blocks, want = oracle(r.name, "uniform2k", nb, 2, True)
    with knobs(mp, **kv):
        if decode:
            got, status, *_ = r.ctx.decode_blocks(r.model, want, cap=2100)
        else:
            got, status, _ = r.ctx.encode_blocks(r.model, blocks)
        assert r.ctx.last_kernel_name == names[decode] and r.ctx.last_slots == nb
        assert (r.ctx.last_line_store > 0) == store
    r.after(keeps, [(len(b), True) for b in blocks])
    assert (status == 0).all() and got == (blocks if decode else want), (which, decode)


# (the small header's tables are smaller than any line store: the knob leaves its launches as they are)
VARIANT_CASES = [(w, n) for w in sorted(VARIANTS) for n in ("level2", "small") if (w, n) != ("line_store", "small")]


@pytest.mark.parametrize("cap_env", [None, "64", "8"])
@pytest.mark.parametrize("which,name", VARIANT_CASES)
def test_another_kernel_on_the_same_model(zpq, gpu_ctx, env, which, name, cap_env):
    """The variant's launch codes uniform data on the model and the pool of the log-keeping launches around it; the launch
    behind it codes zeros, on tables the variant left dirty and -- unless it is one that keeps the log -- unlogged."""
    set_cap(env, cap_env)

    def seq(r):
        for d in VARIANTS[which][1]:
            for behind in ((r.enc, r.dec) if d == "e" else (r.dec, r.enc)):
                r.both("mixed", 40, 1)
                variant_launch(r, env, which, d == "d")
                behind("zeros", 40, 1)
            r.both("zeros", 40, 1)
    twice(zpq, gpu_ctx, name, cap_env, seq, regime=REGIME[cap_env])


_HIO = {}


def hio_blocks(name):
    """64 uniform blocks of 32 KiB (the striped upload's floor) and their first 16 KiB (the early download's slabs), with the
    oracle's streams"""
    if name not in _HIO:
        big = [DL.make("uniform", 4000 + i, 32768) for i in range(64)]
        half = [b[:16384] for b in big]
        _HIO[name] = (big, DL.O.encode_blocks(DL.HEADERS[name], big, nthreads=8), half, DL.O.encode_blocks(DL.HEADERS[name], half, nthreads=8))
    return _HIO[name]


@pytest.mark.parametrize("cap_env", [None, "8"])
@pytest.mark.parametrize("name", ["level2", "small"])
def test_striped_upload_and_early_download_between_logged_launches(zpq, gpu_ctx, env, name, cap_env):
    """The HIO forms of k_pipe and k_chain<decode> run on the same model and pool and keep no log."""
    set_cap(env, cap_env)
    big, want_big, half, want_half = hio_blocks(name)
    bufs = EncBufs(zpq, [32768] * 64, [cap_of(32768)] * 64)
    try:
        def seq(r):
            r.both("mixed", 40, 1)
            coded = bufs.run(r.ctx, r.model, big, zpq.FLAG_PP)
            assert r.ctx.last_host_transfer == 1 << 8 | STRIPED and r.ctx.last_kernel_name == "k_pipe<encode>"
            assert r.ctx.last_slots == 64
            r.after(False)
            assert coded == want_big
            r.both("zeros", 40, 1)
            r.both("mixed", 40, 1)
            got, out = decode_raw(zpq, r.ctx, r.model, want_half, 16384, zpq.FLAG_PP)
            assert r.ctx.last_host_transfer == 1 << 8 | EARLY and r.ctx.last_kernel_name == "k_chain<decode>"
            assert r.ctx.last_slots == 64
            r.after(False)
            assert all(out[64 + i * 16384:64 + (i + 1) * 16384].tobytes() == b for i, b in enumerate(half))
            r.dec("zeros", 40, 1)
            r.both("zeros", 40, 1)
        twice(zpq, gpu_ctx, name, cap_env, seq, regime=REGIME[cap_env])
    finally:
        bufs.free()


# ---------------------------------------------------------------- launches of one block between two pool launches
# Own-slot launches -- a block's later segments (tests/segment_path.py: the replay of the first one and k_generic with the
# kept state, both on the block's slot) and a block set created, used and closed -- touch neither the pool nor the logs:
# the counts read the same afterwards and the residue pass finds nothing.  The one-block launches that do run on the pool
# -- a fresh block's first segment, zpq_debug_encode_trace, zpq_debug_contexts: slot 0, on kernels that keep no log --
# leave no valid log behind, except a fresh block's first decode: one block on the log-keeping decoder, slot 0 logged anew.
SEG = ("level2", "main")


def later_segments(zpq, r, blocks):
    """the sequence's segments behind the first through the two blocks (their first segments went before the pool launch)"""
    segs, want, back = SP.segments(*SEG), SP.coded(*SEG), SP.decoded(*SEG)
    for i in range(1, len(segs)):
        assert blocks[0].encode_segment(segs[i].data, flags=segs[i].flags) == want[i], i
        assert r.ctx.last_kernel_name == "k_generic<encode>"
        out, consumed, code, first = blocks[1].decode_segment(want[i], SP.CAP + 8, flags=segs[i].flags)
        assert r.ctx.last_kernel_name == "k_generic<decode>"
        assert (out, consumed, code, first) == (back[i].data, back[i].consumed, back[i].final_code, back[i].first_byte), i


def first_segments(zpq, r):
    segs, want, back = SP.segments(*SEG), SP.coded(*SEG), SP.decoded(*SEG)
    blocks = [zpq.Block(r.ctx, r.model), zpq.Block(r.ctx, r.model)]
    assert blocks[0].encode_segment(segs[0].data, flags=segs[0].flags) == want[0]
    assert r.ctx.last_kernel_name == "k_chain<encode>"
    assert blocks[1].decode_segment(want[0], SP.CAP + 8, flags=segs[0].flags)[0] == back[0].data
    assert r.ctx.last_kernel_name == "k_chain<decode>"
    return blocks


@pytest.mark.parametrize("cap_env", [None, "64"])
@pytest.mark.parametrize("name,what", [("level2", "segments"), ("level2", "blockset"), ("small", "blockset")])
def test_own_slot_launches_keep_the_logs_valid(zpq, gpu_ctx, env, name, what, cap_env):
    set_cap(env, cap_env)

    def seq(r):
        for first in (r.enc, r.dec):
            blocks = first_segments(zpq, r) if what == "segments" else []
            try:
                first("mixed", 40, 1)
                before = None if r.residue else r.ctx.debug_dlog_counts(40)
                if what == "segments":
                    later_segments(zpq, r, blocks)
                else:
                    r.blockset()
            finally:
                for b in blocks:
                    b.close()
            if r.residue:
                assert r.ctx.debug_dlog_counts(40).sum() == 0      # (the residue pass reset them)
                assert r.ctx.debug_pool_residue(40) == 0
            else:
                assert (r.ctx.debug_dlog_counts(40) == before).all()
            r.both("zeros", 40, 1)
    twice(zpq, gpu_ctx, name, cap_env, seq, regime=REGIME[cap_env])


@pytest.mark.parametrize("cap_env", [None, "64"])
@pytest.mark.parametrize("name,what", [("level2", "first_encode"), ("level2", "first_decode"), ("level2", "trace"), ("small", "trace"),
                                       ("level2", "contexts"), ("small", "contexts")])
def test_one_block_launches_on_the_pool(zpq, gpu_ctx, env, name, what, cap_env):
    set_cap(env, cap_env)
    data = DL.make("uniform", 31, 700)
    segs, want, back = SP.segments(*SEG), SP.coded(*SEG), SP.decoded(*SEG)

    def seq(r):
        for first in (r.enc, r.dec):
            first("mixed", 40, 1)
            before = None if r.residue else r.ctx.debug_dlog_counts(40)
            if what.startswith("first"):
                blk = zpq.Block(r.ctx, r.model)
                try:
                    if what == "first_encode":
                        assert blk.encode_segment(segs[0].data, flags=segs[0].flags) == want[0]
                        assert r.ctx.last_kernel_name == "k_chain<encode>"
                    else:
                        assert blk.decode_segment(want[0], SP.CAP + 8, flags=segs[0].flags)[0] == back[0].data
                        assert r.ctx.last_kernel_name == "k_chain<decode>"
                finally:
                    blk.close()
            elif what == "trace":
                coded, _ = r.ctx.debug_encode_trace(r.model, data, ntrace=200)
                assert coded == DL.O.encode_blocks(DL.HEADERS[r.name], [data])[0] and r.ctx.last_kernel_name == "k_generic<encode>"
            else:
                assert r.ctx.debug_contexts(r.model, data).shape == (700, 3)
            assert r.ctx.last_slots == 1
            if what == "first_decode":                    # slot 0 coded a block of 500 bytes, the others' logs are as they were
                r.after(True, [(len(segs[0].data), True)], nslots=1)
                if not r.residue:
                    assert (r.ctx.debug_dlog_counts(40)[1:] == before[1:]).all()
                else:
                    assert r.ctx.debug_pool_residue(40) == 0
            else:
                r.after(False, nslots=40)
            r.both("zeros", 40, 1)
    twice(zpq, gpu_ctx, name, cap_env, seq, regime=REGIME[cap_env])


# ---------------------------------------------------------------- damaged streams on the log-keeping decoder
def damaged(zpq, r, pp, slab):
    batch, caps, want = DL.damaged_batch(pp, slab)
    assert any(w.status == -7 for w in want) and any(w.status == 0 and c.kind != "exact" for w, c in zip(want, batch))
    got = raw_decode(zpq, r.ctx, r.model, [c.stream for c in batch], caps, zpq.FLAG_PP if pp else 0)
    assert r.ctx.last_kernel_name == "k_chain<decode>"
    r.after(True, [(w.out_len, pp) for w in want])
    check_decode("damaged pp=%s slab %d" % (pp, slab), batch, caps, want, got)


@pytest.mark.parametrize("cap_env", [None, "8"])
@pytest.mark.parametrize("slots", [None, 5])
def test_damaged_streams_then_clean_launches(zpq, gpu_ctx, env, slots, cap_env):
    set_cap(env, cap_env)
    env.setenv("ZPQ_SPARSE_MODE", "never")
    if slots:
        model = zpq.Model(header=DL.HEADERS["level2"])
        zpq.lib().zpq_ctx_set_state_budget(gpu_ctx.h, slots * model.state_bytes + 1000)
        model.close()

    def seq(r):
        r.both("uniform2k", 40, 2)
        damaged(zpq, r, True, 1531)
        r.both("zeros", 40, 1)
        damaged(zpq, r, False, 1531)
        damaged(zpq, r, True, 1531)
        r.dec("zeros", 40, 1)
        r.both("text", 40, 2)
    twice(zpq, gpu_ctx, "level2", cap_env, seq, slots=slots)


# ---------------------------------------------------------------- the device-pointer entry points
def seq_classes(r):
    for i, kind in enumerate(("uniform", "zeros", "text", "uniform")):
        r.both(kind, 40 if i % 2 == 0 else 16, i, pp=i != 2)
    r.both("mixed", 40, 1)


def seq_slot_counts(r):
    r.both("uniform", 40, 0)
    r.both("text", 16, 2, pp=False)
    r.both("zeros", 40, 1)                                # slots 16 .. 39 still hold the first launch's lines
    r.enc("uniform", 11, 5)                               # below twelve blocks the encoder is k_chain<encode>: no log
    r.both("zeros", 40, 1)
    r.dec("uniform", 11, 5)
    r.both("mixed", 16, 3)
    r.both("zeros", 40, 1)


@pytest.mark.parametrize("cap_env", [None, "64", "8"])
@pytest.mark.parametrize("name", ["level2", "small"])
@pytest.mark.parametrize("seq", [seq_classes, seq_slot_counts], ids=["classes", "slot_counts"])
def test_device_pointer_entry_points(zpq, gpu_ctx, env, seq, name, cap_env):
    set_cap(env, cap_env)
    twice(zpq, gpu_ctx, name, cap_env, seq, via="dev", regime=REGIME[cap_env])


# ---------------------------------------------------------------- contexts, threads, models
@pytest.mark.parametrize("cap_env", [None, "64"])
def test_two_contexts_alternate_on_one_model(zpq, gpu_ctx, env, cap_env):
    """Each ctx owns its pool and its logs: what the other one launched in between changes nothing."""
    set_cap(env, cap_env)
    other = zpq.Context(0)
    model = zpq.Model(header=DL.HEADERS["level2"])
    try:
        for residue in (False, True):
            a = Run(zpq, gpu_ctx, "level2", cap_env, residue, model=model, regime=REGIME[cap_env])
            b = Run(zpq, other, "level2", cap_env, residue, model=model, regime=REGIME[cap_env])
            a.both("mixed", 40, 1)
            b.both("uniform2k", 40, 2)
            a.both("zeros", 40, 1)
            b.both("zeros", 16, 1)
            a.enc("uniform2k", 11, 2)
            b.both("mixed", 40, 1)
            a.both("zeros", 40, 1)
            b.both("zeros", 40, 1)
            a.finish()
            b.finish()
    finally:
        model.close()
        other.close()


@pytest.mark.parametrize("cap_env", [None, "64"])
def test_two_threads_take_turns_on_one_ctx(zpq, gpu_ctx, env, cap_env):
    set_cap(env, cap_env)
    for residue in (False, True):
        r = Run(zpq, gpu_ctx, "level2", cap_env, residue, regime=REGIME[cap_env])
        turn, failed = threading.Barrier(2), []
        steps = [("mixed", 40, 1), ("zeros", 40, 1), ("uniform2k", 40, 2), ("zeros", 16, 1), ("mixed", 16, 3), ("zeros", 40, 1)]

        def work(me):
            try:
                for i, step in enumerate(steps):
                    if i % 2 == me:
                        r.both(*step)
                    turn.wait(timeout=60)
            except BaseException as e:                     # noqa: BLE001 (reported by the test's own thread)
                failed.append(e)
                turn.abort()
        threads = [threading.Thread(target=work, args=(me,)) for me in (0, 1)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        try:
            if failed:
                raise failed[0]
            r.finish()
        finally:
            r.model.close()


@pytest.mark.parametrize("cap_env", [None, "64"])
def test_models_closed_and_created_in_turn(zpq, gpu_ctx, env, cap_env):
    set_cap(env, cap_env)
    for residue in (False, True):
        for i in range(6):
            r = Run(zpq, gpu_ctx, "level2" if i % 2 == 0 else "small", cap_env, residue, regime=REGIME[cap_env])
            try:
                r.both("mixed", 40, 1)
                r.both("zeros", 40, 1)
                r.finish()
            finally:
                r.model.close()


# ---------------------------------------------------------------- the variable's edges
@pytest.mark.parametrize("value,on", [("", True), ("-5", False), ("abc", False), ("3", True), ("1048577", True)])
@pytest.mark.parametrize("name", ["level2", "small"])
def test_edges_of_the_capacity_variable(zpq, gpu_ctx, env, name, value, on):
    """Empty = the default, no number or a negative one = off, 3 is no multiple of four, 2^20 + 1 is clamped to 2^20: Run
    reads on / off from the residue call and the counts call (both fail after a launch without a log)."""
    assert (DL.parse_cap(value) != 0) == on and DL.parse_cap("1048577") == 1 << 20 and DL.parse_cap("") == DL.DEFAULT_CAP

    def seq(r):
        set_cap(env, "64")
        r.both("mixed", 16, 3)
        set_cap(env, value)
        assert r.on == on
        r.both("zeros", 16, 1)
        r.both("mixed", 16, 3)
        r.both("zeros", 16, 1)
    twice(zpq, gpu_ctx, name, value, seq)
