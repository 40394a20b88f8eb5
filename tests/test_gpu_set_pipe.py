"""Block sets on the wave-pipelined encoder (ZPQ_SET_PIPE, BlockSet(pipe=True)): k_pipe<..., KEEP> loads a member's state
from its slot and leaves it there in the format k_chain<..., KEEP> keeps, so any round may run on either encoder and every
round is decoded by k_chain<decode>.  Expected bytes come from oracle_lib.Codec, one per member, one encode(seg, pp=True)
per segment -- the yardstick of test_gpu_blockset.py.  Every test that claims the pipeline checks the kernel's name after
every call: none can pass by falling back."""
import os
import random
import sys

import pytest

import chain_models as CM
import oracle_lib as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

pytestmark = pytest.mark.gpu

KNOBS = ("ZPQ_SET_PIPE", "ZPQ_SET_LANES", "ZPQ_ENC_PIPE", "ZPQ_ENC_SPLIT", "ZPQ_PIPE_PER", "ZPQ_PIPE_SHARE", "ZPQ_DEC_PIPE",
         "ZPQ_DEC_HYP16", "ZPQ_SPARSE_MODE", "ZPQ_SPARSE_FORCE_LOG2", "ZPQ_CHAIN_G", "ZPQ_CHAIN_BPW")
# segments shorter than the pipeline is deep (up to nine stages and the coder), the empty one, and a few long ones
LENGTHS = [0, 1, 2, 3, 8, 9, 10, 17, 64, 65, 300, 1500]
NMEMBERS = 53                                            # no multiple of any blocks-per-workgroup; rounds of 53, 39, 26, 13
NAMES = ["l2_mixed", "l2_hh2_hm1", "l1_sizes", "l3_mixed", "l4_rate255", "l4_rate0", "l5_small"]
PIPE, CHAIN, DECODE = "k_pipe<encode>", "k_chain<encode>", "k_chain<decode>"
E_OVERFLOW, E_TOOBIG = -7, -4


def _data(r, kind, n):
    if kind == 0:
        return bytes(n)
    if kind == 1:
        return bytes(r.getrandbits(8) for _ in range(n))
    if kind == 2:
        return bytes(r.choice(b"etaoin shrdlu\n") for _ in range(n))
    per = bytes(r.getrandbits(8) for _ in range(r.randint(1, 40)))
    return (per * (n // len(per) + 1))[:n]


def make_members(seed, nmembers=NMEMBERS, cut=None):
    """member m: 1 + m mod 4 segments, lengths from LENGTHS, data zeros / random / text / periodic"""
    r = random.Random(seed)
    members = [[_data(r, (m + s) % 4, r.choice(LENGTHS)) for s in range(1 + m % 4)] for m in range(nmembers)]
    return [[seg[:cut] for seg in segs] for segs in members] if cut else members


def oracle_history(header, members):
    out = []
    for segs in members:
        codec = O.Codec(header)
        out.append([codec.encode(seg, pp=True) for seg in segs])
    return out


def header_of(zpq, what):
    return zpq.level_header(what) if isinstance(what, int) else CM.NAMED[what][0]


@pytest.fixture()
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def check_every_round(zpq, ctx, header, members, line_store=None):
    """Round r codes the r-th segment of every member that has one on the pipeline: bytes, lengths, statuses against the
    oracle and the kernel's name, every round; a second, plain set decodes every round back on k_chain<decode>."""
    want = oracle_history(header, members)
    model = zpq.Model(header=header)
    total = max(sum(len(s) for s in segs) for segs in members)
    enc = zpq.BlockSet(ctx, model, len(members), max_member_bytes=total, pipe=True)
    dec = zpq.BlockSet(ctx, model, len(members), max_member_bytes=total)
    try:
        assert enc.pipe and not enc.lanes and not dec.pipe
        rounds = max(len(segs) for segs in members)
        assert rounds == 4
        for r in range(rounds):
            idx = [m for m in range(len(members)) if len(members[m]) > r]
            assert len(idx) >= 12
            coded, status, out_len = enc.encode_segments([members[m][r] for m in idx], members=idx)
            assert ctx.last_kernel_name == PIPE, (r, ctx.last_kernel_name)
            if line_store is not None:
                assert ctx.last_line_store == line_store, (r, ctx.last_line_store)
            assert [int(s) for s in status] == [0] * len(idx), (r, list(status))
            for j, m in enumerate(idx):
                assert int(out_len[j]) == len(want[m][r]), ("length", r, m, int(out_len[j]), len(want[m][r]))
                assert coded[j] == want[m][r], ("coded bytes", r, m, len(members[m][r]))
            back, status, consumed, _, first = dec.decode_segments([want[m][r] for m in idx], cap=1500 + 8, members=idx)
            assert ctx.last_kernel_name == DECODE
            assert [int(s) for s in status] == [0] * len(idx), (r, list(status))
            for j, m in enumerate(idx):
                assert back[j] == members[m][r], ("decoded bytes", r, m, len(members[m][r]), len(back[j]))
            assert [int(c) for c in consumed] == [len(want[m][r]) for m in idx], r
    finally:
        enc.close()
        dec.close()
        model.close()


@pytest.mark.parametrize("what", [1, 2, 3, 4, 5] + NAMES, ids=str)
def test_every_shape_every_round(zpq, gpu_ctx, clean_env, what):
    header = header_of(zpq, what)
    members = make_members(2000 + (what if isinstance(what, int) else NAMES.index(what) + 10))
    check_every_round(zpq, gpu_ctx, header, members)


@pytest.mark.parametrize("what", [1, 2, 3], ids=str)
def test_dense_tables(zpq, gpu_ctx, clean_env, what):
    clean_env.setenv("ZPQ_SPARSE_MODE", "never")
    check_every_round(zpq, gpu_ctx, header_of(zpq, what), make_members(300 + what), line_store=0)


@pytest.mark.parametrize("what", [3, "l3_mixed"], ids=str)
def test_line_store_of_1024(zpq, gpu_ctx, clean_env, what):
    # a 1024-line store refuses a member beyond 960 claimed lines per table: keep every member below 2 (n + 2) <= 960
    clean_env.setenv("ZPQ_SPARSE_FORCE_LOG2", "10")
    check_every_round(zpq, gpu_ctx, header_of(zpq, what), make_members(77, cut=100), line_store=1024)


@pytest.mark.parametrize("pipe_first", [True, False], ids=["pipe_first", "chain_first"])
@pytest.mark.parametrize("level", [1, 2, 4, 5])
def test_the_two_encoders_continue_each_other(zpq, gpu_ctx, clean_env, level, pipe_first):
    """The shared slot format: counters, weights, rows, MIX2 weights, prev / m4 / b4 written by one encoder and read by
    the other, round after round."""
    header = zpq.level_header(level)
    r = random.Random(40 + level)
    n, rounds = 16, 6
    members = [[_data(r, (m + s) % 4, r.choice([1, 3, 9, 17, 65, 300])) for s in range(rounds)] for m in range(n)]
    want = oracle_history(header, members)
    model = zpq.Model(header=header)
    enc = zpq.BlockSet(gpu_ctx, model, n, max_member_bytes=rounds * 300, pipe=True)
    try:
        assert enc.pipe
        for s in range(rounds):
            on_pipe = (s % 2 == 0) == pipe_first
            if on_pipe:
                clean_env.delenv("ZPQ_ENC_PIPE", raising=False)
            else:
                clean_env.setenv("ZPQ_ENC_PIPE", "0")
            coded, status, out_len = enc.encode_segments([members[m][s] for m in range(n)])
            assert gpu_ctx.last_kernel_name == (PIPE if on_pipe else CHAIN), (s, gpu_ctx.last_kernel_name)
            assert [int(x) for x in status] == [0] * n, (s, list(status))
            for m in range(n):
                assert coded[m] == want[m][s], ("coded bytes", s, m)
    finally:
        enc.close()
        model.close()


def test_the_floor_subsets_and_a_batch_between(zpq, gpu_ctx, clean_env):
    """Twelve live members run on the pipeline, eleven on the chain encoder, call by call on one set; unordered subsets,
    fresh and kept members in one call, an ordinary batch on the ctx's slot pool between two set calls."""
    header = zpq.level_header(2)
    model = zpq.Model(header=header)
    r = random.Random(19)
    n = 16
    codecs = [O.Codec(header) for _ in range(n)]
    enc = zpq.BlockSet(gpu_ctx, model, n, pipe=True)

    def call(idx):
        segs = [_data(r, (m + len(idx)) % 4, r.choice([0, 1, 17, 65, 300])) for m in idx]
        coded, status, _ = enc.encode_segments(segs, members=idx)
        assert gpu_ctx.last_kernel_name == (PIPE if len(idx) >= 12 else CHAIN), (idx, gpu_ctx.last_kernel_name)
        assert [int(s) for s in status] == [0] * len(idx)
        for j, m in enumerate(idx):
            assert coded[j] == codecs[m].encode(segs[j], pp=True), (idx, m)

    try:
        assert enc.pipe
        call(list(range(12)))                                 # 12: the pipeline
        call(list(range(11)))                                 # 11: the chain encoder
        call([11, 3, 7, 0, 9, 1, 5, 10, 2, 8, 4, 6])          # the same twelve, unordered
        call([15, 2, 13, 0, 14, 4, 12, 6, 8, 10, 1])          # 12-15 are fresh, the others are not: chain
        blocks = [_data(r, k % 4, 200) for k in range(14)]
        coded, status, _ = gpu_ctx.encode_blocks(model, blocks)
        assert (status == 0).all() and coded == O.encode_blocks(header, blocks)
        call([15, 1, 13, 3, 14, 5, 12, 7, 9, 11, 0, 2, 4])    # thirteen, fresh-on-chain members now on the pipeline
        call([6, 4, 2])
        call(list(range(n)))
        call(list(range(n - 1, 4, -1)))                       # eleven, descending
        call(list(range(n - 1, 3, -1)))                       # twelve, descending
    finally:
        enc.close()
        model.close()


def test_store_full_is_sticky(zpq, gpu_ctx, clean_env):
    """test_gpu_blockset's case -- six segments of 300 random bytes into a 1024-line store (refused beyond 960 claimed
    lines) -- with twelve quiet neighbours, so that every call runs on the pipeline: the claim count is carried from launch
    to launch, a later round gets ZPQ_E_TOOBIG, everything before it equals the oracle, everything after it repeats the
    status, and the neighbours never notice."""
    clean_env.setenv("ZPQ_SPARSE_FORCE_LOG2", "10")
    header = zpq.level_header(3)
    r = random.Random(5)
    n, loud = 13, 6
    members = [[_data(r, 1, 300) if m == loud else _data(r, 2 + m % 2, 40) for _ in range(6)] for m in range(n)]
    want = oracle_history(header, members)
    model = zpq.Model(header=header)
    enc = zpq.BlockSet(gpu_ctx, model, n, pipe=True)
    failed_at = None
    try:
        assert enc.pipe
        for s in range(6):
            coded, status, out_len = enc.encode_segments([members[m][s] for m in range(n)])
            assert gpu_ctx.last_line_store == 1024 and gpu_ctx.last_kernel_name == PIPE, (s, gpu_ctx.last_kernel_name)
            for m in range(n):
                if m != loud:
                    assert int(status[m]) == 0 and coded[m] == want[m][s], (s, m)
            if failed_at is None and int(status[loud]) == 0:
                assert coded[loud] == want[loud][s], s
            else:
                assert int(status[loud]) == E_TOOBIG, (s, int(status[loud]))
                failed_at = s if failed_at is None else failed_at
        assert failed_at is not None and failed_at >= 1, failed_at
    finally:
        enc.close()
        model.close()


def test_overflow_is_sticky(zpq, gpu_ctx, clean_env):
    """A slab one byte short on one member: ZPQ_E_OVERFLOW with out_len = the full coded length and the slab holding the
    prefix; later calls repeat the status without coding; the neighbours are untouched."""
    header = zpq.level_header(2)
    model = zpq.Model(header=header)
    r = random.Random(11)
    n, short = 13, 12                                        # (the short slab is the last one: every slab starts 16-aligned)
    codecs = [O.Codec(header) for _ in range(n)]
    enc = zpq.BlockSet(gpu_ctx, model, n, pipe=True)
    try:
        assert enc.pipe
        segs = [_data(r, 2, 64) for _ in range(n)]
        segs[short] = _data(r, 1, 300)
        want = [codecs[m].encode(segs[m], pp=True) for m in range(n)]
        caps = [4096] * n
        caps[short] = len(want[short]) - 1
        coded, status, out_len = enc.encode_segments(segs, cap=caps)
        assert gpu_ctx.last_kernel_name == PIPE
        assert [int(s) for s in status] == [0] * short + [E_OVERFLOW]
        assert int(out_len[short]) == len(want[short]) and coded[short] == want[short][:-1]
        assert coded[:short] == want[:short]
        for _ in range(2):
            segs = [_data(r, 2, 17) for _ in range(n)]
            coded, status, out_len = enc.encode_segments(segs)
            assert gpu_ctx.last_kernel_name == PIPE               # twelve live members
            assert [int(s) for s in status] == [0] * short + [E_OVERFLOW] and int(out_len[short]) == 0
            assert coded[:short] == [codecs[m].encode(segs[m], pp=True) for m in range(short)]
    finally:
        enc.close()
        model.close()


def test_the_request_where_it_decides_nothing(zpq, gpu_ctx, clean_env):
    """chain7 (a runtime-loop route) and C4b (no chain model): pipe stays False, the set codes as without the flag, on the
    kernels it ran on before."""
    from inputs import C4B
    for header, enc_name, nm in ((CM.NAMED["chain7"][0], CHAIN, 13), (C4B, "k_generic<encode>", 3)):
        r = random.Random(3)
        members = [[_data(r, (m + s) % 4, r.choice([1, 17, 65, 300])) for s in range(2)] for m in range(nm)]
        want = oracle_history(header, members)
        model = zpq.Model(header=header)
        names = []
        for pipe in (True, False):
            enc = zpq.BlockSet(gpu_ctx, model, nm, pipe=pipe)
            try:
                assert enc.pipe is False
                for s in range(2):
                    coded, status, _ = enc.encode_segments([members[m][s] for m in range(nm)])
                    names.append(gpu_ctx.last_kernel_name)
                    assert [int(x) for x in status] == [0] * nm
                    assert coded == [want[m][s] for m in range(nm)], (pipe, s)
            finally:
                enc.close()
        assert names == [enc_name] * 4, names
        model.close()
