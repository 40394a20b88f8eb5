"""Block sets (zpq_blockset_*, binding.BlockSet): N blocks that hold several segments each, a segment of every block per
launch, the state handed from launch to launch through the set's slots (k_chain<..., KEEP>).  Expected values come
from oracle_lib.Codec, which keeps its model across encode calls the way the reference's Compressor does between
start_block and end_block (compressor.v:238-245): per member one Codec, one encode per segment."""
import random
import sys
import os

import pytest

import chain_models as CM
import oracle_lib as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

pytestmark = pytest.mark.gpu

KNOBS = ("ZPQ_ENC_PIPE", "ZPQ_ENC_SPLIT", "ZPQ_DEC_PIPE", "ZPQ_DEC_HYP16", "ZPQ_SPARSE_MODE", "ZPQ_SPARSE_FORCE_LOG2",
         "ZPQ_CHAIN_G", "ZPQ_CHAIN_BPW")
LENGTHS = [0, 1, 2, 3, 17, 64, 65, 300, 1500]
NMEMBERS = 21                                            # no multiple of any blocks-per-workgroup (4, 8, 12, 16, 32)
NAMES = ["l1_sizes", "l2_hh2_hm1", "l2_hm0", "l3_mixed", "chain7", "l4_rate255", "l5_small", "mix2_chain3", "chain16"]
E_OVERFLOW, E_TOOBIG, E_CLOSED, E_ARG = -7, -4, -10, -2


def _data(r, kind, n):
    if kind == 0:
        return bytes(n)
    if kind == 1:
        return bytes(r.getrandbits(8) for _ in range(n))
    if kind == 2:
        return bytes(r.choice(b"etaoin shrdlu\n") for _ in range(n))
    per = bytes(r.getrandbits(8) for _ in range(r.randint(1, 40)))
    return (per * (n // len(per) + 1))[:n]


def make_members(seed, nmembers=NMEMBERS):
    """member m: 1 + m mod 4 segments, lengths from LENGTHS, data zeros / random / text / periodic"""
    r = random.Random(seed)
    return [[_data(r, (m + s) % 4, r.choice(LENGTHS)) for s in range(1 + m % 4)] for m in range(nmembers)]


def oracle_history(header, members):
    """coded[m][s]: what the sequential coder writes for segment s of member m"""
    out = []
    for segs in members:
        codec = O.Codec(header)
        out.append([codec.encode(seg, pp=True) for seg in segs])
    return out


def header_of(zpq, what):
    return zpq.level_header(what) if isinstance(what, int) else CM.NAMED[what][0]


def check_parity(zpq, ctx, header, members, want, enc_name="k_chain<encode>", dec_name="k_chain<decode>"):
    """Round r codes the r-th segment of every member that has one: bytes, lengths and status against the oracle, then
    a second set decodes them back."""
    model = zpq.Model(header=header)
    total = max(sum(len(s) for s in segs) for segs in members)
    enc = zpq.BlockSet(ctx, model, len(members), max_member_bytes=total)
    dec = zpq.BlockSet(ctx, model, len(members), max_member_bytes=total)
    try:
        for r in range(max(len(segs) for segs in members)):
            idx = [m for m in range(len(members)) if len(members[m]) > r]
            coded, status, out_len = enc.encode_segments([members[m][r] for m in idx], members=idx)
            assert ctx.last_kernel_name == enc_name
            assert [int(s) for s in status] == [0] * len(idx), (r, list(status))
            for j, m in enumerate(idx):
                assert int(out_len[j]) == len(want[m][r]), ("length", r, m, int(out_len[j]), len(want[m][r]))
                assert coded[j] == want[m][r], ("coded bytes", r, m, len(members[m][r]))
            back, status, consumed, _, first = dec.decode_segments([want[m][r] for m in idx], cap=1500 + 8, members=idx)
            assert ctx.last_kernel_name == dec_name
            assert [int(s) for s in status] == [0] * len(idx), (r, list(status))
            for j, m in enumerate(idx):
                assert back[j] == members[m][r], ("decoded bytes", r, m, len(members[m][r]), len(back[j]))
            assert [int(c) for c in consumed] == [len(want[m][r]) for m in idx], r
            assert all(int(f) == 0 for f in first), r
    finally:
        enc.close()
        dec.close()
        model.close()


@pytest.fixture()
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.mark.parametrize("what", [1, 2, 3, 4, 5] + NAMES, ids=str)
def test_every_route(zpq, gpu_ctx, clean_env, what):
    header = header_of(zpq, what)
    members = make_members(1000 + (what if isinstance(what, int) else NAMES.index(what) + 10))
    check_parity(zpq, gpu_ctx, header, members, oracle_history(header, members))


@pytest.mark.parametrize("what,env", [(3, {"ZPQ_SPARSE_FORCE_LOG2": "10"}), ("l3_mixed", {"ZPQ_SPARSE_FORCE_LOG2": "10"}),
                                      (3, {"ZPQ_DEC_HYP16": "0"}), (4, {"ZPQ_DEC_HYP16": "0"}),
                                      (2, {"ZPQ_SPARSE_MODE": "never"}), (3, {"ZPQ_SPARSE_MODE": "never"}),
                                      (3, {"ZPQ_SPARSE_MODE": "never", "ZPQ_DEC_HYP16": "0"})], ids=str)
def test_other_routes(zpq, gpu_ctx, clean_env, what, env):
    for k, v in env.items():
        clean_env.setenv(k, v)
    header = header_of(zpq, what)
    members = make_members(77, nmembers=9)
    if "ZPQ_SPARSE_FORCE_LOG2" in env:
        # a 1024-line store refuses a member beyond 960 claimed lines per table: keep every member below 2 (n + 2) <= 960
        members = [[seg[:100] for seg in segs] for segs in members]
    check_parity(zpq, gpu_ctx, header, members, oracle_history(header, members))


def test_store_full_is_sticky(zpq, gpu_ctx, clean_env):
    """Six segments of 300 random bytes into a 1024-line store (refused beyond 960 claimed lines): the first fits by the
    2 (n + 2) = 604 bound, a later one gets ZPQ_E_TOOBIG, everything before it equals the oracle, everything after it
    repeats the status, and the neighbours never notice."""
    clean_env.setenv("ZPQ_SPARSE_FORCE_LOG2", "10")
    header = zpq.level_header(3)
    r = random.Random(5)
    members = [[_data(r, 2, 40) for _ in range(6)], [_data(r, 1, 300) for _ in range(6)], [_data(r, 3, 40) for _ in range(6)]]
    want = oracle_history(header, members)
    model = zpq.Model(header=header)
    enc = zpq.BlockSet(gpu_ctx, model, 3)
    failed_at = None
    for s in range(6):
        coded, status, _ = enc.encode_segments([members[m][s] for m in range(3)])
        assert gpu_ctx.last_line_store == 1024 and gpu_ctx.last_kernel_name == "k_chain<encode>"
        assert int(status[0]) == 0 and int(status[2]) == 0 and coded[0] == want[0][s] and coded[2] == want[2][s], s
        if failed_at is None and int(status[1]) == 0:
            assert coded[1] == want[1][s], s
        else:
            assert int(status[1]) == E_TOOBIG, (s, int(status[1]))
            failed_at = s if failed_at is None else failed_at
    assert failed_at is not None and failed_at >= 1, failed_at
    enc.close()
    model.close()


def test_subsets_and_a_batch_between(zpq, gpu_ctx, clean_env):
    """Unordered subsets, fresh and kept members in one call, an ordinary batch on the ctx's slot pool between two set
    calls: every member follows its own history."""
    header = zpq.level_header(2)
    model = zpq.Model(header=header)
    r = random.Random(9)
    codecs = [O.Codec(header) for _ in range(8)]
    enc = zpq.BlockSet(gpu_ctx, model, 8)

    def call(idx):
        segs = [_data(r, (m + len(idx)) % 4, r.choice([1, 17, 65, 300])) for m in idx]
        coded, status, _ = enc.encode_segments(segs, members=idx)
        assert [int(s) for s in status] == [0] * len(idx)
        for j, m in enumerate(idx):
            assert coded[j] == codecs[m].encode(segs[j], pp=True), (idx, m)

    call([5, 2, 7])
    call([2, 0, 5, 1])                                    # 0 and 1 are fresh, 2 and 5 are not
    blocks = [_data(r, k % 4, 200) for k in range(14)]
    coded, status, _ = gpu_ctx.encode_blocks(model, blocks)
    assert (status == 0).all() and coded == O.encode_blocks(header, blocks)
    call([7, 1, 3, 0])
    call([6, 4, 2])
    call(list(range(8)))
    enc.close()
    model.close()


def test_other_models_fall_back_to_the_lane0_kernel(zpq, gpu_ctx, clean_env):
    from inputs import C4B
    members = make_members(3, nmembers=3)
    members = [segs[:2] + [b"x" * 17] * (2 - len(segs[:2])) for segs in members]
    want = oracle_history(C4B, members)
    check_parity(zpq, gpu_ctx, C4B, members, want, "k_generic<encode>", "k_generic<decode>")


def test_overflow_is_sticky(zpq, gpu_ctx, clean_env):
    header = zpq.level_header(2)
    model = zpq.Model(header=header)
    r = random.Random(11)
    codecs = [O.Codec(header) for _ in range(3)]
    enc = zpq.BlockSet(gpu_ctx, model, 3)
    segs = [_data(r, 2, 64), _data(r, 1, 300), _data(r, 2, 64)]
    coded, status, out_len = enc.encode_segments(segs, cap=[4096, 16, 4096])     # 300 random bytes do not fit 16
    assert [int(s) for s in status] == [0, E_OVERFLOW, 0]
    assert coded[0] == codecs[0].encode(segs[0]) and coded[2] == codecs[2].encode(segs[2])
    segs = [_data(r, 2, 17), _data(r, 2, 17), _data(r, 2, 17)]
    coded, status, out_len = enc.encode_segments(segs)
    assert [int(s) for s in status] == [0, E_OVERFLOW, 0] and int(out_len[1]) == 0
    assert coded[0] == codecs[0].encode(segs[0]) and coded[2] == codecs[2].encode(segs[2])
    coded, status, _ = enc.encode_segments([b"abc"], members=[1])
    assert [int(s) for s in status] == [E_OVERFLOW]
    enc.close()
    model.close()


def test_arguments(zpq, gpu_ctx, clean_env):
    import numpy as np
    model = zpq.Model(level=1)
    st = zpq.BlockSet(gpu_ctx, model, 4)
    assert gpu_ctx.blockset_capacity(model) >= 4
    L = zpq.lib()
    off = np.zeros(5, dtype=np.uint64)
    u = np.zeros(4, dtype=np.uint32)
    i4 = np.zeros(4, dtype=np.int32)
    for members in ([0, 0], [0, 4], [-1, 1]):             # not distinct, out of range
        m = np.asarray(members, dtype=np.int32)
        assert L.zpq_blockset_encode_segments(st.h, 2, m.ctypes.data, None, off.ctypes.data, 1, None, off.ctypes.data,
                                              u.ctypes.data, i4.ctypes.data) == E_ARG
    assert L.zpq_blockset_encode_segments(st.h, 5, None, None, off.ctypes.data, 1, None, off.ctypes.data, u.ctypes.data, i4.ctypes.data) == E_ARG
    assert L.zpq_blockset_encode_segments(st.h, 1, None, None, off.ctypes.data, 1 | 4, None, off.ctypes.data, u.ctypes.data, i4.ctypes.data) == E_ARG
    st.close()
    model.close()


def test_lifetime_orders(zpq):
    """On a context of the test's own: the set first; the ctx first (the set is orphaned: ZPQ_E_CLOSED, destroy still
    fine); the model dropped before the set that was built on it."""
    header = zpq.level_header(2)
    want = O.Codec(header).encode(b"abc" * 50)
    ctx = zpq.Context(0)
    model = zpq.Model(header=header)
    a = zpq.BlockSet(ctx, model, 2)
    b = zpq.BlockSet(ctx, model, 3)
    assert a.encode_segments([b"abc" * 50], members=[1])[0][0] == want
    a.close()                                              # the set before its ctx
    zpq.lib().zpq_model_destroy(model.h)                   # the model before the set: the set holds a reference
    model.h = None
    assert b.encode_segments([b"abc" * 50], members=[2])[0][0] == want
    zpq.lib().zpq_ctx_destroy(ctx.h)                       # the ctx before the set, through the raw call
    ctx.h = None
    with pytest.raises(zpq.ZpqError) as e:
        b.encode_segments([b"abc"], members=[0])
    assert e.value.code == E_CLOSED
    b.close()
    ctx2 = zpq.Context(0)
    m2 = zpq.Model(header=header)
    c = zpq.BlockSet(ctx2, m2, 2)
    ctx2.close()                                           # the binding's order: children first
    assert c.h is None
