"""Striped host transfers (host_pipeline in zpq_api.hip) on every kernel that takes part in them.

A single round of 64 or more equally long blocks from pinned memory is UPLOADED IN STRIPES: the first 8 KiB of every
block, then -- beside the running encoder -- the rest, behind an in-kernel gate on a pinned flag.  A decoder's first three
quarters LEAVE EARLY, beside the running kernel, once every block has reported through a pinned counter.  Both paths
have kernels of their own (the HIO instantiations of k_chain, k_pipe and k_pipe2).  Held to the CPU oracle here, at the
smallest sizes at which the paths engage (64 blocks, 32 KiB of input, 16 KiB slabs):
  * every HIO encoder on every chain model that qualifies, all 64 streams;
  * the gate itself: the staging buffer is first filled with the COMPLEMENT of the input and the second stripe is then
    held back (ZPQ_STRIPE_DELAY_US) until every lane waits at the gate -- a lane that read ahead of the gate codes
    complement bytes;
  * the host conditions from both sides, seen through zpq_ctx_last_host_transfer;
  * early download of ragged blocks: which bytes of a slab may be written and which may not;
  * k_gather against numpy at every source / destination alignment.
"""
import contextlib
import random

import numpy as np
import pytest

import chain_models as CM
import oracle_lib as O
import workload as W

pytestmark = pytest.mark.gpu

BUDGET, MAX_BLOCK = 150 << 30, 65536                   # the session context's defaults (restored after every change)
KNOBS = ("ZPQ_ENC_PIPE", "ZPQ_ENC_SPLIT", "ZPQ_DEC_PIPE", "ZPQ_DEC_HYP16", "ZPQ_SPARSE_MODE", "ZPQ_SPARSE_FORCE_LOG2",
         "ZPQ_CHAIN_G", "ZPQ_CHAIN_BPW", "ZPQ_NO_STRIPE", "ZPQ_STRIPE_DELAY_US", "ZPQ_PIPE_MIN_BYTES", "ZPQ_PIPE_PER")
NB = 64                                                # host_pipeline: n >= 64
LEN = 32768                                            # ... L >= 4 * 8192
SLAB = 16384                                           # early download: slabs >= 16384
E = 12288                                              # ... its first stripe: 3/4 of the slab, rounded down to 256
FILL = 0xEE
STRIPED, EARLY = 1, 2                                  # bits of zpq_ctx_last_host_transfer


def header(name):
    """level1 / level2: the shipped headers; everything else: tests/chain_models.py."""
    return O.level_header(int(name[5:])) if name.startswith("level") else CM.NAMED[name][0]


TWO = ("level1", "l1_sizes")                           # chains of two components (k_pipe2 by default)
THREE = ("level2", "l2_mixed", "l2_hh2_hm1")           # chains of three (k_pipe by default)
# encoder variants: knobs and the kernel that must have run
VARIANTS = {
    "default": ({}, {2: "k_pipe2<encode>", 3: "k_pipe<encode>"}),
    "chain": ({"ZPQ_ENC_PIPE": "0"}, {2: "k_chain<encode>", 3: "k_chain<encode>"}),
    "split0": ({"ZPQ_ENC_SPLIT": "0"}, {2: "k_pipe<encode>"}),
    "60cd1": ({"ZPQ_ENC_SPLIT": "60cd1", "ZPQ_SPARSE_MODE": "never"}, {3: "k_pipe2<encode>"}),
}
ENC_CASES = [(m, v) for m in TWO + THREE for v in (("default", "chain", "split0") if m in TWO else ("default", "chain", "60cd1"))]

_BASE = []


def base_blocks():
    """64 blocks of 64 KiB, every one from another seed of the workload generator (text and periodic data: both stripes
    differ between blocks), a few of them all zero and a few uniformly random."""
    if not _BASE:
        for i in range(NB):
            seed = 4 * (i + 3) + (2 if i % 2 == 0 else 3)
            if i in (5, 37, 63):
                seed = 4 * i                           # class 0: zeros
            elif i in (0, 6, 21, 50):
                seed = 4 * i + 1                       # class 1: random
            _BASE.append(bytes(W.make_block(seed, 65536)))
    return _BASE


def blocks_of(L, n=NB):
    return [b[:L] for b in base_blocks()[:n]]


@pytest.fixture(scope="module")
def oracle():
    """want(model name, blocks key, blocks, pp): the oracle's streams, computed once per key."""
    cache = {}

    def want(name, key, blocks, pp=True):
        k = (name, key, pp)
        if k not in cache:
            cache[k] = O.encode_blocks(header(name), blocks, pp=pp, nthreads=8)
        return cache[k]
    return want


@pytest.fixture
def env(monkeypatch, zpq, gpu_ctx):
    """Knobs cleared before, budget and max_block back at the defaults afterwards."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    try:
        yield monkeypatch
    finally:
        zpq.lib().zpq_ctx_set_state_budget(gpu_ctx.h, BUDGET)
        zpq.lib().zpq_ctx_set_max_block_bytes(gpu_ctx.h, MAX_BLOCK)


@contextlib.contextmanager
def knobs(mp, **kv):
    for k, v in kv.items():
        mp.setenv(k, v)
    try:
        yield
    finally:
        for k in kv:
            mp.delenv(k, raising=False)


class EncBufs:
    """Caller-side buffers of one zpq_encode_blocks layout; run() may be called again on the same buffers."""

    def __init__(self, zpq, lens, caps, pinned_in=True, pinned_out=True, in_pad=0, out_pad=0):
        self.zpq, self.nb = zpq, len(lens)
        self.in_off = np.zeros(self.nb + 1, dtype=np.uint64)
        self.in_off[0] = in_pad
        self.in_off[1:] = in_pad + np.cumsum(lens)
        self.out_off = np.zeros(self.nb + 1, dtype=np.uint64)
        self.out_off[0] = out_pad
        self.out_off[1:] = out_pad + np.cumsum(caps)
        nin, nout = int(self.in_off[-1]) + 16, int(self.out_off[-1]) + 16
        self.pinned_out = pinned_out
        self.keep = []
        if pinned_in:
            self.keep.append(zpq.PinnedArray(nin))
            self.src = self.keep[-1].array
        else:
            self.src = np.zeros(nin, dtype=np.uint8)
        if pinned_out:
            self.keep.append(zpq.PinnedArray(nout))
            self.out = self.keep[-1].array
        else:
            self.out = np.zeros(nout, dtype=np.uint8)

    def run(self, ctx, model, blocks, flags):
        a, b = int(self.in_off[0]), int(self.in_off[-1])
        self.src[:] = 0x55
        self.src[a:b] = np.frombuffer(b"".join(blocks), dtype=np.uint8)
        self.out[:] = FILL
        olen = np.zeros(self.nb, dtype=np.uint32); st = np.full(self.nb, -99, dtype=np.int32)
        rc = self.zpq.lib().zpq_encode_blocks(ctx.h, model.h, self.nb, self.src.ctypes.data, self.in_off.ctypes.data, flags,
                                              self.out.ctypes.data, self.out_off.ctypes.data, olen.ctypes.data, st.ctypes.data)
        assert rc == 0 and (st == 0).all(), (rc, st)
        off = [int(x) for x in self.out_off]
        coded = [self.out[off[i]:off[i] + int(olen[i])].tobytes() for i in range(self.nb)]
        assert (self.out[:off[0]] == FILL).all() and (self.out[off[-1]:] == FILL).all()
        if self.pinned_out:                            # bytes behind a block's produced length were never touched
            for i in range(self.nb):
                assert (self.out[off[i] + int(olen[i]):off[i + 1]] == FILL).all(), i
        return coded

    def free(self):
        self.src = self.out = None
        for p in self.keep:
            p.free()


def same_streams(coded, want, what=""):
    """All streams, not a sample; a difference is reported with the offset of the first differing coded byte."""
    assert len(coded) == len(want)
    for i, (c, w) in enumerate(zip(coded, want)):
        if c != w:
            k = next((j for j in range(min(len(c), len(w))) if c[j] != w[j]), min(len(c), len(w)))
            raise AssertionError("%s: block %d differs from the oracle at coded byte %d (lengths %d / %d)" % (what, i, k, len(c), len(w)))


def cap_of(L):
    """The coder's worst case (the models with tiny tables expand their input several times)."""
    return L * 17 + 4096


def encode(zpq, ctx, model, blocks, flags, **kw):
    bufs = EncBufs(zpq, [len(b) for b in blocks], [cap_of(len(b)) for b in blocks], **kw)
    try:
        return bufs.run(ctx, model, blocks, flags)
    finally:
        bufs.free()


# ------------------------------------------------------------------ 1. every HIO encoder, every qualifying model
@pytest.mark.parametrize("name,variant", ENC_CASES)
def test_striped_upload_every_encoder(zpq, gpu_ctx, env, oracle, name, variant):
    model = zpq.Model(header=header(name))
    kv, kernel = VARIANTS[variant]
    blocks = blocks_of(LEN)
    with knobs(env, **kv):
        coded = encode(zpq, gpu_ctx, model, blocks, zpq.FLAG_PP)
        assert gpu_ctx.last_host_transfer & STRIPED and gpu_ctx.last_host_transfer >> 8 == 1
        assert gpu_ctx.last_kernel_name == kernel[model.ncomp]
        assert gpu_ctx.last_line_store == 0
    same_streams(coded, oracle(name, LEN, blocks), "%s %s" % (name, variant))


@pytest.mark.parametrize("name", ["level1", "level2"])
def test_striped_upload_without_pp_byte(zpq, gpu_ctx, env, oracle, name):
    model = zpq.Model(header=header(name))
    blocks = blocks_of(LEN)
    coded = encode(zpq, gpu_ctx, model, blocks, 0)
    assert gpu_ctx.last_host_transfer & STRIPED and gpu_ctx.last_line_store == 0
    assert gpu_ctx.last_kernel_name == VARIANTS["default"][1][model.ncomp]
    same_streams(coded, oracle(name, LEN, blocks, pp=False), name)


# ------------------------------------------------------------------ 2. the gate, deterministically
GATE_DELAY_US = 100000      # far below the kernel's spin bound (2^22 sleeps and system-scope loads: seconds), well above the
                            # ~25 ms a lane needs to reach byte 8192


@pytest.mark.parametrize("pp", [True, False])
@pytest.mark.parametrize("name,variant", [c for c in ENC_CASES if c[0] in ("level1", "level2")])
def test_lanes_wait_at_the_gate(zpq, gpu_ctx, env, oracle, name, variant, pp):
    """The complement of the input goes through the same context, layout and buffers first: the staging buffer then holds
    a wrong byte at every offset.  The real input's second stripe is held back for 100 ms, so every lane arrives at the
    gate before it: a byte read ahead of the gate is a complement byte, and the stream differs from the oracle's from
    the coded byte on that this input byte first influences.
    With and without the PP byte: k_chain's window (enc_byte) looks at the dword it requested only when the NEXT call
    slides into it, and drops it otherwise.  With the PP byte the furthest lane's first position behind the gate is
    gate_pos - 1, no slide, so a dword requested too early is asked for again and never coded; without it that position
    is gate_pos, a slide.  Only flags = 0 can show a k_chain look-ahead beyond its margin.  (The pipe kernels' window
    keeps two dwords across the gate: either form shows theirs.)"""
    model = zpq.Model(header=header(name))
    kv, kernel = VARIANTS[variant]
    flags = zpq.FLAG_PP if pp else 0
    blocks = blocks_of(LEN)
    inverse = [(np.frombuffer(b, dtype=np.uint8) ^ 0xFF).tobytes() for b in blocks]
    bufs = EncBufs(zpq, [LEN] * NB, [cap_of(LEN)] * NB)
    try:
        with knobs(env, **kv):
            bufs.run(gpu_ctx, model, inverse, flags)
            assert gpu_ctx.last_host_transfer & STRIPED
            with knobs(env, ZPQ_STRIPE_DELAY_US=str(GATE_DELAY_US)):
                coded = bufs.run(gpu_ctx, model, blocks, flags)
            assert gpu_ctx.last_host_transfer & STRIPED
            assert gpu_ctx.last_kernel_name == kernel[model.ncomp]
    finally:
        bufs.free()
    same_streams(coded, oracle(name, LEN, blocks, pp=pp), "%s %s pp=%s behind a late second stripe" % (name, variant, pp))


# ------------------------------------------------------------------ 3. where striping must not engage
def test_striping_stays_off_outside_its_conditions(zpq, gpu_ctx, env, oracle):
    L = zpq.lib()
    model = zpq.Model(header=header("level2"))
    blocks = blocks_of(LEN)
    want = oracle("level2", LEN, blocks)

    def plain(coded, wanted, what, rounds=1):
        assert gpu_ctx.last_host_transfer == rounds << 8, (what, gpu_ctx.last_host_transfer)
        same_streams(coded, wanted, what)

    # first the batch itself, so that every case below differs from a striped one in a single condition
    same_streams(encode(zpq, gpu_ctx, model, blocks, zpq.FLAG_PP), want, "64 x 32768")
    assert gpu_ctx.last_host_transfer == 1 << 8 | STRIPED
    plain(encode(zpq, gpu_ctx, model, blocks[:63], zpq.FLAG_PP), want[:63], "63 blocks")
    for n in (32764, 32770):                           # below 4 stripes; not a multiple of 4
        short = blocks_of(n)
        plain(encode(zpq, gpu_ctx, model, short, zpq.FLAG_PP), oracle("level2", n, short), "L = %d" % n)
    odd = list(blocks)
    odd[17] = base_blocks()[17][:LEN + 4]              # one block four bytes longer
    want_odd = list(want)
    want_odd[17] = O.encode_blocks(header("level2"), [odd[17]])[0]
    plain(encode(zpq, gpu_ctx, model, odd, zpq.FLAG_PP), want_odd, "one longer block")
    plain(encode(zpq, gpu_ctx, model, blocks, zpq.FLAG_PP, pinned_in=False), want, "pageable input")
    with knobs(env, ZPQ_NO_STRIPE="1"):
        plain(encode(zpq, gpu_ctx, model, blocks, zpq.FLAG_PP), want, "ZPQ_NO_STRIPE")
    # two rounds of 64 blocks each (the batch twice, 64 slots, rounds forced on this small batch): every round on its own meets
    # all the other conditions
    try:
        L.zpq_ctx_set_state_budget(gpu_ctx.h, 64 * model.state_bytes + 1000)
        with knobs(env, ZPQ_PIPE_MIN_BYTES="0", ZPQ_SPARSE_MODE="never"):
            plain(encode(zpq, gpu_ctx, model, blocks + blocks, zpq.FLAG_PP), want + want, "two rounds", rounds=2)
            assert gpu_ctx.last_slots == 64 and gpu_ctx.last_line_store == 0
    finally:
        L.zpq_ctx_set_state_budget(gpu_ctx.h, BUDGET)


def test_striping_stays_off_for_line_store_and_longer_chains(zpq, gpu_ctx, env, oracle):
    L = zpq.lib()
    blocks = blocks_of(LEN)
    # a forced line store: level 1's 32 MiB ISSE table behind a store sized for 32 KiB blocks
    model = zpq.Model(header=header("level1"))
    try:
        L.zpq_ctx_set_max_block_bytes(gpu_ctx.h, LEN)
        with knobs(env, ZPQ_SPARSE_MODE="always"):
            coded = encode(zpq, gpu_ctx, model, blocks, zpq.FLAG_PP)
            assert gpu_ctx.last_line_store > 0 and gpu_ctx.last_host_transfer == 1 << 8
    finally:
        L.zpq_ctx_set_max_block_bytes(gpu_ctx.h, MAX_BLOCK)
    same_streams(coded, oracle("level1", LEN, blocks), "line store")
    # five components: no HIO kernel
    model = zpq.Model(header=header("l3_mixed"))
    with knobs(env, ZPQ_SPARSE_MODE="never"):
        coded = encode(zpq, gpu_ctx, model, blocks, zpq.FLAG_PP)
        assert gpu_ctx.last_host_transfer == 1 << 8 and gpu_ctx.last_line_store == 0
    same_streams(coded, oracle("l3_mixed", LEN, blocks), "l3_mixed")


# ------------------------------------------------------------------ 4. where striping must still engage
def test_striping_engages_at_the_edges_of_its_conditions(zpq, gpu_ctx, env, oracle):
    L = zpq.lib()
    model = zpq.Model(header=header("level2"))
    blocks = blocks_of(LEN)
    want = oracle("level2", LEN, blocks)
    on = 1 << 8 | STRIPED
    same_streams(encode(zpq, gpu_ctx, model, blocks, zpq.FLAG_PP), want, "L = 32768")
    assert gpu_ctx.last_host_transfer == on
    # buffers that begin at odd offsets (in_off[0] = 5, out_off[0] = 7)
    same_streams(encode(zpq, gpu_ctx, model, blocks, zpq.FLAG_PP, in_pad=5, out_pad=7), want, "odd offsets")
    assert gpu_ctx.last_host_transfer == on
    # 16 slots for the 64 blocks: one round, the resident groups work the blocks off in turn
    try:
        L.zpq_ctx_set_state_budget(gpu_ctx.h, 16 * model.state_bytes + 1000)
        with knobs(env, ZPQ_SPARSE_MODE="never"):
            coded = encode(zpq, gpu_ctx, model, blocks, zpq.FLAG_PP)
            assert gpu_ctx.last_host_transfer == on and gpu_ctx.last_slots == 16 and gpu_ctx.last_line_store == 0
    finally:
        L.zpq_ctx_set_state_budget(gpu_ctx.h, BUDGET)
    same_streams(coded, want, "16 slots")
    big = blocks_of(65536)
    same_streams(encode(zpq, gpu_ctx, model, big, zpq.FLAG_PP), oracle("level2", 65536, big), "L = 65536")
    assert gpu_ctx.last_host_transfer == on


# ------------------------------------------------------------------ 5. early download on ragged blocks
GUARD = 64
RAGGED = [0, 1, 255, E - 1, E, E + 1, E + 255, 16383, 16384]


def ragged_blocks(slab):
    """The nine lengths around the first stripe's end, repeated to 64 blocks and shuffled; no block longer than its slab."""
    lens = [min(n, slab) for n in (RAGGED * 8)[:NB]]
    random.Random(12288).shuffle(lens)
    return [b[:n] for b, n in zip(base_blocks(), lens)]


def decode_raw(zpq, ctx, model, coded, slab, flags):
    """zpq_decode_blocks from pinned input into uniform pinned slabs between two guards."""
    nb = len(coded)
    in_off = np.zeros(nb + 1, dtype=np.uint64)
    in_off[1:] = np.cumsum([len(c) for c in coded])
    out_off = GUARD + np.arange(nb + 1, dtype=np.uint64) * np.uint64(slab)
    p_in, p_out = zpq.PinnedArray(int(in_off[-1]) + 16), zpq.PinnedArray(int(out_off[-1]) + GUARD)
    try:
        p_in.array[:int(in_off[-1])] = np.frombuffer(b"".join(coded), dtype=np.uint8)
        p_out.array[:] = FILL
        res = {k: np.full(nb, 0xABCDEF, dtype=np.uint32) for k in ("out_len", "consumed", "final_code", "first_byte")}
        st = np.full(nb, -99, dtype=np.int32)
        rc = zpq.lib().zpq_decode_blocks(ctx.h, model.h, nb, p_in.array.ctypes.data, in_off.ctypes.data, flags,
                                         p_out.array.ctypes.data, out_off.ctypes.data, res["out_len"].ctypes.data,
                                         res["consumed"].ctypes.data, res["final_code"].ctypes.data, res["first_byte"].ctypes.data,
                                         st.ctypes.data)
        assert rc == 0 and (st == 0).all(), (rc, st)
        return res, p_out.array.copy()
    finally:
        p_in.free(); p_out.free()


def check_early_download(zpq, ctx, mp, oracle, name, pp, slab=SLAB, early=True, kv=None):
    model = zpq.Model(header=header(name))
    blocks = ragged_blocks(slab)
    coded = oracle(name, ("ragged", slab), blocks, pp=pp)
    flags = zpq.FLAG_PP if pp else 0
    with knobs(mp, **(kv or {})):
        got, out = decode_raw(zpq, ctx, model, coded, slab, flags)
        assert ctx.last_host_transfer == (1 << 8 | (EARLY if early else 0))
        assert ctx.last_kernel_name == "k_chain<decode>" and ctx.last_line_store == 0
        with knobs(mp, ZPQ_NO_STRIPE="1"):
            ref, ref_out = decode_raw(zpq, ctx, model, coded, slab, flags)
        assert ctx.last_host_transfer == 1 << 8
    for k in ref:                                      # field by field as the plain path gives them ...
        assert (got[k] == ref[k]).all(), k
    assert [int(x) for x in got["out_len"]] == [len(b) for b in blocks]       # ... and as they must be
    assert [int(x) for x in got["consumed"]] == [len(c) for c in coded]
    if pp:
        assert (got["first_byte"] == 0).all()
    first = E if early else 0
    for view, skip in ((out, first), (ref_out, 0)):
        assert (view[:GUARD] == FILL).all() and (view[GUARD + NB * slab:] == FILL).all()
        for i, b in enumerate(blocks):
            o = GUARD + i * slab
            assert view[o:o + len(b)].tobytes() == b, i
            # behind the block: untouched, except that the first stripe of EVERY slab was copied (unspecified bytes)
            assert (view[o + max(len(b), skip):o + slab] == FILL).all(), (i, len(b))


@pytest.mark.parametrize("pp", [True, False])
@pytest.mark.parametrize("name", ["level1", "level2", "l2_mixed"])
def test_early_download_of_ragged_blocks(zpq, gpu_ctx, env, oracle, name, pp):
    check_early_download(zpq, gpu_ctx, env, oracle, name, pp)


@pytest.mark.parametrize("pp", [True, False])
@pytest.mark.parametrize("name", ["level1", "level2", "l2_mixed"])
def test_early_download_with_fewer_slots_than_blocks(zpq, gpu_ctx, env, oracle, name, pp):
    """16 slots for 64 blocks: a resident group reports once per block it works off."""
    model = zpq.Model(header=header(name))
    try:
        zpq.lib().zpq_ctx_set_state_budget(gpu_ctx.h, 16 * model.state_bytes + 1000)
        check_early_download(zpq, gpu_ctx, env, oracle, name, pp, kv={"ZPQ_SPARSE_MODE": "never"})
        assert gpu_ctx.last_slots == 16
    finally:
        zpq.lib().zpq_ctx_set_state_budget(gpu_ctx.h, BUDGET)


@pytest.mark.parametrize("name", ["level1", "level2", "l2_mixed"])
def test_no_early_download_below_16_kib_slabs(zpq, gpu_ctx, env, oracle, name):
    """Slabs of 16380 bytes (the two longest blocks shortened to fit): everything leaves behind the kernel."""
    check_early_download(zpq, gpu_ctx, env, oracle, name, True, slab=16380, early=False)


@pytest.mark.parametrize("name", ["level1", "level2"])
def test_early_download_keeps_the_reporting_decoder(zpq, gpu_ctx, env, oracle, name):
    """ZPQ_DEC_PIPE=1 asks for the wave-split decoder, which does not report: zpq_launch_chain keeps k_chain<decode>."""
    check_early_download(zpq, gpu_ctx, env, oracle, name, True, kv={"ZPQ_DEC_PIPE": "1"})


# ------------------------------------------------------------------ 6. k_gather against numpy
GATHER_LENS = [0, 1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 255, 4096, 4099]


def test_gather_every_alignment_against_numpy(zpq, gpu_ctx):
    """zpq_gather_dev: one launch with every source misalignment (0-3) x destination misalignment (0-15) x length; the
    destination is 0xEE everywhere else, with at least one such byte between neighbouring ranges."""
    import torch
    cases = [(sm, dm, n) for sm in range(4) for dm in range(16) for n in GATHER_LENS]
    random.Random(6).shuffle(cases)
    src_off, dst_off, s, d = [], [], 0, 16
    for sm, dm, n in cases:
        s = (s + 3) // 4 * 4 + sm
        src_off.append(s)
        s += n
        d = (d + 15) // 16 * 16 + dm
        dst_off.append(d)
        d += n + 1                                     # (a guard byte even where the next range starts at misalignment 0)
    nsrc, ndst = s + 16, d + 32                        # the kernel reads whole dwords: 16 spare bytes behind the source
    rng = np.random.default_rng(66)
    src = rng.integers(0, 256, nsrc, dtype=np.uint8)
    lens = np.array([c[2] for c in cases], dtype=np.uint32)
    want = np.full(ndst, FILL, dtype=np.uint8)
    for so, do, n in zip(src_off, dst_off, lens):
        assert so + int(n) <= nsrc - 16 and do + int(n) < ndst
        want[do:do + int(n)] = src[so:so + int(n)]
    dev = torch.device("cuda:0")
    t_src = torch.from_numpy(src).to(dev)
    t_soff = torch.from_numpy(np.array(src_off, dtype=np.int64)).to(dev)
    t_doff = torch.from_numpy(np.array(dst_off, dtype=np.int64)).to(dev)
    t_len = torch.from_numpy(lens.astype(np.int32)).to(dev)
    t_dst = torch.full((ndst,), FILL, dtype=torch.uint8, device=dev)
    assert t_src.data_ptr() % 16 == 0 and t_dst.data_ptr() % 16 == 0
    torch.cuda.synchronize()                           # the ctx stream does not wait for torch's
    rc = zpq.lib().zpq_gather_dev(gpu_ctx.h, len(cases), t_src.data_ptr(), t_soff.data_ptr(), t_len.data_ptr(),
                                  t_dst.data_ptr(), t_doff.data_ptr())
    assert rc == 0
    gpu_ctx.sync()
    got = t_dst.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, ("first wrong destination byte", int(bad[0]), len(bad))
    # blocks of length 0 wrote nothing: their destination byte and its neighbours are still the fill
    for (sm, dm, n), do in zip(cases, dst_off):
        if n == 0:
            assert (got[do - 1:do + 1] == FILL).all()
