"""GPU parity of the chain kernels on chain models other than the five shipped levels (tests/chain_models.py): every
specialised instantiation at other table sizes, hh / hm and MIX2 parameters, the runtime-loop instantiation at every
chain length, and the models just outside the chain layout -- each against the CPU oracle, through every encoder and
decoder that takes the model, dense tables and the line store, fewer slots than blocks, and the two general kernels."""
import contextlib
import random

import pytest

import chain_models as CM
import oracle_lib as O
import workload as W

pytestmark = pytest.mark.gpu

BUDGET, MAX_BLOCK = 150 << 30, 65536                   # the session context's defaults (restored after every change)
KNOBS = ("ZPQ_ENC_PIPE", "ZPQ_ENC_SPLIT", "ZPQ_DEC_PIPE", "ZPQ_DEC_HYP16", "ZPQ_SPARSE_MODE", "ZPQ_SPARSE_FORCE_LOG2",
         "ZPQ_CHAIN_G", "ZPQ_CHAIN_BPW")
ENC_OTHER = {"k_lanes<encode>", "k_rows<encode>", "k_gpipe<encode>"}
DEC_OTHER = {"k_lanes<decode>", "k_rows<decode>", "k_gdec<decode>"}
GPU_GEN_SEED, GPU_GEN_COUNT = 4, 40                     # (this seed's 40 models reach every route class)
SIZES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 3000, 4096]


def _block(r, kind, n):
    if kind == 0:
        return bytes(n)
    if kind == 1:
        return bytes(r.getrandbits(8) for _ in range(n))
    if kind == 2:
        return bytes(r.choice(b"etaoin shrdlu\n") for _ in range(n))
    if kind == 3:
        per = bytes(r.getrandbits(8) for _ in range(r.randint(1, 40)))
        return (per * (n // len(per) + 1))[:n]
    return bytes(W.make_block(r.randrange(1 << 16), n))


def ragged_blocks(seed, big=True):
    """0, 1, 2, 15-17, 63-65, 255-257 bytes, a few KiB, and one 64 KiB block: 15 blocks, so the pipelines engage."""
    r = random.Random(seed)
    blocks = [_block(r, i % 5, n) for i, n in enumerate(SIZES)]
    if big:
        blocks.append(_block(r, 4, 65536))
    return blocks


@contextlib.contextmanager
def knobs(mp, **env):
    for k, v in env.items():
        mp.setenv(k, v)
    try:
        yield
    finally:
        for k in env:
            mp.delenv(k, raising=False)


def enc_names(rt, ctx, env):
    """The encoder a batch of this route must have run (the library decides on the host, per call)."""
    if rt is None:
        return ENC_OTHER
    if ctx.last_slots >= 12 and env.get("ZPQ_ENC_PIPE") != "0" and rt["nch_spec"]:
        if rt["nch_spec"] == 2 and not ctx.last_line_store and env.get("ZPQ_ENC_SPLIT") != "0":
            return {"k_pipe2<encode>"}
        return {"k_pipe<encode>"}
    return {"k_chain<encode>"}


def dec_names(rt, ctx, env):
    if rt is None:
        return DEC_OTHER
    if (env.get("ZPQ_DEC_PIPE") == "1" and ctx.last_slots >= 12 and not ctx.last_line_store and not rt["has_mix2"]
            and rt["nch_spec"] in (2, 3, 5)):
        return {"k_dpipe<decode>"}
    return {"k_chain<decode>"}


class Run:
    """One model on the session context: encode / decode helpers that check everything a call returns."""

    def __init__(self, zpq, ctx, mp, hdr, offs=None):
        self.zpq, self.ctx, self.mp, self.hdr = zpq, ctx, mp, hdr
        self.model = zpq.Model(header=hdr, offsets=offs)         # (offs: stated (cend, hbegin, hend); None = scanned)
        assert self.model.has_fast_path
        self.rt = CM.route(zpq, self.model)
        self.seen = set()
        for k in KNOBS:
            mp.delenv(k, raising=False)

    def encode(self, blocks, want, pp, flags=0, names=None, **env):
        with knobs(self.mp, **env):
            coded, status, _ = self.ctx.encode_blocks(self.model, blocks, flags=flags | (self.zpq.FLAG_PP if pp else 0))
            name = self.ctx.last_kernel_name
            ok = names if names is not None else enc_names(self.rt, self.ctx, env)
        assert name in ok, (name, ok, env)
        assert [int(s) for s in status] == [0] * len(blocks), (name, env, list(status))
        for i, (c, w) in enumerate(zip(coded, want)):
            assert c == w, (name, env, "block", i, len(blocks[i]), len(c), len(w))
        self.seen.add(name)
        return coded

    def decode(self, coded, blocks, pp, flags=0, names=None, **env):
        cap = max(len(b) for b in blocks) + 64
        with knobs(self.mp, **env):
            dec, status, consumed, code, first = self.ctx.decode_blocks(self.model, coded, cap=cap,
                                                                       flags=flags | (self.zpq.FLAG_PP if pp else 0))
            name = self.ctx.last_kernel_name
            ok = names if names is not None else dec_names(self.rt, self.ctx, env)
        assert name in ok, (name, ok, env)
        assert [int(s) for s in status] == [0] * len(blocks), (name, env, list(status))
        for i in range(len(blocks)):
            assert dec[i] == blocks[i], (name, env, "block", i, len(blocks[i]), len(dec[i]))
        assert [int(c) for c in consumed] == [len(c) for c in coded], (name, env)
        if pp:
            assert all(int(f) == 0 for f in first), (name, env)
        self.seen.add(name)
        return [len(d) for d in dec], [int(c) for c in consumed], [int(c) for c in code], [int(f) for f in first]

    def encoders(self, blocks, want, pp):
        """Default encoder, the lane-per-component one where a pipeline took the batch, k_pipe besides k_pipe2, and a
        batch too small for any pipeline (k_chain<encode>)."""
        coded = self.encode(blocks, want, pp)
        spec = self.rt["nch_spec"] if self.rt else 0
        if spec:
            self.encode(blocks, want, pp, ZPQ_ENC_PIPE="0")
        if spec == 2:
            self.encode(blocks, want, pp, ZPQ_ENC_SPLIT="0")
        self.encode(blocks[:11], want[:11], pp)
        return coded

    def decoders(self, coded, blocks, pp):
        """Default decoder, the eight-lane one besides HYP16, the wave-split one (opt-in); all must agree on what
        they return besides the bytes: out_len, consumed, final_code, first_byte."""
        res = [self.decode(coded, blocks, pp)]
        spec = self.rt["nch_spec"] if self.rt else 0
        if spec in (5, 6):
            res.append(self.decode(coded, blocks, pp, ZPQ_DEC_HYP16="0"))
        if spec in (2, 3, 5) and not self.rt["has_mix2"]:
            res.append(self.decode(coded, blocks, pp, ZPQ_DEC_PIPE="1"))
        for r in res[1:]:
            assert r == res[0]

    def tables(self, blocks, want, pp, max_block=4096):
        """Dense tables only; then the line store for every table larger than a store sized for max_block-byte blocks
        (so that blocks of that size really fill it, and small tables stay dense in the same model)."""
        self.encode(blocks, want, pp, ZPQ_SPARSE_MODE="never")
        small = [i for i, b in enumerate(blocks) if len(b) <= max_block]
        sb, sw = [blocks[i] for i in small], [want[i] for i in small]
        L = self.zpq.lib()
        L.zpq_ctx_set_max_block_bytes(self.ctx.h, max_block)
        try:
            coded = self.encode(sb, sw, pp, ZPQ_SPARSE_MODE="always")
            store = self.ctx.last_line_store
            self.decode(coded, sb, pp, ZPQ_SPARSE_MODE="always")
        finally:
            L.zpq_ctx_set_max_block_bytes(self.ctx.h, MAX_BLOCK)
        return store

    def slot_reuse(self, blocks, want, pp, slots=3):
        L = self.zpq.lib()
        L.zpq_ctx_set_state_budget(self.ctx.h, slots * self.model.state_bytes + 1000)
        try:
            coded = self.encode(blocks, want, pp, ZPQ_SPARSE_MODE="never")
            if self.rt is not None:
                assert self.ctx.last_slots == slots
            self.decode(coded, blocks, pp, ZPQ_SPARSE_MODE="never")
        finally:
            L.zpq_ctx_set_state_budget(self.ctx.h, BUDGET)

    def cross_check(self, blocks, want, pp, generic=True):
        """The lane-per-component kernel and the lane-0 kernel: independent implementations, the same streams."""
        self.encode(blocks, want, pp, flags=self.zpq.FLAG_LANES, names={"k_lanes<encode>", "k_rows<encode>", "k_gpipe<encode>"})
        if generic:                                     # (one lane per block: the 64 KiB block would dominate the test's time)
            small = [i for i, b in enumerate(blocks) if len(b) <= 4096]
            self.encode([blocks[i] for i in small], [want[i] for i in small], pp, flags=self.zpq.FLAG_GENERIC,
                        names={"k_generic<encode>"})


@pytest.mark.parametrize("name", sorted(CM.NAMED))
def test_named_chain_model(zpq, gpu_ctx, monkeypatch, name):
    hdr, route = CM.NAMED[name]
    run = Run(zpq, gpu_ctx, monkeypatch, hdr)
    blocks = ragged_blocks(sum(name.encode()))
    want = O.encode_blocks(hdr, blocks, nthreads=8)
    coded = run.encoders(blocks, want, True)
    run.decoders(coded, blocks, True)
    store = run.tables(blocks, want, True)
    if name in ("l2_mixed", "l3_mixed"):                   # dense and line-store tables in one specialised kernel
        assert store > 0
    run.slot_reuse(blocks, want, True)
    run.cross_check(blocks, want, True)
    raw = O.encode_blocks(hdr, blocks, pp=False, nthreads=8)   # without the PP byte: default encoder and decoder
    run.decode(run.encode(blocks, raw, False), blocks, False)
    assert CM.route_key(run.rt) == route                  # (last: a wrong route shows first as a wrong stream)
    if route is not None:
        assert run.seen & {"k_pipe<encode>", "k_pipe2<encode>"} or not route[0]
        assert "k_chain<encode>" in run.seen and "k_chain<decode>" in run.seen


@pytest.mark.parametrize("index", range(GPU_GEN_COUNT))
def test_generated_chain_model(zpq, gpu_ctx, monkeypatch, index):
    hdr = CM.generated(GPU_GEN_SEED, GPU_GEN_COUNT, big=True)[index]
    run = Run(zpq, gpu_ctx, monkeypatch, hdr)
    blocks = ragged_blocks(1000 + index)
    want = O.encode_blocks(hdr, blocks, nthreads=8)
    coded = run.encoders(blocks, want, True)
    run.decoders(coded, blocks, True)
    if index % 2 == 0:
        run.tables(blocks, want, True)
    if index % 4 == 1:
        run.slot_reuse(blocks, want, True)
    run.cross_check(blocks, want, True, generic=False)
    raw = O.encode_blocks(hdr, blocks, pp=False, nthreads=8)
    run.decode(run.encode(blocks, raw, False), blocks, False)


@pytest.mark.parametrize("name", ["l2_mixed", "l3_mixed", "l4_rate255", "chain9"])
def test_forced_small_store_refuses_a_block_too_large(zpq, gpu_ctx, monkeypatch, name):
    """A 1024-line store: a block that would need more lines is refused (ZPQ_E_TOOBIG) in its own status, the small
    blocks around it (at most 2 * 258 probes per table) are coded and decoded exactly."""
    hdr = CM.NAMED[name][0]
    run = Run(zpq, gpu_ctx, monkeypatch, hdr)
    r = random.Random(55)
    blocks = ragged_blocks(56, big=False)[:12] + [bytes(r.getrandbits(8) for _ in range(3000))] + ragged_blocks(57, big=False)[:6]
    want = O.encode_blocks(hdr, blocks, nthreads=8)
    with knobs(monkeypatch, ZPQ_SPARSE_FORCE_LOG2="10"):
        coded, status, _ = gpu_ctx.encode_blocks(run.model, blocks)
        assert gpu_ctx.last_line_store == 1024
        assert [int(s) for s in status] == [0] * 12 + [-4] + [0] * 6
        assert coded[:12] == want[:12] and coded[13:] == want[13:]
        ok = blocks[:12] + blocks[13:]
        dec, status, consumed, _, first = gpu_ctx.decode_blocks(run.model, want[:12] + want[13:], cap=4200)
        assert (status == 0).all() and dec == ok and (first == 0).all()
