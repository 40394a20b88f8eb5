"""GPU parity of the general-model kernels across the model space (tests/general_models.py): k_gpipe in its byte-batched
and bit-serial forms, k_gdec at 64 / 32 / 16 lanes, k_rows and k_lanes for encode and decode with the hash chain in
registers and with the interpreter, k_generic both ways -- every named case and every generated model against the CPU
oracle on ragged batches, with and without the PP byte, through every encoder and decoder that takes the model, with fewer
slots than blocks, the kernel that ran asserted by name from the route pinned on the CPU (test_general_models_cpu.py)."""
import random

import pytest

import general_models as GM
import oracle_lib as O
from test_gpu_chain_models import BUDGET, _block, knobs, ragged_blocks

pytestmark = pytest.mark.gpu

KNOBS = ("ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE", "ZPQ_GPIPE_BATCH", "ZPQ_LANES_ROWS", "ZPQ_GDEC_BPW")
BIG_BLOCK = 16384                                      # (the 64 KiB block of the chain test costs a 64-component model's
#                                                        oracle and its one-block-per-wave kernels seconds per call)
# more than 64 blocks: a k_gpipe / k_gdec workgroup's lanes are full and a second workgroup starts
WIDE_NAMED = ("cm_alias", "ht_edge", "mix_x4", "sse_small", "n15_deep", "ring136", "sse14", "n16", "mix3_sse3_n22")


def general_blocks(seed, big=True):
    """The chain test's ragged batch (0, 1, 2, 15-17, 63-65, 255-257 bytes, a few KiB) and one block of 16 KiB."""
    blocks = ragged_blocks(seed, big=False)
    if big:
        blocks.append(_block(random.Random(seed + 1), 4, BIG_BLOCK))
    return blocks


def wide_blocks(seed, count=150):
    r = random.Random(seed)
    return [_block(r, i % 5, r.choice([0, 1, 2, 16, 33, 64, 255, 257, 600])) for i in range(count)]


class Run:
    """One model on the session context: encode / decode helpers that check everything a call returns and the kernel that
    ran.  rt is the route with no knob set: (gpipe, gdec, lanes, k_rows | k_lanes)."""

    def __init__(self, zpq, ctx, mp, hdr, offs=None):
        self.zpq, self.ctx, self.mp, self.hdr = zpq, ctx, mp, hdr
        for k in KNOBS:
            mp.delenv(k, raising=False)
        self.model = zpq.Model(header=hdr, offsets=offs)         # (offs: stated (cend, hbegin, hend); None = scanned)
        self.rt = GM.route(zpq, self.model)
        self.rows = self.rt[3] == GM.ROWS
        self.seen = set()

    def kernel(self, decode, flags, env):
        """The kernel a call must run, from the route and the knobs (the library decides on the host, per call)."""
        d = "<decode>" if decode else "<encode>"
        if flags & self.zpq.FLAG_GENERIC or not self.rt[2]:
            return "k_generic" + d
        if self.rt[1 if decode else 0] and env.get("ZPQ_DEC_GPIPE" if decode else "ZPQ_ENC_GPIPE") != "0":
            return "k_gdec<decode>" if decode else "k_gpipe<encode>"
        return (GM.ROWS if self.rows and env.get("ZPQ_LANES_ROWS") != "0" else GM.LANES) + d

    def encode(self, blocks, want, pp, flags=0, slots=None, **env):
        F = flags | self.zpq.FLAG_LANES | (self.zpq.FLAG_PP if pp else 0)
        with knobs(self.mp, **env):
            coded, status, out_len = self.ctx.encode_blocks(self.model, blocks, flags=F)
            name, got_slots = self.ctx.last_kernel_name, self.ctx.last_slots
        assert name == self.kernel(False, flags, env), (name, env)
        assert slots is None or got_slots == slots, (name, env, got_slots)
        assert [int(s) for s in status] == [0] * len(blocks), (name, env, list(status))
        for i, (c, w) in enumerate(zip(coded, want)):
            assert c == w, (name, env, "block", i, len(blocks[i]), len(c), len(w))
        assert [int(x) for x in out_len] == [len(w) for w in want], (name, env)
        self.seen.add(name + (" bit-serial" if name == "k_gpipe<encode>" and env.get("ZPQ_GPIPE_BATCH") == "0" else "")
                      + (" vmh" if GM.is_hashchain(self.hdr) else " interpreter"))
        return coded

    def decode(self, coded, blocks, pp, flags=0, slots=None, **env):
        F = flags | self.zpq.FLAG_LANES | (self.zpq.FLAG_PP if pp else 0)
        cap = max(len(b) for b in blocks) + 64
        with knobs(self.mp, **env):
            dec, status, consumed, code, first = self.ctx.decode_blocks(self.model, coded, cap=cap, flags=F)
            name, got_slots = self.ctx.last_kernel_name, self.ctx.last_slots
        assert name == self.kernel(True, flags, env), (name, env)
        assert slots is None or got_slots == slots, (name, env, got_slots)
        assert [int(s) for s in status] == [0] * len(blocks), (name, env, list(status))
        for i in range(len(blocks)):
            assert dec[i] == blocks[i], (name, env, "block", i, len(blocks[i]), len(dec[i]))
        assert [int(c) for c in consumed] == [len(c) for c in coded], (name, env)
        if pp:
            assert all(int(f) == 0 for f in first), (name, env)
        self.seen.add(name + (" bpw" + env["ZPQ_GDEC_BPW"] if "ZPQ_GDEC_BPW" in env else "")
                      + (" vmh" if GM.is_hashchain(self.hdr) else " interpreter"))
        return list(zip([len(d) for d in dec], [int(s) for s in status], [int(c) for c in consumed], [int(c) for c in code],
                        [int(f) for f in first]))

    def small(self, blocks, *more):
        """The blocks up to 4 KiB (k_generic codes a block per lane: larger ones would dominate the test's time)."""
        at = [i for i, b in enumerate(blocks) if len(b) <= 4096]
        return at, [[x[i] for i in at] for x in (blocks,) + more]

    def encoders(self, blocks, want, pp):
        """Every encoder that takes the model: the default; for a model of the wave pipeline its bit-serial stages and the
        lane-per-component kernel; one block per wave besides four; one lane per block."""
        if not self.rt[2]:                               # (more than 64 components: k_generic is the default and the only one)
            _, (sb, sw) = self.small(blocks, want)
            self.encode(sb, sw, pp)
            return want
        coded = self.encode(blocks, want, pp)
        if self.rt[0]:
            self.encode(blocks, want, pp, ZPQ_GPIPE_BATCH="0")
            self.encode(blocks, want, pp, ZPQ_ENC_GPIPE="0")
        if self.rows:
            self.encode(blocks, want, pp, ZPQ_ENC_GPIPE="0", ZPQ_LANES_ROWS="0")
        _, (sb, sw) = self.small(blocks, want)
        self.encode(sb, sw, pp, flags=self.zpq.FLAG_GENERIC)
        return coded

    def decoders(self, coded, blocks, pp):
        """Every decoder; all must return the same out_len, status, consumed, final_code and first_byte per block."""
        at, (sb, sc) = self.small(blocks, coded)
        if not self.rt[2]:
            self.decode(sc, sb, pp)
            return
        res = [self.decode(coded, blocks, pp)]
        if self.rt[1]:
            res.append(self.decode(coded, blocks, pp, ZPQ_GDEC_BPW="16"))
            res.append(self.decode(coded, blocks, pp, ZPQ_GDEC_BPW="32"))
            res.append(self.decode(coded, blocks, pp, ZPQ_DEC_GPIPE="0"))
        if self.rows:
            res.append(self.decode(coded, blocks, pp, ZPQ_DEC_GPIPE="0", ZPQ_LANES_ROWS="0"))
        for r in res[1:]:
            assert r == res[0]
        assert self.decode(sc, sb, pp, flags=self.zpq.FLAG_GENERIC) == [res[0][i] for i in at]

    def slot_reuse(self, blocks, want, pp, slots):
        """A state budget of `slots` slots: a lane / row / wave codes several blocks in turn."""
        L = self.zpq.lib()
        L.zpq_ctx_set_state_budget(self.ctx.h, slots * self.model.state_bytes + 1000)
        try:
            self.encode(blocks, want, pp, slots=slots)
            self.decode(want, blocks, pp, slots=slots)
            if self.rt[0]:
                self.encode(blocks, want, pp, slots=slots, ZPQ_GPIPE_BATCH="0")
                self.encode(blocks, want, pp, slots=slots, ZPQ_ENC_GPIPE="0")
                self.decode(want, blocks, pp, slots=slots, ZPQ_DEC_GPIPE="0")
                self.decode(want, blocks, pp, slots=slots, ZPQ_GDEC_BPW="16")
            if self.rows and slots <= 8:
                self.encode(blocks, want, pp, slots=slots, ZPQ_ENC_GPIPE="0", ZPQ_LANES_ROWS="0")
                self.decode(want, blocks, pp, slots=slots, ZPQ_DEC_GPIPE="0", ZPQ_LANES_ROWS="0")
        finally:
            L.zpq_ctx_set_state_budget(self.ctx.h, BUDGET)

    def wide(self, seed, pp=True):
        """150 small blocks: full workgroups and a second one; then 70 slots for the 150 (a wave pipeline's second
        workgroup partly filled, every lane coding two or three blocks)."""
        blocks = wide_blocks(seed)
        want = O.encode_blocks(self.hdr, blocks, pp=pp, nthreads=8)
        self.decoders(self.encoders(blocks, want, pp), blocks, pp)
        self.slot_reuse(blocks, want, pp, 70)

    def everything(self, seed, big, reuse, wide):
        blocks = general_blocks(seed, big=big)
        want = O.encode_blocks(self.hdr, blocks, nthreads=8)
        self.decoders(self.encoders(blocks, want, True), blocks, True)
        blocks = [b for b in blocks if len(b) < BIG_BLOCK]                 # without the PP byte (and the one long block)
        want = O.encode_blocks(self.hdr, blocks, pp=False, nthreads=8)
        self.decoders(self.encoders(blocks, want, False), blocks, False)
        want = O.encode_blocks(self.hdr, blocks, nthreads=8)
        if reuse and self.rt[2]:
            self.slot_reuse(blocks, want, True, 3 + seed % 3)
        if wide and self.rt[2]:
            self.wide(seed + 7)


def expected_kernels(rt, vmh):
    """What a model's test must have run, from its route: every kernel and instantiation that takes the model."""
    v = " vmh" if vmh else " interpreter"
    if not rt[2]:
        return {"k_generic<encode>" + v, "k_generic<decode>" + v}
    out = {"k_generic<encode>" + v, "k_generic<decode>" + v, "k_lanes<encode>" + v, "k_lanes<decode>" + v}
    if rt[3] == GM.ROWS:
        out |= {"k_rows<encode>" + v, "k_rows<decode>" + v}
    if rt[0]:
        out |= {"k_gpipe<encode>" + v, "k_gpipe<encode> bit-serial" + v}
    if rt[1]:
        out |= {"k_gdec<decode>" + v, "k_gdec<decode> bpw16" + v, "k_gdec<decode> bpw32" + v}
    return out


@pytest.mark.parametrize("name", sorted(GM.NAMED))
def test_named_general_model(zpq, gpu_ctx, monkeypatch, name):
    hdr, route = GM.NAMED[name]
    run = Run(zpq, gpu_ctx, monkeypatch, hdr)
    run.everything(sum(name.encode()), big=True, reuse=True, wide=name in WIDE_NAMED)
    assert run.rt == route                                # (last: a wrong route shows first as a wrong stream)
    assert run.seen == expected_kernels(route, GM.is_hashchain(hdr)), name
    print("\nkernels %s: %s" % (name, sorted(run.seen)))


@pytest.mark.parametrize("index", range(GM.GPU_GEN_COUNT))
def test_generated_general_model(zpq, gpu_ctx, monkeypatch, index):
    hdr = GM.generated(GM.GPU_GEN_SEED, GM.GPU_GEN_COUNT, big=True)[index]
    run = Run(zpq, gpu_ctx, monkeypatch, hdr)
    run.everything(2000 + index, big=index % 2 == 0, reuse=index % 3 == 0, wide=index % 8 == 1)
    assert run.seen == expected_kernels(run.rt, GM.is_hashchain(hdr)), hdr.hex()
    print("\nkernels generated %d (n %d): %s" % (index, hdr[4], sorted(run.seen)))
