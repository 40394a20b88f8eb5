"""The pool's dirty-line logs (ZPQ_DIRTY_LOG_CAP; DBatch::dlog): what test_gpu_dirty_log.py, test_gpu_dirty_log_paths.py and
test_dirty_log_cpu.py share -- the two headers, the data classes, the batches with the oracle's streams (computed once per
batch, never changed) and Run, which holds one sequence of launches on one ctx to the oracle.

Run also reads the logs' counts back (zpq_debug_dlog_counts) after every launch that keeps them, when it does not run the
residue pass (which resets them): per table of every slot that coded a block, count <= cap, count <= 2 * (n + 1 + pp) for
the slot's last block of n bytes (two row write-backs per coded byte: the data, the PP byte, the end-of-segment byte) and
count == 0 behind an empty block without PP byte.  A sequence names the regime it must reach -- "never" (no log overflows),
"always" (every log of a slot that coded a byte overflows), "mixed" (one launch with a table at 0 < count < cap beside a table
at count == cap) -- and Run.finish asserts it from the counts that were read.
"""
import os
import random
import re

import numpy as np
import pytest

import offnominal_corpus as OC
import oracle_lib as O

WORDS = [b"the", b"of", b"block", b"line", b"table", b"state", b"and", b"zero", b"log", b"clear", b"count", b"a", b"in", b"row"]
DEFAULT_CAP, MAX_CAP = 16384, 1 << 20
BUDGET, MAX_BLOCK = 150 << 30, 65536                      # the session context's defaults
CLEAN = ("zeros", "periodic")                             # data whose stream shows a stale table line: its contexts repeat
SHORT = 24                                                # a block of at most 24 bytes cannot reach 64 write-backs: 2 * (24 + 2) = 52


def small_table_header(bits):
    """Level 2's header with every hash table shrunk to 64 << bits bytes: a block's contexts alias in a few lines."""
    h = bytearray(O.level_header(2))
    sz = [0, 2, 3, 2, 3, 4, 6, 6, 3, 5]
    p = 5
    for _ in range(h[4]):
        if h[p] in (3, 8):
            h[p + 1] = bits
        p += sz[h[p]]
    return bytes(h)


HEADERS = {"level2": O.level_header(2), "small": small_table_header(4)}


def make(kind, seed, n):
    rnd = random.Random(seed)
    if kind == "uniform":
        return bytes(rnd.getrandbits(8) for _ in range(n))
    if kind == "zeros":
        return bytes(n)
    if kind == "text":
        out = bytearray()
        while len(out) < n:
            out += rnd.choice(WORDS) + b" "
        return bytes(out[:n])
    p = 19 + seed % 50                                    # periodic
    unit = bytes(rnd.getrandbits(8) for _ in range(p))
    return (unit * (n // p + 1))[:n]


def batch(kind, nb, seed):
    """nb ragged blocks of 1-8 KiB (and an empty and a one-byte one where there is room for them)."""
    rnd = random.Random(1000 * seed + nb)
    lens = [rnd.choice([1024, 1025, 1531, 2048, 3000, 4099, 6000, 8192]) for _ in range(nb)]
    if nb >= 16:
        lens[3], lens[7] = 0, 1
    return [make(kind, 100 * seed + i, n) for i, n in enumerate(lens)]


# ---------------------------------------------------------------- batches whose blocks differ in class: (kind, length) per block
CYCLE = ("uniform", "zeros", "uniform", "periodic")


def round_plan(nb, seed, shift=0):
    """[(kind, n)] of a batch for launches on fewer slots than blocks, blocks of 0 .. 2048 bytes.  The classes alternate with the
    index (shift: and move on by one every `shift` blocks, for an even slot count), so that a slot codes zeros or periodic data
    right behind uniform data; an empty and a one-byte block in the second and third round; and the last five blocks -- the
    last ones of their slots on any slot count of at least five -- are 24 bytes of text, 2 KiB uniform, nothing, 2 KiB
    uniform and one byte."""
    rnd = random.Random(7000 * seed + nb)
    plan = []
    for i in range(nb):
        kind = CYCLE[(i + (i // shift if shift else 0)) % 4]
        plan.append((kind, 2048 if kind == "uniform" and i % 3 else rnd.choice([300, 777, 1200, 1531, 2048])))
    if nb > 40:
        plan[22] = (plan[22][0], 0)
        plan[29] = (plan[29][0], 1)
        plan[41] = ("text", 5)
    plan[nb - 5:] = [("text", SHORT), ("uniform", 2048), ("zeros", 0), ("uniform", 2048), ("periodic", 1)]
    return plan


def mixed_plan(nb, seed):
    """[(kind, n)] of a batch for one launch at full residency that must reach the "mixed" regime at capacity 64: 2 KiB
    uniform blocks beside blocks of at most 24 bytes, an empty one and a one-byte one among them."""
    rnd = random.Random(9000 * seed + nb)
    plan = [("uniform", 2048) if i % 2 == 0 else (rnd.choice(("text", "zeros", "periodic")), rnd.choice([2, 5, 11, 17, SHORT]))
            for i in range(nb)]
    plan[1], plan[5] = ("zeros", 0), ("text", 1)
    return plan


def plan_blocks(plan, seed):
    return [make(kind, 100 * seed + i, n) for i, (kind, n) in enumerate(plan)]


def last_of_slot(nb, nslots):
    """index of the last block each slot codes in a launch of nb blocks on nslots slots (slot s codes s, s + nslots, ...)"""
    return [s + (nb - 1 - s) // nslots * nslots for s in range(min(nb, nslots))]


def clean_behind_dirty(plan, nslots):
    """the blocks i + nslots of zeros or periodic data that a slot codes directly behind a uniform block i"""
    return [i + nslots for i in range(len(plan) - nslots)
            if plan[i][0] == "uniform" and plan[i][1] >= 1024 and plan[i + nslots][0] in CLEAN and plan[i + nslots][1] >= 256]


def write_back_bound(n, pp):
    return 2 * (n + 1 + (1 if pp else 0))


def parse_cap(env):
    """ZPQ_DIRTY_LOG_CAP as the library reads it: unset or empty = the default, no number or none above zero = off, clamped."""
    if env is None or env == "":
        return DEFAULT_CAP
    m = re.match(r"\s*([+-]?\d+)", env)
    v = int(m.group(1)) if m else 0
    return 0 if v <= 0 else min(v, MAX_CAP)


_want = {}


def oracle(name, kind, nb, seed, pp):
    """(blocks, the oracle's streams) of batch(kind, nb, seed), or of a plan: kind = "rounds" / "rounds16" / "mixed" / "uniform2k"."""
    key = (name, kind, nb, seed, pp)
    if key not in _want:
        blocks = blocks_of(kind, nb, seed)
        _want[key] = (blocks, O.encode_blocks(HEADERS[name], blocks, pp=pp, nthreads=8))
    return _want[key]


def plan_of(kind, nb, seed):
    if kind == "rounds":
        return round_plan(nb, seed)
    if kind == "rounds16":
        return round_plan(nb, seed, shift=16)
    if kind == "mixed":
        return mixed_plan(nb, seed)
    if kind == "uniform2k":                               # (what every kernel takes, a forced line store of 8192 lines included)
        rnd = random.Random(3000 * seed + nb)
        return [("uniform", rnd.choice([1024, 1531, 2047, 2048])) for _ in range(nb)]
    return None


def blocks_of(kind, nb, seed):
    plan = plan_of(kind, nb, seed)
    return batch(kind, nb, seed) if plan is None else plan_blocks(plan, seed)


def _offsets(lengths, first=0):
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[0] = first
    off[1:] = first + np.cumsum(np.asarray(lengths, dtype=np.uint64))
    return off


_DAMAGED = {}


def damaged_batch(pp, slab):
    """39 members, every third one a damaged stream of offnominal_corpus (level 2): truncated at several points, bits flipped,
    an empty coded stream; the others 2 KiB uniform blocks' streams.  With offnominal_corpus.expected per member."""
    key = (pp, slab)
    if key not in _DAMAGED:
        pool = [c for c in OC.cases("level2", pp) if c.kind in ("trunc", "flip") and c.what.split()[0] in ("random1500", "text1500", "random300")]
        picked = [c for c in pool if c.what.split()[1] in ("trunc-1", "trunc-5", "trunc/2", "trunc:3", "trunc:0", "flip-first", "flip-mid", "flip-last")]
        assert len(picked) >= 13 and any(not c.stream for c in picked)
        blocks, streams = oracle("level2", "uniform2k", 26, 9, pp)
        batch, good = [], 0
        for i in range(39):
            if i % 3 == 1:
                batch.append(picked[(i // 3) % len(picked)])
            else:
                batch.append(OC.Case("exact", "uniform block %d" % good, streams[good], len(blocks[good])))
                good += 1
        caps = [slab] * 39
        _DAMAGED[key] = (batch, caps, OC.expectations("level2", pp, batch, caps))
    return _DAMAGED[key]


SENTINEL = 0xA5


def dev_call(ctx, model, decode, streams, caps, flags):
    """zpq_encode_blocks_dev / zpq_decode_blocks_dev on a sentinel-filled output tensor whose windows begin at an odd offset.
    Returns (stored bytes per block, out_len, status); the rest of every window must still hold the sentinel."""
    import torch
    dev = torch.device("cuda:0")
    nb = len(streams)
    d_in = torch.from_numpy(np.frombuffer(b"".join(streams) + b"\xee" * 64, dtype=np.uint8).copy()).to(dev)
    in_off = torch.from_numpy(_offsets([len(s) for s in streams]).astype(np.int64)).to(dev)
    out_off_h = _offsets(caps, first=37)
    out_off = torch.from_numpy(out_off_h.astype(np.int64)).to(dev)
    d_out = torch.full((int(out_off_h[-1]) + 64,), SENTINEL, dtype=torch.uint8, device=dev)
    meta = [torch.full((nb,), -99, dtype=torch.int32, device=dev) for _ in range(5)]
    torch.cuda.synchronize()                               # order torch's fills before the ctx stream's kernels
    if decode:
        ctx.decode_blocks_dev(model, nb, d_in.data_ptr(), in_off.data_ptr(), flags, d_out.data_ptr(), out_off.data_ptr(),
                              *[m.data_ptr() for m in meta])
    else:
        ctx.encode_blocks_dev(model, nb, d_in.data_ptr(), in_off.data_ptr(), flags, d_out.data_ptr(), out_off.data_ptr(),
                              meta[0].data_ptr(), meta[4].data_ptr())
    ctx.sync()
    out = d_out.cpu().numpy()
    out_len, status = meta[0].cpu().numpy().view(np.uint32), meta[4].cpu().numpy()
    res = []
    image = np.full(len(out), SENTINEL, dtype=np.uint8)
    for i in range(nb):
        o, k = int(out_off_h[i]), min(int(out_len[i]), caps[i])
        res.append(out[o:o + k].tobytes())
        image[o:o + k] = out[o:o + k]
    assert (out == image).all(), "a byte outside the stored bytes of a window was written"
    return res, out_len, status


class Run:
    """One sequence of launches of one model on one ctx.  slots: the slot count every launch must run on (None: a slot per
    block); via: "host" or "dev", the entry points; regime: what finish() must find in the counts."""

    def __init__(self, zpq, ctx, name, cap_env, residue, slots=None, via="host", regime=None, model=None):
        self.zpq, self.ctx, self.name, self.residue = zpq, ctx, name, residue
        self.model = model if model is not None else zpq.Model(header=HEADERS[name])
        self.cap_env = cap_env                            # (the variable itself is read per launch, as the library reads it)
        self.slots, self.via, self.regime = slots, via, regime
        self.launches = []                                # per log-keeping launch: [(count, n, pp)] of every table of every slot that coded

    @property
    def cap(self):
        return parse_cap(os.environ.get("ZPQ_DIRTY_LOG_CAP"))

    @property
    def on(self):
        return self.cap != 0

    def resident(self, nb):
        return min(nb, self.slots) if self.slots else nb

    def after(self, keeps, coded=None, nslots=None):
        """keeps: the launch was one of the two kernels that keep the log; coded: [(n, pp)] of the launch's blocks, n an upper
        bound of the bytes each coded; nslots: the slots the call ran on where its last launch ran on fewer"""
        n = nslots if nslots is not None else self.ctx.last_slots
        if coded is not None and nslots is None:
            assert n == self.resident(len(coded)), (n, len(coded), self.slots)
        if self.residue:
            if keeps and self.on:
                assert self.ctx.debug_pool_residue(n) == 0
            else:
                with pytest.raises(self.zpq.ZpqError):       # any other launch leaves no valid log
                    self.ctx.debug_pool_residue(n)
            return
        if not hasattr(self.zpq.lib(), "zpq_debug_dlog_counts"):
            return
        if not (keeps and self.on):
            with pytest.raises(self.zpq.ZpqError):
                self.ctx.debug_dlog_counts(n)
            return
        counts = self.ctx.debug_dlog_counts(n)
        if coded is None:
            return
        rec = []
        for s, i in enumerate(last_of_slot(len(coded), n)):
            nbytes, pp = coded[i]
            for t in range(3):
                c = int(counts[s, t])
                assert c <= self.cap, ("count beyond the capacity", s, t, c, self.cap)
                if self.name == "level2":
                    assert c <= write_back_bound(nbytes, pp), ("more entries than row write-backs", s, t, c, nbytes, pp)
                    if nbytes == 0 and not pp:
                        assert c == 0, ("an empty block logged a line", s, t, c)
                rec.append((c, nbytes, pp))
        self.launches.append(rec)

    def finish(self):
        """the regime, from the counts read back (level 2's header only: on 16-line tables whether a log of 64 overflows
        depends on which victims are logged again)"""
        if self.residue or self.regime is None or self.name != "level2" or not hasattr(self.zpq.lib(), "zpq_debug_dlog_counts"):
            return
        assert self.launches, "no log-keeping launch was read"
        cap = self.cap
        if self.regime == "never":
            # (where the bound on write-backs is below the capacity: every block of up to 8000 bytes at the default)
            sure = [c for rec in self.launches for c, n, pp in rec if write_back_bound(n, pp) < cap]
            assert sure and all(c < cap for c in sure) and any(c > 0 for c in sure)
        elif self.regime == "always":
            assert all(c == cap for rec in self.launches for c, n, pp in rec if n + pp >= 1)
            assert any(n + pp >= 1 for rec in self.launches for _, n, pp in rec)
        else:
            assert self.regime == "mixed"
            assert any(any(0 < c < cap for c, _, _ in rec) and any(c == cap for c, _, _ in rec) for rec in self.launches), \
                [(min(c for c, _, _ in rec), max(c for c, _, _ in rec)) for rec in self.launches]

    def enc_name(self, nb):
        return "k_pipe<encode>" if self.resident(nb) >= 12 else "k_chain<encode>"

    def enc(self, kind, nb, seed, pp=True, cap=None):
        blocks, want = oracle(self.name, kind, nb, seed, pp)
        flags = self.zpq.FLAG_PP if pp else 0
        if self.via == "dev":
            caps = [(cap if cap is not None else len(w) + 5 + 13 * (i % 7)) for i, w in enumerate(want)]
            coded, _, status = dev_call(self.ctx, self.model, False, blocks, caps, flags)
        else:
            coded, status, _ = self.ctx.encode_blocks(self.model, blocks, flags=flags, cap=cap)
        assert self.ctx.last_kernel_name == self.enc_name(nb)
        self.after(self.resident(nb) >= 12, [(len(b), pp) for b in blocks])
        if cap is None:
            assert (status == 0).all() and coded == want, (kind, nb)
        else:
            fits = [len(w) <= cap for w in want]
            assert [s == 0 for s in status] == fits and not all(fits)
            assert all(c == w for c, w, f in zip(coded, want, fits) if f)

    def dec(self, kind, nb, seed, pp=True, cap=8200):
        blocks, want = oracle(self.name, kind, nb, seed, pp)
        flags = self.zpq.FLAG_PP if pp else 0
        if self.via == "dev":
            back, _, status = dev_call(self.ctx, self.model, True, want, [cap + 3 * (i % 5) if len(b) <= cap else cap
                                                                         for i, b in enumerate(blocks)], flags)
        else:
            back, status, *_ = self.ctx.decode_blocks(self.model, want, cap=cap, flags=flags)
        assert self.ctx.last_kernel_name == "k_chain<decode>"
        self.after(True, [(min(len(b), cap + 1), pp) for b in blocks])
        fits = [len(b) <= cap for b in blocks]
        assert [s == 0 for s in status] == fits
        assert all(b == w for b, w, f in zip(back, blocks, fits) if f), (kind, nb)

    def both(self, kind, nb, seed, pp=True):
        self.enc(kind, nb, seed, pp)
        self.dec(kind, nb, seed, pp)

    def other(self, level):
        """a launch of another model on the pool: it keeps no log"""
        m = self.zpq.Model(level=level)
        blocks = batch("text", 16, level)
        coded, status, _ = self.ctx.encode_blocks(m, blocks)
        assert (status == 0).all()
        self.after(False)
        back, status, *_ = self.ctx.decode_blocks(m, coded, cap=8200)
        assert (status == 0).all() and back == blocks
        self.after(False)
        m.close()

    def blockset(self):
        """a block set of the same model codes a segment per member between two pool launches"""
        bs = self.zpq.BlockSet(self.ctx, self.model, 12)
        segs = batch("uniform", 12, 77)
        coded, status, _ = bs.encode_segments(segs)
        assert (status == 0).all()
        bs.close()
