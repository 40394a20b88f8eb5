"""The pool's dirty-line logs (ZPQ_DIRTY_LOG_CAP; DBatch::dlog): level 2's k_pipe<encode> and two-hypothesis k_chain<decode>
note the 64-byte table lines a launch made non-zero, and the next launch of theirs on the pool zeroes those lines instead
of every slot.  A line that was dirtied and not logged, or logged and not cleared, is stale state under the next block: the
sequences below put a block whose result depends on clean tables behind one that dirtied them, on one ctx, and compare every
launch with the C oracle stream for stream.  Each sequence runs twice per log capacity: once as it is (the kernels' own
clear), once with zpq_debug_pool_residue after every launch that keeps the log (it must find nothing left)."""
import random

import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

WORDS = [b"the", b"of", b"block", b"line", b"table", b"state", b"and", b"zero", b"log", b"clear", b"count", b"a", b"in", b"row"]


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


_want = {}


def oracle(name, kind, nb, seed, pp):
    key = (name, kind, nb, seed, pp)
    if key not in _want:
        blocks = batch(kind, nb, seed)
        _want[key] = (blocks, O.encode_blocks(HEADERS[name], blocks, pp=pp, nthreads=8))
    return _want[key]


class Run:
    def __init__(self, zpq, ctx, name, cap_env, residue):
        self.zpq, self.ctx, self.name, self.residue = zpq, ctx, name, residue
        self.model = zpq.Model(header=HEADERS[name])
        self.on = cap_env != "0"

    def after(self, keeps):
        """keeps: the launch was one of the two kernels that keep the log"""
        if not self.residue:
            return
        n = self.ctx.last_slots
        if keeps and self.on:
            assert self.ctx.debug_pool_residue(n) == 0
        else:
            with pytest.raises(self.zpq.ZpqError):       # any other launch leaves no valid log
                self.ctx.debug_pool_residue(n)

    def enc(self, kind, nb, seed, pp=True, cap=None):
        blocks, want = oracle(self.name, kind, nb, seed, pp)
        coded, status, _ = self.ctx.encode_blocks(self.model, blocks, flags=self.zpq.FLAG_PP if pp else 0, cap=cap)
        assert self.ctx.last_kernel_name == ("k_pipe<encode>" if nb >= 12 else "k_chain<encode>")
        self.after(nb >= 12)
        if cap is None:
            assert (status == 0).all() and coded == want, (kind, nb)
        else:
            fits = [len(w) <= cap for w in want]
            assert [s == 0 for s in status] == fits and not all(fits)
            assert all(c == w for c, w, f in zip(coded, want, fits) if f)

    def dec(self, kind, nb, seed, pp=True, cap=8200):
        blocks, want = oracle(self.name, kind, nb, seed, pp)
        back, status, *_ = self.ctx.decode_blocks(self.model, want, cap=cap, flags=self.zpq.FLAG_PP if pp else 0)
        assert self.ctx.last_kernel_name == "k_chain<decode>"
        self.after(True)
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


def seq_classes(r):
    for i, kind in enumerate(("uniform", "zeros", "text", "uniform")):
        r.both(kind, 40 if i % 2 == 0 else 16, i, pp=i != 2)


def seq_decode_only(r):
    for i, kind in enumerate(("uniform", "zeros", "text", "periodic", "uniform", "zeros")):
        r.dec(kind, 16 if i == 3 else 40, i, pp=i != 1)


def seq_slot_counts(r):
    r.both("uniform", 40, 0)
    r.both("text", 16, 2, pp=False)
    r.both("zeros", 40, 1)                                # slots 16 .. 39 still hold the first launch's lines
    r.enc("uniform", 11, 5)                               # below twelve blocks the encoder is k_chain<encode>: no log
    r.both("zeros", 40, 1)
    r.dec("uniform", 11, 5)
    r.both("periodic", 16, 3)
    r.both("zeros", 40, 1)


def seq_other_launches(r):
    r.both("uniform", 40, 0)
    r.other(1)
    r.both("zeros", 40, 1)
    r.both("uniform", 16, 4, pp=False)
    r.other(3)
    r.both("text", 40, 2)
    r.blockset()
    r.both("zeros", 40, 1)


def seq_error_status(r):
    r.both("uniform", 40, 0)
    r.enc("uniform", 40, 0, cap=2100)                     # the larger blocks' coded streams do not fit: status per block
    r.both("zeros", 40, 1)
    r.dec("uniform", 40, 0, cap=2100)                     # ... and the larger blocks do not fit the decoder's slab
    r.both("zeros", 40, 1)
    r.both("text", 16, 2)


SEQUENCES = {"classes": seq_classes, "decode_only": seq_decode_only, "slot_counts": seq_slot_counts,
             "other_launches": seq_other_launches, "error_status": seq_error_status}


@pytest.mark.parametrize("cap_env", [None, "8", "64"])      # the default; every table overflows; some do and some do not
@pytest.mark.parametrize("name", ["level2", "small"])
@pytest.mark.parametrize("seq", sorted(SEQUENCES))
def test_sequences_against_the_oracle(zpq, gpu_ctx, monkeypatch, seq, name, cap_env):
    for v in ("ZPQ_ENC_PIPE", "ZPQ_ENC_SPLIT", "ZPQ_DEC_PIPE", "ZPQ_SPARSE_MODE", "ZPQ_SPARSE_FORCE_LOG2"):
        monkeypatch.delenv(v, raising=False)
    if cap_env is None:
        monkeypatch.delenv("ZPQ_DIRTY_LOG_CAP", raising=False)
    else:
        monkeypatch.setenv("ZPQ_DIRTY_LOG_CAP", cap_env)
    for residue in (False, True):
        r = Run(zpq, gpu_ctx, name, cap_env, residue)
        SEQUENCES[seq](r)
        r.model.close()


def test_cap_zero_switches_the_mechanism_off(zpq, gpu_ctx, monkeypatch):
    monkeypatch.setenv("ZPQ_DIRTY_LOG_CAP", "0")
    r = Run(zpq, gpu_ctx, "small", "0", True)
    seq_classes(r)
    r.model.close()


def test_cap_changes_between_launches(zpq, gpu_ctx, monkeypatch):
    """The capacity is read per call: logs kept at one capacity are not read at another."""
    r = Run(zpq, gpu_ctx, "small", None, False)
    for i, cap in enumerate(("64", "8", None, "0", "16384", "64")):
        if cap is None:
            monkeypatch.delenv("ZPQ_DIRTY_LOG_CAP", raising=False)
        else:
            monkeypatch.setenv("ZPQ_DIRTY_LOG_CAP", cap)
        r.both("uniform" if i % 2 == 0 else "zeros", 40, i % 2)
    r.model.close()
