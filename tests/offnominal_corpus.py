"""Truncated and damaged coded streams for every decoder, with what the CPU oracle makes of each of them.

A decoder in use gets a window that may run past its stream, a stream that lost its tail or holds a flipped bit, and an
output slab that is a guess.  The corpus holds small originals coded by the oracle, mutations of every coded stream and
plain junk; layout() puts them back to back in one input buffer the way a batch call sees them (nonzero neighbours on
both sides of every block, truncated streams ending at every residue mod 4 and starting at every residue mod 16) and
expected() gives status, out_len, the stored bytes, consumed, final_code and first_byte of every block for any slab
size from Codec.decode_prefix -- the oracle's decode stopped where the kernels stop (EOF, or right after byte cap + 1).
The tests: test_offnominal_cpu.py pins the corpus, test_gpu_offnominal.py holds the kernels to it.
"""
import collections
import random

import general_models as GM
import oracle_lib as O
from test_gpu_chain_models import _block

SIZES = (0, 1, 2, 17, 64, 300, 1500)
KINDS = ((0, "zeros"), (2, "text"), (1, "random"), (3, "periodic"))        # (_block's kind, name)
MUTATIONS = ("exact", "trail", "trunc", "flip", "junk")
CHAIN_LEVELS = (1, 2, 3, 4, 5)
# general models and the decoders they reach: the wave pipeline and k_rows (the first two), k_rows only, k_lanes only,
# k_lanes with the interpreter, k_generic only
GENERAL = ("cm_alias", "match_idx_gt_buf", "mix9", "n17", "mix3_sse3_n22_vm", "n65")
SMALL_ONLY = ("n17", "mix3_sse3_n22_vm", "n65")                            # beyond 16 components: originals of at most 300 bytes
MODELS = tuple("level%d" % i for i in CHAIN_LEVELS) + GENERAL
PROBE_CAP = 4032                                                           # (roomy slabs stay within 4 KiB)
NO_BYTE = 0xFFFFFFFF

# kind: one of MUTATIONS, or "filler"; what: how the stream was made; nominal: the original's length (junk and fillers:
# the stream's own), the size of the tight slab
Case = collections.namedtuple("Case", "kind what stream nominal")


def header_of(model):
    return O.level_header(int(model[5:])) if model.startswith("level") else GM.NAMED[model][0]


def originals(model):
    sizes = [n for n in SIZES if n <= 300 or model not in SMALL_ONLY]
    r = random.Random(4711)
    return [("%s%d" % (name, n), _block(r, kind, n)) for n in sizes for kind, name in KINDS]


def mutations(s, r):
    """(kind, label, stream) of one coded stream: itself, with junk behind it, cut short, with one bit flipped."""
    out = [("exact", "exact", s)]
    out += [("trail", "trail+%d" % k, s + bytes(r.randrange(1, 256) for _ in range(k))) for k in (1, 3, 9)]
    out += [("trunc", "trunc-%d" % k, s[:-k]) for k in (1, 4, 5, 8)]
    out += [("trunc", "trunc/2", s[:len(s) // 2]), ("trunc", "trunc:3", s[:3]), ("trunc", "trunc:1", s[:1]), ("trunc", "trunc:0", b"")]
    for label, at in (("first", 0), ("mid", len(s) // 2), ("last", len(s) - 1)):
        t = bytearray(s)
        t[at] ^= 1 << r.randrange(8)
        out.append(("flip", "flip-" + label, bytes(t)))
    return out


_CASES = {}


def cases(model, pp):
    """Every case of one model, coded with or without the PP byte (a decode call takes one flag for all its blocks)."""
    key = (model, pp)
    if key not in _CASES:
        r = random.Random(99)
        hdr = header_of(model)
        out = []
        for name, data in originals(model):
            s = O.Codec(hdr).encode(data, pp=pp)
            out += [Case(kind, name + " " + label, t, len(data)) for kind, label, t in mutations(s, r)]
        for n in (1, 4, 5, 64, 1000):
            out.append(Case("junk", "random%d" % n, bytes(r.getrandbits(8) for _ in range(n)), n))
            out.append(Case("junk", "00x%d" % n, bytes(n), n))
            out.append(Case("junk", "ffx%d" % n, b"\xff" * n, n))
        _CASES[key] = out
    return _CASES[key]


FILLERS = (b"\xa7", b"\x5b\xc3")


def layout(model, pp, seed=7):
    """The cases in the order of one batch: shuffled, so that damaged and good streams alternate on every lane, with a
    one- or two-byte filler block (junk of its own right) wherever a block begins or ends with a zero byte -- every block
    but the fillers then has nonzero bytes on both sides -- and at both ends of the batch."""
    order = list(cases(model, pp))
    random.Random(seed).shuffle(order)
    out, nf = [], 0

    def filler():
        nonlocal nf
        f = FILLERS[nf % 2]
        nf += 1
        out.append(Case("filler", "filler%d" % len(f), f, len(f)))

    filler()
    for c in order:
        if c.stream and c.stream[0] == 0 and out[-1].kind != "filler":
            filler()
        out.append(c)
        if c.stream and c.stream[-1] == 0:
            filler()
    if out[-1].kind != "filler":
        filler()
    return out


def offsets(batch):
    off = [0]
    for c in batch:
        off.append(off[-1] + len(c.stream))
    return off


_SEEN = {}


def prefix(model, stream, cap):
    """Codec.decode_prefix on a fresh model, remembered: a decode that ended by EOF within `cap` bytes is the answer for
    every slab of at least that many bytes."""
    known = _SEEN.setdefault((model, stream), [])
    for kcap, res in known:
        if kcap == cap or (kcap > cap and res[1] <= cap):
            return res
    res = O.Codec(header_of(model)).decode_prefix(stream, cap)
    known.append((cap, res))
    return res


Expected = collections.namedtuple("Expected", "status out_len data consumed final_code first_byte")


def shape(res, cap, pp):
    """Codec.decode_prefix's answer for cap + pp bytes as what a decoder returns for a slab of `cap` bytes.  With the PP
    flag the first decoded byte goes to first_byte and is neither stored nor counted, so the decode stops after byte
    cap + 2 of the stream's."""
    data, n, consumed, code, vm = res
    first = NO_BYTE
    if pp and n:
        first, data, n = data[0], data[1:], n - 1
    status = -8 if vm else -7 if n > cap else 0
    return Expected(status, n, data[:min(n, cap)], consumed, code, first)


def expected(model, pp, stream, cap):
    """What a decoder must return for one block of a fresh model with a slab of `cap` bytes."""
    return shape(prefix(model, stream, cap + (1 if pp else 0)), cap, pp)


def roomy_cap(model, pp, batch):
    """The largest out_len of the batch that ends by EOF within PROBE_CAP bytes, plus 64."""
    ends = expectations(model, pp, batch, [PROBE_CAP] * len(batch))
    return max(e.out_len for e in ends if e.status == 0) + 64


def slabs(model, pp, batch, which):
    """Per-block slab sizes: "roomy" (one size for all), "tight" (the original's length: the exact stream fits with not a
    byte to spare), "tight-1" (one byte less, and one block of 64 bytes gets no slab at all)."""
    if which == "roomy":
        return [roomy_cap(model, pp, batch)] * len(batch)
    if which == "tight":
        return [c.nominal for c in batch]
    assert which == "tight-1"
    caps = [max(c.nominal - 1, 0) for c in batch]
    caps[[i for i, c in enumerate(batch) if c.kind == "exact" and c.nominal == 64][0]] = 0
    return caps


def expectations(model, pp, batch, caps):
    """expected() of every block.  (One after the other: what a decode on a model with large tables costs is the page
    faults of its first touches, and those do not run side by side.)"""
    return [expected(model, pp, c.stream, cap) for c, cap in zip(batch, caps)]
