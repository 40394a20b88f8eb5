"""Damaged segments for the block sets: members of three rounds, with what the CPU oracle makes of every round.

A set hands each member's model state from launch to launch.  A member here decodes a good warm-up segment (round 0), a
damaged one (round 1: every mutation of offnominal_corpus.py, or plain junk) and a good follow-on segment (round 2) coded
on the state the UNDAMAGED round 1 left.  A decoder that survives round 1 (status 0) must leave in the member's slot the
state of the byte boundary where it stopped, wherever the damage moved its end; only round 2 shows whether it did.
expectations() follows every member with a codec of its own through Codec.decode_prefix (the kernels' stop rule), a member
whose round ends with another status than 0 has failed and reports that status without coding from then on.
The tests: test_offnominal_sets_cpu.py pins the corpus and shows that it tells a wrong kept state,
test_gpu_offnominal_sets.py holds the kernels to it.
"""
import collections
import random

import chain_models as CM
import general_models as GM
import offnominal_corpus as OC
import oracle_lib as O
from test_gpu_chain_models import _block

SIZES = (0, 1, 2, 17, 64, 300)
WARM_SIZES, NEXT_SIZES = (17, 64, 300, 1), (64, 17, 120, 2)
ROOMY = 4032
ROUNDS = 3
POLICIES = ("roomy", "tight", "tight-1")
CHAIN_EXTRA = ("chain7", "chain16")                    # the unspecialised chains at 8 and 16 lanes per block
STATEFUL = (OC.MODELS[:5] + CHAIN_EXTRA + ("cm_alias", "match_idx_gt_buf", "mix_x4", "mix9", "hm0", "n17", "mix3_sse3_n22_vm", "n65"))
STATELESS = ("bits0_all", "perturbed_rows")            # their streams do not depend on the kept state: of no use here

# kind, what: as offnominal_corpus.Case; streams: what the decoder is fed in rounds 0, 1, 2; nominal: the length of round
# 1's original (junk and fillers: of the stream), the tight slab; clean: round 1's undamaged stream (junk, fillers: their own)
# data: round 1's original
Member = collections.namedtuple("Member", "kind what streams nominal clean data")


def header_of(model):
    return CM.NAMED[model][0] if model in CHAIN_EXTRA else OC.header_of(model)


def as_case(m, rnd=1):
    """A member's round as an offnominal_corpus.Case (what check_decode names in its messages)."""
    return OC.Case(m.kind, "%s round %d" % (m.what, rnd), m.streams[rnd], m.nominal)


_MEMBERS = {}


def members(model, pp):
    """The mutated members (15 per original, 24 originals), then 15 of junk."""
    key = (model, pp)
    if key not in _MEMBERS:
        hdr = header_of(model)
        r, rm = random.Random(4711), random.Random(99)
        out, i = [], 0
        for n in SIZES:
            for kind, name in OC.KINDS:
                data = _block(r, kind, n)
                warm = _block(r, (kind + 1) % 4, WARM_SIZES[i % 4])
                nxt = _block(r, (kind + 2) % 4, NEXT_SIZES[i % 4])
                enc = O.Codec(hdr)
                cw, s, c2 = enc.encode(warm, pp=pp), enc.encode(data, pp=pp), enc.encode(nxt, pp=pp)
                del enc
                out += [Member(mk, "%s%d %s" % (name, n, label), (cw, t, c2), n, s, data) for mk, label, t in OC.mutations(s, rm)]
                i += 1
        junk = [c for c in OC.cases(model if model not in CHAIN_EXTRA else "level2", pp) if c.kind == "junk" and " " not in c.what]
        assert len(junk) == 15
        for c in junk:                                    # (junk is junk for any model: level 2's list serves the extra chains)
            enc = O.Codec(hdr)
            cw = enc.encode(_block(r, 2, WARM_SIZES[i % 4]), pp=pp)
            c2 = enc.encode(_block(r, 2, NEXT_SIZES[i % 4]), pp=pp)
            del enc
            out.append(Member("junk", c.what, (cw, c.stream, c2), c.nominal, c.stream, b""))
            i += 1
        _MEMBERS[key] = out
    return _MEMBERS[key]


_LAYOUT = {}


def layout(model, pp, seed=7):
    """The members in the order of every call (all three rounds use it): shuffled once, with a one- or two-byte filler
    member (a good warm-up, junk of its own right in round 1) wherever a round-1 stream begins or ends with a zero byte
    and at both ends, as offnominal_corpus.layout does it for a batch."""
    key = (model, pp, seed)
    if key in _LAYOUT:
        return _LAYOUT[key]
    order = list(members(model, pp))
    random.Random(seed).shuffle(order)
    hdr = header_of(model)
    enc = O.Codec(hdr)
    cw = enc.encode(b"filler\n", pp=pp)
    c2 = enc.encode(b"on\n", pp=pp)
    del enc
    out, nf = [], 0

    def filler():
        nonlocal nf
        f = OC.FILLERS[nf % 2]
        nf += 1
        out.append(Member("filler", "filler%d" % len(f), (cw, f, c2), len(f), f, b""))

    filler()
    for m in order:
        s = m.streams[1]
        if s and s[0] == 0 and out[-1].kind != "filler":
            filler()
        out.append(m)
        if s and s[-1] == 0:
            filler()
    if out[-1].kind != "filler":
        filler()
    _LAYOUT[key] = out
    return out


def offsets(batch, rnd=1):
    off = [0]
    for m in batch:
        off.append(off[-1] + len(m.streams[rnd]))
    return off


def slabs(batch, which):
    """Round 1's slab of every member: "roomy" (4032), "tight" (the original's length), "tight-1" (one byte less, and one
    exact member of 64 bytes gets no slab at all).  Rounds 0 and 2 are always roomy."""
    if which == "roomy":
        return [ROOMY] * len(batch)
    if which == "tight":
        return [m.nominal for m in batch]
    assert which == "tight-1"
    caps = [max(m.nominal - 1, 0) for m in batch]
    caps[[i for i, m in enumerate(batch) if m.kind == "exact" and m.nominal == 64][0]] = 0
    return caps


def caps_of(batch, which):
    """The slabs of rounds 0, 1, 2."""
    return [[ROOMY] * len(batch), slabs(batch, which), [ROOMY] * len(batch)]


def follow(hdr, streams, caps, pp):
    """One member through its rounds on a codec of its own: [Expected] per round, a failed member reporting its status
    without coding."""
    dec = O.Codec(hdr)
    out, failed = [], 0
    for s, cap in zip(streams, caps):
        if failed:
            out.append(OC.Expected(failed, 0, b"", 0, 0, OC.NO_BYTE))
            continue
        e = OC.shape(dec.decode_prefix(s, cap + (1 if pp else 0)), cap, pp)
        failed = e.status
        out.append(e)
    del dec                                               # (before the next member's: level 5's tables do not fit 400 times)
    return out


_EXPECT = {}


def expectations(model, pp, which, undamaged=False):
    """want[round][member] for layout(model, pp) under a slab policy, one member after the other.  undamaged: round 1 is fed
    the stream as it was before the damage -- what a kernel that kept the wrong state would go on from."""
    key = (model, pp, which, undamaged)
    if key not in _EXPECT:
        batch, hdr = layout(model, pp), header_of(model)
        caps = caps_of(batch, which)
        per = [follow(hdr, (m.streams[0], m.clean if undamaged else m.streams[1], m.streams[2]), [c[i] for c in caps], pp)
               for i, m in enumerate(batch)]
        _EXPECT[key] = [[p[r] for p in per] for r in range(ROUNDS)]
    return _EXPECT[key]


def fresh_round2(model, pp):
    """Round 2 of every member of the layout on a FRESH model: what a decoder that kept nothing returns."""
    key = (model, pp, "fresh")
    if key not in _EXPECT:
        hdr = header_of(model)
        _EXPECT[key] = [follow(hdr, (m.streams[2],), (ROOMY,), pp)[0] for m in layout(model, pp)]
    return _EXPECT[key]
