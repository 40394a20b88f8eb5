"""The one-block segment path: models, segment sequences and what the CPU oracle makes of them.

A zpq.Block codes its first segment on the batch kernels and every later one on k_generic with ZB_KEEP_STATE, after a
replay of the first segment's symbols into the block's own slot (block_materialise).  The same k_generic launches are
every later segment of the sequential Compressor / Decompresser, of the replay archive_extract falls back to, of a
default-route block set of a general model and of any model with more than 64 components.  What has to outlive a segment
there: the tables, the ZPAQL machine, MATCH's scalars -- and p[], the last bit's predictions, which Predictor.reset()
(predictor.v:827-833) does not touch: a component whose input index is not below its own (quirk Q13) reads at a segment's
first bit what was predicted for the last bit of the segment before.

MODELS are about twenty headers of every family that reaches this path; SEQUENCES are three sequences of five or six
segments, each with an empty segment, a one-byte segment and a segment behind an empty one, that differ in how the block
begins (data, nothing, a stream whose first byte is no PP byte).  TELLS pins, per model with a forward reference, the first
segment at which a coder that zeroed p[] between segments writes other bytes than the oracle (test_segment_path_cpu.py
proves the table); test_gpu_segment_path.py holds the kernels to the oracle on all of it.
"""
import collections
import os
import random
import sys

import chain_models as CM
import general_models as GM
import offnominal_corpus as OC
import oracle_lib as O
import zpaql_programs as ZP
from general_models import AVG, ICM, ISSE, MATCH, cms, hashchain

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from inputs import C4B  # noqa: E402
from test_gpu_lanes import MODELS as LANE_MODELS, hdr as lanes_hdr  # noqa: E402

PP = 1                                                    # ZPQ_FLAG_PP
CAP = 900                                                 # no segment is longer; the decoders' slab is CAP + 8

# 67 components, the forward reference at p[65]: behind the 64-lane stride k_generic loads and stores its scalars with
FWD_N67 = GM.H([[ISSE, 12, 65]] + cms(64, 0, 9) + [[ICM, 12], [AVG, 0, 65, 128]], 7, 8, hashchain(67))
# a MATCH whose buffer of 256 bytes wraps twice within a sequence (its scalars a / b / c / limit / cxt outlive a segment)
MATCH_WRAP = GM.H([[ICM, 10], [MATCH, 8, 8], [AVG, 0, 1, 128]], 2, 8, hashchain(3))

# header, offsets (None: scan_header finds them), family: what codes the FIRST segment of a zpq.Block
Model = collections.namedtuple("Model", "header offsets family")


def _models():
    out = collections.OrderedDict()
    for level in (1, 2, 3, 4, 5):
        out["level%d" % level] = Model(O.level_header(level), None, "chain")
    for name in ("chain7", "l2_hm0", "mix2_chain3"):      # the runtime loop, the interpreter (no M), a runtime MIX2
        out[name] = Model(CM.NAMED[name][0], None, "chain")
    out["c4b"] = Model(C4B, None, "general")
    out["match_wrap"] = Model(MATCH_WRAP, None, "general")
    for prog, shape in (("r_delay", "rows"), ("loop_on_old_f", "lanes")):    # the interpreter's registers and R, n <= 16 and n > 16
        hdr, offs = ZP.embed(ZP.NAMED[prog], shape)
        out["vm_" + shape] = Model(hdr, offs, "general")
    out["n65"] = Model(GM.NAMED["n65"][0], None, "generic")
    for name in ("fwd_avg", "fwd_isse", "fwd_mix_self", "fwd_sse_self", "fwd_mix2", "fwd_chain", "isse_stale_input"):
        out[name] = Model(lanes_hdr(LANE_MODELS[name]), None, "general")
    out["fwd_n20"] = Model(GM.NAMED["fwd_n20"][0], None, "general")
    out["fwd_n67"] = Model(FWD_N67, None, "generic")
    return out


MODELS = _models()
FORWARD = tuple(n for n in MODELS if n.startswith("fwd_") or n == "isse_stale_input")
SMALL = ("vm_lanes", "fwd_n20", "n65", "fwd_n67")          # more than 16 components, walked by one lane: totals below 800 bytes

# The first segment (1-based) at which a zeroed p[] departs from the oracle, per sequence ("main", "empty_first",
# "prog_first"); None: never.  fwd_sse_self's SSE reads its own p[0] only to pick a row beyond its table (Q10: it predicts
# 0 either way), isse_stale_input's ISSE feeds nothing, fwd_n20's forward readers end in a MIX whose prediction stays 0.
TELLS = {
    "fwd_avg": (2, 4, 2), "fwd_isse": (2, 4, 2), "fwd_mix_self": (2, 3, 2), "fwd_n67": (2, 3, 2),
    "fwd_chain": (2, 5, 2), "fwd_mix2": (2, 2, 6),
    "fwd_sse_self": (None, None, None), "isse_stale_input": (None, None, None), "fwd_n20": (None, None, None),
}
SEQUENCES = ("main", "empty_first", "prog_first")

Segment = collections.namedtuple("Segment", "data flags")


def _text(r, n):
    return bytes(r.choice(b"etaoin shr") for _ in range(n))


def _periodic(r, n):
    per = _text(r, 37)
    return (per * (n // 37 + 1))[:n]


_SEQ = {}


def sequence(which, small=False):
    """[Segment] of a sequence.  main: 5 segments, data first; empty_first: the block begins with an empty segment (the
    replay of a block that has coded only its PP byte); prog_first: 6 segments, the first coded with flags = 0 and beginning
    with a byte that is not 0 (a PROG-style stream: the decoder reports it in first_byte and the replay feeds it literally),
    then calls with and without ZPQ_FLAG_PP in turn.  small: the lengths for the models of SMALL."""
    key = (which, small)
    if key not in _SEQ:
        r = random.Random(20 + SEQUENCES.index(which))
        if which == "main":
            lens, flags = ((200, 1, 0, 220, 160) if small else (500, 1, 0, 900, 400)), (PP,) * 5
        elif which == "empty_first":
            lens, flags = ((0, 170, 1, 0, 190) if small else (0, 500, 1, 0, 700)), (PP,) * 5
        else:
            lens, flags = ((150, 0, 1, 180, 0, 120) if small else (400, 0, 1, 600, 0, 300)), (0, PP, 0, PP, 0, PP)
        segs = []
        for i, (n, f) in enumerate(zip(lens, flags)):
            data = _periodic(r, n) if i == 3 else _text(r, n)
            if which == "prog_first" and i == 0:
                data = bytes([1, 2, 0, 57, 56]) + data[5:]
            segs.append(Segment(data, f))
        assert max(lens) <= CAP and sum(lens) <= (800 if small else 4096)
        assert 0 in lens and 1 in lens and any(a == 0 and b > 0 for a, b in zip(lens, lens[1:]))
        _SEQ[key] = segs
    return _SEQ[key]


def segments(name, which):
    return sequence(which, small=name in SMALL)


def codec(name):
    m = MODELS[name]
    return O.Codec(m.header, m.offsets)


_WANT = {}


def coded(name, which):
    """The oracle's stream for every segment of the sequence, one codec for the block.  Computed once, never changed."""
    key = (name, which)
    if key not in _WANT:
        c = codec(name)
        _WANT[key] = tuple(c.encode(s.data, pp=bool(s.flags & PP)) for s in segments(name, which))
        del c
    return _WANT[key]


_DECODED = {}


def decoded(name, which, all_pp=False):
    """offnominal_corpus.Expected per segment for a decoder that reads coded(name, which) with a slab of CAP + 8 bytes and the
    flags the segment was coded with -- or, all_pp, with ZPQ_FLAG_PP throughout, as the readers of an archive do: the first
    byte of every stream then comes back in first_byte (0xFFFFFFFF where the stream holds none)."""
    key = (name, which, all_pp)
    if key not in _DECODED:
        c = codec(name)
        out = []
        for s, stream in zip(segments(name, which), coded(name, which)):
            pp = True if all_pp else bool(s.flags & PP)
            out.append(OC.shape(c.decode_prefix(stream, CAP + 8 + (1 if pp else 0)), CAP + 8, pp))
        del c
        _DECODED[key] = tuple(out)
    return _DECODED[key]


def first_kernels(zpq, name):
    """(encode, decode) kernel of a fresh zpq.Block's first segment, from the library's host predicates: a chain model on
    k_chain (one block is below the pipelined encoder's minimum), a general model on the wave pipelines where they apply and on
    k_rows / k_lanes otherwise, more than 64 components on k_generic.  The environment's knobs count."""
    m = MODELS[name]
    model = zpq.Model(header=m.header, offsets=m.offsets)
    try:
        if CM.route(zpq, model) is not None:
            return "k_chain<encode>", "k_chain<decode>"
        gpipe, gdec, lanes, kernel = GM.route(zpq, model)
        if not lanes:
            return "k_generic<encode>", "k_generic<decode>"
        return ("k_gpipe<encode>" if gpipe else kernel + "<encode>"), ("k_gdec<decode>" if gdec else kernel + "<decode>")
    finally:
        model.close()


# what the GPU file asserts for a block's first segment
FIRST_KERNELS = {
    "chain": ("k_chain<encode>", "k_chain<decode>"),
    "c4b": ("k_gpipe<encode>", "k_gdec<decode>"), "match_wrap": ("k_gpipe<encode>", "k_gdec<decode>"),
    "vm_rows": ("k_rows<encode>", "k_rows<decode>"), "vm_lanes": ("k_lanes<encode>", "k_lanes<decode>"),
    "fwd_n20": ("k_lanes<encode>", "k_lanes<decode>"),
    "generic": ("k_generic<encode>", "k_generic<decode>"),
    "forward4": ("k_rows<encode>", "k_rows<decode>"),     # the small forward-reference models: never the wave pipelines
}


def expected_first_kernels(name):
    fam = MODELS[name].family
    if fam in ("chain", "generic"):
        return FIRST_KERNELS[fam]
    return FIRST_KERNELS.get(name, FIRST_KERNELS["forward4"])


def set_members(name):
    """Three members for a block set, each a whole sequence coded with ZPQ_FLAG_PP throughout (a set's call has one flag word
    for all its members): main and empty_first as they are, prog_first's data.  Each tells a zeroed p[] on the forward-reference
    models that tell at all (test_segment_path_cpu.py)."""
    return [[s.data for s in segments(name, which)] for which in SEQUENCES]


# ---------------------------------------------------------------- archives of a forward-reference model
ARCHIVE_MODELS = ("fwd_isse", "fwd_n67")
ARCHIVE_SPLIT = (2, 4, 5)                                 # segments per block


def archive_files(name):
    """Eleven files (name, comment, data) for blocks of 2, 4 and 5 segments; an empty file opens the second block, a one-byte file follows it."""
    r = random.Random(77)
    sizes = (100, 200, 0, 1, 64, 150, 65, 0, 100, 17, 140) if name in SMALL else (100, 200, 0, 1, 64, 400, 65, 0, 250, 17, 350)
    assert len(sizes) == sum(ARCHIVE_SPLIT)
    return [("f%02d.txt" % i, "%d bytes" % n, _text(r, n)) for i, n in enumerate(sizes)]


def archive_blocks(name):
    files, out, at = archive_files(name), [], 0
    for k in ARCHIVE_SPLIT:
        out.append(files[at:at + k])
        at += k
    return out
