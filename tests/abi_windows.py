"""The batch ABI's buffer layouts: models, blocks, offset windows and what the CPU oracle makes of them.

include/zpaq_hip.h promises that the host-pointer batch calls read only in[in_off[0] .. in_off[n]) and write only inside
out[out_off[0] .. out_off[n]) for any n >= 1, that offsets are 64-bit, that zpq_*_blocks_multi deals contiguous shares
for any number of contexts, and that the host-pointer entry points may be called from several threads.  The cases here
are the layouts that hold the library to it: first offsets other than 0, a batch that straddles 2^32 in both buffers,
and the (nblocks, contexts) pairs whose deal leaves a context a share of ONE block at a block index other than 0.

Blocks are 0, 1, 63, 700 and 2048 bytes (tests/golden/inputs.py, tests/workload.py), caps 17 * len + 4096, the models one
per kernel family.  test_abi_windows_cpu.py checks this builder alone; test_gpu_abi_windows.py and
test_gpu_abi_threads.py hold the library to the oracle on it.
"""
import collections
import os
import sys

import numpy as np

import general_models as GM
import oracle_lib as O
import vpipe_models as VM
import workload as W

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from inputs import INPUTS, lcg_bytes, text_bytes  # noqa: E402

FILL = 0xEE
PP, VMPIPE = 1, 16                                        # ZPQ_FLAG_PP, ZPQ_FLAG_VMPIPE
E_OVERFLOW = -7
SIZES = (0, 1, 63, 700, 2048)
NO_BYTE = 0xFFFFFFFF                                      # first_byte[] without ZPQ_FLAG_PP
TWO32 = 1 << 32

# header, offsets (None: scan_header finds them), flags every call on the model carries besides ZPQ_FLAG_PP
Model = collections.namedtuple("Model", "header offsets flags")


def _models():
    out = collections.OrderedDict()
    for level in (1, 2, 3):
        out["level%d" % level] = Model(O.level_header(level), None, 0)
    for name in ("mix_x4", "n16", "n17", "n65"):           # the wave pipelines, k_rows, k_lanes, k_generic
        out[name] = Model(GM.NAMED[name][0], None, 0)
    out["c4b_vm"] = Model(VM.C4B_VM, None, VMPIPE)        # k_vpipe / k_vdec, on request
    return out


MODELS = _models()
# the batch kernels a model's default route runs for a batch of at least 12 blocks, where one name says it all (the chain
# models' names depend on the line store: test_gpu_chain_models.enc_names / dec_names answer for them)
KERNELS = {"mix_x4": ("k_gpipe<encode>", "k_gdec<decode>"), "n16": ("k_rows<encode>", "k_rows<decode>"),
           "n17": ("k_lanes<encode>", "k_lanes<decode>"), "n65": ("k_generic<encode>", "k_generic<decode>"),
           "c4b_vm": ("k_vpipe<encode>", "k_vdec<decode>")}


def cap_of(n):
    return 17 * n + 4096


def _make(size, kind, seed):
    """kind 0: the golden inputs' own bytes of that size; 1: uniform; 2: text; 3: the workload generator's block `seed`."""
    if kind == 0:
        return {0: INPUTS["empty"], 1: INPUTS["a"], 2048: INPUTS["text2k"]}.get(size, text_bytes(size))
    if kind == 1:
        return lcg_bytes(size, seed=12345 + seed)
    if kind == 2:
        return text_bytes(size + seed)[seed:]
    return bytes(W.make_block(seed, size))


# ---------------------------------------------------------------- the block lists
# five blocks, one of every size: the one-block cases
BASE = [_make(0, 0, 0), _make(1, 0, 0), _make(63, 3, 7), _make(700, 1, 3), _make(2048, 0, 0)]
# 13 ragged blocks: every size at least twice, every class of data, no two alike but the empty ones
RAGGED = BASE + [_make(2048, 3, 10), _make(0, 0, 0), _make(700, 3, 9), _make(1, 1, 5), _make(63, 2, 11), _make(700, 2, 4),
                 _make(2048, 1, 6), _make(63, 1, 8)]
# 13 blocks in the order the layout across 2^32 needs (far_layout): a 2048-byte block of uniform bytes third, so that its
# CODED bytes cross 2^32 in the output buffer, and a 700-byte block seventh, whose bytes cross it in the input buffer
FAR = [_make(0, 0, 0), _make(1, 0, 0), _make(2048, 1, 6), _make(63, 3, 7), _make(700, 1, 3), _make(2048, 0, 0),
       _make(700, 3, 9), _make(63, 2, 11), _make(1, 1, 5), _make(0, 0, 0), _make(2048, 3, 10), _make(700, 2, 4), _make(63, 1, 8)]
FAR_IN0, FAR_OUT0 = TWO32 - 5000, TWO32 - 9001
FAR_DEC_IN0 = TWO32 - 1000                                # the coded streams back to back from here: block 2's cross 2^32
FAR_DEC_SLACK = 1600                                      # decode slabs of len + 1600: block 4's 700 bytes cross 2^32
BIG_BUFFER = TWO32 + (1 << 21)

WINDOWS = ((0, 0), (1, 4099), (4099, 1))                  # (in_off[0], out_off[0]) of the one-block cases
SHIFT = (4099, 777)                                       # ... of the 13 ragged blocks
# (nblocks, the contexts by name): with G = min(nctx, nblocks), context g codes blocks [nblocks * g / G, nblocks * (g + 1) / G)
MULTI = ((1, "ab"), (2, "ab"), (3, "ab"), (3, "aba"), (5, "abab"))


def shares(nblocks, nctx):
    """The library's deal (multi_batch in zpq_api.hip), restated: [(b0, b1)] per context that gets any block."""
    G = min(nctx, nblocks)
    return [(nblocks * g // G, nblocks * (g + 1) // G) for g in range(G)]


def layout(lens, first=0):
    """Offsets of consecutive slabs of these lengths, the first one at `first`."""
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[0] = first
    if len(lens):
        off[1:] = first + np.cumsum(np.asarray(lens, dtype=np.uint64))
    return off


def straddler(off, ends=None):
    """Index of the one slab with off[b] < 2^32 < off[b] + (ends[b] if given: the bytes that exist; else the slab), or None."""
    hit = []
    for b in range(len(off) - 1):
        lo = int(off[b])
        hi = lo + int(ends[b]) if ends is not None else int(off[b + 1])
        if lo < TWO32 < hi:
            hit.append(b)
    return hit[0] if len(hit) == 1 else None


# ---------------------------------------------------------------- the oracle's answers, computed once
_CODED, _DEC = {}, {}


def coded(name, which, pp=True):
    """The oracle's streams of a model for one of the block lists ("base", "ragged", "far")."""
    k = (name, which, pp)
    if k not in _CODED:
        blocks = {"base": BASE, "ragged": RAGGED, "far": FAR}[which]
        _CODED[k] = O.encode_blocks(MODELS[name].header, blocks, pp=pp, nthreads=8)
    return _CODED[k]


Decoded = collections.namedtuple("Decoded", "stored out_len consumed final_code first_byte status")


def decoded(name, stream, cap, pp=True):
    """What zpq_decode_blocks must return for one stream into a slab of `cap` bytes (zo_decode_prefix, the GPU decoders'
    stop rule: EOF, or right after byte cap + 1, the PP byte not counted)."""
    k = (name, stream, cap, pp)
    if k not in _DEC:
        m = MODELS[name]
        stored, olen, cons, code, vmo = O.Codec(m.header, m.offsets).decode_prefix(stream, cap + (1 if pp else 0))
        assert not vmo
        first = NO_BYTE
        if pp:
            assert olen >= 1
            first, stored, olen = stored[0], stored[1:], olen - 1
        _DEC[k] = Decoded(stored, olen, cons, code, first, E_OVERFLOW if olen > cap else 0)
    return _DEC[k]


def far_layouts(name, n):
    """The four offset arrays of the batch across 2^32 for the first n blocks of FAR: encode input, encode output
    (slabs of 17 * len + 4096), decode input (the coded streams back to back) and decode output (slabs of len + 1600)."""
    lens = [len(b) for b in FAR[:n]]
    streams = coded(name, "far")[:n]
    return (layout(lens, FAR_IN0), layout([cap_of(x) for x in lens], FAR_OUT0),
            layout([len(c) for c in streams], FAR_DEC_IN0), layout([x + FAR_DEC_SLACK for x in lens], FAR_OUT0))


# ---------------------------------------------------------------- SHA-1 ranges
def sha1_grid():
    """768 messages in one arena: every (len & 63, addr & 3) at 0, 1 and 2 full chunks.  Returns (arena bytes, begin[],
    end[]) with a byte of slack between neighbours."""
    begin, end, at = [], [], 0
    for chunks in (0, 1, 2):
        for rem in range(64):
            for mis in range(4):
                at = (at + 3) // 4 * 4 + mis
                begin.append(at)
                at += 64 * chunks + rem
                end.append(at)
                at += 1
    return lcg_bytes(at + 16, seed=777), begin, end


def sha1_odd_ranges(size):
    """Ranges inside an arena of `size` bytes that no contiguous in_off[] can express: empty ones, overlapping ones, the
    list in descending address order, a start at every addr & 3."""
    out = []
    for i in range(12):                                   # descending, each overlapping its predecessor by half
        b = size - 200 - 90 * i + (i & 3)
        out.append((b, b + 180))
    out += [(0, 0), (7, 7), (size, size)]                 # empty, also at the arena's very end
    out += [(5, 70), (5, 70), (6, 69), (4, 133)]          # the same range twice, nested ranges
    out += [(k, k + 64 + k) for k in range(8)]            # a start at every addr & 3, twice
    assert all(0 <= b <= e <= size for b, e in out)
    return out
