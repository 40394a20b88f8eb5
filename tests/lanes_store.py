"""General models on the compact line store (ZPQ_FLAG_LINESTORE / ZPQ_LANES_STORE): the models and blocks that
test_lanes_store_cpu.py and test_gpu_lanes_store.py share.

The store is 256 lines (ZPQ_SPARSE_FORCE_LOG2=8, 68 bytes a line: 17 408 bytes): an ICM / ISSE of 9 bits or more (a table of
32 KiB or more) goes on the store, one of 8 bits (16 KiB) stays dense, and a lane's store refuses the block after 240 claims.
A block of L bytes with its PP byte probes each table 2 (L + 1) times, once per nibble: the blocks of up to 100 bytes make at
most 202 probes and fit whatever they hold; 400 random bytes under a context of order two touch more than 480 lines of a
large table -- twice the limit, so that block is refused for certain.
"""
import os
import random
import sys

import chain_models as CM_
import general_models as GM
import oracle_lib as O  # noqa: F401  (the tests' reference, re-exported)
from general_models import AVG, CM, CONST, ICM, ISSE, MATCH, MIX, MIX2, SSE, H  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "pyref"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import zpaq_pyref as P  # noqa: E402
from inputs import C4B  # noqa: E402

LOG2 = 8
CAP = 1 << LOG2                       # lines
STORE_BYTES = 68 * CAP                # 64 a line and 4 its tag
LIMIT = CAP - CAP // 16               # claims
DENSE_CAP = 1 << 20                   # a store of 68 MiB: larger than every hashed table below

_A = [[ICM, 9], [ICM, 10], [ISSE, 8, 0], [ISSE, 11, 1], [CM, 10, 255], [MIX, 2, 0, 5, 24, 255]]
_C = ([[ICM, 10], [ISSE, 9, 0], [ISSE, 8, 1], [ISSE, 12, 2], [ICM, 11], [MATCH, 8, 9], [CONST, 200]] + GM.cms(9, 0, 8)
      + [[MIX2, 3, 3, 4, 24, 255], [MIX, 1, 0, 17, 24, 255], [SSE, 2, 17, 32, 255]])
# hash *d=a d++ *d=a halt behind the hash chain's head: H[0] = H[1], one order-two context for two components
_SAME_CTX = CM_.HC_HEAD + [59, 112, 25, 112, 56]

MODELS = {
    # (a) k_rows with the hash chain in registers; without the request the wave pipelines take it
    "a_rows_vmh": H(_A, 3, 8, GM.hashchain(6)),
    # (b) the same components behind another program: k_rows with its interpreter
    "b_rows_vm": H(_A, 3, 8, GM.perturbed_hashchain(6, random.Random(1))),
    # (c) 19 components: k_lanes, with both programs
    "c_lanes_vmh": H(_C, 5, 8, GM.hashchain(19)),
    "c_lanes_vm": H(_C, 5, 8, GM.perturbed_hashchain(19, random.Random(2))),
    # (d) all nine types; both hashed tables (16 bits) on the store
    "d_c4b": C4B,
    # (e) two hashed components of equal size under equal contexts: two stores, the same lines claimed in each
    "e_twins": H([[ICM, 10], [ICM, 10], [AVG, 0, 1, 128]], 2, 8, _SAME_CTX),
}
ROWS0 = ("a_rows_vmh", "b_rows_vm")   # also with ZPQ_LANES_ROWS=0: k_lanes
OVERFLOW_MODEL = "a_rows_vmh"

TEXT = b"the quick brown fox jumps over the lazy dog, and then the dog sleeps on. "


def block(r, kind, n):
    if kind == 0:
        return bytes(r.getrandbits(8) for _ in range(n))
    if kind == 1:
        return bytes(n)
    if kind == 2:
        at = r.randrange(len(TEXT))
        return (TEXT[at:] + TEXT * (n // len(TEXT) + 1))[:n]
    per = bytes(r.getrandbits(8) for _ in range(r.randint(1, 7)))
    return (per * (n // len(per) + 1))[:n]


def fitting_blocks(seed=5):
    """21 blocks (no multiple of 4 or 16) of 0, 1, 2 ... 100 bytes: random, zeros, text, periodic."""
    r = random.Random(seed)
    sizes = [0, 1, 2, 3, 7, 8, 15, 16, 17, 31, 33, 47, 50, 63, 64, 65, 80, 90, 99, 100, 100]
    return [block(r, i % 4, n) for i, n in enumerate(sizes)]


def overflow_block(seed=9):
    return block(random.Random(seed), 0, 400)


def hashed(hdr):
    """(component index, size bits) of the header's ICMs and ISSEs."""
    return [(i, c[1]) for i, c in enumerate(GM.components(hdr)) if c[0] in (ICM, ISSE)]


def compact(hdr, cap=CAP):
    """The hashed components whose table (64 << bits bytes) is larger than a store of `cap` lines."""
    return [(i, b) for i, b in hashed(hdr) if (64 << b) > 68 * cap]


def distinct_lines(hdr, data, pp=True):
    """{component: number of distinct 64-byte lines of its dense table the block touches}, from the pure-Python
    reference's contexts: find_ht is asked once per nibble with hctx + 16 c8 (predictor.v:558-560), c8 = 1 at a byte's
    start and 16 + its high nibble behind it, and its three candidate rows share the line
    ((hctx + 16 c8) * 16 & (ht_len - 16)) >> 6."""
    cend, hbegin, hend = P.scan_header(hdr)
    z = P.ZPAQL(hdr, cend, hbegin, hend)
    lines = {i: set() for i, _ in hashed(hdr)}
    hctx = {i: 0 for i in lines}
    for byte in ([0] if pp else []) + list(data):
        for i, bits in hashed(hdr):
            ht_len = 64 << bits
            for c8 in (1, 16 + (byte >> 4)):
                lines[i].add((((hctx[i] + 16 * c8) * 16) & 0xFFFFFFFF & (ht_len - 16)) >> 6)
        z.run(byte)
        for i in lines:
            hctx[i] = z.h_get(i) if i < len(z.h) else 0
    return {i: len(s) for i, s in lines.items()}
