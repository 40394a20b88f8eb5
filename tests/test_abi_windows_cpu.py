"""The case builder of the batch-ABI tests (tests/abi_windows.py), checked on its own: no GPU.

What the GPU tests rely on and do not check themselves: that every stream fits its slab (so that no ZPQ_E_OVERFLOW can
stand in for a pass), that the two CPU references agree on these blocks, that the listed (nblocks, contexts) pairs really
deal a context one block at a block index other than 0, and that the layout across 2^32 really has bytes on both sides
of it in every buffer.
"""
import hashlib
import os
import sys

import pytest

import abi_windows as A
import oracle_lib as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "pyref"))
import zpaq_pyref as P  # noqa: E402


def test_blocks_are_the_sizes_the_kernels_go_wrong_at():
    assert sorted(len(b) for b in A.BASE) == list(A.SIZES)
    for blocks in (A.RAGGED, A.FAR):
        assert len(blocks) == 13 and {len(b) for b in blocks} == set(A.SIZES)
        assert all(len(b) <= 4096 for b in blocks)
        live = [b for b in blocks if b]
        assert len(set(live)) == len(live)                # no two alike: a block delivered to the wrong slab shows


@pytest.mark.parametrize("name", list(A.MODELS))
def test_every_stream_fits_its_slab(name):
    for which, blocks in (("base", A.BASE), ("ragged", A.RAGGED), ("far", A.FAR)):
        for pp in (True, False):
            for b, c in zip(blocks, A.coded(name, which, pp)):
                assert 0 < len(c) <= A.cap_of(len(b)), (which, pp, len(b), len(c))


@pytest.mark.parametrize("name", list(A.MODELS))
def test_pyref_agrees_with_the_c_oracle(name):
    """Every block the GPU tests use: the 13 ragged ones with the PP byte (the first five are the one-block cases and are
    decoded by pyref too; the list across 2^32 holds the same 13 in another order), the 700 uniform bytes also without it."""
    m = A.MODELS[name]
    assert sorted(A.FAR) == sorted(A.RAGGED) and A.RAGGED[:5] == A.BASE
    assert A.coded(name, "ragged")[:5] == A.coded(name, "base")
    assert sorted(A.coded(name, "far")) == sorted(A.coded(name, "ragged"))
    for i, (b, w) in enumerate(zip(A.RAGGED, A.coded(name, "ragged"))):
        assert P.encode_segment(P.new_model(m.header, m.offsets), b) == w, (i, len(b))
        if i < 5:
            assert P.decode_segment(P.new_model(m.header, m.offsets), w)[0] == b"\0" + b, len(b)
    assert P.encode_segment(P.new_model(m.header, m.offsets), A.BASE[3], pp=False) == A.coded(name, "base", False)[3]


@pytest.mark.parametrize("name", list(A.MODELS))
def test_decode_expectations(name):
    m = A.MODELS[name]
    for pp in (True, False):
        for b, c in zip(A.BASE, A.coded(name, "base", pp)):
            d = A.decoded(name, c, len(b) + 64, pp)
            assert (d.stored, d.out_len, d.consumed, d.status) == (b, len(b), len(c), 0)
            assert d.first_byte == (0 if pp else A.NO_BYTE)
            if len(b) > 17:                                # a slab too small: the prefix, cap + 1, and the decoder's place there
                s = A.decoded(name, c, 17, pp)
                assert (s.stored, s.out_len, s.status) == (b[:17], 18, A.E_OVERFLOW) and 0 < s.consumed <= len(c)
    assert O.Codec(m.header, m.offsets).decode(A.coded(name, "base")[4])[0] == b"\0" + A.BASE[4]


def test_multi_cases_pin_the_deal_and_its_one_block_shares():
    """G = min(nctx, nblocks), context g gets [nblocks * g / G, nblocks * (g + 1) / G): the deal of multi_batch.  Every
    listed case deals a share of one block; in three of the five it lies behind block 0, where the one-block path must
    honour out_off[0] != 0.  The other two are the deal's remaining edges: one block for two contexts (no index but 0),
    and three blocks for two (the integer division gives the FIRST context the short share)."""
    behind = {}
    for nblocks, ctxs in A.MULTI:
        sh = A.shares(nblocks, len(ctxs))
        assert sh[0][0] == 0 and sh[-1][1] == nblocks and all(a[1] == b[0] for a, b in zip(sh, sh[1:]))
        assert all(b1 > b0 for b0, b1 in sh)
        assert any(b1 - b0 == 1 for b0, b1 in sh), (nblocks, ctxs, sh)
        behind[(nblocks, ctxs)] = [b0 for b0, b1 in sh if b1 - b0 == 1 and b0 > 0]
    assert behind == {(1, "ab"): [], (2, "ab"): [1], (3, "ab"): [], (3, "aba"): [1, 2], (5, "abab"): [1, 2]}
    assert A.shares(1, 2) == [(0, 1)] and A.shares(3, 2) == [(0, 1), (1, 3)]
    assert A.shares(9, 8).count((0, 1)) == 1 and sum(b1 - b0 == 1 and b0 > 0 for b0, b1 in A.shares(9, 8)) == 6
    assert A.shares(3, 3) == [(0, 1), (1, 2), (2, 3)] and A.shares(5, 4) == [(0, 1), (1, 2), (2, 3), (3, 5)]
    assert A.shares(61, 3) == [(0, 20), (20, 40), (40, 61)]


@pytest.mark.parametrize("name", list(A.MODELS))
def test_far_layout_has_bytes_on_both_sides_of_2_32(name):
    """In each of the four buffers' layouts: blocks that end below 2^32, ONE block whose slab straddles it -- and whose
    bytes do, raw, coded or decoded -- and blocks above."""
    for n in (12, 13):
        lens = [len(b) for b in A.FAR[:n]]
        clens = [len(c) for c in A.coded(name, "far")[:n]]
        enc_in, enc_out, dec_in, dec_out = A.far_layouts(name, n)
        for off, ends in ((enc_in, lens), (enc_out, clens), (dec_in, clens), (dec_out, lens)):
            b = A.straddler(off)
            assert b is not None and 0 < b < n - 1, (n, off)
            assert int(off[b]) < A.TWO32 < int(off[b + 1])
            assert A.straddler(off, ends) == b             # the bytes that exist cross it, not only the slab
            assert int(off[b - 1]) + ends[b - 1] <= A.TWO32 <= int(off[b + 1])
            assert int(off[-1]) + (1 << 16) <= A.BIG_BUFFER and int(off[0]) >= 1 << 16
        assert int(enc_in[0]) == A.TWO32 - 5000 and int(enc_out[0]) == A.TWO32 - 9001
        assert [int(enc_out[i + 1] - enc_out[i]) for i in range(n)] == [A.cap_of(x) for x in lens]


def test_sha1_cases():
    arena, begin, end = A.sha1_grid()
    assert len(begin) == 768 and end[-1] + 16 <= len(arena)
    assert {((e - b) & 63, b & 3, (e - b) >> 6) for b, e in zip(begin, end)} == {(r, m, c) for r in range(64) for m in range(4) for c in range(3)}
    assert all(e < b2 for e, b2 in zip(end, begin[1:]))
    odd = A.sha1_odd_ranges(4000)
    assert {b & 3 for b, e in odd if e > b} == {0, 1, 2, 3} and sum(b == e for b, e in odd) >= 3
    desc = odd[:12]
    assert all(x[0] > y[0] and y[1] > x[0] for x, y in zip(desc, desc[1:]))    # descending, overlapping
    assert hashlib.sha1(b"").hexdigest() == "da39a3ee5e6b4b0d3255bfef95601890afd80709"
