"""Solid extraction of a general-model header with ZPQ_SET_LANES=1: the sets zpq_archive.cpp creates follow the variable,
so the blocks of one header decode round by round on k_rows<decode> instead of a k_generic launch per block and round.

The archive holds three blocks of C4B's header (all nine component types) with 2, 4 and 5 segments, an empty file among
them.  It is assembled here from the oracle -- the block head as the writer lays it out (locator, "zPQ", level, 1, hsize,
COMP, HCOMP), per file `01 name 00 comment 00 00`, the bytes oracle_lib.Codec writes for that segment on the block's running
model, `00 00 00 00 FD` + SHA-1, and `FF` behind the block's last file -- because the project's writers cannot make it:
archive_add writes the shipped levels only, and Compressor.start_block_hcomp reproduces the reference's quirk Q14 (no
block header is written and every component stays type 0: compressor.v:191-209)."""
import hashlib
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import oracle_lib as O  # noqa: E402
from inputs import C4B  # noqa: E402
from test_archive import file_set  # noqa: E402
from test_gpu_solid_archive import block_head, sequential_extract, triples  # noqa: E402

pytestmark = pytest.mark.gpu

SPLIT = (2, 4, 5)                                            # segments per block


def general_head(header):
    """The block head of `header`: compressor.v:63-75,157-167 as framing::block_header writes it."""
    shipped = block_head(2)
    locator = shipped[:shipped.index(b"zPQ")]
    assert len(locator) == 13
    cend, hbegin, hend = O.scan_header(header)
    body = header[:cend + 1] + header[hbegin:hend + 1]
    return locator + b"zPQ" + bytes([1 if header[4] else 2, 1, len(body) & 255, len(body) >> 8]) + body


def solid_block(header, files, offsets=None):
    codec = O.Codec(header)
    out = general_head(header)
    for nm, cm, d in files:
        out += b"\x01" + nm.encode() + b"\x00" + cm.encode() + b"\x00\x00"
        coded = codec.encode(d, pp=True)
        if offsets is not None:
            offsets.append((len(out), len(out) + len(coded)))
        out += coded + b"\x00\x00\x00\x00\xfd" + hashlib.sha1(d).digest()
    return out + b"\xff"


def blocks_of(files):
    assert len(files) == sum(SPLIT)
    out, at = [], 0
    for k in SPLIT:
        out.append(files[at:at + k])
        at += k
    return out


@pytest.fixture(scope="module")
def files():
    """Eleven small files (the sequential replay of a damaged block codes on the one-lane kernel): the first six of
    test_archive.file_set cut to 600 bytes -- an empty one among them -- and five more."""
    fs = [(nm, d[:600]) for nm, _, d in file_set(seed=3, n=5)]
    assert len(fs[0][1]) == 0 and len({nm for nm, _ in fs}) == sum(SPLIT)
    return [(nm, "%d bytes" % len(d), d) for nm, d in fs]


@pytest.fixture(scope="module")
def archive(files):
    return b"".join(solid_block(C4B, b) for b in blocks_of(files))


@pytest.fixture()
def env(monkeypatch):
    for k in ("ZPQ_SET_LANES", "ZPQ_LANES_ROWS", "ZPQ_DEC_GPIPE", "ZPQ_ENC_GPIPE", "ZPQ_VM_PIPE"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_the_sequential_front_end_reads_the_archive(zpq, gpu_ctx, env, files, archive):
    """The hand-assembled archive is one the project's own sequential Decompresser reads file by file."""
    got = sequential_extract(zpq, gpu_ctx, archive)
    assert [(nm, d, st) for nm, d, st in got] == [(nm, d, 0) for nm, _, d in files]


def test_solid_extraction_on_the_lane_kernels(zpq, gpu_ctx, env, files, archive):
    env.setenv("ZPQ_SET_LANES", "1")
    got = zpq.archive_extract(gpu_ctx, archive)
    assert gpu_ctx.last_kernel_name == "k_rows<decode>"
    assert triples(got) == files
    assert all(g["sha1_ok"] and g["status"] == 0 for g in got)
    env.delenv("ZPQ_SET_LANES")
    plain = zpq.archive_extract(gpu_ctx, archive)
    assert gpu_ctx.last_kernel_name == "k_generic<decode>"   # the default route of a general-model set
    assert plain == got
    env.setenv("ZPQ_SET_LANES", "0")
    assert zpq.archive_extract(gpu_ctx, archive) == got
    assert gpu_ctx.last_kernel_name == "k_generic<decode>"


def test_a_damaged_later_segment_falls_back_to_the_replay(zpq, gpu_ctx, env, files, archive):
    """One payload byte of the THIRD segment of the four-segment block flipped: every other file of the archive comes out
    as before, and the damaged block is what the sequential replay makes of it, with and without the variable."""
    blocks = blocks_of(files)
    offsets = []
    damaged = bytearray(solid_block(C4B, blocks[1], offsets))
    lo, hi = offsets[2]
    damaged[(lo + hi) // 2] ^= 0x10
    arc = solid_block(C4B, blocks[0]) + bytes(damaged) + solid_block(C4B, blocks[2])
    alone = sequential_extract(zpq, gpu_ctx, bytes(damaged))
    assert [(nm, d) for nm, d, _ in alone[:2]] == [(nm, d) for nm, _, d in blocks[1][:2]]
    results = []
    for value in ("1", None):
        if value is None:
            env.delenv("ZPQ_SET_LANES")
        else:
            env.setenv("ZPQ_SET_LANES", value)
        got = zpq.archive_extract(gpu_ctx, arc)
        by_name = {g["name"]: g for g in got}
        for nm, cm, d in blocks[0] + blocks[2] + blocks[1][:2]:
            g = by_name[nm]
            assert (g["comment"], g["data"], g["sha1_ok"], g["status"]) == (cm, d, True, 0), nm
        for g in got:                                      # the damaged file, if it is reported at all, is never accepted
            if g["name"] == blocks[1][2][0]:
                assert not g["sha1_ok"] or g["status"] != 0, g["status"]
        middle = [g for g in got if g["name"] not in {nm for nm, _, _ in blocks[0] + blocks[2]}]
        assert [(g["name"], g["data"], g["status"]) for g in middle] == alone
        results.append(got)
    assert results[0] == results[1]
