"""Solid extraction of a general-model header with ZPQ_SET_LANES=1 ZPQ_SET_WAVES=1: the sets zpq_archive.cpp creates follow both
variables, so the blocks of one header decode round by round on k_wsetd<decode>, the wave-per-component decoder, instead of
k_rows<decode> (ZPQ_SET_LANES alone) or a k_generic launch per block and round (neither).  The archive is the one
tests/test_gpu_set_lanes_archive.py assembles from the oracle: three blocks of C4B's header with 2, 4 and 5 segments."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from inputs import C4B  # noqa: E402
from test_archive import CLI  # noqa: E402
from test_gpu_set_lanes_archive import archive, blocks_of, files, solid_block  # noqa: E402,F401  (fixtures and helpers)
from test_gpu_solid_archive import sequential_extract, triples  # noqa: E402

pytestmark = pytest.mark.gpu

KNOBS = ("ZPQ_SET_LANES", "ZPQ_SET_WAVES", "ZPQ_LANES_ROWS", "ZPQ_DEC_GPIPE", "ZPQ_ENC_GPIPE", "ZPQ_VM_PIPE", "ZPQ_GDEC_BPW")


@pytest.fixture()
def env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_solid_extraction_on_the_wave_decoder(zpq, gpu_ctx, env, files, archive):
    env.setenv("ZPQ_SET_LANES", "1")
    env.setenv("ZPQ_SET_WAVES", "1")
    got = zpq.archive_extract(gpu_ctx, archive)
    assert gpu_ctx.last_kernel_name == "k_wsetd<decode>"
    assert triples(got) == files
    assert all(g["sha1_ok"] and g["status"] == 0 for g in got)
    env.setenv("ZPQ_DEC_GPIPE", "0")                         # the per-call choice: the lane kernels again, the same files
    assert zpq.archive_extract(gpu_ctx, archive) == got
    assert gpu_ctx.last_kernel_name == "k_rows<decode>"
    env.delenv("ZPQ_DEC_GPIPE")
    env.setenv("ZPQ_SET_WAVES", "0")                         # withdrawn: the parent's run under ZPQ_SET_LANES=1
    assert zpq.archive_extract(gpu_ctx, archive) == got
    assert gpu_ctx.last_kernel_name == "k_rows<decode>"
    env.delenv("ZPQ_SET_LANES")
    env.setenv("ZPQ_SET_WAVES", "1")                         # alone it decides nothing: the default route of a general-model set
    assert zpq.archive_extract(gpu_ctx, archive) == got
    assert gpu_ctx.last_kernel_name == "k_generic<decode>"


def test_the_command_line_tool_extracts_under_both_variables(tmp_path, files, archive):
    """`zpaqv x` checks every file's SHA-1 against the one stored behind its segment and counts a mismatch as an error.  (The tool
    does not say which decoder ran; that the sets follow the variables is what the test above asserts through the kernel's name.)"""
    arc = tmp_path / "c4b.zpaq"
    arc.write_bytes(archive)
    runs = []
    for waves in ("1", "0"):
        e = dict(os.environ, ZPQ_SET_LANES="1", ZPQ_SET_WAVES=waves)
        for k in KNOBS[2:]:
            e.pop(k, None)
        out = tmp_path / ("out" + waves)
        r = subprocess.run([CLI, "x", str(arc), "-to", str(out)], capture_output=True, text=True, env=e)
        assert r.returncode == 0 and "Files extracted: %d" % len(files) in r.stdout, (r.stdout, r.stderr)
        for nm, _, d in files:
            assert (out / nm).read_bytes() == d, nm
        runs.append(r.stdout)
    assert runs[0] == runs[1].replace(str(tmp_path / "out0"), str(tmp_path / "out1"))


def test_a_damaged_later_segment_still_falls_back_to_the_replay(zpq, gpu_ctx, env, files, archive):
    """One payload byte of the THIRD segment of the four-segment block flipped: every other file comes out as before and the
    damaged block is what the sequential replay makes of it -- with both variables, with ZPQ_SET_WAVES=0, and with neither."""
    blocks = blocks_of(files)
    offsets = []
    damaged = bytearray(solid_block(C4B, blocks[1], offsets))
    lo, hi = offsets[2]
    damaged[(lo + hi) // 2] ^= 0x10
    arc = solid_block(C4B, blocks[0]) + bytes(damaged) + solid_block(C4B, blocks[2])
    alone = sequential_extract(zpq, gpu_ctx, bytes(damaged))
    assert [(nm, d) for nm, d, _ in alone[:2]] == [(nm, d) for nm, _, d in blocks[1][:2]]
    results = []
    for lanes, waves in (("1", "1"), ("1", "0"), (None, None)):
        for var, val in (("ZPQ_SET_LANES", lanes), ("ZPQ_SET_WAVES", waves)):
            if val is None:
                env.delenv(var, raising=False)
            else:
                env.setenv(var, val)
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
    assert results[0] == results[1] == results[2]
