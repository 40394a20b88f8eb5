"""Solid extraction of a header whose HCOMP program is not the shipped hash chain, with ZPQ_SET_LANES=1 ZPQ_SET_VMWAVES=1: the
sets zpq_archive.cpp creates follow both variables, so the blocks of one header decode round by round on k_vsetd<decode>, the
wave-per-component decoder with an interpreter wave, instead of k_rows<decode> (ZPQ_SET_LANES alone) or a k_generic launch per
block and round (neither).  The archive is assembled from the oracle as tests/test_gpu_set_lanes_archive.py does, from
vpipe_models.C4B_VM (C4b's components behind a program no recogniser takes): three blocks of 2, 4 and 5 segments."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vpipe_models as VM  # noqa: E402
from test_archive import CLI  # noqa: E402
from test_gpu_set_lanes_archive import blocks_of, files, solid_block  # noqa: E402,F401  (fixture and helpers)
from test_gpu_solid_archive import sequential_extract, triples  # noqa: E402

pytestmark = pytest.mark.gpu

KNOBS = ("ZPQ_SET_LANES", "ZPQ_SET_VMWAVES", "ZPQ_SET_WAVES", "ZPQ_LANES_ROWS", "ZPQ_DEC_GPIPE", "ZPQ_ENC_GPIPE", "ZPQ_VM_PIPE",
         "ZPQ_GDEC_BPW")
HEADER = bytes(VM.C4B_VM)


@pytest.fixture()
def env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def vm_archive(files):
    return b"".join(solid_block(HEADER, b) for b in blocks_of(files))


def test_solid_extraction_on_the_interpreter_wave_decoder(zpq, gpu_ctx, env, files, vm_archive):
    env.setenv("ZPQ_SET_LANES", "1")
    env.setenv("ZPQ_SET_VMWAVES", "1")
    got = zpq.archive_extract(gpu_ctx, vm_archive)
    assert gpu_ctx.last_kernel_name == "k_vsetd<decode>"
    assert triples(got) == files
    assert all(g["sha1_ok"] and g["status"] == 0 for g in got)
    env.setenv("ZPQ_DEC_GPIPE", "0")                         # the per-call choice: the lane kernels again, the same files
    assert zpq.archive_extract(gpu_ctx, vm_archive) == got
    assert gpu_ctx.last_kernel_name == "k_rows<decode>"
    env.delenv("ZPQ_DEC_GPIPE")
    env.setenv("ZPQ_SET_VMWAVES", "0")                       # withdrawn: the parent's run under ZPQ_SET_LANES=1
    assert zpq.archive_extract(gpu_ctx, vm_archive) == got
    assert gpu_ctx.last_kernel_name == "k_rows<decode>"
    env.delenv("ZPQ_SET_LANES")
    env.delenv("ZPQ_SET_VMWAVES")                            # neither: the default route of a general-model set
    assert zpq.archive_extract(gpu_ctx, vm_archive) == got
    assert gpu_ctx.last_kernel_name == "k_generic<decode>"
    env.setenv("ZPQ_SET_VMWAVES", "1")                       # alone it decides nothing
    assert zpq.archive_extract(gpu_ctx, vm_archive) == got
    assert gpu_ctx.last_kernel_name == "k_generic<decode>"


def test_the_command_line_tool_extracts_under_both_variables(tmp_path, files, vm_archive):
    """`zpaqv x` checks every file's SHA-1 against the one stored behind its segment and counts a mismatch as an error."""
    arc = tmp_path / "c4b_vm.zpaq"
    arc.write_bytes(vm_archive)
    e = dict(os.environ, ZPQ_SET_LANES="1", ZPQ_SET_VMWAVES="1")
    for k in KNOBS[2:]:
        e.pop(k, None)
    out = tmp_path / "out"
    r = subprocess.run([CLI, "x", str(arc), "-to", str(out)], capture_output=True, text=True, env=e)
    assert r.returncode == 0 and "Files extracted: %d" % len(files) in r.stdout, (r.stdout, r.stderr)
    for nm, _, d in files:
        assert (out / nm).read_bytes() == d, nm


def test_a_damaged_later_segment_still_falls_back_to_the_replay(zpq, gpu_ctx, env, files):
    """One payload byte of the THIRD segment of the four-segment block flipped: every other file comes out as before and the
    damaged block is what the sequential replay makes of it -- with both variables, with ZPQ_SET_VMWAVES=0, and with neither."""
    blocks = blocks_of(files)
    offsets = []
    damaged = bytearray(solid_block(HEADER, blocks[1], offsets))
    lo, hi = offsets[2]
    damaged[(lo + hi) // 2] ^= 0x10
    arc = solid_block(HEADER, blocks[0]) + bytes(damaged) + solid_block(HEADER, blocks[2])
    alone = sequential_extract(zpq, gpu_ctx, bytes(damaged))
    assert [(nm, d) for nm, d, _ in alone[:2]] == [(nm, d) for nm, _, d in blocks[1][:2]]
    results = []
    for lanes, vmwaves in (("1", "1"), ("1", "0"), (None, None)):
        for var, val in (("ZPQ_SET_LANES", lanes), ("ZPQ_SET_VMWAVES", vmwaves)):
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
