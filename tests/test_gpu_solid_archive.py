"""Solid archives (archive_add(..., solid=N), `zpaqv a -solid N`): N files per block, a segment each, written and read
back through block sets.  The expected archive is assembled here from the oracle: the block head of a one-file oracle
archive, per file `01 name 00 comment 00 00`, the bytes oracle_lib.Codec writes for that segment on the block's running
model, `00 00 00 00 FD` + SHA-1, and `FF` behind the block's last file."""
import hashlib
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import oracle_lib as O  # noqa: E402
from inputs import INPUTS  # noqa: E402
from test_archive import CLI, file_set, oracle_archive, oracle_one  # noqa: E402

pytestmark = pytest.mark.gpu


def block_head(level):
    one = oracle_one(level, "headprobe", "", b"")
    return one[:one.index(b"\x01headprobe\x00")]


def solid_block(level, files, offsets=None):
    """One block holding `files`; offsets (if a list) receives where each file's coded payload starts and ends."""
    codec = O.Codec(O.level_header(level))
    out = block_head(level)
    for nm, cm, d in files:
        out += b"\x01" + nm.encode() + b"\x00" + cm.encode() + b"\x00\x00"
        coded = codec.encode(d, pp=True)
        if offsets is not None:
            offsets.append((len(out), len(out) + len(coded)))
        out += coded + b"\x00\x00\x00\x00\xfd" + hashlib.sha1(d).digest()
    return out + b"\xff"


def solid_archive(level, files, n):
    return b"".join(solid_block(level, files[i:i + n]) for i in range(0, len(files), n))


def triples(got):
    return [(g["name"], g["comment"], g["data"]) for g in got]


@pytest.mark.parametrize("level", [1, 2, 3])
@pytest.mark.parametrize("n", [2, 5])
def test_solid_archive_bytes_and_extraction(zpq, gpu_ctx, level, n):
    files = file_set(seed=level, n=12)
    arc = zpq.archive_add(gpu_ctx, level, files, solid=n)
    assert gpu_ctx.last_kernel_name == "k_chain<encode>"
    assert arc == solid_archive(level, files, n)
    got = zpq.archive_extract(gpu_ctx, arc)
    assert gpu_ctx.last_kernel_name == "k_chain<decode>"       # (the sequential replay decodes later segments on k_generic)
    assert triples(got) == files
    assert all(g["sha1_ok"] and g["status"] == 0 for g in got)
    listed = zpq.archive_extract(gpu_ctx, arc, want_data=False)
    assert [(g["name"], g["size"]) for g in listed] == [(nm, len(d)) for nm, _, d in files]


def test_solid_1_is_the_reference_layout(zpq, gpu_ctx):
    files = file_set(seed=4, n=6)
    assert zpq.archive_add(gpu_ctx, 2, files, solid=1) == zpq.archive_add(gpu_ctx, 2, files, solid=0) == oracle_archive(2, files)


def sequential_extract(zpq, ctx, arc):
    """What the sequential front end makes of a stream: (name, data, status) per segment, stopping at the first error."""
    d = zpq.Decompresser(ctx)
    d.set_input(arc)
    out, seen = [], 0
    while d.find_block():
        while d.find_filename():
            name = d.get_filename()
            while d.decompress(65536):
                pass
            d.read_segment_end()
            data = d.output_bytes()
            out.append((name, data[seen:], d.last_error))
            seen = len(data)
            if d.last_error != 0:
                return out
    return out


def test_mixed_archive_with_a_damaged_solid_block(zpq, gpu_ctx):
    files = file_set(seed=9, n=10)
    offsets = []
    damaged = bytearray(solid_block(2, files[12:16], offsets))
    lo, hi = offsets[1]
    damaged[(lo + hi) // 2] ^= 0x10                           # one payload byte of the block's SECOND segment
    parts = [solid_archive(2, files[0:6], 3), zpq.archive_add(gpu_ctx, 2, files[6:8]), zpq.archive_add(None, 0, files[8:10]),
             solid_archive(1, files[10:12], 2), bytes(damaged)]
    got = zpq.archive_extract(gpu_ctx, b"".join(parts))
    assert triples(got[:12]) == files[:12] and all(g["sha1_ok"] and g["status"] == 0 for g in got[:12])
    # the damaged block: what the sequential path makes of it (first file right, the second one reported, never accepted)
    alone = zpq.archive_extract(gpu_ctx, bytes(damaged))
    assert [(g["name"], g["data"], g["status"], g["sha1_ok"]) for g in got[12:]] == [(g["name"], g["data"], g["status"], g["sha1_ok"]) for g in alone]
    seq = sequential_extract(zpq, gpu_ctx, bytes(damaged))
    assert [(g["name"], g["data"], g["status"]) for g in alone] == seq
    assert (alone[0]["name"], alone[0]["data"], alone[0]["sha1_ok"]) == (files[12][0], files[12][2], True)
    assert len(alone) >= 2 and not (alone[1]["sha1_ok"] and alone[1]["status"] == 0 and alone[1]["data"] == files[13][2])


def test_two_contexts_are_position_stable(zpq, gpu_ctx):
    other = zpq.Context(0)
    try:
        files = file_set(seed=21, n=14)
        one = zpq.archive_add(gpu_ctx, 2, files, solid=3)
        two = zpq.archive_add([gpu_ctx, other], 2, files, solid=3)
        assert one == two == solid_archive(2, files, 3)
        a = zpq.archive_extract(gpu_ctx, one)
        b = zpq.archive_extract([gpu_ctx, other], one)
        assert a == b and triples(b) == files
    finally:
        other.close()


def test_cli_solid_round_trips(tmp_path):
    files = file_set(seed=5, n=10)
    src = tmp_path / "in"
    src.mkdir()
    for nm, _, d in files:
        (src / nm).write_bytes(d)
    arc = str(tmp_path / "arc.zpaq")
    r = subprocess.run([CLI, "a", arc, str(src), "-m2", "-solid", "4"], capture_output=True, text=True)
    assert r.returncode == 0 and "Files added: %d" % len(files) in r.stdout, r.stderr
    by_name = {nm: (nm, cm, d) for nm, cm, d in files}
    listed = subprocess.run([CLI, "l", arc], capture_output=True, text=True).stdout.splitlines()
    order = [ln.split(" (")[0] for ln in listed[2:-2]]
    assert sorted(order) == sorted(by_name)
    assert open(arc, "rb").read() == solid_archive(2, [by_name[nm] for nm in order], 4)
    out = tmp_path / "out"
    r = subprocess.run([CLI, "x", arc, "-to", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and "Files extracted: %d" % len(files) in r.stdout, r.stderr
    for nm, _, d in files:
        assert (out / nm).read_bytes() == d
    # one 20 KiB file cut into 1 KiB pieces, eight pieces per block
    big = (INPUTS["text2k"] * 11)[:20480]
    (tmp_path / "big.txt").write_bytes(big)
    arc2 = str(tmp_path / "big.zpaq")
    r = subprocess.run([CLI, "a", arc2, str(tmp_path / "big.txt"), "-m2", "-fragment", "0", "-solid", "8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    pieces = [("big.txt", "20480 bytes", big[:1024])] + [("", "", big[o:o + 1024]) for o in range(1024, len(big), 1024)]
    assert open(arc2, "rb").read() == solid_archive(2, pieces, 8)
    r = subprocess.run([CLI, "l", arc2], capture_output=True, text=True)
    assert "big.txt (20480 bytes)" in r.stdout and "Total files: 1" in r.stdout
    r = subprocess.run([CLI, "x", arc2, "-to", str(tmp_path / "out2")], capture_output=True, text=True)
    assert r.returncode == 0 and (tmp_path / "out2" / "big.txt").read_bytes() == big
