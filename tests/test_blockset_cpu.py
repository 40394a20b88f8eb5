"""Block sets and solid archives, the part that needs no GPU: the argument checks of zpq_blockset_* (NULL and ctx-less
calls are ZPQ_E_ARG, never a crash), and the exports the header declares (tests/test_abi_cpu.py checks every name)."""
import ctypes as C

E_ARG = -2


def test_blockset_calls_without_a_ctx_are_argument_errors(zpq):
    L = zpq.lib()
    model = zpq.Model(level=2)
    out = C.c_void_p(1)
    assert L.zpq_blockset_create(None, model.h, 4, 0, C.byref(out)) == E_ARG and not out.value
    assert L.zpq_blockset_create(None, model.h, 4, 0, None) == E_ARG
    assert L.zpq_blockset_create(None, None, 4, 0, C.byref(out)) == E_ARG
    assert L.zpq_blockset_capacity(None, model.h, 0) == E_ARG
    off = (C.c_uint64 * 2)(0, 0)
    u = (C.c_uint32 * 1)()
    st = (C.c_int32 * 1)()
    assert L.zpq_blockset_encode_segments(None, 1, None, None, off, 1, None, off, u, st) == E_ARG
    assert L.zpq_blockset_decode_segments(None, 1, None, None, off, 1, None, off, u, None, None, None, st) == E_ARG
    L.zpq_blockset_destroy(None)                           # a no-op
    model.close()


# ---------------------------------------------------------------- solid archives at level 0 (the host Compressor, no coder)
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_archive import CLI, file_set  # noqa: E402


def sequential_solid(zpq, ctx, level, files, solid):
    """The same layout through the sequential front end: `solid` files per block, a segment each."""
    out = b""
    for i in range(0, len(files), solid):
        c = zpq.Compressor(ctx)
        c.start_block(level)
        for nm, cm, d in files[i:i + solid]:
            c.start_segment(nm, cm)
            c.set_input(d)
            while c.compress(65536):
                pass
            c.end_segment()
        c.end_block()
        out += c.output_bytes()
    return out


def test_store_mode_solid_archive_equals_the_sequential_compressor(zpq):
    files = file_set(n=5)                                   # 11 files: blocks of 3, 3, 3, 2
    arc = zpq.archive_add(None, 0, files, solid=3)
    assert arc == sequential_solid(zpq, None, 0, files, 3)
    assert arc != zpq.archive_add(None, 0, files)
    assert zpq.archive_add(None, 0, files, solid=1) == zpq.archive_add(None, 0, files) == zpq.archive_add(None, 0, files, solid=0)
    got = zpq.archive_extract(None, arc)
    assert [(g["name"], g["comment"], g["data"]) for g in got] == files
    assert all(g["sha1_ok"] and g["status"] == 0 for g in got)


def test_cli_store_mode_solid_round_trip(tmp_path):
    files = file_set(n=4)
    src = tmp_path / "in"
    src.mkdir()
    for nm, _, d in files:
        (src / nm).write_bytes(d)
    arc = str(tmp_path / "arc")
    r = subprocess.run([CLI, "a", arc, str(src), "-m0", "-solid", "3"], capture_output=True, text=True)
    assert r.returncode == 0 and "Files added: %d" % len(files) in r.stdout, r.stderr
    r = subprocess.run([CLI, "l", arc], capture_output=True, text=True)
    assert "Total files: %d" % len(files) in r.stdout, r.stdout
    out = tmp_path / "out"
    r = subprocess.run([CLI, "x", arc, "-to", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and "Files extracted: %d" % len(files) in r.stdout, r.stderr
    for nm, _, d in files:
        assert (out / nm).read_bytes() == d
    one = str(tmp_path / "one")
    assert subprocess.run([CLI, "a", one, str(src), "-m0"], capture_output=True).returncode == 0
    assert os.path.getsize(arc + ".zpaq") < os.path.getsize(one + ".zpaq")      # fewer block headers


def test_cli_rejects_a_bad_solid_value(tmp_path):
    (tmp_path / "f").write_bytes(b"abc")
    for bad in ("0", "x", "-3"):
        r = subprocess.run([CLI, "a", str(tmp_path / "arc"), str(tmp_path / "f"), "-m0", "-solid", bad], capture_output=True, text=True)
        assert r.returncode == 1 and "-solid" in r.stderr, (bad, r.stderr)
    r = subprocess.run([CLI, "a", str(tmp_path / "arc"), str(tmp_path / "f"), "-m0", "-solid"], capture_output=True, text=True)
    assert r.returncode == 1
    assert "-solid N" in subprocess.run([CLI, "help"], capture_output=True, text=True).stdout
