"""Solid archives with ZPQ_SET_PIPE=1: the sets archive_add and `zpaqv a -solid N` create follow the variable, so a round of
fifteen blocks is coded by the wave-pipelined encoder (k_pipe<..., KEEP>) instead of k_chain<encode>.  The archive is the
same, byte for byte, and extraction (k_chain<decode>) returns every file."""
import os
import random
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_archive import CLI  # noqa: E402
from test_gpu_solid_archive import solid_archive, triples  # noqa: E402

pytestmark = pytest.mark.gpu

SOLID = 4


@pytest.fixture(scope="module")
def files():
    """Sixty files of 0-3000 bytes (zeros / random / text / periodic): fifteen blocks of four, so fifteen members per round."""
    r = random.Random(60)
    out = []
    for i in range(60):
        n = 0 if i == 7 else r.choice([1, 2, 9, 17, 64, 65, 300, 1000, 2048, 3000])
        kind = i % 4
        if kind == 0:
            d = bytes(n)
        elif kind == 1:
            d = bytes(r.getrandbits(8) for _ in range(n))
        elif kind == 2:
            d = bytes(r.choice(b"etaoin shrdlu\n") for _ in range(n))
        else:
            d = (b"abcabcabd" * (n // 9 + 1))[:n]
        out.append(("f%02d.bin" % i, "%d bytes" % n, d))
    return out


@pytest.fixture()
def env(monkeypatch):
    for k in ("ZPQ_SET_PIPE", "ZPQ_SET_LANES", "ZPQ_ENC_PIPE", "ZPQ_ENC_SPLIT", "ZPQ_SPARSE_MODE", "ZPQ_SPARSE_FORCE_LOG2"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.mark.parametrize("level", [1, 2, 3])
def test_the_archive_is_the_same_and_extracts(zpq, gpu_ctx, env, files, level):
    plain = zpq.archive_add(gpu_ctx, level, files, solid=SOLID)
    assert gpu_ctx.last_kernel_name == "k_chain<encode>"
    env.setenv("ZPQ_SET_PIPE", "1")
    piped = zpq.archive_add(gpu_ctx, level, files, solid=SOLID)
    assert gpu_ctx.last_kernel_name == "k_pipe<encode>"
    assert piped == plain == solid_archive(level, files, SOLID)
    got = zpq.archive_extract(gpu_ctx, piped)
    assert gpu_ctx.last_kernel_name == "k_chain<decode>"
    assert triples(got) == files
    assert all(g["sha1_ok"] and g["status"] == 0 for g in got)
    env.setenv("ZPQ_SET_PIPE", "0")
    assert zpq.archive_add(gpu_ctx, level, files, solid=SOLID) == plain
    assert gpu_ctx.last_kernel_name == "k_chain<encode>"


def test_cli_round_trips_under_the_variable(tmp_path, files):
    """The round trip only: the command-line tool does not say which encoder ran, so this case would also pass if it ignored the
    variable.  That the sets archive_add creates follow it is what the test above asserts through the kernel's name."""
    src = tmp_path / "in"
    src.mkdir()
    for nm, _, d in files:
        (src / nm).write_bytes(d)
    arc = str(tmp_path / "arc.zpaq")
    env = dict(os.environ, ZPQ_SET_PIPE="1")
    for k in ("ZPQ_ENC_PIPE", "ZPQ_SPARSE_MODE", "ZPQ_SPARSE_FORCE_LOG2"):
        env.pop(k, None)
    r = subprocess.run([CLI, "a", arc, str(src), "-m2", "-solid", str(SOLID)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "Files added: %d" % len(files) in r.stdout, r.stderr
    by_name = {nm: (nm, cm, d) for nm, cm, d in files}
    listed = subprocess.run([CLI, "l", arc], capture_output=True, text=True, env=env).stdout.splitlines()
    order = [ln.split(" (")[0] for ln in listed[2:-2]]
    assert sorted(order) == sorted(by_name)
    assert open(arc, "rb").read() == solid_archive(2, [by_name[nm] for nm in order], SOLID)
    out = tmp_path / "out"
    r = subprocess.run([CLI, "x", arc, "-to", str(out)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "Files extracted: %d" % len(files) in r.stdout, r.stderr
    for nm, _, d in files:
        assert (out / nm).read_bytes() == d
