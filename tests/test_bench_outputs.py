"""bench.py --dump-outputs: what the last timed step returned, as float32 / float64 .npy files of at most 64 MB in all.
The CPU test holds dump_outputs to a batch of known buffers; the GPU test holds a small plain run's files to the oracle."""
import json
import os
import subprocess
import sys
import types
import zlib

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(d):
    arrays = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values()), {k: a.dtype for k, a in arrays.items()}
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 * 10 ** 6
    return arrays


def test_dump_outputs_writes_what_the_step_returned(tmp_path):
    import torch
    nb, size = 300, 1000
    cap = int(size * 1.125) + 1024
    rng = np.random.default_rng(7)

    def i32(v):
        return torch.from_numpy(np.asarray(v, dtype=np.uint32).view(np.int32).copy())
    coded = rng.integers(0, 256, (nb, cap), dtype=np.uint8)
    dec = rng.integers(0, 256, (nb, size), dtype=np.uint8)
    clen = rng.integers(0, cap + 1, nb)
    dlen = np.full(nb, size)
    dlen[5] = 17
    code = rng.integers(0, 2 ** 32, nb, dtype=np.uint64)            # the final coder state is a full 32-bit value
    rb = types.SimpleNamespace(nb=nb, size=size, cap=cap, d_out=torch.from_numpy(coded.reshape(-1).copy()),
                               d_dec=torch.from_numpy(dec.reshape(-1).copy()), d_len=i32(clen), d_st=i32(np.zeros(nb)),
                               d_dlen=i32(dlen), d_cons=i32(clen + 3), d_code=i32(code), d_first=i32(np.zeros(nb)),
                               d_dst=i32(np.arange(nb) % 2))
    bench.dump_outputs(str(tmp_path), rb)
    a = _load(str(tmp_path))
    assert np.array_equal(a["coded_len"], clen) and np.array_equal(a["decode_consumed"], clen + 3)
    assert np.array_equal(a["decoded_len"], dlen) and np.array_equal(a["decode_final_code"], code)
    assert np.array_equal(a["decode_status"], np.arange(nb) % 2) and not a["encode_status"].any()
    assert a["coded_crc32"].tolist() == [zlib.crc32(coded[i, :clen[i]].tobytes()) for i in range(nb)]
    assert a["decoded_crc32"].tolist() == [zlib.crc32(dec[i, :dlen[i]].tobytes()) for i in range(nb)]
    sample = a["sample_blocks"].astype(int)
    assert len(sample) == 64 and len(set(sample)) == 64 and 0 <= sample.min() and sample.max() < nb
    for j, b in enumerate(sample):
        assert np.array_equal(a["coded_sample"][j, :clen[b]], coded[b, :clen[b]]) and not a["coded_sample"][j, clen[b]:].any()
        assert np.array_equal(a["decoded_sample"][j, :dlen[b]], dec[b, :dlen[b]]) and not a["decoded_sample"][j, dlen[b]:].any()
    again = tmp_path / "again"
    bench.dump_outputs(str(again), rb)
    assert all(np.array_equal(v, _load(str(again))[k]) for k, v in a.items())     # the sample is fixed


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_oracle_streams(tmp_path):
    """A plain run (no --full) times exactly --steps steps, stays lean, and dumps the coded streams the oracle writes."""
    import oracle_lib as O
    import workload as W
    nb = 64
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--blocks", str(nb), "--steps", "2",
                        "--warmup", "1", "--state-budget-gib", "24", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["roundtrip_bit_exact"]
    assert "roofline" not in line and "secondary" not in line and "cpu_baseline" not in line
    a = _load(str(tmp_path))
    blocks = [W.make_block(b, 65536).tobytes() for b in range(nb)]
    want = O.encode_blocks(O.level_header(2), blocks, nthreads=8)
    assert a["coded_len"].tolist() == [len(c) for c in want] and sum(map(len, want)) == line["coded_bytes"]
    assert a["coded_crc32"].tolist() == [zlib.crc32(c) for c in want]
    assert a["decoded_crc32"].tolist() == [zlib.crc32(b) for b in blocks]
    assert not a["encode_status"].any() and not a["decode_status"].any() and (a["decoded_len"] == 65536).all()
    for j, b in enumerate(a["sample_blocks"].astype(int)):
        assert a["coded_sample"][j, :len(want[b])].astype(np.uint8).tobytes() == want[b]
        assert a["decoded_sample"][j].astype(np.uint8).tobytes() == blocks[b]
