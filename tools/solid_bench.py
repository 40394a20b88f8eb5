"""Solid archives against one block per file, end to end (host buffers in, archive bytes out; PCIe, framing and SHA-1
included): add / extract MB/s and archive size for `solid` files per block.
    python tools/solid_bench.py [files=8192] [file bytes=4096] [level=2] [solid=16]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import workload as W  # noqa: E402

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
size = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
level = int(sys.argv[3]) if len(sys.argv) > 3 else 2
solid = int(sys.argv[4]) if len(sys.argv) > 4 else 16
z = ge.load()
ctx = z.Context(0)
arr = W.make_blocks_fast(nb, size)                       # classes b mod 4: zeros / uniform / order-1 text / periodic
files = [("f%05d" % i, "%d bytes" % size, arr[i].tobytes()) for i in range(nb)]
total = nb * size
for n in (1, solid):
    best = None
    for rep in range(2):
        t0 = time.time()
        arc = z.archive_add(ctx, level, files, solid=n)
        t1 = time.time()
        out = z.archive_extract(ctx, arc)
        t2 = time.time()
        dec_kernel = ctx.last_kernel_name
        ok = len(out) == nb and all(o["data"] == f[2] and o["sha1_ok"] and o["status"] == 0 for o, f in zip(out, files))
        r = dict(workload="%d files x %d B, level %d" % (nb, size, level), files_per_block=n, archive_bytes=len(arc),
                 ratio=round(len(arc) / total, 4), add_s=round(t1 - t0, 3), add_MBps=round(total / (t1 - t0) / 1e6, 1),
                 extract_s=round(t2 - t1, 3), extract_MBps=round(total / (t2 - t1) / 1e6, 1), last_decode_kernel=dec_kernel,
                 roundtrip_ok=ok)
        if best is None or r["add_s"] + r["extract_s"] < best["add_s"] + best["extract_s"]:
            best = r
    print(json.dumps(best), flush=True)
ctx.close()
