"""Block sets of the shipped chain models, encode: the default route (k_chain<encode, KEEP>) against the ZPQ_SET_PIPE route
(k_pipe<..., KEEP>), and for scale a plain single-segment batch of as many fresh blocks on the pipeline (k_pipe / k_pipe2:
what load + save cost on top of the byte loop, and what dense level 1 leaves on the table without split stages).
    python tools/set_pipe_bench.py [--levels 1,2,3,5] [--members 512,4096] [--out profiles/FILE.json]
Sets of M members x 4 rounds x 4 KiB segments of tests/workload.py's generator (M is cut to the set's capacity where that is
smaller).  Per round: the wall time of zpq_blockset_encode_segments (host pointers in and out, so transfers and the host's
packing are in it) and zpq_ctx_last_kernel_ms.  Routes a (default) and b (ZPQ_SET_PIPE) run in one process in the order
a b and in another in the order b a, their streams compared (process-to-process variation on one box is 2-4 %, EXPERIMENTS
R4.11); route c follows them in both.  Every step is a child process of its own under a time limit, and the first step that
fails, faults or runs out of time ends the run."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, SEG = 4, 4096
STEP_LIMIT = 240                                            # seconds per child process


def offsets(np, lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(lengths, dtype=np.uint64))
    return off


def run_route(z, np, ctx, model, route, data):
    """One route over all rounds.  data[r]: M x SEG bytes.  Returns (result dict, coded streams per round)."""
    M = data[0].shape[0]
    L = z.lib()
    F = z.FLAG_PP
    cap = SEG + SEG // 4 + 1024
    in_off, out_off = offsets(np, [SEG] * M), offsets(np, [cap] * M)
    out = np.zeros(int(out_off[-1]) + 16, dtype=np.uint8)
    out_len, status = np.zeros(M, dtype=np.uint32), np.zeros(M, dtype=np.int32)
    res = dict(route=route, members=M, enc_wall_ms=[], enc_kernel_ms=[])
    coded = []
    st = None
    t0 = time.perf_counter()
    if route in "ab":
        st = z.BlockSet(ctx, model, M, max_member_bytes=ROUNDS * (SEG + 1), pipe=route == "b")
        assert st.pipe == (route == "b")
    res["create_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    for r in range(ROUNDS):
        src = np.ascontiguousarray(data[r]).reshape(-1)
        t0 = time.perf_counter()
        if st:
            rc = L.zpq_blockset_encode_segments(st.h, M, None, src.ctypes.data, in_off.ctypes.data, F, out.ctypes.data,
                                                out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data)
        else:
            rc = L.zpq_encode_blocks(ctx.h, model.h, M, src.ctypes.data, in_off.ctypes.data, F, out.ctypes.data,
                                     out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data)
        res["enc_wall_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
        res["enc_kernel_ms"].append(round(ctx.last_kernel_ms, 3))
        res["enc_kernel"] = ctx.last_kernel_name
        res["line_store"] = ctx.last_line_store
        assert rc == 0 and (status == 0).all(), (rc, status[:8])
        coded.append([out[int(out_off[i]):int(out_off[i]) + int(out_len[i])].tobytes() for i in range(M)])
    if st:
        st.close()
    res["enc_wall_ms_per_round"] = round(sum(res["enc_wall_ms"]) / ROUNDS, 3)
    res["enc_kernel_ms_per_round"] = round(sum(res["enc_kernel_ms"]) / ROUNDS, 3)
    res["coded_bytes"] = sum(len(s) for rnd in coded for s in rnd)
    return res, coded


def step(level, M, order):
    """A child process: the routes of `order` one after the other on one context."""
    import numpy as np
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    import workload as W
    os.environ.pop("ZPQ_SET_PIPE", None)
    z = ge.load()
    ctx = z.Context(0)
    model = z.Model(level=level)
    M = min(M, ctx.blockset_capacity(model, max_member_bytes=ROUNDS * (SEG + 1)))
    arr = W.make_blocks_fast(M * ROUNDS, SEG)               # classes b mod 4: zeros / uniform / order-1 text / periodic
    data = [arr[r * M:(r + 1) * M] for r in range(ROUNDS)]
    first = None
    for route in order:
        res, coded = run_route(z, np, ctx, model, route, data)
        if route != "c":                                    # (route c: every round a batch of fresh blocks, streams of its own)
            if first is None:
                first = coded
            else:
                assert coded == first, "routes a and b wrote different streams"
        res.update(level=level, order=order)
        print("RESULT " + json.dumps(res), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", default="1,2,3,5")
    ap.add_argument("--members", default="512,4096")
    ap.add_argument("--out", default="")
    ap.add_argument("--step", nargs=3, metavar=("LEVEL", "M", "ORDER"))
    a = ap.parse_args()
    if a.step:
        step(int(a.step[0]), int(a.step[1]), a.step[2])
        return 0
    results = []
    for level in a.levels.split(","):
        for M in a.members.split(","):
            for order in ("abc", "bac"):
                cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--step", level, M, order]
                p = subprocess.run(cmd, capture_output=True, text=True)
                for ln in p.stdout.splitlines():
                    if ln.startswith("RESULT "):
                        results.append(json.loads(ln[7:]))
                        print(ln[7:], flush=True)
                if a.out:
                    with open(a.out, "w") as f:
                        json.dump(results, f, indent=1)
                if p.returncode != 0:                       # a failure, a fault or the time limit: nothing more is started
                    print("step %s %s %s ended with %d\n%s" % (level, M, order, p.returncode, p.stderr[-2000:]), flush=True)
                    return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
