"""Block sets of general models: the default route (k_generic, a launch per member and round) against the ZPQ_SET_LANES
route (k_rows / k_lanes<..., KEEP>, a launch per round), and for scale a plain single-segment batch of as many blocks on
k_rows / k_lanes (what load + save cost on top of the byte loop).
    python tools/set_lanes_bench.py [--models C4B,n17] [--max-small 64] [--large 4096] [--out profiles/FILE.json]
Sets of M members x 4 rounds x 4 KiB segments, encode and decode.  The small M is chosen per model: a set of ONE member is
timed on the default route first, and M is the largest power of two (4 .. --max-small) at which that route's eight rounds
stay below ROUTE_A_BUDGET seconds; the large M is given to routes b and c only.  Per round: the wall time of the library call (host
pointers in and out, so transfers and the host's packing are in it) and zpq_ctx_last_kernel_ms (the last launch only: one
member's on the default route).  Routes a and b alternate in one process, in both orders (process-to-process variation
on one box is 2-4 %, EXPERIMENTS R4.11); every step is a child process of its own under a time limit, and the first step
that fails, faults or runs out of time ends the run."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, SEG = 4, 4096
ROUTE_A_BUDGET = 45                                         # seconds route a's 2 x 4 rounds may take: M follows from it
STEP_LIMIT = 180                                            # seconds per child process (route a, route b or c, start-up)


def header_of(name):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    if name == "C4B":
        from inputs import C4B
        return C4B
    import general_models as GM
    return GM.NAMED[name][0]


def offsets(np, lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(lengths, dtype=np.uint64))
    return off


def run_route(z, np, ctx, model, route, data, coded_in):
    """One route over all rounds, both directions.  data[r]: M x SEG bytes.  Returns (result dict, coded streams per round)."""
    M = data[0].shape[0]
    L = z.lib()
    F = z.FLAG_PP
    cap = SEG * 17 + 4096                                   # (C4B expands uniform bytes more than threefold)
    in_off, out_off = offsets(np, [SEG] * M), offsets(np, [cap] * M)
    out = np.zeros(int(out_off[-1]) + 16, dtype=np.uint8)
    out_len, status = np.zeros(M, dtype=np.uint32), np.zeros(M, dtype=np.int32)
    u = [np.zeros(M, dtype=np.uint32) for _ in range(3)]
    res = dict(route=route, members=M, enc_wall_ms=[], enc_kernel_ms=[], dec_wall_ms=[], dec_kernel_ms=[])
    coded = []
    sets = None
    t0 = time.perf_counter()
    if route in "ab":
        sets = [z.BlockSet(ctx, model, M, lanes=route == "b") for _ in range(2)]
        assert sets[0].lanes == (route == "b")
    res["create_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    for r in range(ROUNDS):
        src = np.ascontiguousarray(data[r]).reshape(-1)
        t0 = time.perf_counter()
        if sets:
            rc = L.zpq_blockset_encode_segments(sets[0].h, M, None, src.ctypes.data, in_off.ctypes.data, F, out.ctypes.data,
                                                out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data)
        else:
            rc = L.zpq_encode_blocks(ctx.h, model.h, M, src.ctypes.data, in_off.ctypes.data, F | z.FLAG_LANES, out.ctypes.data,
                                     out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data)
        res["enc_wall_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
        res["enc_kernel_ms"].append(round(ctx.last_kernel_ms, 3))
        res["enc_kernel"] = ctx.last_kernel_name
        assert rc == 0 and (status == 0).all(), (rc, status[:8])
        coded.append([out[int(out_off[i]):int(out_off[i]) + int(out_len[i])].tobytes() for i in range(M)])
    for r in range(ROUNDS):
        streams = coded_in[r] if coded_in else coded[r]
        cin = np.frombuffer(b"".join(streams) + bytes(16), dtype=np.uint8)
        c_off = offsets(np, [len(s) for s in streams])
        t0 = time.perf_counter()
        if sets:
            rc = L.zpq_blockset_decode_segments(sets[1].h, M, None, cin.ctypes.data, c_off.ctypes.data, F, out.ctypes.data,
                                                out_off.ctypes.data, out_len.ctypes.data, u[0].ctypes.data, u[1].ctypes.data,
                                                u[2].ctypes.data, status.ctypes.data)
        else:
            rc = L.zpq_decode_blocks(ctx.h, model.h, M, cin.ctypes.data, c_off.ctypes.data, F | z.FLAG_LANES, out.ctypes.data,
                                     out_off.ctypes.data, out_len.ctypes.data, u[0].ctypes.data, u[1].ctypes.data,
                                     u[2].ctypes.data, status.ctypes.data)
        res["dec_wall_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
        res["dec_kernel_ms"].append(round(ctx.last_kernel_ms, 3))
        res["dec_kernel"] = ctx.last_kernel_name
        assert rc == 0 and (status == 0).all() and (out_len == SEG).all(), (rc, status[:8], out_len[:8])
        for i in (0, M // 2, M - 1):
            assert out[int(out_off[i]):int(out_off[i]) + SEG].tobytes() == data[r][i].tobytes(), ("round trip", route, r, i)
    for s in sets or []:
        s.close()
    for k in ("enc", "dec"):
        res[k + "_wall_ms_per_round"] = round(sum(res[k + "_wall_ms"]) / ROUNDS, 3)
    return res, coded


def step(model_name, M, order):
    """A child process: the routes of `order` one after the other on one context."""
    import numpy as np
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    import workload as W
    os.environ.pop("ZPQ_SET_LANES", None)
    os.environ["ZPQ_ENC_GPIPE"] = "0"                       # route c: the lane-per-component kernels, not the wave pipelines
    os.environ["ZPQ_DEC_GPIPE"] = "0"
    z = ge.load()
    ctx = z.Context(0)
    model = z.Model(header=header_of(model_name))
    arr = W.make_blocks_fast(M * ROUNDS, SEG)               # classes b mod 4: zeros / uniform / order-1 text / periodic
    data = [arr[r * M:(r + 1) * M] for r in range(ROUNDS)]
    first = None
    for route in order:
        if route == "c":                                    # every round a batch of fresh blocks: its streams are its own
            res, _ = run_route(z, np, ctx, model, route, data, None)
        else:
            res, coded = run_route(z, np, ctx, model, route, data, None)
            if first is None:
                first = coded
            else:
                assert coded == first, "routes a and b wrote different streams"
        res.update(model=model_name, order=order)
        print("RESULT " + json.dumps(res), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="C4B,n17")
    ap.add_argument("--max-small", type=int, default=64)
    ap.add_argument("--large", type=int, default=4096)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", nargs=3, metavar=("MODEL", "M", "ORDER"))
    a = ap.parse_args()
    if a.step:
        step(a.step[0], int(a.step[1]), a.step[2])
        return 0
    results = []
    for name in a.models.split(","):
        small = 0
        # (the first step times one member on the default route; the small M of the others follows from it)
        for M, order in ((1, "a"), (0, "ab"), (0, "ba"), (0, "bc"), (a.large, "cb"), (a.large, "bc")):
            M = M or small
            cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--step", name, str(M), order]
            p = subprocess.run(cmd, capture_output=True, text=True)
            for ln in p.stdout.splitlines():
                if ln.startswith("RESULT "):
                    results.append(json.loads(ln[7:]))
                    print(ln[7:], flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(results, f, indent=1)
            if p.returncode != 0:                           # a failure, a fault or the time limit: nothing more is started
                print("step %s %d %s ended with %d\n%s" % (name, M, order, p.returncode, p.stderr[-2000:]), flush=True)
                return 1
            if order == "a":
                one = results[-1]
                per_member_s = (sum(one["enc_wall_ms"]) + sum(one["dec_wall_ms"])) / 1e3     # its eight rounds
                small = 4
                while small * 2 <= a.max_small and small * 2 * per_member_s <= ROUTE_A_BUDGET:
                    small *= 2
                print("%s: one member takes %.2f s on the default route: M = %d" % (name, per_member_s, small), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
