"""Block sets of general models whose HCOMP program is not the shipped hash chain on the interpreter-wave kernels: (a)
ZPQ_SET_LANES alone (k_rows<..., KEEP>, the route such a set had before), (b) with ZPQ_SET_VMWAVES (k_vset / k_vsetd), and for
scale (c) a plain batch of as many fresh blocks on k_vpipe / k_vdec under ZPQ_FLAG_VMPIPE (what the slot map, load and save
cost on top of the byte loops, and what k_set_init saves).  The method is tools/set_waves_bench.py's.
    python tools/set_vmwaves_bench.py [--models C4B_VM,loop_count] [--members 16,512,4096] [--reps 3] [--out profiles/FILE.json]
C4B_VM: C4b's components behind `a=a` and their own hash chain (the contexts of C4b, from the interpreter); loop_count: the same
components behind zpaql_programs.NAMED["loop_count"], 1 to 16 interpreter loop iterations per byte.
Sets of M members x 4 rounds x 4 KiB segments (tests/workload.py's classes: zeros / uniform / order-1 text / periodic), encode
and decode, every round decoded back and compared.  Per round: the wall time of the library call (host pointers in and out, so
transfers and the host's packing are in it; the call ends in a stream synchronise) and zpq_ctx_last_kernel_ms (device events
around the launch).  Every arm is warmed up on a two-member set first (code objects load at the first launch), then runs
`reps` times on fresh sets; the figures are per-round means, the median over the repetitions, all repetitions kept.  Arms a
and b run in one process in the order a b (then c) and in a second process in the order b a -- process-to-process variation
on one box is 2-4 % (EXPERIMENTS R4.11) -- and their coded streams are compared: they must be equal.  Every step is a child
process of its own under a time limit, and the first step that fails, faults or runs out of time ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, SEG = 4, 4096
STEP_LIMIT = 240                                            # seconds per child process
KERNELS = {"a": ("k_rows<encode>", "k_rows<decode>"), "b": ("k_vset<encode>", "k_vsetd<decode>"),
           "c": ("k_vpipe<encode>", "k_vdec<decode>")}


def header_of(name):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import vpipe_models as VM
    import zpaql_programs as ZP
    if name == "C4B_VM":
        return VM.C4B_VM
    return VM.c4b_with(lambda n: list(ZP.assemble(ZP.NAMED[name], n)))


def offsets(np, lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(lengths, dtype=np.uint64))
    return off


def run_arm(z, np, ctx, model, arm, data):
    """One arm over all rounds, both directions.  data[r]: M x SEG bytes.  Returns (per-round timings, coded streams per round)."""
    M = data[0].shape[0]
    L = z.lib()
    F = z.FLAG_PP | (z.FLAG_VMPIPE if arm == "c" else 0)
    cap = SEG * 17 + 4096                                   # (C4B expands uniform bytes more than threefold)
    in_off, out_off = offsets(np, [SEG] * M), offsets(np, [cap] * M)
    out = np.zeros(int(out_off[-1]) + 16, dtype=np.uint8)
    out_len, status = np.zeros(M, dtype=np.uint32), np.zeros(M, dtype=np.int32)
    u = [np.zeros(M, dtype=np.uint32) for _ in range(3)]
    res = dict(enc_wall_ms=[], enc_kernel_ms=[], dec_wall_ms=[], dec_kernel_ms=[])
    coded = []
    sets = None
    t0 = time.perf_counter()
    if arm in "ab":
        sets = [z.BlockSet(ctx, model, M, lanes=True, vmwaves=arm == "b") for _ in range(2)]
        assert sets[0].lanes and sets[0].vmwaves == (arm == "b") and sets[1].vmwaves == (arm == "b")
    res["create_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    for r in range(ROUNDS):
        src = np.ascontiguousarray(data[r]).reshape(-1)
        t0 = time.perf_counter()
        if sets:
            rc = L.zpq_blockset_encode_segments(sets[0].h, M, None, src.ctypes.data, in_off.ctypes.data, F, out.ctypes.data,
                                                out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data)
        else:
            rc = L.zpq_encode_blocks(ctx.h, model.h, M, src.ctypes.data, in_off.ctypes.data, F, out.ctypes.data,
                                     out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data)
        res["enc_wall_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
        res["enc_kernel_ms"].append(round(ctx.last_kernel_ms, 3))
        assert ctx.last_kernel_name == KERNELS[arm][0], (arm, ctx.last_kernel_name)
        assert rc == 0 and (status == 0).all(), (rc, status[:8])
        coded.append([out[int(out_off[i]):int(out_off[i]) + int(out_len[i])].tobytes() for i in range(M)])
    for r in range(ROUNDS):
        cin = np.frombuffer(b"".join(coded[r]) + bytes(16), dtype=np.uint8)
        c_off = offsets(np, [len(s) for s in coded[r]])
        t0 = time.perf_counter()
        if sets:
            rc = L.zpq_blockset_decode_segments(sets[1].h, M, None, cin.ctypes.data, c_off.ctypes.data, F, out.ctypes.data,
                                                out_off.ctypes.data, out_len.ctypes.data, u[0].ctypes.data, u[1].ctypes.data,
                                                u[2].ctypes.data, status.ctypes.data)
        else:
            rc = L.zpq_decode_blocks(ctx.h, model.h, M, cin.ctypes.data, c_off.ctypes.data, F, out.ctypes.data,
                                     out_off.ctypes.data, out_len.ctypes.data, u[0].ctypes.data, u[1].ctypes.data,
                                     u[2].ctypes.data, status.ctypes.data)
        res["dec_wall_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
        res["dec_kernel_ms"].append(round(ctx.last_kernel_ms, 3))
        assert ctx.last_kernel_name == KERNELS[arm][1], (arm, ctx.last_kernel_name)
        assert rc == 0 and (status == 0).all() and (out_len == SEG).all(), (rc, status[:8], out_len[:8])
        got = np.stack([out[int(out_off[i]):int(out_off[i]) + SEG] for i in range(M)])
        assert (got == data[r]).all(), ("round trip", arm, r)          # every member of every round decoded back
    for s in sets or []:
        s.close()
    return res, coded


def step(model_name, M, order, reps):
    """A child process: the arms of `order` one after the other on one context."""
    import numpy as np
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    import workload as W
    for k in ("ZPQ_SET_LANES", "ZPQ_SET_WAVES", "ZPQ_SET_VMWAVES", "ZPQ_VM_PIPE", "ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE", "ZPQ_LANES_ROWS", "ZPQ_GPIPE_BATCH", "ZPQ_GDEC_BPW"):
        os.environ.pop(k, None)
    z = ge.load()
    ctx = z.Context(0)
    model = z.Model(header=header_of(model_name))
    arr = W.make_blocks_fast(M * ROUNDS, SEG)               # classes b mod 4: zeros / uniform / order-1 text / periodic
    data = [arr[r * M:(r + 1) * M] for r in range(ROUNDS)]
    warm = [arr[r * 2:r * 2 + 2] for r in range(ROUNDS)]
    first = None
    for arm in order:
        run_arm(z, np, ctx, model, arm, warm)               # warm-up: code objects, the pool's first allocation
        runs = []
        for _ in range(reps):
            res, coded = run_arm(z, np, ctx, model, arm, data)
            runs.append(res)
            if arm != "c":                                  # (c: every round a batch of fresh blocks, its streams are its own)
                if first is None:
                    first = coded
                else:
                    assert coded == first, "arms a and b wrote different streams"
        out = dict(model=model_name, members=M, order=order, arm=arm, enc_kernel=KERNELS[arm][0], dec_kernel=KERNELS[arm][1], runs=runs)
        for k in ("enc_wall_ms", "enc_kernel_ms", "dec_wall_ms", "dec_kernel_ms"):
            out[k + "_per_round"] = round(statistics.median(sum(r[k]) / ROUNDS for r in runs), 3)
        out["streams_equal"] = len(order.replace("c", "")) == 2 and arm != "c" and first is not None
        print("RESULT " + json.dumps(out), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="C4B_VM,loop_count")
    ap.add_argument("--members", default="16,512,4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", nargs=3, metavar=("MODEL", "M", "ORDER"))
    a = ap.parse_args()
    if a.step:
        step(a.step[0], int(a.step[1]), a.step[2], a.reps)
        return 0
    results = []
    for name in a.models.split(","):
        for M in [int(x) for x in a.members.split(",")]:
            for order in ("abc", "ba"):
                cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps),
                       "--step", name, str(M), order]
                p = subprocess.run(cmd, capture_output=True, text=True)
                for ln in p.stdout.splitlines():
                    if ln.startswith("RESULT "):
                        results.append(json.loads(ln[7:]))
                        r = results[-1]
                        print("%-7s M=%-5d %-3s %s  enc %9.3f ms wall %9.3f kernel   dec %9.3f wall %9.3f kernel" % (
                            r["model"], r["members"], r["order"], r["arm"], r["enc_wall_ms_per_round"], r["enc_kernel_ms_per_round"],
                            r["dec_wall_ms_per_round"], r["dec_kernel_ms_per_round"]), flush=True)
                if a.out:
                    with open(a.out, "w") as f:
                        json.dump(results, f, indent=1)
                if p.returncode != 0:                       # a failure, a fault or the time limit: nothing more is started
                    print("step %s %d %s ended with %d\n%s" % (name, M, order, p.returncode, p.stderr[-2000:]), flush=True)
                    return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
