"""What a pause costs: a block set of a shipped chain model (or, --model C4B, of the all-nine-types general model) coded a
whole segment per call against the same data in chunk calls (zpq_blockset_{encode,decode}_chunks), kernel time from
zpq_ctx_last_kernel_ms, summed over the calls.
    python tools/set_chunks_bench.py [--level 2 | --model C4B] [--set-flags 0] [--members 4096] [--seg 65536] [--chunk 4096]
                                     [--arms shipped,parent] [--rounds 2] [--call-flags 129,0] [--out profiles/FILE.txt]
--set-flags: the ZPQ_SET_* the sets are created with (1: k_rows / k_lanes; 129: and their chunk calls; 0: a general model on the
lane-0 kernel, a launch per member).  Mode `one` always creates them without ZPQ_SET_CHUNKS (128): its whole-segment calls are the
same launches either way, and an arm other than `shipped` may not know the flag.
Modes, each sample a child process of its own under a time limit (the first that fails, faults or runs out of time ends the run):
  one      zpq_blockset_encode_segments + zpq_blockset_decode_segments, ONE call each for the members' one segment
  chunks   the same segments in seg / chunk encode_chunks calls and as many decode_chunks calls (+ the one that finds the EOF
           behind an exact fit), every decode call with a slab of `chunk` bytes
`one` runs for every arm in the balanced order of tools/ab_balanced.py (A B B A ...: consecutive processes on one box differ by
2-4 %, EXPERIMENTS R4.11), so that the KEEP kernels' prologue and epilogue, which chunked coding changed, can be held against a
library built from the parent commit (an arm other than `shipped` is zpaq-v_amd/lib/libzpaq_hip_<arm>.so, tools/variant.sh's
naming; such a library need not have the chunk calls).  `chunks` runs for `shipped`, once per round.  The coded streams of both
modes are compared inside the `chunks` process.
  call     --call-flags A,B: ONE encode_chunks call of `chunk` bytes (more = 1) and ONE decode_chunks call with a slab of `chunk`
           bytes on a set created with flags A, then the same on one created with B, wall-clock time of each call (a set on
           the lane-0 kernel is a launch per member: no one kernel time tells what the call cost); same coded bytes asserted"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT = 280                                            # seconds per child process


def offsets(np, lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(lengths, dtype=np.uint64))
    return off


def step(mode, level, M, seg, chunk, model_name="level", set_flags=0, call_flags=(129, 0)):
    import time
    import numpy as np
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    import workload as W
    for k in ("ZPQ_SET_PIPE", "ZPQ_SET_LANES"):
        os.environ.pop(k, None)
    z = ge.load()
    L = z.lib()
    ctx = z.Context(0)
    if model_name == "C4B":
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        from inputs import C4B
        model = z.Model(header=C4B)
    else:
        model = z.Model(level=level)

    def new_set(flags=None):
        f = set_flags if flags is None else flags
        return z.BlockSet(ctx, model, M, max_member_bytes=seg + 1, lanes=bool(f & 1), pipe=bool(f & 4), waves=bool(f & 16),
                          vmwaves=bool(f & 64), chunks=bool(f & 128))

    M = min(M, ctx.blockset_capacity(model, max_member_bytes=seg + 1, lanes=bool(set_flags & 1)))
    data = np.ascontiguousarray(W.make_blocks_fast(M, seg)).reshape(-1)     # classes b mod 4: zeros / uniform / order-1 text / periodic
    F = z.FLAG_PP
    grow = (lambda n: n * 17 + 4096) if model_name == "C4B" else (lambda n: n + n // 4 + 1024)   # (C4B expands uniform bytes more than threefold)
    cap = grow(seg)
    in_off, out_off = offsets(np, [seg] * M), offsets(np, [cap] * M)
    out = np.zeros(int(out_off[-1]) + 16, dtype=np.uint8)
    out_len, status = np.zeros(M, dtype=np.uint32), np.zeros(M, dtype=np.int32)
    res = dict(mode=mode, level=level, members=M, seg=seg, lib=os.environ.get("ZPQ_LIB_PATH", "shipped"))
    if model_name != "level":
        res.update(model=model_name, set_flags=set_flags)
        del res["level"]
    if mode == "call":
        # one chunk call per direction on a set of each of the two flag words; the coded piece comes from the first
        part = np.ascontiguousarray(data.reshape(M, seg)[:, :chunk]).reshape(-1)
        k_off, ko_off, dk_off = offsets(np, [chunk] * M), offsets(np, [grow(chunk)] * M), offsets(np, [chunk] * M)
        more, opened = np.ones(M, dtype=np.uint8), np.zeros(M, dtype=np.uint8)
        back = np.zeros(int(dk_off[-1]) + 16, dtype=np.uint8)
        r4 = [np.zeros(M, dtype=np.uint32) for _ in range(4)]
        pieces = None
        for f in call_flags:
            enc, dec = new_set(f), new_set(f)
            assert L.zpq_blockset_flags(enc.h) == f, (f, L.zpq_blockset_flags(enc.h))
            t0 = time.perf_counter()
            rc = L.zpq_blockset_encode_chunks(enc.h, M, None, part.ctypes.data, k_off.ctypes.data, F, more.ctypes.data, out.ctypes.data,
                                              ko_off.ctypes.data, out_len.ctypes.data, status.ctypes.data)
            t1 = time.perf_counter()
            assert rc == 0 and (status == 0).all(), (f, rc, status[:8])
            res["enc_call_ms_%d" % f], res["enc_kernel_%d" % f] = round((t1 - t0) * 1e3, 3), ctx.last_kernel_name
            got = [out[int(ko_off[i]):int(ko_off[i]) + int(out_len[i])].copy() for i in range(M)]
            if pieces is None:
                pieces = got
            assert all(np.array_equal(a, b) for a, b in zip(pieces, got)), "the two sets' coded pieces differ"
            # (the decoder's window: the piece and zeros behind it -- a chunk's own bytes do not end on a decodable boundary)
            wins = [np.concatenate([p, np.zeros(8, dtype=np.uint8)]) for p in pieces]
            w_off, w_src = offsets(np, [len(w) for w in wins]), np.concatenate(wins + [np.zeros(16, dtype=np.uint8)])
            dcap = offsets(np, [chunk // 2] * M)             # (half the piece: every byte asked for is in the window)
            t0 = time.perf_counter()
            rc = L.zpq_blockset_decode_chunks(dec.h, M, None, w_src.ctypes.data, w_off.ctypes.data, F, back.ctypes.data, dcap.ctypes.data,
                                              r4[0].ctypes.data, r4[1].ctypes.data, r4[2].ctypes.data, r4[3].ctypes.data,
                                              opened.ctypes.data, status.ctypes.data)
            t1 = time.perf_counter()
            assert rc == 0 and (status == 0).all() and opened.all() and (r4[0] == chunk // 2).all(), (f, rc, status[:8])
            res["dec_call_ms_%d" % f], res["dec_kernel_%d" % f] = round((t1 - t0) * 1e3, 3), ctx.last_kernel_name
            arr = data.reshape(M, seg)
            assert all(np.array_equal(back[int(dcap[i]):int(dcap[i]) + chunk // 2], arr[i, :chunk // 2]) for i in range(M))
            enc.close()
            dec.close()
        print("RESULT " + json.dumps(res), flush=True)
        ctx.close()
        return

    # ---- one call per direction
    enc, dec = new_set(set_flags & ~128), new_set(set_flags & ~128)
    rc = L.zpq_blockset_encode_segments(enc.h, M, None, data.ctypes.data, in_off.ctypes.data, F, out.ctypes.data,
                                        out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data)
    assert rc == 0 and (status == 0).all(), (rc, status[:8])
    res["enc_one_ms"], res["enc_kernel"] = round(ctx.last_kernel_ms, 3), ctx.last_kernel_name
    coded = [out[int(out_off[i]):int(out_off[i]) + int(out_len[i])].copy() for i in range(M)]
    c_off = offsets(np, [len(c) for c in coded])
    c_src = np.concatenate(coded + [np.zeros(16, dtype=np.uint8)])
    d_off = offsets(np, [seg + 8] * M)
    back = np.zeros(int(d_off[-1]) + 16, dtype=np.uint8)
    r4 = [np.zeros(M, dtype=np.uint32) for _ in range(4)]
    rc = L.zpq_blockset_decode_segments(dec.h, M, None, c_src.ctypes.data, c_off.ctypes.data, F, back.ctypes.data, d_off.ctypes.data,
                                        r4[0].ctypes.data, r4[1].ctypes.data, r4[2].ctypes.data, r4[3].ctypes.data, status.ctypes.data)
    assert rc == 0 and (status == 0).all() and (r4[0] == seg).all(), (rc, status[:8])
    res["dec_one_ms"], res["dec_kernel"] = round(ctx.last_kernel_ms, 3), ctx.last_kernel_name
    enc.close()
    dec.close()

    if mode == "chunks":
        enc, dec = new_set(), new_set()
        ncalls = seg // chunk
        assert ncalls * chunk == seg
        arr = data.reshape(M, seg)
        k_off, ko_off = offsets(np, [chunk] * M), offsets(np, [grow(chunk)] * M)
        more = np.ones(M, dtype=np.uint8)
        got = [[] for _ in range(M)]
        ms = []
        for k in range(ncalls):
            part = np.ascontiguousarray(arr[:, k * chunk:(k + 1) * chunk]).reshape(-1)
            rc = L.zpq_blockset_encode_chunks(enc.h, M, None, part.ctypes.data, k_off.ctypes.data, F,
                                              more.ctypes.data if k + 1 < ncalls else None, out.ctypes.data, ko_off.ctypes.data,
                                              out_len.ctypes.data, status.ctypes.data)
            assert rc == 0 and (status == 0).all(), (k, rc, status[:8])
            ms.append(ctx.last_kernel_ms)
            for i in range(M):
                got[i].append(out[int(ko_off[i]):int(ko_off[i]) + int(out_len[i])].copy())
        res["enc_chunks_ms"], res["enc_calls"], res["enc_chunk_kernel"] = round(sum(ms), 3), len(ms), ctx.last_kernel_name
        assert all(np.array_equal(np.concatenate(got[i]), coded[i]) for i in range(M)), "chunked and whole streams differ"
        # decode: a slab of `chunk` bytes per call, the window what the decoder may read for it (the rest of the stream at most)
        win = grow(chunk)
        pos = np.zeros(M, dtype=np.int64)
        dk_off = offsets(np, [chunk] * M)
        opened = np.zeros(M, dtype=np.uint8)
        plain = [[] for _ in range(M)]
        ms = []
        while True:
            parts = [coded[i][int(pos[i]):int(pos[i]) + win] for i in range(M)]
            w_off = offsets(np, [len(p) for p in parts])
            w_src = np.concatenate(parts + [np.zeros(16, dtype=np.uint8)])
            rc = L.zpq_blockset_decode_chunks(dec.h, M, None, w_src.ctypes.data, w_off.ctypes.data, F, back.ctypes.data, dk_off.ctypes.data,
                                              r4[0].ctypes.data, r4[1].ctypes.data, r4[2].ctypes.data, r4[3].ctypes.data,
                                              opened.ctypes.data, status.ctypes.data)
            assert rc == 0 and (status == 0).all(), (rc, status[:8])
            ms.append(ctx.last_kernel_ms)
            pos += r4[1]
            for i in range(M):
                plain[i].append(back[int(dk_off[i]):int(dk_off[i]) + int(r4[0][i])].copy())
            if not opened.any():
                break
            assert opened.all() and len(ms) <= ncalls + 1
        res["dec_chunks_ms"], res["dec_calls"], res["dec_chunk_kernel"] = round(sum(ms), 3), len(ms), ctx.last_kernel_name
        res["dec_last_call_ms"] = round(ms[-1], 3)           # (the call that only finds the EOF behind the exact fit)
        assert all(np.array_equal(np.concatenate(plain[i]), arr[i]) for i in range(M)), "chunked decode differs from the input"
        assert (pos == np.asarray([len(c) for c in coded])).all()
        enc.close()
        dec.close()
    print("RESULT " + json.dumps(res), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=2)
    ap.add_argument("--model", default="level", choices=("level", "C4B"), help="level: the shipped chain model of --level")
    ap.add_argument("--set-flags", type=int, default=0, help="ZPQ_SET_* of the sets (modes one and chunks)")
    ap.add_argument("--call-flags", default="", help="A,B: add one `call` step per round on sets of these two flag words")
    ap.add_argument("--members", type=int, default=4096)
    ap.add_argument("--seg", type=int, default=65536)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--arms", default="shipped")
    ap.add_argument("--rounds", type=int, default=2, help="passes over the arms (even: every arm in odd and even places)")
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="")
    a = ap.parse_args()
    if a.step:
        step(a.step, a.level, a.members, a.seg, a.chunk, a.model, a.set_flags,
             tuple(int(x) for x in a.call_flags.split(",")) if a.call_flags else (129, 0))
        return 0
    arms = a.arms.split(",")
    order = []
    for r in range(a.rounds):
        order += [(arm, "one") for arm in (arms if r % 2 == 0 else arms[::-1])] + [("shipped", "chunks")]
        if a.call_flags:
            order.append(("shipped", "call"))
    results, lines = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            open(a.out, "w").write("\n".join(lines) + "\n")

    say("# tools/set_chunks_bench.py %s --members %d --seg %d --chunk %d --arms %s --rounds %d%s" %
        ("--level %d" % a.level if a.model == "level" else "--model %s --set-flags %d" % (a.model, a.set_flags),
         a.members, a.seg, a.chunk, a.arms, a.rounds, " --call-flags " + a.call_flags if a.call_flags else ""))
    for arm, mode in order:
        env = dict(os.environ)
        env.pop("ZPQ_LIB_PATH", None)
        if arm != "shipped":
            env["ZPQ_LIB_PATH"] = os.path.join(ROOT, "zpaq-v_amd", "lib", "libzpaq_hip_%s.so" % arm)
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--step", mode, "--level", str(a.level),
               "--members", str(a.members), "--seg", str(a.seg), "--chunk", str(a.chunk), "--model", a.model,
               "--set-flags", str(a.set_flags)] + (["--call-flags", a.call_flags] if a.call_flags else [])
        p = subprocess.run(cmd, env=env, capture_output=True, text=True)
        for ln in p.stdout.splitlines():
            if ln.startswith("RESULT "):
                r = json.loads(ln[7:])
                r["arm"] = arm
                results.append(r)
                say("%-8s %-6s %s" % (arm, mode, json.dumps({k: v for k, v in r.items() if k not in ("lib", "arm", "mode")})))
        if p.returncode != 0:                               # a failure, a fault or the time limit: nothing more is started
            say("step %s %s ended with %d\n%s" % (arm, mode, p.returncode, p.stderr[-2000:]))
            return 1
    for arm in arms:
        for key in ("enc_one_ms", "dec_one_ms"):
            xs = [r[key] for r in results if r["arm"] == arm and r["mode"] == "one"]
            say("%-8s %-11s one call: mean %.2f  min %.2f  max %.2f  (n=%d)" % (arm, key, statistics.mean(xs), min(xs), max(xs), len(xs)))
    for r in results:
        if r["mode"] == "call":
            fa, fb = (int(x) for x in a.call_flags.split(","))
            say("one chunk call, %d members: encode %.2f ms (%s, flags %d) against %.2f ms (%s, flags %d), x%.1f; decode %.2f ms "
                "against %.2f ms, x%.1f" % (r["members"], r["enc_call_ms_%d" % fa], r["enc_kernel_%d" % fa], fa, r["enc_call_ms_%d" % fb],
                                           r["enc_kernel_%d" % fb], fb, r["enc_call_ms_%d" % fb] / r["enc_call_ms_%d" % fa],
                                           r["dec_call_ms_%d" % fa], r["dec_call_ms_%d" % fb],
                                           r["dec_call_ms_%d" % fb] / r["dec_call_ms_%d" % fa]))
        if r["mode"] == "chunks":
            say("chunks: encode %d calls %.2f ms against %.2f ms in one (x%.3f); decode %d calls %.2f ms against %.2f ms in one (x%.3f), "
                "its last call %.3f ms" % (r["enc_calls"], r["enc_chunks_ms"], r["enc_one_ms"], r["enc_chunks_ms"] / r["enc_one_ms"],
                                           r["dec_calls"], r["dec_chunks_ms"], r["dec_one_ms"], r["dec_chunks_ms"] / r["dec_one_ms"],
                                           r["dec_last_call_ms"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
