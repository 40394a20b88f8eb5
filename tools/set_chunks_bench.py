"""What a pause costs: a block set of a shipped chain model coded a whole segment per call against the same data in chunk calls
(zpq_blockset_{encode,decode}_chunks), kernel time from zpq_ctx_last_kernel_ms, summed over the calls.
    python tools/set_chunks_bench.py [--level 2] [--members 4096] [--seg 65536] [--chunk 4096] [--arms shipped,parent]
                                     [--rounds 2] [--out profiles/FILE.txt]
Modes, each sample a child process of its own under a time limit (the first that fails, faults or runs out of time ends the run):
  one      zpq_blockset_encode_segments + zpq_blockset_decode_segments, ONE call each for the members' one segment
  chunks   the same segments in seg / chunk encode_chunks calls and as many decode_chunks calls (+ the one that finds the EOF
           behind an exact fit), every decode call with a slab of `chunk` bytes
`one` runs for every arm in the balanced order of tools/ab_balanced.py (A B B A ...: consecutive processes on one box differ by
2-4 %, EXPERIMENTS R4.11), so that the KEEP kernels' prologue and epilogue, which chunked coding changed, can be held against a
library built from the parent commit (an arm other than `shipped` is zpaq-v_amd/lib/libzpaq_hip_<arm>.so, tools/variant.sh's
naming; such a library need not have the chunk calls).  `chunks` runs for `shipped`, once per round.  The coded streams of both
modes are compared inside the `chunks` process."""
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


def step(mode, level, M, seg, chunk):
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
    model = z.Model(level=level)
    M = min(M, ctx.blockset_capacity(model, max_member_bytes=seg + 1))
    data = np.ascontiguousarray(W.make_blocks_fast(M, seg)).reshape(-1)     # classes b mod 4: zeros / uniform / order-1 text / periodic
    F = z.FLAG_PP
    cap = seg + seg // 4 + 1024
    in_off, out_off = offsets(np, [seg] * M), offsets(np, [cap] * M)
    out = np.zeros(int(out_off[-1]) + 16, dtype=np.uint8)
    out_len, status = np.zeros(M, dtype=np.uint32), np.zeros(M, dtype=np.int32)
    res = dict(mode=mode, level=level, members=M, seg=seg, lib=os.environ.get("ZPQ_LIB_PATH", "shipped"))

    # ---- one call per direction
    enc, dec = z.BlockSet(ctx, model, M, max_member_bytes=seg + 1), z.BlockSet(ctx, model, M, max_member_bytes=seg + 1)
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
        enc, dec = z.BlockSet(ctx, model, M, max_member_bytes=seg + 1), z.BlockSet(ctx, model, M, max_member_bytes=seg + 1)
        ncalls = seg // chunk
        assert ncalls * chunk == seg
        arr = data.reshape(M, seg)
        k_off, ko_off = offsets(np, [chunk] * M), offsets(np, [chunk + chunk // 4 + 1024] * M)
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
        win = chunk + chunk // 4 + 64
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
    ap.add_argument("--members", type=int, default=4096)
    ap.add_argument("--seg", type=int, default=65536)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--arms", default="shipped")
    ap.add_argument("--rounds", type=int, default=2, help="passes over the arms (even: every arm in odd and even places)")
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="")
    a = ap.parse_args()
    if a.step:
        step(a.step, a.level, a.members, a.seg, a.chunk)
        return 0
    arms = a.arms.split(",")
    order = []
    for r in range(a.rounds):
        order += [(arm, "one") for arm in (arms if r % 2 == 0 else arms[::-1])] + [("shipped", "chunks")]
    results, lines = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            open(a.out, "w").write("\n".join(lines) + "\n")

    say("# tools/set_chunks_bench.py --level %d --members %d --seg %d --chunk %d --arms %s --rounds %d" %
        (a.level, a.members, a.seg, a.chunk, a.arms, a.rounds))
    for arm, mode in order:
        env = dict(os.environ)
        env.pop("ZPQ_LIB_PATH", None)
        if arm != "shipped":
            env["ZPQ_LIB_PATH"] = os.path.join(ROOT, "zpaq-v_amd", "lib", "libzpaq_hip_%s.so" % arm)
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--step", mode, "--level", str(a.level),
               "--members", str(a.members), "--seg", str(a.seg), "--chunk", str(a.chunk)]
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
        if r["mode"] == "chunks":
            say("chunks: encode %d calls %.2f ms against %.2f ms in one (x%.3f); decode %d calls %.2f ms against %.2f ms in one (x%.3f), "
                "its last call %.3f ms" % (r["enc_calls"], r["enc_chunks_ms"], r["enc_one_ms"], r["enc_chunks_ms"] / r["enc_one_ms"],
                                           r["dec_calls"], r["dec_chunks_ms"], r["dec_one_ms"], r["dec_chunks_ms"] / r["dec_one_ms"],
                                           r["dec_last_call_ms"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
