"""A general model with large hashed tables, dense against the compact line store (ZPQ_FLAG_LINESTORE).
    python tools/lanes_store_bench.py [--bits 22] [--blocks 256,2048,8192] [--out profiles/FILE.txt]
The model is C4b (tests/golden/inputs.py: all nine component types) with its ICM and its ISSE at --bits size bits: at 22, two
tables of 256 MiB, a dense slot of 513 MiB.  The batch is 64 KiB blocks of the bench's four classes (tests/workload.py),
resident on the device, coded through the _dev calls; per batch size the same blocks run without the request -- the route of
a plain call today: the wave pipelines k_gpipe / k_gdec on dense tables --, without it on k_rows (ZPQ_ENC_GPIPE=0 /
ZPQ_DEC_GPIPE=0: the store's own kernel, dense), and with it.  Reported per run and direction: the kernel and its time
(zpq_ctx_last_kernel_ms, HIP events around the launch), the slots the launch held (zpq_ctx_last_slots), the rounds (blocks /
slots, rounded up) and the slot size.  The streams of the three routes are compared, and the decoded blocks with the input.
Every run is a child process of its own under a time limit; the first one that fails, faults or runs out of time ends the tool."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 65536
CAPMUL = 6.0                                                 # (C4b expands uniform bytes: bench.py gives it the same room)
STEP_LIMIT = 420                                             # seconds per child process
ROUTES = ("dense", "dense_rows", "store")


def model_header(bits):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import general_models as GM
    from inputs import C4B
    comps = GM.components(C4B)
    for c in comps:
        if c[0] in (GM.ICM, GM.ISSE):
            c[1] = bits
    return GM.H(comps, C4B[0], C4B[1], GM.program_of(C4B))


def step(bits, nb, route):
    """A child process: one route at one batch size, one warm-up pass and one timed pass in each direction."""
    import zlib
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    import workload as W
    for k in ("ZPQ_LANES_STORE", "ZPQ_SPARSE_MODE", "ZPQ_SPARSE_FORCE_LOG2", "ZPQ_LANES_ROWS", "ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE"):
        os.environ.pop(k, None)
    if route == "dense_rows":
        os.environ["ZPQ_ENC_GPIPE"] = os.environ["ZPQ_DEC_GPIPE"] = "0"
    z = ge.load()
    ctx = z.Context(0)
    model = z.Model(header=model_header(bits))
    flags = z.FLAG_PP | (z.FLAG_LINESTORE if route == "store" else 0)
    dev = torch.device("cuda:0")
    arr = W.make_blocks_fast(nb, SIZE)
    d_in = torch.from_numpy(arr.reshape(-1)).to(dev)
    cap = int(SIZE * CAPMUL) + 1024
    i64, i32 = dict(dtype=torch.int64, device=dev), dict(dtype=torch.int32, device=dev)
    in_off, out_off = torch.arange(nb + 1, **i64) * SIZE, torch.arange(nb + 1, **i64) * cap
    d_out = torch.zeros(nb * cap, dtype=torch.uint8, device=dev)
    d_dec = torch.zeros(nb * SIZE, dtype=torch.uint8, device=dev)
    d_len, d_st, d_dlen, d_cons, d_code, d_first, d_dst = (torch.zeros(nb, **i32) for _ in range(7))
    torch.cuda.synchronize()
    res = dict(route=route, bits=bits, blocks=nb, dense_slot_bytes=model.state_bytes,
               resident_capacity=ctx.resident_capacity(model, flags))
    for timed in (False, True):
        ctx.encode_blocks_dev(model, nb, d_in.data_ptr(), in_off.data_ptr(), flags, d_out.data_ptr(), out_off.data_ptr(),
                              d_len.data_ptr(), d_st.data_ptr())
        ctx.sync()
        res.update(enc_kernel=ctx.last_kernel_name, enc_ms=round(ctx.last_kernel_ms, 2), enc_slots=ctx.last_slots,
                   line_store=ctx.last_line_store)
        ctx.decode_blocks_dev(model, nb, d_out.data_ptr(), out_off.data_ptr(), flags, d_dec.data_ptr(), in_off.data_ptr(),
                              d_dlen.data_ptr(), d_cons.data_ptr(), d_code.data_ptr(), d_first.data_ptr(), d_dst.data_ptr())
        ctx.sync()
        res.update(dec_kernel=ctx.last_kernel_name, dec_ms=round(ctx.last_kernel_ms, 2), dec_slots=ctx.last_slots)
        if not timed:
            res.update(first_enc_ms=res["enc_ms"], first_dec_ms=res["dec_ms"])
    assert bool((d_st == 0).all()) and bool((d_dst == 0).all()), "a block failed"
    assert bool((d_dlen == SIZE).all()) and bool(torch.equal(d_dec, d_in)) and bool((d_first == 0).all()), "round trip"
    lens = d_len.cpu().numpy().astype(np.int64)
    coded = d_out.cpu().numpy().reshape(nb, cap)
    crc = 0
    for i in range(nb):
        crc = zlib.crc32(coded[i, :lens[i]].tobytes(), crc)
    store = ctx.last_line_store
    slot = model.lanes_store_slot_bytes(store) if store else model.state_bytes
    res.update(slot_bytes=slot, coded_bytes=int(lens.sum()), coded_crc32=crc,
               enc_rounds=-(-nb // res["enc_slots"]), dec_rounds=-(-nb // res["dec_slots"]))
    print("RESULT " + json.dumps(res), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=22)
    ap.add_argument("--blocks", default="256,2048,8192")
    ap.add_argument("--routes", default=",".join(ROUTES))
    ap.add_argument("--out", default="")
    ap.add_argument("--step", nargs=3, metavar=("BITS", "BLOCKS", "ROUTE"))
    a = ap.parse_args()
    if a.step:
        step(int(a.step[0]), int(a.step[1]), a.step[2])
        return 0
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say("C4b with ICM and ISSE at %d bits, 64 KiB blocks of the four classes, one warm-up and one timed pass per direction" % a.bits)
    say("%-10s %6s  %-16s %9s %6s %6s  %-16s %9s %6s %6s  %12s %6s" % ("route", "blocks", "encode kernel", "ms", "slots", "rounds",
                                                                   "decode kernel", "ms", "slots", "rounds", "slot bytes", "store"))
    for nb in [int(x) for x in a.blocks.split(",")]:
        seen = {}
        for route in a.routes.split(","):
            cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--step", str(a.bits), str(nb), route]
            p = subprocess.run(cmd, capture_output=True, text=True)
            got = [json.loads(ln[7:]) for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not got:                 # a failure, a fault or the time limit: nothing more is started
                say("step %d %s ended with %d\n%s" % (nb, route, p.returncode, p.stderr[-2000:]))
                return 1
            r = got[0]
            seen[route] = r
            say("%-10s %6d  %-16s %9.2f %6d %6d  %-16s %9.2f %6d %6d  %12d %6d" % (
                route, nb, r["enc_kernel"], r["enc_ms"], r["enc_slots"], r["enc_rounds"], r["dec_kernel"], r["dec_ms"],
                r["dec_slots"], r["dec_rounds"], r["slot_bytes"], r["line_store"]))
            say("           first pass %.2f / %.2f ms, resident capacity %d, coded bytes %d, crc32 %08x" % (
                r["first_enc_ms"], r["first_dec_ms"], r["resident_capacity"], r["coded_bytes"], r["coded_crc32"]))
        if len({(r["coded_bytes"], r["coded_crc32"]) for r in seen.values()}) != 1:
            say("the routes wrote different streams at %d blocks" % nb)
            return 1
        if "dense" in seen and "store" in seen:
            d, s = seen["dense"], seen["store"]
            say("%d blocks: store / dense time: encode %.2f, decode %.2f" % (nb, s["enc_ms"] / d["enc_ms"], s["dec_ms"] / d["dec_ms"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
