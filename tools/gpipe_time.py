"""The wave-per-component encoder (k_gpipe) against the lane-per-component one (k_rows) on C4b (all nine component types) or a
shipped level run as a general model: device-resident encode at resident capacity, checked by decoding back and by comparing
the two encoders' streams.   python tools/gpipe_time.py [c4b|2|3|4|5] [blocks]
c4b_vm / c4b_loop: C4b's components behind a program that is NOT the recognised hash chain (the chain with a=a in front; loop_count of
tests/zpaql_programs.py) -- the interpreter wave's pipelines (k_vpipe / k_vdec, ZPQ_FLAG_VMPIPE) against the route such a model has
without the flag (k_rows with the interpreter) and, as a ceiling, k_gpipe / k_gdec on the true C4b, in ONE process in a balanced order
(A B C C B A ..., tools/ab_balanced.py's rule), kernel times from zpq_ctx_last_kernel_ms.
    python tools/gpipe_time.py c4b_vm|c4b_loop [blocks] [rounds]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import numpy as np, torch
import __graft_entry__ as ge
import workload as W
from inputs import C4B
z = ge.load(); ctx = z.Context(0)
which = sys.argv[1] if len(sys.argv) > 1 else "c4b"
if which in ("c4b_vm", "c4b_loop"):
    import statistics
    import vpipe_models as VM, zpaql_programs as ZP
    hdr = VM.C4B_VM if which == "c4b_vm" else VM.c4b_with(lambda k: ZP.assemble(ZP.NAMED["loop_count"], k))
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    size, cap, dev = 65536, 65536 * 6 + 1024, torch.device('cuda:0')
    os.environ.pop("ZPQ_VM_PIPE", None)
    arms = {"vm": (z.Model(header=hdr), z.FLAG_PP | z.FLAG_VMPIPE), "rows": (z.Model(header=hdr), z.FLAG_PP), "chain": (z.Model(header=C4B), z.FLAG_PP)}
    d_in = torch.from_numpy(W.make_blocks_fast(n, size).reshape(-1)).to(dev)
    i64 = dict(dtype=torch.int64, device=dev); i32 = dict(dtype=torch.int32, device=dev)
    in_off = torch.arange(n + 1, **i64) * size; out_off = torch.arange(n + 1, **i64) * cap
    d_out = torch.zeros(n * cap, dtype=torch.uint8, device=dev); d_dec = torch.zeros(n * size, dtype=torch.uint8, device=dev)
    d_len, d_st, d_dlen, d_cons, d_code, d_first, d_dst = (torch.zeros(n, **i32) for _ in range(7))
    torch.cuda.synchronize()
    got, total = {a: [] for a in arms}, {}
    for r in range(rounds):
        for arm in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
            model, flags = arms[arm]
            ctx.encode_blocks_dev(model, n, d_in.data_ptr(), in_off.data_ptr(), flags, d_out.data_ptr(), out_off.data_ptr(), d_len.data_ptr(), d_st.data_ptr())
            ctx.sync(); e, en, sl = ctx.last_kernel_ms, ctx.last_kernel_name, ctx.last_slots
            ctx.decode_blocks_dev(model, n, d_out.data_ptr(), out_off.data_ptr(), flags, d_dec.data_ptr(), in_off.data_ptr(), d_dlen.data_ptr(), d_cons.data_ptr(), d_code.data_ptr(), d_first.data_ptr(), d_dst.data_ptr())
            ctx.sync(); d, dn, dsl = ctx.last_kernel_ms, ctx.last_kernel_name, ctx.last_slots
            ok = bool((d_st == 0).all()) and bool((d_dst == 0).all()) and bool(torch.equal(d_dec, d_in))
            total.setdefault(arm, int(d_len.sum()))
            got[arm].append((e, d))
            print("%s round %d %-5s %s slots %d: %.1f ms   %s slots %d: %.1f ms   decoded back %s, %d coded bytes" % (which, r, arm, en, sl, e, dn, dsl, d, ok, total[arm]), flush=True)
            if not ok or total[arm] != int(d_len.sum()):
                sys.exit(1)
    for arm, xs in got.items():
        for k, what in ((0, "encode"), (1, "decode")):
            v = [x[k] for x in xs]
            print("%s %-5s %s: mean %.1f ms, min %.1f, max %.1f (n=%d)" % (which, arm, what, statistics.mean(v), min(v), max(v), len(v)))
    same = total["vm"] == total["rows"] and (which != "c4b_vm" or total["chain"] == total["vm"])   # (c4b_loop's ceiling arm codes another model)
    print("coded bytes the same on %s:" % ("all three routes" if which == "c4b_vm" else "vm and rows"), same, total)
    sys.exit(0 if same else 1)
model = z.Model(header=C4B) if which == "c4b" else z.Model(level=int(which))
flags = z.FLAG_PP | (0 if which == "c4b" else z.FLAG_LANES)
nb = int(sys.argv[2]) if len(sys.argv) > 2 else 0
size = 65536
dev = torch.device('cuda:0')
res = {}
n = nb or ctx.resident_capacity(model, flags)
for gp in ("1", "0"):
    os.environ["ZPQ_ENC_GPIPE"] = gp
    os.environ["ZPQ_DEC_GPIPE"] = gp
    arr = W.make_blocks_fast(n, size)
    d_in = torch.from_numpy(arr.reshape(-1)).to(dev)
    cap = size * (6 if which == "c4b" else 2) + 1024
    i64 = dict(dtype=torch.int64, device=dev); i32 = dict(dtype=torch.int32, device=dev)
    in_off = torch.arange(n + 1, **i64) * size; out_off = torch.arange(n + 1, **i64) * cap
    d_out = torch.zeros(n * cap, dtype=torch.uint8, device=dev); d_dec = torch.zeros(n * size, dtype=torch.uint8, device=dev)
    d_len, d_st, d_dlen, d_cons, d_code, d_first, d_dst = (torch.zeros(n, **i32) for _ in range(7))
    torch.cuda.synchronize()
    for rep in range(2):
        ctx.encode_blocks_dev(model, n, d_in.data_ptr(), in_off.data_ptr(), flags, d_out.data_ptr(), out_off.data_ptr(), d_len.data_ptr(), d_st.data_ptr())
        ctx.sync(); e = ctx.last_kernel_ms; en = ctx.last_kernel_name; sl = ctx.last_slots
    ctx.decode_blocks_dev(model, n, d_out.data_ptr(), out_off.data_ptr(), flags, d_dec.data_ptr(), in_off.data_ptr(), d_dlen.data_ptr(), d_cons.data_ptr(), d_code.data_ptr(), d_first.data_ptr(), d_dst.data_ptr())
    ctx.sync(); d = ctx.last_kernel_ms; dn = ctx.last_kernel_name
    ok = bool((d_st == 0).all()) and bool((d_dst == 0).all()) and bool(torch.equal(d_dec, d_in))
    lens = d_len.cpu().numpy().astype(np.int64)
    import hashlib
    out = d_out.cpu().numpy()
    hh = hashlib.sha256()
    for i in range(0, n, max(1, n // 64)):
        hh.update(out[i * cap:i * cap + int(lens[i])].tobytes())
    res[gp] = (int(lens.sum()), hh.hexdigest())
    print("%s: %s / %s: %d blocks, slots %d: encode %.1f ms (%.1f MB/s), decode %.1f ms, round trip %.1f MB/s, decoded back %s" %
          (which, en, dn, n, sl, e, n * size / e / 1e3, d, n * size / (e + d) / 1e3, ok), flush=True)
    del d_in, d_out, d_dec
    torch.cuda.empty_cache()
print("streams of the two encoders identical (total bytes, sha256 over a 64-block sample):", res["1"] == res["0"])
