"""The header's threading contract, checked once: the host-pointer entry points -- batches, zpq_block_*, zpq_blockset_*,
zpq_sha1_blocks, zpq_*_blocks_multi -- serialise on a per-ctx mutex and may be called from several threads; the _dev forms
take one thread per ctx.  ctypes releases the GIL inside a library call, so Python threads are concurrent callers.

Every expectation comes from the oracle (or hashlib) before a thread starts; the same work runs sequentially first.  Each
thread does its work twice and that is all: this checks the contract, it does not hunt for a race.  Threads are daemons
joined with a 120 s hang guard; one still alive afterwards ends the session, so that nothing more is started on the GPU.
"""
import hashlib
import threading
import time

import numpy as np
import pytest

import abi_windows as A
import oracle_lib as O
from test_gpu_abi_windows import KNOBS, decode_host, encode_host, flags_of

pytestmark = pytest.mark.gpu

HANG_GUARD_S = 120
PASSES = 2


@pytest.fixture(scope="module")
def models(zpq):
    return {name: zpq.Model(header=m.header, offsets=m.offsets) for name, m in A.MODELS.items()}


@pytest.fixture(scope="module")
def other_ctx(zpq):
    ctx = zpq.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def run_threads(jobs):
    """Every job on a thread of its own, released together; returns the wall time.  The first exception a job raised is
    raised here; a thread that outlives the hang guard ends the session."""
    barrier = threading.Barrier(len(jobs))
    errors = [None] * len(jobs)

    def body(i, job):
        try:
            barrier.wait(HANG_GUARD_S)
            job()
        except BaseException as e:  # noqa: BLE001
            errors[i] = e

    threads = [threading.Thread(target=body, args=(i, j), daemon=True) for i, j in enumerate(jobs)]
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, t0 + HANG_GUARD_S - time.perf_counter()))
    took = time.perf_counter() - t0
    alive = [i for i, t in enumerate(threads) if t.is_alive()]
    if alive:
        pytest.exit("threads %s still running after %d s: a call hangs; nothing more is started on the GPU" % (alive, HANG_GUARD_S),
                    returncode=1)
    for e in errors:
        if e is not None:
            raise e
    return took


def twice(job):
    def run():
        for _ in range(PASSES):
            job()
    return run


def batch_job(zpq, ctx, models, name, which="ragged", first=(0, 0)):
    """Batch encode + decode of the 13 blocks through the host-pointer forms, every stream and field held to the oracle."""
    blocks, want, m = {"ragged": A.RAGGED, "far": A.FAR}[which], A.coded(name, which), models[name]
    for b, c in zip(blocks, want):
        A.decoded(name, c, len(b) + 64)                    # (the expectation exists before a thread asks for it)

    def job():
        encode_host(zpq, lambda *a: ctx.encode_blocks_raw(m, *a), name, blocks, want, first)
        decode_host(zpq, lambda *a: ctx.decode_blocks_raw(m, *a), name, want, blocks, first)
    return job


def block_job(zpq, ctx, models):
    """A zpq_block of level 1 coded as three segments: the batch kernel, the replay into the block's own slot, k_generic --
    three separate acquisitions of the lock, each way."""
    segs = [A.RAGGED[4], A.RAGGED[3], A.RAGGED[2]]
    ref = O.Codec(A.MODELS["level1"].header)
    want = [ref.encode(s) for s in segs]
    codes = []                                            # Decoder.code at each segment's end
    back = O.Codec(A.MODELS["level1"].header)
    for s, w in zip(segs, want):
        stored, n, cons, code, _ = back.decode_prefix(w, len(s) + 9)
        assert (stored, n, cons) == (b"\0" + s, len(s) + 1, len(w))
        codes.append(code)

    def job():
        enc, dec = zpq.Block(ctx, models["level1"]), zpq.Block(ctx, models["level1"])
        try:
            for s, w, code in zip(segs, want, codes):
                assert enc.encode_segment(s) == w
                assert dec.decode_segment(w, len(s) + 8) == (s, len(w), code, 0)
        finally:
            enc.close(); dec.close()
    return job


def blockset_job(zpq, ctx, models):
    """A BlockSet of level 2 with 4 members, two rounds, encode then decode."""
    rounds = [[A.RAGGED[(3 * r + k + 1) % 13] for k in range(4)] for r in range(2)]
    refs = [O.Codec(A.MODELS["level2"].header) for _ in range(4)]
    want = [[refs[k].encode(segs[k]) for k in range(4)] for segs in rounds]

    def job():
        enc, dec = zpq.BlockSet(ctx, models["level2"], 4), zpq.BlockSet(ctx, models["level2"], 4)
        try:
            for segs, w in zip(rounds, want):
                coded, status, out_len = enc.encode_segments(segs)
                assert coded == w and not status.any() and [int(x) for x in out_len] == [len(x) for x in w]
            for segs, w in zip(rounds, want):
                back, status, consumed, _, first = dec.decode_segments(w, cap=2048 + 8)
                assert back == segs and not status.any() and not first.any()
                assert [int(x) for x in consumed] == [len(x) for x in w]
        finally:
            enc.close(); dec.close()
    return job


def sha1_job(ctx):
    msgs = [A.lcg_bytes((i * 37) % 150, seed=i + 1) for i in range(200)]
    want = [hashlib.sha1(x).digest() for x in msgs]

    def job():
        assert ctx.sha1_blocks(msgs) == want
    return job


def test_one_context_six_threads(zpq, gpu_ctx, models):
    jobs = [twice(j) for j in (batch_job(zpq, gpu_ctx, models, "level2"), batch_job(zpq, gpu_ctx, models, "mix_x4"),
                               batch_job(zpq, gpu_ctx, models, "n17"), block_job(zpq, gpu_ctx, models),
                               blockset_job(zpq, gpu_ctx, models), sha1_job(gpu_ctx))]
    t0 = time.perf_counter()
    for j in jobs:
        j()
    sequential = time.perf_counter() - t0
    threaded = run_threads(jobs)
    print("\none context, six threads: sequential %.2f s, threaded %.2f s" % (sequential, threaded))


class DevJob:
    """One batch through zpq_encode_blocks_dev and zpq_decode_blocks_dev on torch buffers of its own.  The buffers are made
    on the caller's thread (and torch's stream synchronised) before run() goes to a thread; check() reads them afterwards."""

    def __init__(self, zpq, ctx, models, name):
        import torch
        self.ctx, self.m, self.name, self.F = ctx, models[name], name, flags_of(zpq, name, True)
        self.blocks, self.want, self.n = A.RAGGED, A.coded(name, "ragged"), len(A.RAGGED)
        dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).astype(t)).to("cuda:0")   # noqa: E731
        self.in_off, self.out_off = A.layout([len(b) for b in self.blocks]), A.layout([A.cap_of(len(b)) for b in self.blocks])
        self.mid_off, self.back_off = A.layout([len(c) for c in self.want]), A.layout([len(b) + 64 for b in self.blocks])
        self.t_off = [dev(x, np.int64) for x in (self.in_off, self.out_off, self.mid_off, self.back_off)]
        self.src = dev(np.frombuffer(b"".join(self.blocks) + bytes(16), dtype=np.uint8), np.uint8)
        self.mid = dev(np.frombuffer(b"".join(self.want) + bytes(16), dtype=np.uint8), np.uint8)
        self.out = torch.full((int(self.out_off[-1]) + 64,), A.FILL, dtype=torch.uint8, device="cuda:0")
        self.back = torch.full((int(self.back_off[-1]) + 64,), A.FILL, dtype=torch.uint8, device="cuda:0")
        self.res = [torch.full((self.n,), -99, dtype=torch.int32, device="cuda:0") for _ in range(7)]

    def run(self):
        p = lambda t: t.data_ptr()                          # noqa: E731
        r = self.res
        self.ctx.encode_blocks_dev(self.m, self.n, p(self.src), p(self.t_off[0]), self.F, p(self.out), p(self.t_off[1]), p(r[0]), p(r[1]))
        self.ctx.sync()
        self.ctx.decode_blocks_dev(self.m, self.n, p(self.mid), p(self.t_off[2]), self.F, p(self.back), p(self.t_off[3]), p(r[2]),
                                   p(r[3]), p(r[4]), p(r[5]), p(r[6]))
        self.ctx.sync()

    def check(self):
        olen, st, dlen, cons, code, fb, dst = [[x & 0xFFFFFFFF for x in t.cpu().tolist()] for t in self.res]
        assert olen == [len(w) for w in self.want] and st == [0] * self.n and dst == [0] * self.n and fb == [0] * self.n
        assert dlen == [len(b) for b in self.blocks] and cons == [len(w) for w in self.want]
        assert code == [A.decoded(self.name, c, len(b) + 64).final_code for b, c in zip(self.blocks, self.want)]
        out, back = self.out.cpu().numpy(), self.back.cpu().numpy()
        for i in range(self.n):                            # the _dev forms write no byte from min(out_len, cap) on
            for buf, off, w in ((out, self.out_off, self.want[i]), (back, self.back_off, self.blocks[i])):
                o = int(off[i])
                assert buf[o:o + len(w)].tobytes() == w, (self.name, i)
                assert (buf[o + len(w):int(off[i + 1])] == A.FILL).all(), (self.name, i)


def test_two_contexts_two_threads(zpq, gpu_ctx, other_ctx, models):
    """Host forms of different kernel families at once, one thread per context, then swapped; then the _dev forms, one
    thread per context, as the header allows."""
    import torch
    a, b = gpu_ctx, other_ctx
    waves = lambda ctx: batch_job(zpq, ctx, models, "mix_x4")                      # noqa: E731
    vm = lambda ctx: batch_job(zpq, ctx, models, "c4b_vm")                         # noqa: E731  (under ZPQ_FLAG_VMPIPE)
    run_threads([twice(waves(a)), twice(vm(b))])
    run_threads([twice(vm(a)), twice(waves(b))])
    one, two = DevJob(zpq, a, models, "level2"), DevJob(zpq, b, models, "n17")
    torch.cuda.synchronize()                               # the ctx streams do not wait for torch's
    run_threads([one.run, two.run])
    one.check(); two.check()


def test_multi_from_two_threads(zpq, gpu_ctx, other_ctx, models):
    """zpq_*_blocks_multi over [a, b, a] -- three shares of one block -- called from two threads at once on buffers of their
    own: four threads of the library's and two of the caller's meet on two contexts."""
    group = [gpu_ctx, other_ctx, gpu_ctx]

    def job(name, lo):
        m, blocks, want = models[name], A.RAGGED[lo:lo + 3], A.coded(name, "ragged")[lo:lo + 3]
        for x, c in zip(blocks, want):
            A.decoded(name, c, len(x) + 64)

        def run():
            encode_host(zpq, lambda *a: zpq.encode_blocks_multi(group, m, *a), name, blocks, want, (0, 0), tails=True)
            decode_host(zpq, lambda *a: zpq.decode_blocks_multi(group, m, *a), name, want, blocks, (0, 0), tails=True)
        return run
    run_threads([twice(job("level2", 2)), twice(job("level2", 7))])
    run_threads([twice(job("level2", 2)), twice(job("mix_x4", 7))])
