"""The batch ABI held to the oracle on the layouts of tests/abi_windows.py: first offsets other than 0 through every
host-pointer entry point (one block, several blocks in one round and in rounds, pageable and pinned, the striped
transfers, SHA-1, block sets), the one-block shares zpq_*_blocks_multi deals, and batches that straddle 2^32 through the
device-pointer forms, the side kernels and the host pipeline.

Every output buffer starts as 0xEE, every assertion compares with the oracle's coded bytes (or the original blocks), and
every byte the header says a call does not write must still be 0xEE afterwards.
"""
import hashlib

import numpy as np
import pytest

import abi_windows as A
import chain_models as CM
import oracle_lib as O
from test_gpu_chain_models import BUDGET, KNOBS as CHAIN_KNOBS, dec_names, enc_names, knobs
from test_gpu_host_stripes import E, EARLY, LEN, NB, SLAB, STRIPED, blocks_of, ragged_blocks

pytestmark = pytest.mark.gpu

FILL = A.FILL
# the chain kernels' knobs, and those of the host pipeline, the general-model kernels and the block sets
KNOBS = CHAIN_KNOBS + ("ZPQ_NO_STRIPE", "ZPQ_STRIPE_DELAY_US", "ZPQ_PIPE_MIN_BYTES", "ZPQ_PIPE_PER", "ZPQ_ENC_GPIPE",
                       "ZPQ_DEC_GPIPE", "ZPQ_GPIPE_BATCH", "ZPQ_LANES_ROWS", "ZPQ_GDEC_BPW", "ZPQ_VM_PIPE", "ZPQ_SET_LANES",
                       "ZPQ_SET_PIPE", "ZPQ_SET_WAVES", "ZPQ_SET_VMWAVES")
MARGIN = 1 << 16


@pytest.fixture
def env(monkeypatch, zpq, gpu_ctx):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    try:
        yield monkeypatch
    finally:
        zpq.lib().zpq_ctx_set_state_budget(gpu_ctx.h, BUDGET)


@pytest.fixture(scope="module")
def models(zpq):
    return {name: zpq.Model(header=m.header, offsets=m.offsets) for name, m in A.MODELS.items()}


@pytest.fixture(scope="module")
def other_ctx(zpq):
    ctx = zpq.Context(0)
    yield ctx
    ctx.close()


class Buf:
    """A host buffer, pageable or pinned, filled with one byte.  free() is for the path on which every check has passed: a
    failed assertion's traceback still holds views of the array, and pinned memory must outlive them (it is released
    with the Buf)."""

    def __init__(self, zpq, n, pinned, fill):
        self.pin = zpq.PinnedArray(n) if pinned else None
        self.a = self.pin.array if pinned else np.empty(n, dtype=np.uint8)
        self.a[:] = fill
        self.ptr = self.a.ctypes.data

    def put(self, off, chunks):
        for o, c in zip(off, chunks):
            self.a[int(o):int(o) + len(c)] = np.frombuffer(c, dtype=np.uint8)

    def free(self):
        self.a = None
        if self.pin:
            self.pin.free()


def flags_of(zpq, name, pp):
    return A.MODELS[name].flags | (zpq.FLAG_PP if pp else 0)


def untouched(a, lo, hi, what):
    bad = np.nonzero(a[lo:hi] != FILL)[0]
    assert bad.size == 0, "%s: byte %d was written (%d bytes in [%d, %d))" % (what, lo + int(bad[0]), bad.size, lo, hi)


def check_slabs(out, out_off, want, what, tails):
    """Every slab holds the first min(len, cap) bytes of what is wanted; with `tails`, the rest of it is untouched."""
    for i, w in enumerate(want):
        o, cap = int(out_off[i]), int(out_off[i + 1] - out_off[i])
        got = min(len(w), cap)
        assert out[o:o + got].tobytes() == w[:got], (what, "block", i, len(w))
        if tails:
            untouched(out, o + got, o + cap, "%s: behind block %d" % (what, i))


def encode_host(zpq, call, name, blocks, want, first, pp=True, pinned=False, caps=None, tails=None):
    """One encode call through `call(nblocks, in_ptr, in_off, flags, out_ptr, out_off)` on fresh buffers, held to `want`."""
    caps = caps or [A.cap_of(len(b)) for b in blocks]
    in_off, out_off = A.layout([len(b) for b in blocks], first[0]), A.layout(caps, first[1])
    src, out = Buf(zpq, int(in_off[-1]) + 16, pinned, 0x55), Buf(zpq, int(out_off[-1]) + 64, pinned, FILL)
    src.put(in_off, blocks)
    rc, olen, st = call(len(blocks), src.ptr, in_off, flags_of(zpq, name, pp), out.ptr, out_off)
    what = "%s encode %d at %s" % (name, len(blocks), first)
    assert rc == 0, (what, rc)
    assert [int(x) for x in olen] == [len(w) for w in want], what
    assert [int(s) for s in st] == [0 if len(w) <= c else A.E_OVERFLOW for w, c in zip(want, caps)], what
    check_slabs(out.a, out_off, want, what, pinned if tails is None else tails)
    untouched(out.a, 0, int(out_off[0]), what + ": in front of the window")
    untouched(out.a, int(out_off[-1]), len(out.a), what + ": behind the window")
    src.free(); out.free()


def decode_host(zpq, call, name, streams, blocks, first, pp=True, pinned=False, caps=None, tails=None):
    caps = caps or [len(b) + 64 for b in blocks]
    in_off, out_off = A.layout([len(c) for c in streams], first[0]), A.layout(caps, first[1])
    src, out = Buf(zpq, int(in_off[-1]) + 16, pinned, 0x55), Buf(zpq, int(out_off[-1]) + 64, pinned, FILL)
    src.put(in_off, streams)
    rc, olen, cons, code, fb, st = call(len(streams), src.ptr, in_off, flags_of(zpq, name, pp), out.ptr, out_off)
    what = "%s decode %d at %s" % (name, len(streams), first)
    assert rc == 0, (what, rc)
    exp = [A.decoded(name, c, cap, pp) for c, cap in zip(streams, caps)]
    for i, d in enumerate(exp):
        got = (int(olen[i]), int(cons[i]), int(code[i]), int(fb[i]), int(st[i]))
        assert got == (d.out_len, d.consumed, d.final_code, d.first_byte, d.status), (what, "block", i, got, d[1:])
    check_slabs(out.a, out_off, [d.stored for d in exp], what, pinned if tails is None else tails)
    untouched(out.a, 0, int(out_off[0]), what + ": in front of the window")
    untouched(out.a, int(out_off[-1]), len(out.a), what + ": behind the window")
    src.free(); out.free()


# ------------------------------------------------------------------ a. one block, shifted window
@pytest.mark.parametrize("first", A.WINDOWS, ids=["at_%d_%d" % w for w in A.WINDOWS])
@pytest.mark.parametrize("pp", [True, False], ids=["pp", "raw"])
@pytest.mark.parametrize("name", list(A.MODELS))
def test_one_block_shifted_window(zpq, gpu_ctx, env, models, name, pp, first):
    """nblocks = 1 with (in_off[0], out_off[0]) = (0, 0), (1, 4099), (4099, 1): out_len, status and every byte of `out` --
    the produced bytes at out_off[0], 0xEE everywhere else.  With and without the PP byte, every size, both directions.
    (A case per model, flag and window: the lane-0 kernel, which codes n65, takes half a second for 2048 bytes.)"""
    m = models[name]
    for b, c in zip(A.BASE, A.coded(name, "base", pp)):
        encode_host(zpq, lambda *a: gpu_ctx.encode_blocks_raw(m, *a), name, [b], [c], first, pp, tails=True)
        decode_host(zpq, lambda *a: gpu_ctx.decode_blocks_raw(m, *a), name, [c], [b], first, pp, tails=True)


@pytest.mark.parametrize("name", list(A.MODELS))
def test_one_block_shifted_window_slab_too_small(zpq, gpu_ctx, env, models, name):
    """ZPQ_E_OVERFLOW: the slab holds the prefix the header promises, out_len what it promises, and nothing lies behind."""
    m = models[name]
    b, c = A.BASE[3], A.coded(name, "base")[3]
    for first in A.WINDOWS[1:]:
        encode_host(zpq, lambda *a: gpu_ctx.encode_blocks_raw(m, *a), name, [b], [c], first, caps=[100], tails=True)
        decode_host(zpq, lambda *a: gpu_ctx.decode_blocks_raw(m, *a), name, [c], [b], first, caps=[17], tails=True)


# ------------------------------------------------------------------ b. several blocks, shifted window
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("name", ["level2", "mix_x4", "n17"])
def test_batch_shifted_window(zpq, gpu_ctx, env, models, name, pinned):
    """13 ragged blocks at (4099, 777), in a single round and in rounds of at most 5."""
    m = models[name]
    enc = lambda *a: gpu_ctx.encode_blocks_raw(m, *a)      # noqa: E731
    dec = lambda *a: gpu_ctx.decode_blocks_raw(m, *a)      # noqa: E731
    want = A.coded(name, "ragged")
    encode_host(zpq, enc, name, A.RAGGED, want, A.SHIFT, pinned=pinned)
    assert gpu_ctx.last_host_transfer == 1 << 8
    if name == "level2":
        assert gpu_ctx.last_kernel_name == "k_pipe<encode>"
    decode_host(zpq, dec, name, want, A.RAGGED, A.SHIFT, pinned=pinned)
    assert gpu_ctx.last_host_transfer == 1 << 8
    # two slabs too small, one in the middle and the last one: their neighbours, and what lies behind the window, stay
    # whole (a pinned slab is filled by the GPU from out_len[], which then says more than the slab holds)
    caps = [A.cap_of(len(b)) for b in A.RAGGED]
    caps[3], caps[12] = 100, 10
    encode_host(zpq, enc, name, A.RAGGED, want, A.SHIFT, pinned=pinned, caps=caps)
    caps = [len(b) + 64 for b in A.RAGGED]
    caps[3], caps[12] = 17, 5
    decode_host(zpq, dec, name, want, A.RAGGED, A.SHIFT, pinned=pinned, caps=caps)
    zpq.lib().zpq_ctx_set_state_budget(gpu_ctx.h, 5 * m.state_bytes + 1000)
    with knobs(env, ZPQ_PIPE_MIN_BYTES="0", ZPQ_SPARSE_MODE="never"):
        encode_host(zpq, enc, name, A.RAGGED, want, A.SHIFT, pinned=pinned)
        rounds = gpu_ctx.last_host_transfer >> 8
        assert rounds >= 3 and gpu_ctx.last_host_transfer & 255 == 0, gpu_ctx.last_host_transfer
        decode_host(zpq, dec, name, want, A.RAGGED, A.SHIFT, pinned=pinned)
        assert gpu_ctx.last_host_transfer >> 8 >= 3
        if name == "level2":
            assert rounds == 3 and gpu_ctx.last_slots == 3    # 5 + 5 + 3


# ------------------------------------------------------------------ c. stripes, shifted window
def test_striped_upload_shifted_window(zpq, gpu_ctx, env, models):
    """64 blocks of 32 KiB from pinned memory, in_off[0] = out_off[0] = 4099: every stripe address is odd."""
    m = models["level2"]
    blocks = blocks_of(LEN)
    want = O.encode_blocks(A.MODELS["level2"].header, blocks, nthreads=8)
    encode_host(zpq, lambda *a: gpu_ctx.encode_blocks_raw(m, *a), "level2", blocks, want, (4099, 4099), pinned=True)
    assert gpu_ctx.last_host_transfer == 1 << 8 | STRIPED


def test_early_download_shifted_window(zpq, gpu_ctx, env, models):
    """64 ragged blocks into pinned slabs of 16 KiB from out_off[0] = 4099: the first stripe of every slab leaves early."""
    m = models["level2"]
    blocks = ragged_blocks(SLAB)
    streams = O.encode_blocks(A.MODELS["level2"].header, blocks, nthreads=8)
    in_off, out_off = A.layout([len(c) for c in streams], 4099), A.layout([SLAB] * NB, 4099)
    src, out = Buf(zpq, int(in_off[-1]) + 16, True, 0x55), Buf(zpq, int(out_off[-1]) + 64, True, FILL)
    src.put(in_off, streams)
    rc, olen, cons, code, fb, st = gpu_ctx.decode_blocks_raw(m, NB, src.ptr, in_off, zpq.FLAG_PP, out.ptr, out_off)
    assert rc == 0 and (st == 0).all() and (fb == 0).all()
    assert gpu_ctx.last_host_transfer == 1 << 8 | EARLY
    assert [int(x) for x in olen] == [len(b) for b in blocks] and [int(x) for x in cons] == [len(c) for c in streams]
    for i, b in enumerate(blocks):
        o = int(out_off[i])
        assert out.a[o:o + len(b)].tobytes() == b, i
        untouched(out.a, o + max(len(b), E), o + SLAB, "behind block %d" % i)   # ([len, E) is unspecified: the early stripe)
    untouched(out.a, 0, 4099, "in front of the window")
    untouched(out.a, int(out_off[-1]), len(out.a), "behind the window")
    src.free(); out.free()


# ------------------------------------------------------------------ d. the other host-pointer entry points
def test_sha1_blocks_shifted_window(zpq, gpu_ctx):
    msgs = [A.lcg_bytes((i * 37) % 150, seed=i + 1) for i in range(200)]
    in_off = A.layout([len(x) for x in msgs], 4099)
    src = Buf(zpq, int(in_off[-1]) + 16, False, 0x55)
    src.put(in_off, msgs)
    rc, got = gpu_ctx.sha1_blocks_raw(len(msgs), src.ptr, in_off)
    assert rc == 0 and got == [hashlib.sha1(x).digest() for x in msgs]


SET_MEMBERS = ([3, 0, 2], [2, 3, 0])                       # per round: a subset, not ascending; member 1 is never coded
SET_SEGMENTS = ({3: A.RAGGED[3], 0: A.RAGGED[11], 2: A.RAGGED[2]}, {2: A.RAGGED[4], 3: A.RAGGED[1], 0: A.RAGGED[9]})


@pytest.mark.parametrize("name,lanes", [("level2", False), ("n17", True)])
def test_blockset_shifted_window(zpq, gpu_ctx, env, models, name, lanes):
    """Two rounds on a set of four through windows at (4099, 777).  Member 0's slab is too small in round 1 -- every listed
    member is live there, the whole window comes back; in round 2 it has failed before, and only the stored bytes of
    the live members may be written."""
    hdr = A.MODELS[name].header
    m = models[name]
    enc_ref = {k: O.Codec(hdr) for k in range(4)}
    dec_ref = {k: O.Codec(hdr) for k in range(4)}
    full0 = O.Codec(hdr).encode(SET_SEGMENTS[0][0])         # member 0's first segment, whole (its slab holds a prefix)
    enc_set, dec_set = zpq.BlockSet(gpu_ctx, m, 4, lanes=lanes), zpq.BlockSet(gpu_ctx, m, 4, lanes=lanes)
    assert enc_set.lanes == lanes
    try:
        for rnd, (members, segs) in enumerate(zip(SET_MEMBERS, SET_SEGMENTS)):
            failed_before = rnd == 1
            data = [segs[k] for k in members]
            want = [full0 if (k == 0 and rnd == 0) else enc_ref[k].encode(segs[k]) for k in members]
            # ---- encode
            caps = [16 if k == 0 else A.cap_of(len(segs[k])) for k in members]
            in_off, out_off = A.layout([len(d) for d in data], A.SHIFT[0]), A.layout(caps, A.SHIFT[1])
            src, out = Buf(zpq, int(in_off[-1]) + 16, False, 0x55), Buf(zpq, int(out_off[-1]) + 64, False, FILL)
            src.put(in_off, data)
            rc, olen, st = enc_set.encode_segments_raw(members, src.ptr, in_off, zpq.FLAG_PP, out.ptr, out_off)
            assert rc == 0
            for i, k in enumerate(members):
                o, w = int(out_off[i]), want[i]
                if k == 0 and failed_before:
                    assert (int(olen[i]), int(st[i])) == (0, A.E_OVERFLOW)
                    untouched(out.a, o, o + caps[i], "the failed member's slab")
                    continue
                assert (int(olen[i]), int(st[i])) == (len(w), A.E_OVERFLOW if k == 0 else 0), (rnd, k)
                got = min(len(w), caps[i])
                assert out.a[o:o + got].tobytes() == w[:got], (rnd, k)
                if failed_before:
                    untouched(out.a, o + got, o + caps[i], "round 2: behind member %d" % k)
            untouched(out.a, 0, int(out_off[0]), "in front of the window")
            untouched(out.a, int(out_off[-1]), len(out.a), "behind the window")
            # ---- decode, the same way: member 0's slab holds 16 of its 2048 bytes
            dcaps = [16 if k == 0 else len(segs[k]) + 8 for k in members]
            in_off, out_off = A.layout([len(w) for w in want], A.SHIFT[0]), A.layout(dcaps, A.SHIFT[1])
            src, out = Buf(zpq, int(in_off[-1]) + 16, False, 0x55), Buf(zpq, int(out_off[-1]) + 64, False, FILL)
            src.put(in_off, want)
            rc, olen, cons, code, fb, st = dec_set.decode_segments_raw(members, src.ptr, in_off, zpq.FLAG_PP, out.ptr, out_off)
            assert rc == 0
            for i, k in enumerate(members):
                o = int(out_off[i])
                got = (int(olen[i]), int(cons[i]), int(code[i]), int(fb[i]), int(st[i]))
                if k == 0 and failed_before:
                    assert got == (0, 0, 0, A.NO_BYTE, A.E_OVERFLOW)
                    untouched(out.a, o, o + dcaps[i], "the failed member's slab")
                    continue
                stored, n, c_, code_, _ = dec_ref[k].decode_prefix(want[i], dcaps[i] + 1)
                assert got == (n - 1, c_, code_, stored[0], A.E_OVERFLOW if k == 0 else 0), (rnd, k, got)
                assert out.a[o:o + len(stored) - 1].tobytes() == stored[1:] == segs[k][:dcaps[i]], (rnd, k)
                if failed_before:
                    untouched(out.a, o + len(stored) - 1, o + dcaps[i], "round 2: behind member %d" % k)
            untouched(out.a, 0, int(out_off[0]), "in front of the window")
            untouched(out.a, int(out_off[-1]), len(out.a), "behind the window")
    finally:
        enc_set.close(); dec_set.close()


# ------------------------------------------------------------------ e. one-block shares of _multi
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("name", ["level2", "mix_x4"])
@pytest.mark.parametrize("nblocks,ctxs", A.MULTI, ids=["%d%s" % c for c in A.MULTI])
def test_multi_one_block_shares(zpq, gpu_ctx, other_ctx, env, models, nblocks, ctxs, name, pinned):
    """Every stream against the oracle, through the listed contexts and through the first one alone; a share of one block
    behind block 0 must land in its own slab and nowhere else."""
    m = models[name]
    blocks, want = A.RAGGED[2:2 + nblocks], A.coded(name, "ragged")[2:2 + nblocks]
    both = [{"a": gpu_ctx, "b": other_ctx}[c] for c in ctxs]
    for group in (both, both[:1]):
        encode_host(zpq, lambda *a: zpq.encode_blocks_multi(group, m, *a), name, blocks, want, (0, 0), pinned=pinned,
                    tails=pinned or nblocks == 1)
        decode_host(zpq, lambda *a: zpq.decode_blocks_multi(group, m, *a), name, want, blocks, (0, 0), pinned=pinned,
                    tails=pinned or nblocks == 1)


# ------------------------------------------------------------------ f. device-pointer forms across 2^32
DEV_CASES = [(name, {}) for name in A.MODELS] + [("level3", {"ZPQ_SPARSE_MODE": "always"}), ("level2", {"ZPQ_DEC_PIPE": "1"})]


def _dev(a, dtype=np.int64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).to("cuda:0")


class TestDeviceFormsAcross2_32:
    """Two device buffers of 4 GiB + 2 MiB, untouched but for a window around 2^32 each; freed when the class is through."""

    @pytest.fixture(scope="class")
    def far(self):
        import torch
        free, _ = torch.cuda.mem_get_info()
        if free < 12 << 30:
            pytest.skip("less than 12 GiB of device memory free (%d MiB)" % (free >> 20))
        bufs = [torch.empty(A.BIG_BUFFER, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
        yield bufs
        del bufs[:]
        torch.cuda.empty_cache()

    @staticmethod
    def paint(t, off, value):
        lo, hi = int(off[0]) - MARGIN, int(off[-1]) + MARGIN
        t[lo:hi] = value
        return lo, hi

    @staticmethod
    def window(t, lo, hi):
        return t[lo:hi].cpu().numpy()

    @pytest.mark.parametrize("name,kv", DEV_CASES, ids=[n + "".join("-" + k for k in kv) for n, kv in DEV_CASES])
    def test_encode_gather_sha1_decode(self, zpq, gpu_ctx, env, models, far, name, kv):
        import torch
        d_in, d_out = far
        m, n = models[name], 12
        blocks, want = A.FAR[:n], A.coded(name, "far")[:n]
        enc_in, enc_out, dec_in, dec_out = A.far_layouts(name, n)
        rt = CM.route(zpq, m) if name.startswith("level") else None
        F = flags_of(zpq, name, True)
        small = lambda: (torch.full((n,), -99, dtype=torch.int32, device="cuda:0") for _ in range(5))   # noqa: E731
        with knobs(env, **kv):
            # ---- encode: raw blocks below, across and above 2^32 -> slabs below, across and above it
            self.paint(d_in, enc_in, 0x55)
            lo, hi = self.paint(d_out, enc_out, FILL)
            d_in[int(enc_in[0]):int(enc_in[-1])] = _dev(np.frombuffer(b"".join(blocks), dtype=np.uint8), np.uint8)
            t_in, t_out = _dev(enc_in), _dev(enc_out)
            olen, st, cons, code, fb = small()
            torch.cuda.synchronize()                       # the ctx stream does not wait for torch's
            gpu_ctx.encode_blocks_dev(m, n, d_in.data_ptr(), t_in.data_ptr(), F, d_out.data_ptr(), t_out.data_ptr(),
                                      olen.data_ptr(), st.data_ptr())
            gpu_ctx.sync()
            kernel = gpu_ctx.last_kernel_name
            assert kernel in (enc_names(rt, gpu_ctx, kv) if rt else {A.KERNELS[name][0]}), kernel
            if kv.get("ZPQ_SPARSE_MODE") == "always":
                assert gpu_ctx.last_line_store > 0
            assert olen.cpu().tolist() == [len(w) for w in want] and st.cpu().tolist() == [0] * n
            w = self.window(d_out, lo, hi)
            check_slabs(w, enc_out - np.uint64(lo), want, name + " encode_dev", True)
            untouched(w, 0, MARGIN, "in front of the window")
            untouched(w, len(w) - MARGIN, len(w), "behind the window")
            # ---- gather: the streams out of their slabs, back to back into the other buffer across 2^32
            lo, hi = self.paint(d_in, dec_in, FILL)
            t_src, t_dst = _dev(enc_out[:-1]), _dev(dec_in[:-1])
            torch.cuda.synchronize()
            gpu_ctx.gather_dev(n, d_out.data_ptr(), t_src.data_ptr(), olen.data_ptr(), d_in.data_ptr(), t_dst.data_ptr())
            gpu_ctx.sync()
            w = self.window(d_in, lo, hi)
            assert w[MARGIN:len(w) - MARGIN].tobytes() == b"".join(want)
            untouched(w, 0, MARGIN, "gather: in front")
            untouched(w, len(w) - MARGIN, len(w), "gather: behind")
            # ---- SHA-1 of the streams where they lie
            t_in = _dev(dec_in)
            d20 = torch.zeros(20 * n, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            gpu_ctx.sha1_blocks_dev(n, d_in.data_ptr(), t_in.data_ptr(), d20.data_ptr())
            gpu_ctx.sync()
            assert d20.cpu().numpy().tobytes() == b"".join(hashlib.sha1(c).digest() for c in want)
            # ---- decode them into slabs of len + 1600 across 2^32
            lo, hi = self.paint(d_out, dec_out, FILL)
            t_out = _dev(dec_out)
            olen, st, cons, code, fb = small()
            torch.cuda.synchronize()
            gpu_ctx.decode_blocks_dev(m, n, d_in.data_ptr(), t_in.data_ptr(), F, d_out.data_ptr(), t_out.data_ptr(),
                                      olen.data_ptr(), cons.data_ptr(), code.data_ptr(), fb.data_ptr(), st.data_ptr())
            gpu_ctx.sync()
            kernel = gpu_ctx.last_kernel_name
            assert kernel in (dec_names(rt, gpu_ctx, kv) if rt else {A.KERNELS[name][1]}), kernel
            if kv.get("ZPQ_DEC_PIPE") == "1":
                assert kernel == "k_dpipe<decode>"
            exp = [A.decoded(name, c, len(b) + A.FAR_DEC_SLACK) for b, c in zip(blocks, want)]
            u32 = lambda t: [x & 0xFFFFFFFF for x in t.cpu().tolist()]   # noqa: E731
            assert u32(olen) == [d.out_len for d in exp] and u32(cons) == [d.consumed for d in exp]
            assert u32(code) == [d.final_code for d in exp] and u32(fb) == [0] * n and st.cpu().tolist() == [0] * n
            w = self.window(d_out, lo, hi)
            check_slabs(w, dec_out - np.uint64(lo), blocks, name + " decode_dev", True)
            untouched(w, 0, MARGIN, "in front of the window")
            untouched(w, len(w) - MARGIN, len(w), "behind the window")

    def test_sha1_ranges(self, zpq, gpu_ctx, far):
        """zpq_sha1_ranges_dev on an arena that straddles 2^32: every (len & 63, addr & 3) at 0, 1 and 2 full chunks in one
        launch; then ranges that are empty, overlap, come in descending order."""
        import torch
        d_in = far[0]
        arena, begin, end = A.sha1_grid()
        base = A.TWO32 - 30000                             # 16-aligned: addr & 3 is that of the offsets
        assert d_in.data_ptr() % 16 == 0 and base % 16 == 0 and base + len(arena) > A.TWO32 + 30000
        d_in[base:base + len(arena)] = _dev(np.frombuffer(arena, dtype=np.uint8), np.uint8)
        for ranges in (list(zip(begin, end)), A.sha1_odd_ranges(len(arena))):
            nr = len(ranges)
            t_b, t_e = _dev([base + b for b, e in ranges]), _dev([base + e for b, e in ranges])
            d20 = torch.zeros(20 * nr, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            gpu_ctx.sha1_ranges_dev(nr, d_in.data_ptr(), t_b.data_ptr(), t_e.data_ptr(), d20.data_ptr())
            gpu_ctx.sync()
            got = d20.cpu().numpy().tobytes()
            for i, (b, e) in enumerate(ranges):
                assert got[20 * i:20 * i + 20] == hashlib.sha1(arena[b:e]).digest(), (i, b, e)


# ------------------------------------------------------------------ g. host-pointer form across 2^32
def test_host_batch_across_2_32(zpq, gpu_ctx, env, models):
    """13 level-2 blocks in pageable arrays of 4 GiB + 2 MiB, placed as above: only the batch's window is read or written
    (the arrays are never touched elsewhere, so their pages do not even exist).
    What this test can see: a byte written outside the window within 64 KiB of it, and offsets that lose their upper half.
    It cannot see an upload that is wider than the window -- reading is invisible, only the call's time would show it --
    nor a write further away; the one-block and _multi tests above are what holds the library to the window."""
    name, n = "level2", 13
    m = models[name]
    blocks, want = A.FAR, A.coded(name, "far")
    enc_in, enc_out, dec_in, dec_out = A.far_layouts(name, n)
    a, b = np.empty(A.BIG_BUFFER, dtype=np.uint8), np.empty(A.BIG_BUFFER, dtype=np.uint8)
    try:
        def paint(x, off, value):
            lo, hi = int(off[0]) - MARGIN, int(off[-1]) + MARGIN
            x[lo:hi] = value
            return lo, hi

        def put(x, off, chunks):
            for o, c in zip(off, chunks):
                x[int(o):int(o) + len(c)] = np.frombuffer(c, dtype=np.uint8)

        paint(a, enc_in, 0x55)
        put(a, enc_in, blocks)
        lo, hi = paint(b, enc_out, FILL)
        rc, olen, st = gpu_ctx.encode_blocks_raw(m, n, a.ctypes.data, enc_in, zpq.FLAG_PP, b.ctypes.data, enc_out)
        assert rc == 0 and (st == 0).all() and [int(x) for x in olen] == [len(w) for w in want]
        assert gpu_ctx.last_host_transfer == 1 << 8 and gpu_ctx.last_kernel_name == "k_pipe<encode>"
        check_slabs(b, enc_out, want, "encode across 2^32", False)
        untouched(b, lo, int(enc_out[0]), "in front of the window")
        untouched(b, int(enc_out[-1]), hi, "behind the window")
        # back: the streams, back to back across 2^32 in `a`, into slabs of len + 1600 in `b`
        paint(a, dec_in, 0x55)
        put(a, dec_in, want)
        lo, hi = paint(b, dec_out, FILL)
        rc, olen, cons, code, fb, st = gpu_ctx.decode_blocks_raw(m, n, a.ctypes.data, dec_in, zpq.FLAG_PP, b.ctypes.data, dec_out)
        assert rc == 0 and (st == 0).all() and (fb == 0).all()
        assert [int(x) for x in olen] == [len(x) for x in blocks] and [int(x) for x in cons] == [len(w) for w in want]
        assert [int(x) for x in code] == [A.decoded(name, c, len(x) + A.FAR_DEC_SLACK).final_code for x, c in zip(blocks, want)]
        check_slabs(b, dec_out, blocks, "decode across 2^32", False)
        untouched(b, lo, int(dec_out[0]), "in front of the window")
        untouched(b, int(dec_out[-1]), hi, "behind the window")
    finally:
        del a, b
