"""Every decoder and encoder held to the oracle where the nominal tests do not look: input windows that run past the
stream, streams without their tail or with a flipped bit, junk, and output slabs that are too small, exactly big enough
or empty (tests/offnominal_corpus.py).  All of status, out_len, the stored bytes, consumed, final_code and first_byte
come from the oracle's decode stopped where the kernels stop (Codec.decode_prefix); the device-pointer forms run on
sentinel-filled slabs, so that a byte stored behind min(out_len, cap) shows; the encoders meet slabs of 0, 1, 3, 4,
len - 1 and len bytes; and the handles that keep state between segments are followed through a damaged segment."""
import random

import numpy as np
import pytest

import general_models as GM
import offnominal_corpus as OC
import oracle_lib as O
from test_gpu_chain_models import BUDGET, Run as ChainRun, _block, dec_names, enc_names, knobs
from test_gpu_general_models import Run as GeneralRun

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
PAD = 256                                                   # sentinel bytes behind the last slab; junk behind the last stream
SPECIALISED = ("level1", "level2", "level3", "level4", "level5")        # (one shipped level per k_chain specialisation)
DEV_MODELS = SPECIALISED + ("cm_alias", "n17")


def _offsets(lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(lengths, dtype=np.uint64))
    return off


def _source(streams):
    return np.frombuffer(b"".join(streams) + b"\xee" * PAD, dtype=np.uint8).copy()


def raw_decode(zpq, ctx, model, streams, caps, flags):
    """zpq_decode_blocks with a slab size per block.  Returns (out, out_off, out_len, consumed, final_code, first_byte,
    status)."""
    nb = len(streams)
    src, in_off, out_off = _source(streams), _offsets([len(s) for s in streams]), _offsets(caps)
    out = np.full(int(out_off[-1]) + PAD, SENTINEL, dtype=np.uint8)
    u32 = [np.zeros(nb, dtype=np.uint32) for _ in range(4)]
    status = np.full(nb, -99, dtype=np.int32)
    rc = zpq.lib().zpq_decode_blocks(ctx.h, model.h, nb, src.ctypes.data, in_off.ctypes.data, flags, out.ctypes.data,
                                     out_off.ctypes.data, u32[0].ctypes.data, u32[1].ctypes.data, u32[2].ctypes.data,
                                     u32[3].ctypes.data, status.ctypes.data)
    assert rc == 0, "library call failed: %d" % rc
    return (out, out_off) + tuple(u32) + (status,)


def raw_encode(zpq, ctx, model, blocks, caps, flags):
    nb = len(blocks)
    src, in_off, out_off = _source(blocks), _offsets([len(b) for b in blocks]), _offsets(caps)
    out = np.full(int(out_off[-1]) + PAD, SENTINEL, dtype=np.uint8)
    out_len = np.zeros(nb, dtype=np.uint32)
    status = np.full(nb, -99, dtype=np.int32)
    rc = zpq.lib().zpq_encode_blocks(ctx.h, model.h, nb, src.ctypes.data, in_off.ctypes.data, flags, out.ctypes.data,
                                     out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data)
    assert rc == 0, "library call failed: %d" % rc
    return out, out_off, out_len, status


def raw_set_decode(zpq, bs, streams, caps, flags, members=None):
    """zpq_blockset_decode_segments on set `bs` with a slab size per member (the binding takes one per call), the output
    sentinel-filled with a pad behind the last slab.  Returns what raw_decode returns."""
    n = len(streams)
    src, in_off, out_off = _source(streams), _offsets([len(s) for s in streams]), _offsets(caps)
    out = np.full(int(out_off[-1]) + PAD, SENTINEL, dtype=np.uint8)
    u32 = [np.zeros(n, dtype=np.uint32) for _ in range(4)]
    status = np.full(n, -99, dtype=np.int32)
    mem = None if members is None else np.asarray(members, dtype=np.int32)
    rc = zpq.lib().zpq_blockset_decode_segments(bs.h, n, None if mem is None else mem.ctypes.data, src.ctypes.data,
                                                in_off.ctypes.data, flags, out.ctypes.data, out_off.ctypes.data, u32[0].ctypes.data,
                                                u32[1].ctypes.data, u32[2].ctypes.data, u32[3].ctypes.data, status.ctypes.data)
    assert rc == 0, "library call failed: %d" % rc
    return (out, out_off) + tuple(u32) + (status,)


def dev_call(zpq, ctx, model, decode, streams, caps, flags):
    """The device-pointer form on an output tensor filled with the sentinel, a pad of it behind the last slab."""
    import torch
    dev = torch.device("cuda:0")
    nb = len(streams)
    d_in = torch.from_numpy(_source(streams)).to(dev)
    in_off = torch.from_numpy(_offsets([len(s) for s in streams]).astype(np.int64)).to(dev)
    out_off_h = _offsets(caps)
    out_off = torch.from_numpy(out_off_h.astype(np.int64)).to(dev)
    d_out = torch.full((int(out_off_h[-1]) + PAD,), SENTINEL, dtype=torch.uint8, device=dev)
    meta = [torch.full((nb,), -99, dtype=torch.int32, device=dev) for _ in range(5)]
    torch.cuda.synchronize()                               # order torch's fills before the ctx stream's kernels
    if decode:
        ctx.decode_blocks_dev(model, nb, d_in.data_ptr(), in_off.data_ptr(), flags, d_out.data_ptr(), out_off.data_ptr(),
                              *[m.data_ptr() for m in meta])
    else:
        ctx.encode_blocks_dev(model, nb, d_in.data_ptr(), in_off.data_ptr(), flags, d_out.data_ptr(), out_off.data_ptr(),
                              meta[0].data_ptr(), meta[4].data_ptr())
    ctx.sync()
    host = [m.cpu().numpy() for m in meta]
    return (d_out.cpu().numpy(), out_off_h) + tuple(h.view(np.uint32) for h in host[:4]) + (host[4],)


def check_decode(tag, batch, caps, want, got, whole=False):
    """All six outputs of every block against the oracle's.  whole: the output buffer was sentinel-filled on the device --
    every byte of it that is not a stored byte of some block, the pad included, must still hold the sentinel."""
    out, out_off, out_len, consumed, code, first, status = got
    cols = (("status", status.astype(np.int64), [w.status for w in want]), ("out_len", out_len, [w.out_len for w in want]),
            ("consumed", consumed, [w.consumed for w in want]), ("final_code", code, [w.final_code for w in want]),
            ("first_byte", first, [w.first_byte for w in want]))
    for name, have, exp in cols:
        bad = np.nonzero(have.astype(np.int64) != np.asarray(exp, dtype=np.int64))[0]
        if len(bad):
            i = int(bad[0])
            raise AssertionError("%s: %s of block %d (%s, %d coded bytes, slab %d): got %d, oracle %d; %d blocks differ; oracle %r"
                                 % (tag, name, i, batch[i].what, len(batch[i].stream), caps[i], int(have[i]), exp[i], len(bad),
                                    want[i]._replace(data=len(want[i].data))))
    image = np.full(len(out), SENTINEL, dtype=np.uint8)
    for i, w in enumerate(want):
        o = int(out_off[i])
        image[o:o + len(w.data)] = np.frombuffer(w.data, dtype=np.uint8)
        if not whole:
            assert out[o:o + len(w.data)].tobytes() == w.data, (tag, "bytes of block", i, batch[i].what, caps[i])
    if whole:
        bad = np.nonzero(out != image)[0]
        if len(bad):
            at = int(bad[0])
            i = int(np.searchsorted(out_off, at, side="right")) - 1
            raise AssertionError("%s: byte %d (block %d%s, slab %d, out_len %d, offset %d in its slab) is %#x, expected %#x; %d bytes differ"
                                 % (tag, at, i, " " + batch[i].what if i < len(batch) else " = the pad", caps[min(i, len(caps) - 1)],
                                    want[min(i, len(want) - 1)].out_len, at - int(out_off[min(i, len(caps))]), int(out[at]),
                                    int(image[at]), len(bad)))


def three_slabs(model, pp, batch):
    for which in ("roomy", "tight", "tight-1"):
        caps = OC.slabs(model, pp, batch, which)
        yield which, caps, OC.expectations(model, pp, batch, caps)


# ---------------------------------------------------------------- (a) every decoder, through the host-pointer form
@pytest.mark.parametrize("pp", [True, False], ids=["pp", "raw"])
@pytest.mark.parametrize("level", OC.CHAIN_LEVELS)
def test_chain_decoders_on_damaged_streams(zpq, gpu_ctx, monkeypatch, level, pp):
    name = "level%d" % level
    run = ChainRun(zpq, gpu_ctx, monkeypatch, OC.header_of(name))
    spec, batch = run.rt["nch_spec"], OC.layout(name, pp)
    F = zpq.FLAG_PP if pp else 0
    variants = [({}, 0), ({"ZPQ_SPARSE_MODE": "never"}, 0), ({"ZPQ_SPARSE_MODE": "always"}, 0), ({}, zpq.FLAG_GENERIC)]
    if spec in (5, 6):
        variants.append(({"ZPQ_DEC_HYP16": "0"}, 0))
    if spec in (2, 3, 5) and not run.rt["has_mix2"]:
        variants.append(({"ZPQ_DEC_PIPE": "1", "ZPQ_SPARSE_MODE": "never"}, 0))
    seen = set()

    def decode(which, caps, want, env, flags, slots=None):
        with knobs(monkeypatch, **env):
            got = raw_decode(zpq, gpu_ctx, run.model, [c.stream for c in batch], caps, F | flags)
            kernel = gpu_ctx.last_kernel_name
            ok = {"k_generic<decode>"} if flags else dec_names(run.rt, gpu_ctx, env)
            assert kernel in ok, (kernel, ok, env)
            assert slots is None or gpu_ctx.last_slots == slots
        seen.add(kernel + "".join(" %s=%s" % kv for kv in sorted(env.items())) + (" store" if gpu_ctx.last_line_store else ""))
        check_decode("%s pp=%d %s %s %s" % (name, pp, which, kernel, env), batch, caps, want, got)

    for which, caps, want in three_slabs(name, pp, batch):
        for env, flags in variants:
            decode(which, caps, want, env, flags)
        if level == 2 and which == "tight":
            # five state slots: a lane decodes a damaged block and then a good one
            zpq.lib().zpq_ctx_set_state_budget(gpu_ctx.h, 5 * run.model.state_bytes + 1000)
            try:
                decode(which, caps, want, {"ZPQ_SPARSE_MODE": "never"}, 0, slots=5)
            finally:
                zpq.lib().zpq_ctx_set_state_budget(gpu_ctx.h, BUDGET)
    print("\nkernels %s pp=%d (%d blocks): %s" % (name, pp, len(batch), sorted(seen)))
    kernels = {s.split()[0] for s in seen}
    assert kernels == {"k_chain<decode>", "k_generic<decode>"} | ({"k_dpipe<decode>"} if level <= 3 else set()), seen
    assert any("ZPQ_DEC_HYP16=0" in s for s in seen) == (level in (3, 4))


@pytest.mark.parametrize("pp", [True, False], ids=["pp", "raw"])
@pytest.mark.parametrize("name", OC.GENERAL)
def test_general_decoders_on_damaged_streams(zpq, gpu_ctx, monkeypatch, name, pp):
    run = GeneralRun(zpq, gpu_ctx, monkeypatch, OC.header_of(name))
    assert run.rt == GM.NAMED[name][1]
    batch = OC.layout(name, pp)
    F = zpq.FLAG_LANES | (zpq.FLAG_PP if pp else 0)
    variants = [({}, 0)]
    if run.rt[2]:
        if run.rt[1]:
            variants += [({"ZPQ_GDEC_BPW": "32"}, 0), ({"ZPQ_GDEC_BPW": "16"}, 0), ({"ZPQ_DEC_GPIPE": "0"}, 0)]
        if run.rows:
            variants.append(({"ZPQ_DEC_GPIPE": "0", "ZPQ_LANES_ROWS": "0"}, 0))
        variants.append(({}, zpq.FLAG_GENERIC))
    seen = set()

    def decode(which, caps, want, env, flags, slots=None):
        with knobs(monkeypatch, **env):
            got = raw_decode(zpq, gpu_ctx, run.model, [c.stream for c in batch], caps, F | flags)
            kernel = gpu_ctx.last_kernel_name
            assert kernel == run.kernel(True, flags, env), (kernel, env)
            assert slots is None or gpu_ctx.last_slots == slots
        seen.add(kernel + (" bpw" + env["ZPQ_GDEC_BPW"] if "ZPQ_GDEC_BPW" in env else ""))
        check_decode("%s pp=%d %s %s %s" % (name, pp, which, kernel, env), batch, caps, want, got)

    for which, caps, want in three_slabs(name, pp, batch):
        for env, flags in variants:
            decode(which, caps, want, env, flags)
        if name == "cm_alias" and which == "tight":
            zpq.lib().zpq_ctx_set_state_budget(gpu_ctx.h, 5 * run.model.state_bytes + 1000)
            try:
                for env, flags in variants[:1] + variants[3:5]:             # k_gdec, k_rows, k_lanes
                    decode(which, caps, want, env, flags, slots=5)
            finally:
                zpq.lib().zpq_ctx_set_state_budget(gpu_ctx.h, BUDGET)
    print("\nkernels %s pp=%d (%d blocks): %s" % (name, pp, len(batch), sorted(seen)))
    want_seen = {"k_generic<decode>"}
    if run.rt[2]:
        want_seen.add("k_lanes<decode>")
    if run.rows:
        want_seen.add("k_rows<decode>")
    if run.rt[1]:
        want_seen |= {"k_gdec<decode>", "k_gdec<decode> bpw32", "k_gdec<decode> bpw16"}
    assert seen == want_seen


# ---------------------------------------------------------------- (b) device-pointer form, sentinel-filled slabs
@pytest.mark.parametrize("name", DEV_MODELS)
def test_device_pointer_decode_leaves_the_rest_of_every_slab_alone(zpq, gpu_ctx, monkeypatch, name):
    """Tight slabs (the original's length, then a byte less and one empty slab) on an output tensor filled with 0xA5: all
    six outputs as above, and every byte from min(out_len, cap) on of every slab and the 256 bytes behind the last slab
    still hold 0xA5."""
    chain = name.startswith("level")
    run = (ChainRun if chain else GeneralRun)(zpq, gpu_ctx, monkeypatch, OC.header_of(name))
    batch = OC.layout(name, True)
    F = zpq.FLAG_PP | (0 if chain else zpq.FLAG_LANES)
    for which in ("tight", "tight-1"):
        caps = OC.slabs(name, True, batch, which)
        got = dev_call(zpq, gpu_ctx, run.model, True, [c.stream for c in batch], caps, F)
        kernel = gpu_ctx.last_kernel_name
        assert kernel == ("k_chain<decode>" if chain else run.kernel(True, 0, {}))
        check_decode("%s dev %s %s" % (name, which, kernel), batch, caps, OC.expectations(name, True, batch, caps), got, whole=True)
    print("\nkernel %s: %s" % (name, kernel))


# ---------------------------------------------------------------- (c) encoders and slabs that are too small
ENC_SIZES = (0, 1, 2, 17, 64, 300, 1500)


def encoder_blocks(name, pp):
    """42 blocks: every length of ENC_SIZES with every slab of 0, 1, 3, 4, len - 1 and len bytes (len = the oracle's coded
    length).  Returns (blocks, the oracle's streams, slab sizes)."""
    r = random.Random(313)
    sizes = [n for n in ENC_SIZES if n <= 300 or name not in OC.SMALL_ONLY]
    blocks = [_block(r, i % 4, sizes[i % len(sizes)]) for i in range(6 * len(sizes))]
    want = O.encode_blocks(OC.header_of(name), blocks, pp=pp, nthreads=8)
    caps = [(0, 1, 3, 4, len(w) - 1, len(w))[i % 6] for i, w in enumerate(want)]
    return blocks, want, caps


def check_encode(tag, blocks, want, caps, got, whole=False):
    out, out_off, out_len, status = got
    assert [int(x) for x in out_len] == [len(w) for w in want], (tag, "out_len: the encoders keep counting")
    assert [int(s) for s in status] == [0 if cap >= len(w) else -7 for w, cap in zip(want, caps)], (tag, list(status))
    assert any(cap == len(w) for w, cap in zip(want, caps)) and any(cap == len(w) - 1 for w, cap in zip(want, caps))
    image = np.full(len(out), SENTINEL, dtype=np.uint8)
    for i, (w, cap) in enumerate(zip(want, caps)):
        o = int(out_off[i])
        image[o:o + min(cap, len(w))] = np.frombuffer(w[:cap], dtype=np.uint8)
        assert out[o:o + min(cap, len(w))].tobytes() == w[:cap], (tag, "stored prefix of block", i, len(blocks[i]), cap, len(w))
    if whole:
        bad = np.nonzero(out != image)[0]
        assert not len(bad), (tag, "byte", int(bad[0]), "of", len(out), "block", int(np.searchsorted(out_off, bad[0], side="right")) - 1,
                              hex(int(out[bad[0]])), len(bad))


@pytest.mark.parametrize("pp", [True, False], ids=["pp", "raw"])
@pytest.mark.parametrize("level", OC.CHAIN_LEVELS)
def test_chain_encoders_on_slabs_too_small(zpq, gpu_ctx, monkeypatch, level, pp):
    name = "level%d" % level
    run = ChainRun(zpq, gpu_ctx, monkeypatch, OC.header_of(name))
    blocks, want, caps = encoder_blocks(name, pp)
    F = zpq.FLAG_PP if pp else 0
    seen = set()

    def encode(n, env):
        with knobs(monkeypatch, **env):
            got = raw_encode(zpq, gpu_ctx, run.model, blocks[:n], caps[:n], F)
            kernel = gpu_ctx.last_kernel_name
            assert kernel in enc_names(run.rt, gpu_ctx, env), (kernel, env)
        seen.add(kernel)
        check_encode("%s pp=%d %s %s" % (name, pp, kernel, env), blocks[:n], want[:n], caps[:n], got)

    encode(len(blocks), {})
    encode(len(blocks), {"ZPQ_ENC_PIPE": "0"})
    if run.rt["nch_spec"] == 2:
        encode(len(blocks), {"ZPQ_ENC_SPLIT": "0"})
    encode(11, {})                                           # (too few blocks for a pipeline)
    print("\nkernels %s pp=%d: %s" % (name, pp, sorted(seen)))
    assert seen == {"k_pipe<encode>", "k_chain<encode>"} | ({"k_pipe2<encode>"} if level == 1 else set())


@pytest.mark.parametrize("pp", [True, False], ids=["pp", "raw"])
@pytest.mark.parametrize("name", ["cm_alias", "match_idx_gt_buf", "n65"])
def test_general_encoders_on_slabs_too_small(zpq, gpu_ctx, monkeypatch, name, pp):
    run = GeneralRun(zpq, gpu_ctx, monkeypatch, OC.header_of(name))
    blocks, want, caps = encoder_blocks(name, pp)
    F = zpq.FLAG_LANES | (zpq.FLAG_PP if pp else 0)
    variants = [({}, 0)]
    if run.rt[0]:
        variants += [({"ZPQ_GPIPE_BATCH": "0"}, 0), ({"ZPQ_ENC_GPIPE": "0"}, 0), ({"ZPQ_ENC_GPIPE": "0", "ZPQ_LANES_ROWS": "0"}, 0),
                     ({}, zpq.FLAG_GENERIC)]
    seen = set()
    for env, flags in variants:
        with knobs(monkeypatch, **env):
            got = raw_encode(zpq, gpu_ctx, run.model, blocks, caps, F | flags)
            kernel = gpu_ctx.last_kernel_name
            assert kernel == run.kernel(False, flags, env), (kernel, env)
        seen.add(kernel + (" bit-serial" if env.get("ZPQ_GPIPE_BATCH") == "0" else ""))
        check_encode("%s pp=%d %s %s" % (name, pp, kernel, env), blocks, want, caps, got)
    print("\nkernels %s pp=%d: %s" % (name, pp, sorted(seen)))
    assert seen == ({"k_gpipe<encode>", "k_gpipe<encode> bit-serial", "k_rows<encode>", "k_lanes<encode>", "k_generic<encode>"}
                    if run.rt[0] else {"k_generic<encode>"})


@pytest.mark.parametrize("name", DEV_MODELS)
def test_device_pointer_encode_leaves_the_rest_of_every_slab_alone(zpq, gpu_ctx, monkeypatch, name):
    chain = name.startswith("level")
    run = (ChainRun if chain else GeneralRun)(zpq, gpu_ctx, monkeypatch, OC.header_of(name))
    blocks, want, caps = encoder_blocks(name, True)
    F = zpq.FLAG_PP | (0 if chain else zpq.FLAG_LANES)
    out, out_off, out_len, _, _, _, status = dev_call(zpq, gpu_ctx, run.model, False, blocks, caps, F)
    kernel = gpu_ctx.last_kernel_name
    assert kernel in (enc_names(run.rt, gpu_ctx, {}) if chain else {run.kernel(False, 0, {})})
    check_encode("%s dev %s" % (name, kernel), blocks, want, caps, (out, out_off, out_len, status), whole=True)
    print("\nkernel %s: %s" % (name, kernel))


# ---------------------------------------------------------------- (d) state that outlives a damaged segment
def _text(r, n):
    return bytes(r.choice(b"etaoin shrdlu\n") for _ in range(n))


@pytest.mark.parametrize("name", ["level2", "cm_alias"])
def test_block_decodes_on_after_a_truncated_segment(zpq, gpu_ctx, monkeypatch, name):
    """Three segments of one block, the second without its last 5 bytes: every output of every segment equals one oracle
    Codec decoding the three in turn (the third on the state the damaged second one left)."""
    ChainRun(zpq, gpu_ctx, monkeypatch, OC.header_of("level2"))            # (clears the knobs)
    hdr = OC.header_of(name)
    r = random.Random(61)
    enc = O.Codec(hdr)
    coded = [enc.encode(_text(r, n)) for n in (300, 257, 120)]
    coded[1] = coded[1][:-5]
    cap = 1024
    block = zpq.Block(gpu_ctx, zpq.Model(header=hdr))
    dec = O.Codec(hdr)
    try:
        for i, s in enumerate(coded):
            want = OC.shape(dec.decode_prefix(s, cap + 1), cap, True)
            assert want.status == 0 and want.consumed == len(s) and (i != 1 or want.final_code == 0)
            data, consumed, code, first = block.decode_segment(s, cap)
            assert (len(data), data, consumed, code, first) == (want.out_len, want.data, want.consumed, want.final_code,
                                                               want.first_byte), (name, "segment", i)
    finally:
        block.close()


def test_blockset_follows_damaged_segments_per_member(zpq, gpu_ctx, monkeypatch):
    """Level 2, 12 members, two segments each and a third.  Member 3's second segment has a flipped bit (roomy slab: it
    ends somewhere else), member 7's is truncated and meets a slab of the original's length (overflow): every member
    equals its own oracle Codec's sequence, member 7 stays failed, the other eleven decode a third segment -- member 3
    on the state its damaged segment left."""
    ChainRun(zpq, gpu_ctx, monkeypatch, OC.header_of("level2"))
    hdr = OC.header_of("level2")
    r = random.Random(62)
    nm, roomy = 12, 2048
    data = [[_text(r, r.choice([200, 255, 300])) for _ in range(3)] for _ in range(nm)]
    coded = []
    for m in range(nm):
        enc = O.Codec(hdr)
        coded.append([enc.encode(seg) for seg in data[m]])
    for bit in range(64):                                    # a flipped bit after which the stream still ends inside the slab
        t = bytearray(coded[3][1])
        t[len(t) // 2 + bit // 8] ^= 1 << (bit % 8)
        probe = O.Codec(hdr)
        probe.decode_prefix(coded[3][0], roomy + 1)
        res = probe.decode_prefix(bytes(t), roomy + 1)
        if res[1] <= roomy and res[1] != len(data[3][1]) + 1:
            coded[3][1] = bytes(t)
            break
    else:
        raise AssertionError("no flipped bit ends inside the slab")
    coded[7][1] = coded[7][1][:-5]
    model = zpq.Model(header=hdr)
    bs = zpq.BlockSet(gpu_ctx, model, nm, max_member_bytes=8192)
    oracles = [O.Codec(hdr) for _ in range(nm)]
    try:
        for seg in range(3):
            streams = [coded[m][seg] for m in range(nm)]
            caps = [roomy] * nm
            if seg == 1:
                caps[7] = len(data[7][1])
            want = [OC.shape(oracles[m].decode_prefix(streams[m], caps[m] + 1), caps[m], True) for m in range(nm)]
            if seg == 1:
                assert want[7].status == -7 and want[3].status == 0 and want[3].out_len != len(data[3][1])
            if seg == 2:
                want[7] = OC.Expected(-7, 0, b"", 0, 0, OC.NO_BYTE)         # failed: reported without coding
            got = raw_set_decode(zpq, bs, streams, caps, zpq.FLAG_PP)
            assert gpu_ctx.last_kernel_name == "k_chain<decode>"
            batch = [OC.Case("segment", "member %d segment %d" % (m, seg), streams[m], len(data[m][seg])) for m in range(nm)]
            check_decode("blockset segment %d" % seg, batch, caps, want, got)
            for m in range(nm):
                if seg == 0 or m not in (3, 7):                              # (the undamaged ones are the data)
                    assert want[m].data == data[m][seg] and want[m].status == 0, (seg, m)
    finally:
        bs.close()
        model.close()
