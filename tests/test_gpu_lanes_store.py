"""k_rows / k_lanes on the compact line store (ZPQ_FLAG_LINESTORE / ZPQ_LANES_STORE) against the CPU oracle: parity of every
store form with the request made by flag and by environment, slots reused by several blocks (stale tags and lines), batches
that only fit on the store, a block the store refuses next to blocks it codes, the cases in which the request decides
nothing, and a chain model forced onto the route.  Models and blocks: tests/lanes_store.py (a store of 256 lines)."""
import numpy as np
import pytest

import general_models as GM
import lanes_store as LS
import oracle_lib as O

pytestmark = pytest.mark.gpu

KNOBS = ("ZPQ_LANES_STORE", "ZPQ_SPARSE_MODE", "ZPQ_SPARSE_FORCE_LOG2", "ZPQ_LANES_ROWS", "ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE",
         "ZPQ_VM_PIPE", "ZPQ_GPIPE_BATCH", "ZPQ_GDEC_BPW")
E_NOMEM, E_TOOBIG = -6, -4
CASES = [(n, how, False) for n in sorted(LS.MODELS) for how in ("flag", "env")] + [(n, how, True) for n in LS.ROWS0 for how in ("flag", "env")]

_WANT = {}


def want(name):
    """The oracle's streams of the 21 fitting blocks, computed once per model."""
    if name not in _WANT:
        _WANT[name] = [O.Codec(LS.MODELS[name]).encode(b, pp=True) for b in LS.fitting_blocks()]
    return _WANT[name]


def clean(mp, log2=LS.LOG2, rows0=False):
    for k in KNOBS:
        mp.delenv(k, raising=False)
    if log2:
        mp.setenv("ZPQ_SPARSE_FORCE_LOG2", str(log2))
    if rows0:
        mp.setenv("ZPQ_LANES_ROWS", "0")


def lanes_name(zpq, model, decode):
    return GM._lib(zpq).zpq_lanes_kernel_name(model.h, decode).decode()


def code_both_ways(zpq, ctx, model, blocks, streams, flags):
    """Encode the blocks, decode the streams; everything the two calls return and what the ctx reports about them."""
    coded, st, olen = ctx.encode_blocks(model, blocks, flags=flags)
    enc = (coded, [int(s) for s in st], [int(x) for x in olen], ctx.last_kernel_name, ctx.last_line_store, ctx.last_slots)
    dec, st, cons, code, first = ctx.decode_blocks(model, streams, cap=max(len(b) for b in blocks) + 64, flags=flags)
    return enc, (dec, [int(s) for s in st], [int(c) for c in cons], [int(c) for c in code], [int(f) for f in first],
                 ctx.last_kernel_name, ctx.last_line_store, ctx.last_slots)


def check_parity(zpq, ctx, model, blocks, streams, flags, store, names=None, slots=None):
    enc, dec = code_both_ways(zpq, ctx, model, blocks, streams, flags)
    assert enc[1] == [0] * len(blocks) and dec[1] == [0] * len(blocks), (enc[1], dec[1])
    for i, (c, w) in enumerate(zip(enc[0], streams)):
        assert c == w, ("encode, block", i, len(blocks[i]), len(c), len(w))
    assert enc[2] == [len(w) for w in streams]
    for i, (d, b) in enumerate(zip(dec[0], blocks)):
        assert d == b, ("decode, block", i, len(b), len(d))
    assert dec[2] == [len(w) for w in streams] and dec[4] == [0] * len(blocks)
    assert (enc[4], dec[6]) == (store, store), (enc[4], dec[6])
    if names:
        assert (enc[3], dec[5]) == names, (enc[3], dec[5])
    if slots:
        assert (enc[5], dec[7]) == (slots, slots), (enc[5], dec[7])
    return enc, dec


@pytest.mark.parametrize("name,how,rows0", CASES)
def test_parity_on_the_store(zpq, gpu_ctx, monkeypatch, name, how, rows0):
    clean(monkeypatch, rows0=rows0)
    hdr, blocks, streams = LS.MODELS[name], LS.fitting_blocks(), want(name)
    model = zpq.Model(header=hdr)
    assert not model.has_fast_path or name == "e_twins"          # (no chain kernel takes any of them: no ZPQ_FLAG_LANES needed)
    rt = GM.route(zpq, model)
    today = ("k_gpipe<encode>" if rt[0] else rt[3] + "<encode>", "k_gdec<decode>" if rt[1] else rt[3] + "<decode>")
    # without the request: dense tables and the kernels of today (ZPQ_SPARSE_FORCE_LOG2 alone decides nothing here)
    _, dense = check_parity(zpq, gpu_ctx, model, blocks, streams, zpq.FLAG_PP, 0, names=today)
    flags = zpq.FLAG_PP
    if how == "flag":
        flags |= zpq.FLAG_LINESTORE
    else:
        monkeypatch.setenv("ZPQ_LANES_STORE", "1")
    names = (lanes_name(zpq, model, 0), lanes_name(zpq, model, 1))
    assert names == ((GM.LANES if rows0 or hdr[4] > 16 else GM.ROWS) + "<encode>", (GM.LANES if rows0 or hdr[4] > 16 else GM.ROWS) + "<decode>")
    _, dec = check_parity(zpq, gpu_ctx, model, blocks, streams, flags, LS.CAP, names=names)
    assert dec[:5] == dense[:5]                                   # the blocks, status, consumed, final_code, first_byte


@pytest.mark.parametrize("name", ["a_rows_vmh", "c_lanes_vmh", "c_lanes_vm", "d_c4b"])
def test_five_slots_code_21_blocks_in_turn(zpq, monkeypatch, name):
    clean(monkeypatch)
    model = zpq.Model(header=LS.MODELS[name])
    ctx = zpq.Context(0)
    try:
        zpq.lib().zpq_ctx_set_state_budget(ctx.h, 5 * model.lanes_store_slot_bytes(LS.CAP) + 1000)
        check_parity(zpq, ctx, model, LS.fitting_blocks(), want(name), zpq.FLAG_PP | zpq.FLAG_LINESTORE, LS.CAP, slots=5)
    finally:
        ctx.close()


def test_a_batch_that_fits_on_the_store_alone(zpq, monkeypatch):
    clean(monkeypatch)
    hdr = LS.H([[LS.ICM, 20], [LS.CM, 8, 255], [LS.MIX2, 4, 0, 1, 24, 255]], 2, 8, GM.hashchain(3))   # a table of 64 MiB
    model = zpq.Model(header=hdr)
    blocks = LS.fitting_blocks()
    streams = [O.Codec(hdr).encode(b, pp=True) for b in blocks]
    ctx = zpq.Context(0)
    try:
        L = zpq.lib()
        L.zpq_ctx_set_state_budget(ctx.h, 200 << 20)             # three dense slots (nothing is allocated before a launch)
        plain, asked = ctx.resident_capacity(model, zpq.FLAG_PP), ctx.resident_capacity(model, zpq.FLAG_PP | zpq.FLAG_LINESTORE)
        assert 1 <= plain <= 3 < asked, (plain, asked)
        L.zpq_ctx_set_state_budget(ctx.h, 4 << 20)               # no dense slot
        with pytest.raises(zpq.ZpqError) as e:
            ctx.encode_blocks(model, blocks, flags=zpq.FLAG_PP)
        assert e.value.code == E_NOMEM
        with pytest.raises(zpq.ZpqError) as e:
            ctx.decode_blocks(model, streams, cap=164, flags=zpq.FLAG_PP)
        assert e.value.code == E_NOMEM
        check_parity(zpq, ctx, model, blocks, streams, zpq.FLAG_PP | zpq.FLAG_LINESTORE, LS.CAP,
                     names=("k_rows<encode>", "k_rows<decode>"))
    finally:
        ctx.close()


def _raw(ctx, model, decode, items, cap, flags):
    """A raw batch call on a sentinel-filled output buffer with equal slabs: (out_len, status, the whole buffer)."""
    off = np.zeros(len(items) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in items])
    src = np.frombuffer(b"".join(items) + b"\0", dtype=np.uint8)
    out_off = np.arange(len(items) + 1, dtype=np.uint64) * np.uint64(cap)
    out = np.full(int(out_off[-1]) + 1, 0xA5, dtype=np.uint8)
    fn = ctx.decode_blocks_raw if decode else ctx.encode_blocks_raw
    r = fn(model, len(items), src.ctypes.data, off, flags, out.ctypes.data, out_off)
    assert r[0] == 0, r[0]
    return [int(x) for x in r[1]], [int(s) for s in r[-1]], out


@pytest.mark.parametrize("rows0", [False, True])
def test_the_store_refuses_one_block_and_codes_the_others(zpq, gpu_ctx, monkeypatch, rows0):
    clean(monkeypatch, rows0=rows0)
    hdr = LS.MODELS[LS.OVERFLOW_MODEL]
    model = zpq.Model(header=hdr)
    flags = zpq.FLAG_PP | zpq.FLAG_LINESTORE
    blocks, streams = LS.fitting_blocks(), list(want(LS.OVERFLOW_MODEL))
    big = LS.overflow_block()
    with_big = blocks[:7] + [big] + blocks[8:]
    for decode, items, calm, cap in ((0, with_big, blocks, 17 * 400 + 4096),
                                     (1, streams[:7] + [O.Codec(hdr).encode(big, pp=True)] + streams[8:], streams, 464)):
        olen, status, out = _raw(gpu_ctx, model, decode, items, cap, flags)
        assert gpu_ctx.last_line_store == LS.CAP and gpu_ctx.last_kernel_name == lanes_name(zpq, model, decode)
        olen0, status0, out0 = _raw(gpu_ctx, model, decode, calm, cap, flags)
        assert status0 == [0] * 21
        assert status[7] == E_TOOBIG and status[:7] + status[8:] == [0] * 20, status
        assert olen[:7] + olen[8:] == olen0[:7] + olen0[8:]
        # nothing outside block 7's slab differs from the batch without the block: coded bytes, untouched sentinels
        assert np.array_equal(out[:7 * cap], out0[:7 * cap]) and np.array_equal(out[8 * cap:], out0[8 * cap:])
        expect = blocks if decode else streams
        for i in range(21):
            if i != 7:
                assert out[i * cap:i * cap + olen[i]].tobytes() == expect[i], i


def _same_as_without(zpq, ctx, model, blocks, streams, base_flags):
    plain = code_both_ways(zpq, ctx, model, blocks, streams, base_flags)
    asked = code_both_ways(zpq, ctx, model, blocks, streams, base_flags | zpq.FLAG_LINESTORE)
    assert asked == plain                                          # bytes, results, kernel, line store figure, slots
    assert plain[0][0] == streams and plain[1][0] == blocks
    return plain


def test_a_request_that_is_not_honoured_decides_nothing(zpq, gpu_ctx, monkeypatch):
    blocks = LS.fitting_blocks()
    name = "a_rows_vmh"
    model = zpq.Model(header=LS.MODELS[name])
    # a level-2 call without ZPQ_FLAG_LANES: the chain kernels have the model
    clean(monkeypatch, log2=0)
    l2 = zpq.Model(level=2)
    plain = _same_as_without(zpq, gpu_ctx, l2, blocks, O.encode_blocks(l2.header, blocks), zpq.FLAG_PP)
    assert plain[0][3] in ("k_pipe<encode>", "k_chain<encode>") and plain[0][4] == 0
    # ZPQ_SPARSE_MODE=never; ZPQ_LANES_STORE=0 against the flag; a store larger than every table
    for env in ({"ZPQ_SPARSE_MODE": "never"}, {"ZPQ_LANES_STORE": "0"}, {"ZPQ_SPARSE_FORCE_LOG2": "20"}):
        clean(monkeypatch)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        plain = _same_as_without(zpq, gpu_ctx, model, blocks, want(name), zpq.FLAG_PP)
        assert plain[0][3:5] == ("k_gpipe<encode>", 0) and plain[1][5:7] == ("k_gdec<decode>", 0), env


def test_level_3_forced_onto_the_route(zpq, gpu_ctx, monkeypatch):
    clean(monkeypatch)
    model = zpq.Model(level=3)
    blocks = LS.fitting_blocks()
    streams = [O.Codec(model.header).encode(b, pp=True) for b in blocks]
    check_parity(zpq, gpu_ctx, model, blocks, streams, zpq.FLAG_PP | zpq.FLAG_LANES | zpq.FLAG_LINESTORE, LS.CAP,
                 names=("k_rows<encode>", "k_rows<decode>"))
