"""The oracle's decode with the kernels' stop rule (zo_decode_prefix) and the corpus of truncated and damaged streams
built on it (tests/offnominal_corpus.py), on the host: the C oracle against the independent restatement (oracle/pyref)
driven by hand to the same stop rule; the conditions that keep the GPU test (test_gpu_offnominal.py) from going hollow;
the batch layout; and what truncation and a flipped bit do to a stream, as relations."""
import collections
import os
import random
import sys

import pytest

import offnominal_corpus as OC
import oracle_lib as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "pyref"))
import zpaq_pyref as P  # noqa: E402


def pyref_prefix(hdr, stream, cap):
    """Decoder.decompress by hand: a byte is stored while fewer than cap are, stop at EOF or right after byte cap + 1."""
    pr = P.new_model(hdr)
    pr.reset()
    d = P.Decoder(pr, stream)
    out, n = bytearray(), 0
    while True:
        c = d.decompress()
        if c < 0:
            break
        if n < cap:
            out.append(c)
        n += 1
        if n > cap:
            break
    return bytes(out), n, d.pos, d.code


@pytest.mark.parametrize("model", ["level1", "level2", "level3", "cm_alias", "match_idx_gt_buf"])
def test_prefix_decode_matches_second_restatement(model):
    """A dozen damaged streams per model (originals of at most 300 bytes), each with a slab that holds everything, one
    that is a byte short of the original and one of a third of it; an empty slab for the first."""
    hdr = OC.header_of(model)
    r = random.Random(len(model))
    picked = []
    for pp in (True, False):
        pool = [c for c in OC.cases(model, pp) if c.nominal <= 300 and len(c.stream) <= 400]
        for kind in OC.MUTATIONS:
            of_kind = [c for c in pool if c.kind == kind]
            picked += [(pp, c) for c in r.sample(of_kind, 2 if kind in ("trunc", "flip") else 1)]
    assert len(picked) >= 12
    for i, (pp, c) in enumerate(picked):
        for cap in [700, max(c.nominal - 1, 0), c.nominal // 3] + ([0] if i == 0 else []):
            got = O.Codec(hdr).decode_prefix(c.stream, cap)
            assert got[:4] == pyref_prefix(hdr, c.stream, cap), (model, c.what, cap)
            assert not got[4]


def test_prefix_decode_agrees_with_the_full_decode():
    """Where the stream ends by EOF inside the slab the two entries return the same; the stored bytes of a smaller slab are
    a prefix, out_len is cap + 1 and consumed is no larger."""
    hdr = O.level_header(2)
    data = bytes(random.Random(3).choice(b"etaoin shrdlu\n") for _ in range(500))
    s = O.Codec(hdr).encode(data)
    full, cons = O.Codec(hdr).decode(s)
    assert O.Codec(hdr).decode_prefix(s, 501)[:3] == (full, 501, cons) and full[1:] == data
    assert O.Codec(hdr).decode_prefix(s, 502)[:3] == (full, 501, cons)
    for cap in (0, 1, 100, 500):
        got = O.Codec(hdr).decode_prefix(s, cap)
        assert got[0] == full[:cap] and got[1] == cap + 1 and got[2] <= cons
    with pytest.raises(OverflowError):
        O.Codec(hdr).decode(s, cap=500)


@pytest.mark.parametrize("model", OC.MODELS)
def test_corpus_conditions(model):
    """Per model and mutation kind, by the oracle: a stream that ends by EOF inside the roomy slab, one that overflows a
    tight slab (exact and trail decode to the original's length: those overflow the slab that is a byte shorter, the
    other kinds the one of the original's length); a quarter of all cases ends with another length than the original's;
    no VM step overflow; and the layout has nonzero neighbours and truncated streams at every alignment."""
    total = differ = 0
    for pp in (True, False):
        batch = OC.layout(model, pp)
        assert len(batch) >= 70
        assert sorted(c for c in batch if c.kind != "filler") == sorted(OC.cases(model, pp))
        res = {w: OC.expectations(model, pp, batch, OC.slabs(model, pp, batch, w)) for w in ("roomy", "tight", "tight-1")}
        assert max(OC.slabs(model, pp, batch, "roomy")) <= OC.PROBE_CAP + 64
        count = collections.Counter()
        for i, c in enumerate(batch):
            for w in res:
                e = res[w][i]
                assert e.status in (0, -7), (model, c.what, w)
                count[c.kind, w, e.status] += 1
            if c.kind == "exact":
                short = -7 if OC.slabs(model, pp, batch, "tight-1")[i] < c.nominal else 0      # (an empty original has no shorter slab)
                assert (res["roomy"][i].status, res["tight"][i].status, res["tight-1"][i].status) == (0, 0, short)
                assert res["roomy"][i].out_len == res["tight"][i].out_len == c.nominal
                assert res["tight-1"][i].out_len == min(c.nominal, OC.slabs(model, pp, batch, "tight-1")[i] + 1)
                assert res["roomy"][i].consumed == len(c.stream)
            if c.kind == "trail":
                assert res["roomy"][i].out_len == c.nominal and res["roomy"][i].consumed < len(c.stream)
            if c.kind != "filler":
                total += 1
                differ += res["roomy"][i].out_len != c.nominal
        for kind in OC.MUTATIONS:
            assert count[kind, "roomy", 0] >= 1, (model, kind)
            assert count[kind, "tight-1", -7] >= 1, (model, kind)
            if kind not in ("exact", "trail"):
                assert count[kind, "tight", -7] >= 1, (model, kind)
        # the layout: back to back, nonzero bytes on both sides of every block, truncated streams at every alignment
        buf, off = b"".join(c.stream for c in batch), OC.offsets(batch)
        for i, c in enumerate(batch):
            if c.kind != "filler":                                              # (the fillers are what stands next to a zero)
                assert buf[off[i] - 1] != 0 and buf[off[i + 1]] != 0, (model, i, c.what)
        assert batch[0].kind == batch[-1].kind == "filler"
        trunc = [i for i, c in enumerate(batch) if c.kind == "trunc"]
        assert {off[i + 1] % 4 for i in trunc} == set(range(4))
        assert {off[i] % 16 for i in trunc} == set(range(16))
        assert {off[i + 1] % 4 for i in trunc if batch[i].stream} == set(range(4))
        print("\n%s pp=%d: %d blocks, roomy %d;" % (model, pp, len(batch), OC.slabs(model, pp, batch, "roomy")[0]),
              " ".join("%s %s eof %d ovf %d" % (k, w, count[k, w, 0], count[k, w, -7]) for k in OC.MUTATIONS for w in res))
    assert differ * 4 >= total, (model, differ, total)
    print("%s: %d of %d cases end with another length than the original's" % (model, differ, total))


def _text(n):
    r = random.Random(21)
    return bytes(r.choice(b"etaoin shrdlu\n") for _ in range(n))


SAMPLES = {"text1500": _text(1500), "random600": random.Random(22).randbytes(600), "zeros3000": bytes(3000)}


@pytest.mark.parametrize("level", [1, 2, 3])
def test_what_truncation_and_a_flipped_bit_do(level):
    """Measured with the oracle and held as relations (the counts per level are in EXPERIMENTS.md).  The last four bytes of
    a stream are the flushed coder state and carry nothing the decoder still needs: without them the bytes are the same
    and consumed is shorter.  From the fifth on the end-of-stream bit is damaged: a stream that spends about a byte per
    byte (text, random) is never cut short by it, runs on for a few bytes for at least one of 5 and 8, and is right up to
    its last four bytes; the stream of 3000 zeros is 11 to 13 bytes long, so 5 missing bytes are the last few data bytes
    (a few bytes longer) and 8 are most of it (far shorter).  Its first 3 bytes alone still decode to hundreds of bytes.
    A flipped bit in the middle moves the end by ten bytes or more, either way, or loses it."""
    hdr = O.level_header(level)
    for name, data in SAMPLES.items():
        s = O.Codec(hdr).encode(data)
        n = len(data) + 1                                                      # (the PP byte is byte 0)
        full, olen, cons, code, _ = O.Codec(hdr).decode_prefix(s, 8192)
        assert (full, olen, cons) == (b"\0" + data, n, len(s))
        for k in (1, 2, 3, 4):
            got = O.Codec(hdr).decode_prefix(s[:-k], 8192)
            assert got[0] == full and got[1] == n and got[2] == len(s) - k < cons, (level, name, k)
        more = {}
        for k in (5, 8):
            got = O.Codec(hdr).decode_prefix(s[:-k], 8192)
            more[k] = got[1] - n
            assert got[2] == len(s) - k and got[3] == 0, (level, name, k)
            if name != "zeros3000":
                assert 0 <= more[k] <= 16 and got[0][:n - 4] == full[:n - 4], (level, name, k, more)
        assert max(more.values()) > 0, (level, name, more)
        if name == "zeros3000":
            assert len(s) <= 13 and 0 < more[5] <= 16 and more[8] < -100, (level, len(s), more)
        t = bytearray(s)
        t[len(s) // 2] ^= 0x10
        got = O.Codec(hdr).decode_prefix(bytes(t), 8192)
        assert abs(got[1] - n) >= 10, (level, name, got[1])
        print("\nlevel %d %s: %d coded, drop 5 -> %+d, drop 8 -> %+d, flipped bit -> %s" % (
            level, name, len(s), more[5], more[8], "overflow" if got[1] == 8193 else "%+d" % (got[1] - n)))
    s = O.Codec(hdr).encode(SAMPLES["zeros3000"])
    head = O.Codec(hdr).decode_prefix(s[:3], 8192)
    assert 100 <= head[1] < 8192 and head[2] == 3 and head[3] == 0, (level, head[1:])
    print("level %d: the first 3 bytes of zeros3000 decode to %d bytes" % (level, head[1]))
