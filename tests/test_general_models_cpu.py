"""General models across the model space, on the host: which kernels the recognisers (gpipe_cfg, lanes_cfg) send each named
case to, every bound of theirs from both sides on otherwise equal models, that the seeded generator reaches every class it
exists for, and that the two reference implementations (the C oracle and oracle/pyref) agree on exactly the models the GPU
tests (test_gpu_general_models.py) compare the kernels with."""
import collections
import os
import random
import sys

import pytest

import general_models as GM
import oracle_lib as O
from general_models import AVG, CM, ICM, ISSE, MATCH, MIX, SSE, H, cms, hashchain, isse_chain
from general_models import GPU_GEN_COUNT, GPU_GEN_SEED

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "pyref"))
import zpaq_pyref as P  # noqa: E402

CPU_GEN_SEED, CPU_GEN_COUNT = 7, 20
KNOBS = ("ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE", "ZPQ_LANES_ROWS")


def _route(zpq, hdr):
    return GM.route(zpq, zpq.Model(header=hdr))


@pytest.fixture
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.mark.parametrize("name", sorted(GM.NAMED))
def test_named_case_route(zpq, no_knobs, name):
    hdr, want = GM.NAMED[name]
    m = zpq.Model(header=hdr)
    assert GM.components(hdr) and len(GM.components(hdr)) == hdr[4]
    assert GM.route(zpq, m) == want, name
    # the program: in registers (VMH) or through the interpreter; the pipelines take the hash chain only
    interpreted = name in ("hh_small", "hm0", "perturbed_rows", "perturbed_lanes", "hh_small_lanes", "mix3_sse3_n22_vm")
    assert GM.is_hashchain(hdr) == (not interpreted) and (GM.is_hashchain(hdr) or not want[0])
    no_knobs.setenv("ZPQ_ENC_GPIPE", "0")
    assert GM.route(zpq, m) == (0,) + want[1:]
    no_knobs.setenv("ZPQ_DEC_GPIPE", "0")
    assert GM.route(zpq, m) == (0, 0) + want[2:]
    no_knobs.setenv("ZPQ_LANES_ROWS", "0")
    assert GM.route(zpq, m) == (0, 0, want[2], GM.LANES)


def test_recogniser_bounds(zpq, no_knobs):
    """Every bound of gpipe_cfg and lanes_cfg from both sides, on models that differ in nothing else."""
    def deep(nisse):
        return H(isse_chain(nisse, [SSE, 6, nisse, 32, 255]), 5, 8, hashchain(nisse + 2))
    # n: the pipelines up to 15, four blocks per wave up to 16, one block per wave up to 64, then k_generic alone
    for n, want in ((14, GM.PIPE), (15, GM.PIPE), (16, GM.ROWS_ONLY), (17, GM.LANES_ONLY)):
        assert _route(zpq, deep(n - 2)) == want, n
    for n, want in ((16, GM.ROWS_ONLY), (17, GM.LANES_ONLY), (64, GM.LANES_ONLY), (65, GM.GENERIC_ONLY), (66, GM.GENERIC_ONLY)):
        assert _route(zpq, H(cms(n - 1, 0, 9) + [[MIX, 2, n - 9, 8, 24, 255]], 7, 8, hashchain(n))) == want, n
    # a MIX over at most 8 inputs, all of them earlier components
    for m, want in ((1, GM.PIPE), (8, GM.PIPE), (9, GM.ROWS_ONLY), (10, GM.ROWS_ONLY)):
        assert _route(zpq, H(cms(10, 0, 7) + [[MIX, 4, 0, m, 24, 255]], 4, 8, hashchain(11))) == want, m
    for j, want in ((2, GM.PIPE), (3, GM.ROWS_ONLY)):                       # j + m <= i
        assert _route(zpq, H(cms(10, 0, 7) + [[MIX, 4, j, 8, 24, 255]], 4, 8, hashchain(11))) == want, j
    # a MATCH buffer of at least two bytes
    for bits, want in ((0, GM.ROWS_ONLY), (1, GM.PIPE), (2, GM.PIPE)):
        assert _route(zpq, H([[MATCH, 4, bits]], 1, 8, hashchain(1))) == want, bits
    # every input an earlier component: the consumer's own index and the one after it are left to k_rows
    for j, want in ((1, GM.PIPE), (2, GM.ROWS_ONLY), (3, GM.ROWS_ONLY)):
        assert _route(zpq, H([[ICM, 8], [CM, 8, 9], [ISSE, 8, j], [AVG, 0, 1, 9]], 2, 8, hashchain(4))) == want, j
        assert _route(zpq, H([[ICM, 8], [CM, 8, 9], [SSE, 3, j, 32, 255], [AVG, 0, 1, 9]], 2, 8, hashchain(4))) == want, j
        assert _route(zpq, H([[ICM, 8], [CM, 8, 9], [AVG, 0, j, 9], [AVG, 0, 1, 9]], 2, 8, hashchain(4))) == want, j
    # the rings' LDS.  zpq_gpipe.hip: lds = L_LINK + ring * BPW * 16 + 16 <= 160 KiB with BPW = 64 blocks per workgroup and
    # L_LINK = (2048 + 128) * 4 + 4096 * 2 + 1024 + 4096 + 512 + 16 * 64 = 23552: ring <= (163840 - 23552 - 16) / 1024 =
    # 136.98.  A component's ring is the power of two above the distance to its farthest consumer, at least 2: the two
    # models differ in one component (CM / ISSE fed by component 10) and so in one ring of 2 / 4.
    l_link = (2048 + 128) * 4 + 4096 * 2 + 1024 + 4096 + 512 + 16 * 64
    assert (160 * 1024 - l_link - 16) // (64 * 16) == 136
    assert _ring_total(GM.NAMED["ring136"][0]) == 136 and _ring_total(GM.NAMED["ring138"][0]) == 138
    assert _route(zpq, GM.NAMED["ring136"][0]) == GM.PIPE and _route(zpq, GM.NAMED["ring138"][0]) == GM.ROWS_ONLY
    # the hash chain: H must hold a word per link and M two bytes; fewer links than components are taken
    for hh, hm, links, want in ((2, 1, 4, GM.PIPE), (1, 1, 4, GM.ROWS_ONLY), (2, 0, 4, GM.ROWS_ONLY), (1, 1, 2, GM.PIPE), (0, 1, 1, GM.ROWS_ONLY),
                                (1, 1, 1, GM.PIPE)):
        assert _route(zpq, H([[ICM, 8], [CM, 8, 9], [ISSE, 8, 0], [AVG, 0, 1, 9]], hh, hm, hashchain(links))) == want, (hh, hm, links)


def _ring_total(hdr):
    """gpipe_cfg's ring sizes restated: per component the power of two above the distance to its farthest consumer (the
    coder reads the last component at distance 1), at least 2."""
    comps = GM.components(hdr)
    far = [0] * len(comps)
    far[-1] = 1
    for i, c in enumerate(comps):
        ins = {AVG: c[1:3], GM.MIX2: c[2:4], ISSE: c[2:3], SSE: c[2:3]}.get(c[0], [])
        if c[0] == MIX:
            ins = range(c[2], c[2] + c[3])
        for j in ins:
            far[j] = max(far[j], i - j)
    total = 0
    for f in far:
        depth = 2
        while depth <= f:
            depth *= 2
        total += depth
    return total


def _inputs(seed):
    r = random.Random(seed)
    return [b"", bytes(r.getrandbits(8) for _ in range(r.randint(1, 160))),
            bytes(r.choice(b"abcab \n") for _ in range(400))]


def _oracle_equals_pyref(hdr, seed):
    for d in _inputs(seed):
        for pp in (True, False):
            want = O.Codec(hdr).encode(d, pp=pp)
            assert P.encode_segment(P.new_model(hdr), d, pp=pp) == want, (hdr.hex(), len(d), pp)
            dec, used = O.Codec(hdr).decode(want, cap=1000)      # (the oracle's decoder hands the PP byte on as data)
            assert dec == (b"\0" if pp else b"") + d and used == len(want)


@pytest.mark.parametrize("name", sorted(GM.NAMED))
def test_oracle_equals_pyref_on_named_case(name):
    _oracle_equals_pyref(GM.NAMED[name][0], sum(name.encode()))


@pytest.mark.parametrize("index", range(CPU_GEN_COUNT))
def test_oracle_equals_pyref_on_generated_model(index):
    _oracle_equals_pyref(GM.generated(CPU_GEN_SEED, CPU_GEN_COUNT)[index], index)


def test_generator_reaches_every_class(zpq, no_knobs):
    """The generator is only as good as the classes it reaches.  Among the very models the GPU test draws: every route (the
    wave pipelines; k_rows and k_lanes with the hash chain in registers and with the interpreter), forward or self
    references, a third MIX and a third SSE, a table of at most 4 bits for each type whose batched stage forwards within a
    byte, ICM / ISSE tables on both sides of the 8192-byte switch."""
    count = collections.Counter()
    for hdr in GM.generated(GPU_GEN_SEED, GPU_GEN_COUNT, big=True):
        m = zpq.Model(header=hdr)                                # (none is refused: no MIX with m = 0, no table too big)
        for cls in GM.classes(hdr, GM.route(zpq, m)):
            count[cls] += 1
    for cls in GM.GENERATOR_CLASSES:
        assert count[cls] >= 3, (cls, dict(count))
    # a wider draw also leaves the lane kernels' range now and then, and the named cases' classes are what they say
    wide = collections.Counter()
    for hdr in GM.generated(CPU_GEN_SEED, 300):
        wide.update(GM.classes(hdr, _route(zpq, hdr)))
    for cls in GM.GENERATOR_CLASSES + ("generic_only",):
        assert wide[cls] >= 3, (cls, dict(wide))
    assert "lanes_interpreter" in GM.classes(*_named(zpq, "perturbed_lanes")) and "rows_interpreter" in GM.classes(*_named(zpq, "hm0"))
    assert {"mix3", "sse3", "lanes_hashchain"} <= GM.classes(*_named(zpq, "mix3_sse3_n22"))
    assert "forward" in GM.classes(*_named(zpq, "fwd_n20")) and "forward" not in GM.classes(*_named(zpq, "n64"))
    # the seeded sequences are the same everywhere
    assert GM.generated(3, 5) == GM.generated(3, 5) and GM.generated(3, 5) != GM.generated(4, 5)


def _named(zpq, name):
    hdr = GM.NAMED[name][0]
    return hdr, _route(zpq, hdr)
