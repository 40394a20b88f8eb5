"""Chain models beyond the shipped levels, on the host: which k_chain instantiation build_cfg routes each named case to
(zpq_chain_route, internal), which pipelined kernels apply to the specialised ones, that the seeded generator reaches
every route, and that the two reference implementations (the C oracle and oracle/pyref) agree on exactly the models the
GPU tests (test_gpu_chain_models.py) compare the kernels with."""
import collections
import ctypes as C
import os
import random
import sys

import pytest

import chain_models as CM
import oracle_lib as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "pyref"))
import zpaq_pyref as P  # noqa: E402

# (k_pipe / k_pipe2 encodes a batch of 15 resident blocks, k_dpipe decodes it under ZPQ_DEC_PIPE=1, striped host
# transfers exist) for every specialised named case
SPEC_KERNELS = {
    "l2_mixed": (1, 1, 1),
    "l2_hh2_hm1": (1, 1, 1),
    "l1_sizes": (1, 1, 1),
    "l3_mixed": (1, 1, 0),
    "l4_rate255": (1, 0, 0),
    "l4_rate0": (1, 0, 0),
    "l5_small": (1, 0, 0),
}

CPU_GEN_SEED, CPU_GEN_COUNT = 7, 30


def _lib(zpq):
    L = zpq.lib()
    for f in (L.zpq_pipe_applies, L.zpq_dpipe_applies):
        f.argtypes = [C.c_void_p, C.c_int, C.c_int]
        f.restype = C.c_int
    for f in (L.zpq_chain_has_hio, L.zpq_chain_blocks_per_wg):
        f.argtypes = [C.c_void_p]
        f.restype = C.c_int
    return L


@pytest.mark.parametrize("name", sorted(CM.NAMED))
def test_named_case_route(zpq, monkeypatch, name):
    hdr, want = CM.NAMED[name]
    L = _lib(zpq)
    monkeypatch.delenv("ZPQ_CHAIN_G", raising=False)
    monkeypatch.delenv("ZPQ_ENC_PIPE", raising=False)
    monkeypatch.delenv("ZPQ_DEC_PIPE", raising=False)
    m = zpq.Model(header=hdr)
    assert m.has_fast_path
    rt = CM.route(zpq, m)
    assert CM.route_key(rt) == want, (name, rt)
    if rt is None:
        assert L.zpq_chain_blocks_per_wg(m.h) == 0
        return
    assert rt["nisse_end"] == rt["n"] - rt["has_mix2"] and rt["sparse"] == 0
    assert rt["blocks_per_wg"] == L.zpq_chain_blocks_per_wg(m.h)
    if name in CM.NAMED_BPW:
        assert rt["blocks_per_wg"] == CM.NAMED_BPW[name]
    bpw = min(16, rt["blocks_per_wg"])
    pipe, dpipe, hio = SPEC_KERNELS.get(name, (0, 0, 0))
    assert (rt["nch_spec"] != 0) == (name in SPEC_KERNELS)
    assert L.zpq_pipe_applies(m.h, bpw, 15) == pipe
    assert L.zpq_pipe_applies(m.h, bpw, 11) == 0
    assert L.zpq_chain_has_hio(m.h) == hio
    assert L.zpq_dpipe_applies(m.h, bpw, 15) == 0                  # opt-in
    monkeypatch.setenv("ZPQ_DEC_PIPE", "1")
    assert L.zpq_dpipe_applies(m.h, bpw, 15) == dpipe


def test_recogniser_bounds(zpq):
    """Each recogniser's bounds from both sides, on otherwise equal models: H must hold one word per context and M
    two bytes for the hash chain; level 1's program only with hh 1, hm 2."""
    for hh, hm, vm in ((2, 1, CM.VM_HASHCHAIN), (1, 1, CM.VM_GENERIC), (2, 0, CM.VM_GENERIC), (9, 16, CM.VM_HASHCHAIN)):
        rt = CM.route(zpq, zpq.Model(header=CM.chain([12, 12, 12], hh=hh, hm=hm)))
        assert rt["vm_kind"] == vm and rt["nch_spec"] == (3 if vm else 0), (hh, hm, rt)
    for hh, hm, vm in ((1, 2, CM.VM_LEVEL1), (1, 1, CM.VM_GENERIC), (1, 3, CM.VM_GENERIC), (0, 2, CM.VM_GENERIC), (2, 2, CM.VM_GENERIC)):
        rt = CM.route(zpq, zpq.Model(header=CM.chain([12, 12], hh=hh, hm=hm, program=CM.L1_PROG)))
        assert rt["vm_kind"] == vm and rt["nch_spec"] == (2 if vm else 0), (hh, hm, rt)
    # a MIX2 of the level-4 shape: >= 256 weights, mask 255 and the last two components, else the runtime MIX2
    for mix, spec in (((8, None, None, 24, 255), 6), ((7, None, None, 24, 255), 0), ((8, None, None, 24, 127), 0),
                      ((8, 3, 5, 24, 255), 0), ((8, 4, 4, 24, 255), 0), ((12, None, None, 255, 255), 6)):
        rt = CM.route(zpq, zpq.Model(header=CM.chain([10] * 6, mix=mix, hh=3, hm=4)))
        assert rt["nch_spec"] == spec and rt["has_mix2"] == 1, (mix, rt)


def _inputs(seed):
    r = random.Random(seed)
    return [b"", bytes(r.getrandbits(8) for _ in range(r.randint(1, 160))),
            bytes(r.choice(b"abcab \n") for _ in range(400))]


def _oracle_equals_pyref(hdr, seed):
    for d in _inputs(seed):
        for pp in (True, False):
            want = O.Codec(hdr).encode(d, pp=pp)
            assert P.encode_segment(P.new_model(hdr), d, pp=pp) == want, (hdr.hex(), len(d), pp)
    dec, used = O.Codec(hdr).decode(want, cap=1000)
    assert dec == d and used == len(want)


@pytest.mark.parametrize("name", sorted(CM.NAMED))
def test_oracle_equals_pyref_on_named_case(name):
    _oracle_equals_pyref(CM.NAMED[name][0], sum(name.encode()))


@pytest.mark.parametrize("index", range(CPU_GEN_COUNT))
def test_oracle_equals_pyref_on_generated_model(index):
    hdr = CM.generated(CPU_GEN_SEED, CPU_GEN_COUNT)[index]
    assert max(CM.table_bits(hdr)) <= 16
    _oracle_equals_pyref(hdr, index)


def test_generator_reaches_every_route(zpq):
    """The generator is only as good as the routes it reaches: every specialisation, the runtime-loop kernel with and
    without a MIX2 at 8 and 16 lanes, each program kind, and models just outside the chain layout."""
    classes, vms = collections.Counter(), collections.Counter()
    for hdr in CM.generated(CPU_GEN_SEED, 400):
        m = zpq.Model(header=hdr)
        assert m.has_fast_path
        rt = CM.route(zpq, m)
        classes[CM.route_class(rt)] += 1
        if rt is not None:
            vms[rt["vm_kind"]] += 1
    for cls in ("spec2", "spec3", "spec5", "spec6", "spec8", "runtime_plain_g8", "runtime_plain_g16",
                "runtime_mix2_g8", "runtime_mix2_g16", "not_chain"):
        assert classes[cls] >= 3, (cls, classes)
    for vm in (CM.VM_GENERIC, CM.VM_HASHCHAIN, CM.VM_LEVEL1):
        assert vms[vm] >= 3, vms
    # the seeded sequences are the same everywhere
    assert CM.generated(3, 5) == CM.generated(3, 5) and CM.generated(3, 5) != CM.generated(4, 5)
