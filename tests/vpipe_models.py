"""Models for k_vpipe / k_vdec (zpq_gpipe.hip: the wave-per-component pipelines with an interpreter wave, on request:
ZPQ_FLAG_VMPIPE / ZPQ_VM_PIPE) and the envelope vpipe_cfg states, restated: shared by test_vpipe_cpu.py and
test_gpu_vpipe.py."""
import ctypes as C
import os
import random
import sys

import general_models as GM
from chain_models import hashchain, perturbed_hashchain

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from inputs import C4B  # noqa: E402

LDS_MAX = 160 * 1024
L_LINK, D_SSE, D_SSE_BYTES, BPW = 23552, 27152, 9216, 64      # zpq_gpipe.hip's LDS layout


def applies(zpq, model):
    """(zpq_vpipe_applies, zpq_vdec_applies) for a zpq.Model."""
    L = zpq.lib()
    for f in (L.zpq_vpipe_applies, L.zpq_vdec_applies):
        f.argtypes = [C.c_void_p]
        f.restype = C.c_int
    return L.zpq_vpipe_applies(model.h), L.zpq_vdec_applies(model.h)


def with_program(hdr, program):
    """The components, hh and hm of `hdr` in front of another program."""
    return GM.H(GM.components(hdr), hdr[0], hdr[1], program)


def perturbed(hdr, seed=5):
    return with_program(hdr, perturbed_hashchain(hdr[4], random.Random(seed)))


def chain(n, seed=4):
    """An ISSE chain of n components behind a perturbed hash chain."""
    return GM.H(GM.isse_chain(n - 1), 4, 8, perturbed_hashchain(n, random.Random(seed)))


# C4b's components behind its own hash chain with `a=a` (opcode 64) in front: the same contexts, hence the same coded
# bytes, from a program that no recogniser takes
C4B_VM = with_program(C4B, [64] + GM.program_of(C4B))


def c4b_with(program_of_n):
    """C4b's components behind another program (a function of the number of contexts)."""
    return with_program(C4B, program_of_n(C4B[4]))


def lds_bytes(hdr):
    """(encoder, decoder) LDS of k_vpipe / k_vdec by the formula above vpipe_cfg, for a header whose inputs are all
    earlier components."""
    comps = GM.components(hdr)
    n = len(comps)
    far = [0] * n
    far[n - 1] = 1
    for i, c in enumerate(comps):
        ins = {GM.AVG: c[1:3], GM.MIX2: c[2:4], GM.ISSE: c[2:3], GM.SSE: c[2:3]}.get(c[0], [])
        if c[0] == GM.MIX:
            ins = range(c[2], c[2] + c[3])
        for j in ins:
            assert j < i
            far[j] = max(far[j], i - j)

    def pow2(least):
        d = 2
        while d < least:
            d *= 2
        return d

    ring = sum(pow2(f + 1) for f in far)
    ctx = sum(pow2(i + 2) for i in range(n))
    h16 = (len(hdr) + 15) & ~15
    nsse = sum(c[0] == GM.SSE for c in comps)
    return (L_LINK + 1024 * ring + 16 + 256 * ctx + 256 + h16, D_SSE + D_SSE_BYTES * nsse + 256 * n + 256 + h16)


def lds_edge(pad):
    """Fourteen components whose prediction rings add up to 98 entries (four of 16, two of 8, one of 4, seven of 2) behind a
    perturbed hash chain followed by `pad` unreachable two-byte instructions: (header, offsets).  The header's length is
    101 + 2 * pad; the encoder's LDS reaches 160 KiB exactly at a length of 225 .. 240."""
    comps = GM.cms(6, 4, 9) + [[GM.ICM, 7]] + GM.cms(2, 3, 5)
    comps += [[GM.ISSE, 8, 6], [GM.ISSE, 6, 9], [GM.AVG, 4, 5, 100], [GM.MIX, 4, 0, 4, 24, 255], [GM.SSE, 5, 12, 32, 255]]
    code = perturbed_hashchain(14, random.Random(6)) + [71, 1] * pad
    hdr = GM.H(comps, 4, 8, code)
    cend = 5 + sum(len(c) for c in comps)
    return hdr, (cend, cend + 1, cend + 1 + len(code))


assert hashchain(8) == GM.program_of(C4B)                    # (nine components, eight links: the SSE's context stays 0)
