"""General ZPAQ models (any mix of the nine component types) across the model space: named cases and a seeded generator.

The kernels that take general models are k_gpipe<batched / bit-serial> and k_gdec (zpq_gpipe.hip: wave = component, lane =
block), k_rows and k_lanes (zpq_lanes.hip: lane = component; four blocks or one block per wave; the program evaluated in
registers when it is the shipped hash chain, VMH, or run by the interpreter) and k_generic (one lane per block).  Which of
them takes a model is decided on the host by gpipe_cfg and lanes_cfg; the named cases stand on both sides of every bound
those recognisers have and on the parameter edges the kernels treat specially (tables so small that two bits of a byte
share an entry, the 8192-byte switch of the ICM / ISSE stages, the third MIX / SSE of the lane kernels, rates, limits and
weights of 0 and 255).  The tests (test_general_models_cpu.py, test_gpu_general_models.py) and tools/fuzz_gpu.py --general
hold every route to the oracle on models built here.

Components (predictor.v:300-331): CONST = (1, c), CM = (2, bits, limit), ICM = (3, bits), MATCH = (4, index bits, buffer
bits), AVG = (5, j, k, weight), MIX2 = (6, bits, j, k, rate, mask), MIX = (7, bits, j, m, rate, mask), ISSE = (8, bits, j),
SSE = (9, bits, j, start, limit).
"""
import ctypes as C
import random

from chain_models import hashchain, header, perturbed_hashchain

CONST, CM, ICM, MATCH, AVG, MIX2, MIX, ISSE, SSE = range(1, 10)
COMP_SIZE = {0: 1, CONST: 2, CM: 3, ICM: 2, MATCH: 3, AVG: 4, MIX2: 6, MIX: 6, ISSE: 3, SSE: 5}

ROWS, LANES = "k_rows", "k_lanes"
# A route is (zpq_gpipe_applies, zpq_gdec_applies, zpq_lanes_supported, zpq_lanes_kernel_name without its <...>).
PIPE = (1, 1, 1, ROWS)            # the wave pipelines take it; k_rows is their lane-per-component counterpart
ROWS_ONLY = (0, 0, 1, ROWS)
LANES_ONLY = (0, 0, 1, LANES)
GENERIC_ONLY = (0, 0, 0, LANES)   # more than 64 components: k_generic alone (the kernel name is not used)

GPU_GEN_SEED, GPU_GEN_COUNT = 11, 24  # the GPU test's generated models (this seed's 24 reach every class at least 3 times)


def H(comps, hh, hm, program):
    return header(comps, hh, hm, program)


def components(hdr):
    """The component list of a header built here."""
    out, p = [], 5
    for _ in range(hdr[4]):
        size = COMP_SIZE[hdr[p]]
        out.append(list(hdr[p:p + size]))
        p += size
    return out


def program_of(hdr):
    p = 5 + sum(len(c) for c in components(hdr)) + 1
    return list(hdr[p:-1])


def isse_chain(nisse, tail=None, bits=(10, 8, 12, 6, 7, 9, 11, 5)):
    """ICM, then `nisse` ISSEs each fed by its predecessor (one more level of the prediction chain each), then `tail`."""
    comps = [[ICM, bits[0]]] + [[ISSE, bits[(i + 1) % len(bits)], i] for i in range(nisse)]
    return comps + ([tail] if tail else [])


def cms(count, lo=0, hi=10):
    """`count` CMs with table bits cycling through lo..hi and limits through the edges."""
    lim = [255, 3, 0, 60, 1, 127]
    return [[CM, lo + i % (hi - lo + 1), lim[i % len(lim)]] for i in range(count)]


def ring_model(isse):
    """Fifteen components whose prediction rings add up to 136 (a CM at 12) or 138 (an ISSE fed by component 10 there:
    component 10 then needs a ring of 4 instead of 2).  MIX over 0..7 from position 14: seven rings of 16 and one of 8."""
    comps = cms(8, 4, 9) + [[ICM, 6 + i] for i in range(4)]
    comps += [[ISSE, 9, 10] if isse else [CM, 9, 40], [AVG, 11, 12, 100], [MIX, 5, 0, 8, 20, 255]]
    return H(comps, 4, 8, hashchain(15))


def _three_mix_three_sse(n, program, bits=(0, 3, 5)):
    """More than 16 components, three MIXes and three SSEs: the lane kernels prefetch the weights / rows of the first two
    of each, the third takes the other code path."""
    base = cms(4, 0, 6) + [[ICM, 6], [ICM, 7], [ISSE, 6, 4], [ISSE, 7, 5], [MATCH, 8, 9], [CONST, 200]]
    base += cms(n - 16, 3, 12)
    i = len(base)
    base += [[MIX, 0, 0, 6, 24, 255], [MIX, 2, 2, 9, 10, 15], [MIX, 4, i - 5, 7, 255, 255]]
    base += [[SSE, bits[0], i, 32, 255], [SSE, bits[1], i + 1, 0, 0], [SSE, bits[2], i + 2, 200, 1]]
    assert len(base) == n
    return H(base, 6, 8, program(n))


def _perturbed(contexts, seed):
    return perturbed_hashchain(contexts, random.Random(seed))


NAMED = {
    # ---- tables so small that two bits of one byte share an entry: the batched stages' within-byte forwarding
    "cm_alias": (H([[CM, 0, 255], [CM, 2, 3], [CM, 4, 0], [MIX, 0, 0, 3, 24, 255]], 2, 8, hashchain(4)), PIPE),
    "sse_small": (H([[CM, 8, 60], [SSE, 0, 0, 0, 0], [SSE, 1, 1, 255, 255], [SSE, 3, 2, 32, 1]], 2, 8, hashchain(4)), PIPE),
    "mix_x4": (H([[CM, 6, 255], [ICM, 6], [MIX, 0, 0, 2, 0, 255], [MIX, 1, 0, 3, 255, 15], [MIX, 2, 0, 4, 24, 0],
                  [MIX, 3, 1, 4, 1, 255]], 3, 8, hashchain(6)), PIPE),
    "mix2_edges": (H([[ICM, 8], [CM, 8, 20], [MIX2, 0, 0, 1, 0, 255], [MIX2, 1, 0, 1, 255, 1], [MIX2, 10, 2, 3, 24, 3],
                      [MIX2, 4, 1, 1, 24, 255]], 3, 8, hashchain(6)), PIPE),
    "mix_masks": (H([[CM, 3, 255], [CM, 1, 8], [ICM, 7], [MIX, 2, 0, 3, 24, 1], [MIX, 8, 0, 4, 24, 3], [MIX2, 2, 3, 4, 40, 3]],
                    3, 8, hashchain(6)), PIPE),
    # ---- the 8192-byte switch of the ICM / ISSE stages (6 against 7 size bits), and no size bits at all
    "ht_edge": (H([[ICM, 6], [ICM, 7], [ISSE, 6, 0], [ISSE, 7, 1], [MIX2, 0, 2, 3, 24, 255]], 3, 8, hashchain(5)), PIPE),
    "ht_bits0": (H([[ICM, 0], [ISSE, 0, 0]], 1, 1, hashchain(2)), PIPE),
    "bits0_all": (H([[CM, 0, 1], [ICM, 0], [MATCH, 0, 1], [ISSE, 0, 1], [MIX2, 0, 0, 3, 1, 255], [MIX, 0, 0, 5, 1, 255],
                     [SSE, 0, 5, 1, 1]], 3, 2, hashchain(7)), PIPE),
    # ---- MATCH: the least buffer the pipeline takes, the one it leaves, index against buffer
    "match_min": (H([[MATCH, 0, 1]], 1, 1, hashchain(1)), PIPE),
    "match_buf0": (H([[MATCH, 4, 0]], 1, 8, hashchain(1)), ROWS_ONLY),
    "match_idx_gt_buf": (H([[MATCH, 10, 3], [MATCH, 2, 12], [AVG, 0, 1, 128]], 2, 8, hashchain(3)), PIPE),
    # ---- parameter edges
    "avg_edges": (H([[CONST, 0], [CONST, 255], [AVG, 0, 1, 0], [AVG, 0, 1, 255], [AVG, 2, 2, 128]], 3, 8, hashchain(5)), PIPE),
    "rates": (H([[ICM, 9], [CM, 9, 1], [MIX2, 6, 0, 1, 1, 255], [MIX, 6, 0, 3, 255, 255], [SSE, 6, 3, 1, 0], [SSE, 2, 4, 33, 255]],
                3, 8, hashchain(6)), PIPE),
    "hashes_lt_n": (H([[ICM, 10], [CM, 10, 30], [ISSE, 9, 0], [CM, 4, 255], [MIX, 3, 0, 4, 16, 255]], 3, 8, hashchain(2)), PIPE),
    "big_next_to_tiny": (H([[CM, 20, 255], [CM, 0, 255], [ICM, 18], [ISSE, 0, 2], [MIX2, 1, 1, 3, 24, 255], [SSE, 0, 4, 32, 255]],
                           3, 8, hashchain(6)), PIPE),
    # ---- gpipe_cfg's bounds: n 15 / 16, MIX over 8 / 9 inputs, the rings' LDS, k_gdec's SSE rows and barriers per bit
    "n15_deep": (H(isse_chain(13, [SSE, 6, 13, 32, 255]), 4, 8, hashchain(15)), PIPE),
    "n16": (H(isse_chain(14, [SSE, 6, 14, 32, 255]), 4, 8, hashchain(16)), ROWS_ONLY),
    "n17": (H(isse_chain(15, [SSE, 6, 15, 32, 255]), 5, 8, hashchain(17)), LANES_ONLY),
    "mix8": (H(cms(8, 0, 7) + [[MIX, 4, 0, 8, 24, 255]], 4, 8, hashchain(9)), PIPE),
    "mix9": (H(cms(9, 0, 7) + [[MIX, 4, 0, 9, 24, 255]], 4, 8, hashchain(10)), ROWS_ONLY),
    "ring136": (ring_model(False), PIPE),
    "ring138": (ring_model(True), ROWS_ONLY),
    "sse14": (H([[CM, 10, 255]] + [[SSE, i % 5, i, [32, 0, 255, 1, 100][i % 5], [255, 0, 1, 60][i % 4]] for i in range(14)],
                4, 8, hashchain(15)), PIPE),
    "wide_level0": (H(cms(14, 0, 6) + [[MIX2, 3, 12, 13, 24, 255]], 4, 8, hashchain(15)), PIPE),
    # ---- lanes_cfg's bounds: rows / lanes at 16 / 17 (above), lanes / generic at 64 / 65
    "n64": (H(cms(63, 0, 9) + [[MIX, 2, 55, 8, 24, 255]], 6, 8, hashchain(64)), LANES_ONLY),
    "n65": (H(cms(64, 0, 9) + [[MIX, 2, 56, 8, 24, 255]], 7, 8, hashchain(65)), GENERIC_ONLY),
    # ---- the interpreter (VMH = false): H too small for the chain, no M, one opcode exchanged; at n <= 16 and above
    "hh_small": (H([[ICM, 10], [ISSE, 10, 0], [CM, 3, 255], [MIX, 0, 0, 3, 24, 255]], 1, 8, hashchain(4)), ROWS_ONLY),
    "hm0": (H([[ICM, 10], [ISSE, 6, 0], [CM, 2, 255], [SSE, 1, 2, 32, 255]], 2, 0, hashchain(4)), ROWS_ONLY),
    "perturbed_rows": (H([[CM, 4, 255], [ICM, 7], [ISSE, 6, 1], [MIX2, 2, 0, 2, 24, 255], [SSE, 0, 3, 32, 255]], 3, 8,
                         _perturbed(5, 1)), ROWS_ONLY),
    "perturbed_lanes": (H(isse_chain(8) + cms(9, 0, 8) + [[MIX, 1, 9, 9, 24, 255]], 5, 8, _perturbed(19, 2)), LANES_ONLY),
    "hh_small_lanes": (H(isse_chain(8) + cms(9, 0, 8) + [[MIX, 1, 9, 9, 24, 255]], 4, 8, hashchain(19)), LANES_ONLY),
    # ---- the third MIX and the third SSE of the lane kernels, at n <= 16 (above: mix_x4, sse_small, sse14) and beyond
    "mix3_sse3_n22": (_three_mix_three_sse(22, hashchain), LANES_ONLY),
    "mix3_sse3_n22_vm": (_three_mix_three_sse(22, lambda n: _perturbed(n, 3)), LANES_ONLY),
    # ---- SSE rows in range all the time.  An SSE's row is (H[i] + c8) * 32, unmasked: with a hash in H[i] it lies beyond any
    # table after a block's first byte and the SSE predicts 0 (quirk Q10).  Components past the chain's last link keep H[i] = 0:
    # the row is c8 * 32, inside a table of 8 bits for every bit, inside one of 5 bits for the first five bits of a byte.
    "sse_order0": (H([[CM, 10, 255], [SSE, 8, 0, 32, 255], [SSE, 8, 1, 0, 0], [SSE, 9, 2, 255, 1], [SSE, 5, 3, 1, 255],
                      [MIX2, 4, 3, 4, 24, 255]], 1, 8, hashchain(1)), PIPE),
    "mix3_sse3_n22_h16": (_three_mix_three_sse(22, lambda n: hashchain(16), bits=(8, 5, 8)), LANES_ONLY),
    # ---- a MIX whose weights' lanes wrap the 16-lane row / the 64-lane wave (lane = (index + l) mod 16 / 64)
    "mix_row16": (H(cms(10, 0, 5) + isse_chain(4) + [[MIX, 3, 0, 15, 24, 255]], 4, 8, hashchain(16)), ROWS_ONLY),
    "mix_wave64": (H(cms(50, 0, 8) + isse_chain(12) + [[MIX, 2, 0, 63, 24, 255]], 6, 8, hashchain(64)), LANES_ONLY),
    # ---- forward and self references (an input index >= the consumer's own: last bit's prediction) beyond one row
    "fwd_n20": (H([[MIX, 2, 0, 20, 24, 255], [ISSE, 6, 5], [AVG, 2, 19, 77], [MIX2, 1, 3, 18, 24, 255], [SSE, 1, 4, 32, 255]]
                  + cms(10, 0, 7) + [[ICM, 7], [ISSE, 7, 15], [MIX, 0, 10, 12, 24, 15], [SSE, 0, 17, 0, 0], [MIX, 1, 19, 1, 255, 255]],
                  5, 8, hashchain(20)), LANES_ONLY),
}


def _lib(zpq):
    L = zpq.lib()
    for f in (L.zpq_gpipe_applies, L.zpq_gdec_applies, L.zpq_lanes_supported):
        f.argtypes = [C.c_void_p]
        f.restype = C.c_int
    L.zpq_lanes_kernel_name.argtypes = [C.c_void_p, C.c_int]
    L.zpq_lanes_kernel_name.restype = C.c_char_p
    return L


def route(zpq, model):
    """(gpipe, gdec, lanes, kernel) as the library's host logic answers for a zpq.Model (a zpq_model starts with its
    DModel); the environment's knobs (ZPQ_ENC_GPIPE, ZPQ_DEC_GPIPE, ZPQ_LANES_ROWS) count."""
    L = _lib(zpq)
    name = L.zpq_lanes_kernel_name(model.h, 0).decode()
    assert name.endswith("<encode>") and L.zpq_lanes_kernel_name(model.h, 1).decode() == name[:-8] + "<decode>"
    return (L.zpq_gpipe_applies(model.h), L.zpq_gdec_applies(model.h), L.zpq_lanes_supported(model.h), name[:-8])


def is_hashchain(hdr):
    """What zpq_vm_hashchain recognises (zpq_model.cpp), restated: the shipped program of K links, M >= 2 bytes, H >= K words."""
    p = program_of(hdr)
    if len(p) < 8:
        return False
    k = (len(p) - 8) // 3 + 1
    hlen, mlen = (1 << hdr[0] if hdr[0] else 0), (1 << hdr[1] if hdr[1] else 0)
    return p == hashchain(k) and mlen >= 2 and hlen >= k


def has_forward_reference(hdr):
    for i, c in enumerate(components(hdr)):
        t = c[0]
        ins = {AVG: c[1:3], MIX2: c[2:4], ISSE: c[2:3], SSE: c[2:3]}.get(t, [])
        if t == MIX:
            ins = range(c[2], c[2] + c[3])
        if any(j >= i for j in ins):
            return True
    return False


def route_class(hdr, rt):
    """Coarse class of a route for coverage counts: the most specialised kernels that take the model."""
    vmh = is_hashchain(hdr)
    if rt[0] and rt[1]:
        return "gpipe"
    if rt[2] and rt[3] == ROWS:
        return "rows_hashchain" if vmh else "rows_interpreter"
    if rt[2]:
        return "lanes_hashchain" if vmh else "lanes_interpreter"
    return "generic_only"


def classes(hdr, rt):
    """The classes a model belongs to, for the generator's coverage conditions (test_general_models_cpu.py)."""
    comps = components(hdr)
    out = {route_class(hdr, rt)}
    if has_forward_reference(hdr):
        out.add("forward")
    if sum(c[0] == MIX for c in comps) >= 3:
        out.add("mix3")
    if sum(c[0] == SSE for c in comps) >= 3:
        out.add("sse3")
    for t, name in ((CM, "cm"), (MIX, "mix"), (MIX2, "mix2"), (SSE, "sse")):
        if any(c[0] == t and c[1] <= 4 for c in comps):
            out.add("tiny_" + name)
    for b in (6, 7):
        if any(c[0] in (ICM, ISSE) and c[1] == b for c in comps):
            out.add("ht%d" % b)
    return out


GENERATOR_CLASSES = ("gpipe", "rows_hashchain", "rows_interpreter", "lanes_hashchain", "lanes_interpreter", "forward", "mix3",
                     "sse3", "tiny_cm", "tiny_mix", "tiny_mix2", "tiny_sse", "ht6", "ht7")


def _edge(r, typical):
    """A rate, limit, start, weight or CONST value: the edges, a typical one, any."""
    return r.choice([0, 1, 255, typical, typical, r.randrange(256)])


def _bits(r, hi, big=False):
    """Table size bits from 0, with weight on 0-4 (two bits of a byte share an entry) and on the 6 / 7 switch."""
    if big and r.random() < 0.04:
        return r.randint(18, 20)
    return r.choice([0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 6, 7, 6, 7, 5, 8, r.randint(0, hi), r.randint(0, hi), r.randint(0, hi)])


def _at_least(x):
    return max(0, (x - 1).bit_length())


def random_general(r, big=False):
    """One random general model from random.Random r: n from 1-15 mostly, 16, 17-64 sometimes, 65+ rarely; every component
    type with size bits from 0, rates / limits / starts / weights on their edges, masks 255 / 15 / 3 / 1 / 0; inputs earlier
    components for most models and any index below n (forward and self references) for the rest; MIX widths up to the
    pipeline's bound and past it; the hash chain with n links, fewer, or perturbed; hh / hm on both sides of what the hash
    chain needs.  Several MIX and SSE components per model are common.  With big, a few tables of 18-20 bits."""
    x = r.random()
    n = r.randint(1, 15) if x < 0.62 else 16 if x < 0.70 else r.randint(17, 64) if x < 0.97 else r.randint(65, 68)
    forward = r.random() < 0.22
    flavour = r.choice(["any", "any", "mixes", "sses", "hashed"])
    comps, nbig = [], 0
    for i in range(n):
        free = [CONST, CM, CM, ICM, ICM, MATCH]
        fed = [AVG, MIX2, MIX2, MIX, MIX, ISSE, ISSE, SSE, SSE] + {"mixes": [MIX] * 8, "sses": [SSE] * 8, "hashed": [ISSE, ICM] * 4}.get(flavour, [])
        t = r.choice(free + (fed if i or forward else []) + ([ICM] * 4 if flavour == "hashed" else []))
        if i == n - 1 and n > 1 and r.random() < 0.5:
            t = r.choice([MIX, MIX2, SSE])                       # models mostly end in a mixer or an SSE
        top = n if forward else max(i, 1)
        j, k = r.randrange(top), r.randrange(top)
        if t in (ISSE, SSE) and not forward and r.random() < 0.6:
            j = i - 1
        wide = big and nbig < 2
        if t == CONST:
            c = [CONST, _edge(r, 160)]
        elif t == CM:
            c = [CM, _bits(r, 16, wide), _edge(r, 60)]
        elif t == ICM:
            c = [ICM, _bits(r, 14, wide)]
        elif t == MATCH:
            c = [MATCH, _bits(r, 14), r.choice([1, 1, 2, 3, r.randint(1, 14), r.randint(1, 14), 0])]
        elif t == AVG:
            c = [AVG, j, k, _edge(r, 128)]
        elif t == MIX2:
            c = [MIX2, _bits(r, 10), j, k, _edge(r, 24), r.choice([255, 255, 15, 3, 1, 0])]
        elif t == MIX:
            if forward:
                j = r.randrange(n)
                m = r.randint(1, min(n, 12) + 1)                  # (may reach past n: the sum stops at n)
            else:
                m = r.choice([min(8, i), min(9, i), r.randint(1, min(i, 8)), r.randint(1, min(i, 8)), r.randint(1, i)])
                j = r.choice([0, i - m, r.randint(0, i - m)])
            c = [MIX, _bits(r, 8), j, m, _edge(r, 24), r.choice([255, 255, 15, 3, 1, 0])]
        elif t == ISSE:
            c = [ISSE, _bits(r, 14, wide), j]
        else:
            c = [SSE, _bits(r, 8), j, _edge(r, 32), _edge(r, 255)]
        nbig += t in (CM, ICM, ISSE) and c[1] >= 18
        comps.append(c)
    kind = r.random()
    links = n if kind < 0.6 else r.randint(1, n) if kind < 0.72 else n
    program = perturbed_hashchain(n, r) if kind >= 0.72 and kind < 0.9 else hashchain(links)
    need = max(1, _at_least(links))
    if kind >= 0.9:                                              # H or M too small for the recogniser: the interpreter
        hh, hm = r.choice([(need - 1, 8), (need, 0), (need - 1, 0)]) if links > 1 else (need, 0)
    else:
        hh = r.choice([need, need, need + r.randint(1, 3)])
        hm = r.choice([1, 2, 8, 16, r.randint(1, 16)])
    return header(comps, hh, hm, program)


def generated(seed, count, big=False):
    """`count` headers from a seeded sequence (the same on every machine)."""
    r = random.Random(seed)
    return [random_general(r, big=big) for _ in range(count)]
