"""Chain-shaped ZPAQ models beyond the five shipped levels: named cases and a seeded generator.

A chain model is an ICM, then ISSEs fed by their predecessor (j = i - 1), then an optional MIX2.  zpq_chain.hip
routes every such model by its SHAPE -- chain length, program, MIX2 parameters -- to a specialised k_chain / k_pipe /
k_dpipe instantiation or to the runtime-loop one (NCH = 0, with the ZPAQL interpreter); table sizes, hh / hm and the
MIX2's size and rate stay free parameters of all of them.  The tests (test_chain_models_cpu.py,
test_gpu_chain_models.py) and tools/fuzz_gpu.py --chains hold every route to the oracle on models built here.

Header layout (predictor.v:300-331, compressor.v:96-145): hh hm ph pm n, the components, 0, the HCOMP program, 0.
ICM = (3, bits), ISSE = (8, bits, j), MIX2 = (6, bits, j, k, rate, mask).
"""
import ctypes as C
import random

# The shipped hash-chain program (levels 2-5): b=c c-- *c=a d=0, then per context "hash *d=a d++", the last one
# "hash *d=a halt".  zpq_vm_hashchain recognises it when M has >= 2 bytes and H >= one word per context.
HC_HEAD = [74, 18, 104, 95, 0]
HC_LINK = [59, 112, 25]
HC_TAIL = [59, 112, 56]
# Level 1's program (levels.v:34); recognised only with hh 1, hm 2 and two components.
L1_PROG = [96, 4, 28, 59, 10, 59, 112, 25, 10, 59, 10, 59, 112, 56]

VM_GENERIC, VM_HASHCHAIN, VM_LEVEL1 = 0, 1, 2


def hashchain(contexts):
    """The hash-chain program for `contexts` components (one context each, a MIX2 included)."""
    return HC_HEAD + HC_LINK * (contexts - 1) + HC_TAIL


def perturbed_hashchain(contexts, r):
    """The hash chain with one opcode exchanged for another one-byte, jump-free opcode: the program still halts
    and fills H, but no recogniser takes it (d++ <-> d--, hash -> hashd, *d=a -> *d=b, c-- -> c++)."""
    p = hashchain(contexts)
    swaps = {25: 26, 59: 60, 112: 113, 18: 17}
    at = [i for i, op in enumerate(p) if op in swaps]
    i = r.choice(at)
    p[i] = swaps[p[i]]
    return p


def header(comps, hh, hm, program):
    b = [hh, hm, 0, 0, len(comps)]
    for c in comps:
        b += c
    return bytes(b + [0] + list(program) + [0])


def chain(sizes, mix=None, hh=9, hm=16, program=None):
    """ICM sizes[0], ISSE sizes[i] fed by component i - 1, then a MIX2 when mix = (bits, j, k, rate, mask)
    (j / k default to the last two components when None).  program: default the hash chain over every component."""
    comps = [[3, sizes[0]]] + [[8, s, i] for i, s in enumerate(sizes[1:])]
    if mix is not None:
        bits, j, k, rate, mask = mix
        n = len(sizes)
        comps.append([6, bits, n - 2 if j is None else j, n - 1 if k is None else k, rate, mask])
    if program is None:
        program = hashchain(len(comps))
    return header(comps, hh, hm, program)


def table_bits(hdr):
    """Table size (bits) of every hashed component (ICM / ISSE) of a header built here."""
    out, p = [], 5
    for _ in range(hdr[4]):
        t = hdr[p]
        if t in (3, 8):
            out.append(hdr[p + 1])
        p += {3: 2, 8: 3, 6: 6}[t]
    return out


# name -> (header, expected route).  A route is (nch_spec, g, vm_kind, has_mix2, n), or None: not a chain model
# (has_fast_path, but no chain layout: k_lanes / k_rows / k_gpipe take it).  Routes as build_cfg gives them, read back
# through zpq_chain_route; spec 0 = the runtime-loop instantiation.
NAMED = {
    # three components: the level-2 specialisation (k_pipe, two-hypothesis decoder, k_dpipe, striped transfers)
    "l2_mixed": (chain([10, 18, 4], hh=9, hm=16), (3, 8, VM_HASHCHAIN, 0, 3)),
    "l2_hh2_hm1": (chain([16, 16, 16], hh=2, hm=1), (3, 8, VM_HASHCHAIN, 0, 3)),      # H 4 words, M 2 bytes: the least taken
    "l2_hm0": (chain([16, 16, 16], hh=9, hm=0), (0, 8, VM_GENERIC, 0, 3)),            # no M: the program reads zeros
    "l2_hh1": (chain([16, 16, 16], hh=1, hm=16), (0, 8, VM_GENERIC, 0, 3)),           # H 2 words < 3 contexts: they wrap
    # two components with level 1's program: the level-1 specialisation (k_pipe2, DST decoder, k_dpipe)
    "l1_sizes": (chain([4, 12], hh=1, hm=2, program=L1_PROG), (2, 8, VM_LEVEL1, 0, 2)),
    "l1_hm3": (chain([16, 19], hh=1, hm=3, program=L1_PROG), (0, 8, VM_GENERIC, 0, 2)),
    "l1_hh2": (chain([16, 19], hh=2, hm=2, program=L1_PROG), (0, 8, VM_GENERIC, 0, 2)),
    # five: HYP16 decoder; dense and line-store tables in one model once the store is small
    "l3_mixed": (chain([6, 20, 12, 0, 14], hh=3, hm=4), (5, 8, VM_HASHCHAIN, 0, 5)),
    # six + MIX2: the level-4 specialisation at other MIX2 sizes and rates
    "l4_rate255": (chain([12, 14, 10, 16, 8, 12], mix=(8, None, None, 255, 255), hh=3, hm=8), (6, 8, VM_HASHCHAIN, 1, 7)),
    "l4_rate0": (chain([12, 14, 10, 16, 8, 12], mix=(12, None, None, 0, 255), hh=4, hm=3), (6, 8, VM_HASHCHAIN, 1, 7)),
    # ... and what the specialisation refuses: mask != 255, fewer than 256 weights, other inputs -> runtime MIX2
    "l4_mask15": (chain([12, 14, 10, 16, 8, 12], mix=(10, None, None, 24, 15), hh=3, hm=8), (0, 8, VM_HASHCHAIN, 1, 7)),
    "l4_s7": (chain([12, 14, 10, 16, 8, 12], mix=(7, None, None, 24, 255), hh=3, hm=8), (0, 8, VM_HASHCHAIN, 1, 7)),
    "l4_jk01": (chain([12, 14, 10, 16, 8, 12], mix=(10, 0, 1, 24, 255), hh=3, hm=8), (0, 8, VM_HASHCHAIN, 1, 7)),
    # eight + MIX2: the level-5 specialisation (16 lanes per block) with small tables
    "l5_small": (chain([10] * 8, mix=(10, None, None, 24, 255), hh=4, hm=10), (8, 16, VM_HASHCHAIN, 1, 9)),
    # runtime-loop instantiations: other chain lengths, 8 and 16 lanes per block, a runtime MIX2
    "icm_only": (chain([14], hh=1, hm=4), (0, 8, VM_HASHCHAIN, 0, 1)),
    "chain4": (chain([8, 16, 12, 3], hh=2, hm=6), (0, 8, VM_HASHCHAIN, 0, 4)),
    "chain7": (chain([9, 11, 13, 15, 5, 0, 16], hh=3, hm=9), (0, 8, VM_HASHCHAIN, 0, 7)),
    "chain9": (chain([12, 6, 14, 8, 16, 10, 2, 12, 9], hh=4, hm=12), (0, 16, VM_HASHCHAIN, 0, 9)),
    "chain16": (chain([(5 * i + 3) % 17 for i in range(16)], hh=4, hm=16), (0, 16, VM_HASHCHAIN, 0, 16)),
    "mix2_chain3": (chain([12, 16, 8], mix=(9, None, None, 40, 255), hh=2, hm=5), (0, 8, VM_HASHCHAIN, 1, 4)),
    "chain15_mix2": (chain([(3 * i + 1) % 15 for i in range(15)], mix=(11, 13, 14, 200, 255), hh=4, hm=7),
                     (0, 16, VM_HASHCHAIN, 1, 16)),
    # chain-like, but not a chain layout: 17 components; an ISSE fed by a component other than its predecessor
    "chain17": (chain([(7 * i) % 12 + 1 for i in range(17)], hh=5, hm=8), None),
    "isse_j_skip": (header([[3, 12], [8, 10, 0], [8, 14, 0], [8, 9, 2]], 2, 8, hashchain(4)), None),
}

# blocks per workgroup pinned where they are not the LDS cap of a short chain (the longest chains)
NAMED_BPW = {"chain16": 4, "chain15_mix2": 4, "l5_small": 12}


def route(zpq, model):
    """build_cfg's verdict on a zpq.Model via the internal zpq_chain_route: a dict, or None (not a chain model)."""
    L = zpq.lib()
    f = L.zpq_chain_route
    f.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    f.restype = C.c_int
    out = (C.c_int32 * 8)()
    if not f(model.h, out):
        return None
    keys = ("n", "nisse_end", "has_mix2", "nch_spec", "g", "vm_kind", "blocks_per_wg", "sparse")
    return dict(zip(keys, list(out)))


def route_key(rt):
    """A route as the (nch_spec, g, vm_kind, has_mix2, n) of NAMED, or None."""
    return None if rt is None else (rt["nch_spec"], rt["g"], rt["vm_kind"], rt["has_mix2"], rt["n"])


def route_class(rt):
    """Coarse class of a route for coverage counts."""
    if rt is None:
        return "not_chain"
    if rt["nch_spec"]:
        return "spec%d" % rt["nch_spec"]
    return "runtime_%s_g%d" % ("mix2" if rt["has_mix2"] else "plain", rt["g"])


def _bits(r, big):
    if big and r.random() < 0.06:
        return r.randint(18, 20)
    return r.choice([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 12, 13, 14, 14, 15, 16, 16])


def _at_least(x):
    """Smallest hh / hm with 1 << h >= x."""
    return max(0, (x - 1).bit_length())


def random_chain(r, big=False, max_big=2):
    """One random chain-shaped header from random.Random r.  Draws the shape (near a specialisation, any length 1-16, or
    now and then one step outside the chain layout: 17 components, or an ISSE fed by an older component), table bits per
    component (0-16; with big, a few 18-20), hh / hm on both sides of the recognisers' bounds, the program (hash chain,
    level 1's, or a perturbed hash chain) and the MIX2 (bits 0-12, rate 0-255, mask 255 / 15 / 0, j / k the last two or
    any earlier pair)."""
    shape = r.choice(["any"] * 6 + ["s2", "s2", "s3", "s3", "s5", "s5", "s6", "s6", "s8", "s8", "nc"])
    if shape == "any":
        nch = r.randint(1, 16)
        mix = nch < 16 and r.random() < 0.35
    elif shape == "nc":
        nch = r.choice([17, r.randint(3, 8)])
        mix = nch < 17 and r.random() < 0.3
    else:
        nch, mix = {"s2": (2, False), "s3": (3, False), "s5": (5, False), "s6": (6, True), "s8": (8, True)}[shape]
    sizes, nbig = [], 0
    for _ in range(nch):
        b = _bits(r, big and nbig < max_big)
        nbig += b >= 18
        sizes.append(b)
    n = nch + (1 if mix else 0)
    kind = r.random()
    if shape == "s2" and kind < 0.7 or kind < 0.08:
        program = L1_PROG
        hh = r.choice([1, 1, 1, 0, 2])
        hm = r.choice([2, 2, 2, 1, 3])
    else:
        program = hashchain(n) if kind < 0.85 else perturbed_hashchain(n, r)
        need = max(1, _at_least(n))                       # H holds >= n words (hh 0: no H at all)
        hh = r.choice([need, need, need + r.randint(1, 4), need - 1])
        hm = r.choice([1, 2, r.randint(3, 16), r.randint(3, 16), 0])
    m = None
    if mix:
        bits = r.choice([8, 8, 9, 10, 11, 12, r.randint(0, 12)])
        rate = r.choice([24, 255, 0, r.randint(0, 255)])
        mask = r.choice([255, 255, 255, 15, 0])
        if nch >= 2 and r.random() < 0.75:
            j, k = nch - 2, nch - 1
        else:
            j, k = r.randrange(nch), r.randrange(nch)
        m = (bits, j, k, rate, mask)
    hdr = chain(sizes, mix=m, hh=hh, hm=hm, program=program)
    if shape == "nc" and nch < 17:                        # ISSE i fed by component i - 2 instead of i - 1
        i = r.randint(2, nch - 1)
        hdr = bytearray(hdr)
        hdr[5 + 2 + 3 * (i - 1) + 2] = i - 2
        hdr = bytes(hdr)
    return hdr


def generated(seed, count, big=False):
    """`count` headers from a seeded sequence (the same on every machine)."""
    r = random.Random(seed)
    return [random_chain(r, big=big) for _ in range(count)]
