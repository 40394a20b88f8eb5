"""HCOMP programs that loop, carry state from run to run and end in every way a run can end: an assembler, named
programs, a seeded generator of structured programs, and the model shapes that put a program in front of each kernel
that embeds the interpreter (zpq_vm.h::vm_run): k_chain's runtime instantiation at 8 and 16 lanes per block, k_rows,
k_lanes with H in LDS and in the slot, k_generic.  test_zpaql_programs_cpu.py pins the corpus (two reference VMs agree,
every run ends, what it covers); test_gpu_zpaql_programs.py holds every route to the oracle on it.

A program is a dict: body (assembler items, or a function of the number of contexts n), tail ("acc" | "set" | None: how
the n contexts are written after the body), end (the items after the tail; default halt), hh / hm, and to_len (the
header ends with the program's last byte: hend == len(header), no trailing 0).

Assembler items: an int is a raw byte; "name:" defines a label; a string is a one-byte mnemonic; a tuple is
(mnemonic, operand) with an int operand or, for jt / jf / jmp / lj, a label.
"""
import random

from chain_models import HC_HEAD, HC_LINK, HC_TAIL, header
from general_models import CM, ICM, ISSE, MATCH, MIX, cms, isse_chain

TARGETS = ["a", "b", "c", "d", "*b", "*c", "*d"]
SOURCES = TARGETS + ["N"]


def _mnemonics():
    one, two = {"halt": 56, "out": 57, "hash": 59, "hashd": 60, "nop": 0}, {"jt": 39, "jf": 47, "jmp": 63, "r=a": 55}
    for t, x in enumerate(TARGETS):
        if t:
            one[x + "<>a"] = 8 * t
        one[x + "++"], one[x + "--"], one[x + "!"], one[x + "=0"] = 8 * t + 1, 8 * t + 2, 8 * t + 3, 8 * t + 4
        if t < 4:
            two[x + "=r"] = 8 * t + 7
        for s, y in enumerate(SOURCES):
            (two if s == 7 else one)[x + "=" + (y if s < 7 else "")] = 64 + 8 * t + s
    for g, name in enumerate(["a+=", "a-=", "a*=", "a/=", "a%=", "a&=", "a&~", "a|=", "a^=", "a<<=", "a>>=", "a==", "a<", "a>"]):
        for s, y in enumerate(SOURCES):
            (two if s == 7 else one)[name + (y if s < 7 else "")] = 128 + 8 * g + s
    return one, two


ONE, TWO = _mnemonics()
JUMPS = (39, 47, 63)


def defined(op):
    """An opcode the reference executes (everything else ends the run silently)."""
    if op < 56:
        return op & 7 not in (5, 6)
    if op < 64:
        return op in (56, 57, 59, 60, 63)
    return op < 120 or 128 <= op < 240 or op == 255


def oplen(op):
    return 3 if op == 255 else 2 if op & 7 == 7 else 1


def asm(items):
    """Program bytes of `items`.  JT / JF / JMP operands follow the reference's rule: the jump adds
    ((N + 128) & 255) - 127 to the pc AFTER the operand fetch, so N = 0 skips one byte and 63 0xFD jumps to itself;
    an LJ target is relative to hbegin, i.e. to the program's first byte."""
    pos, labels, out = 0, {}, []
    for it in items:                                     # pass 1: sizes and labels
        if isinstance(it, str) and it.endswith(":"):
            assert it[:-1] not in labels, it
            labels[it[:-1]] = pos
        elif isinstance(it, tuple):
            pos += 3 if it[0] == "lj" else 2
        else:
            pos += 1
    for it in items:
        if isinstance(it, int):
            out.append(it & 255)
        elif isinstance(it, tuple):
            m, x = it
            if m == "lj":
                x = labels[x] if isinstance(x, str) else x
                out += [255, x & 255, (x >> 8) & 255]
                continue
            op = TWO[m]
            if isinstance(x, str):
                assert op in JUMPS, it
                rel = labels[x] - (len(out) + 2)
                assert -127 <= rel <= 128, (it, rel)
                x = (rel - 1) & 255
            out += [op, x & 255]
        elif not it.endswith(":"):
            out.append(ONE[it])
    assert len(out) == pos
    return out


def tail_acc(n):
    """n contexts, each folded into what it held: H[i] = (H[i] + a + 512) * 773, a += H[i].  H keeps its history, so
    whatever an earlier run, the loop before it or a neighbour did to H stays visible in every later context."""
    return ["d=0"] + ["hashd", "a+=*d", "d++"] * n


def tail_set(n):
    """n contexts set from a alone, the way the shipped chain does: (hash *d=a d++) n times."""
    return ["d=0"] + ["hash", "*d=a", "d++"] * n


def _fold(n=1):
    """c = (c + a) * 251: the arithmetic program's running result."""
    return ["a+=c", ("a*=", 251), "c=a"] * n


def _arith(n):
    f = ["a=0", ("jf", 0), "a++"] + _fold()              # a = F (jf 0 skips the one-byte a++), folded
    p = ["b=a", "c=0"]
    for op in (("a/=", 0), ("a%=", 0)):                  # division and modulo by zero: no-ops
        p += ["a=b", op] + _fold()
    p += ["*b=0", "a=b", "a/=*b", "a%=*b"] + _fold()    # ... by a zero in M
    p += ["a=b", "a++", "*b=a", "a!", "a/=*b"] + _fold() + ["a=b", "a!", "a%=*b"] + _fold()
    for s in (0, 31, 32, 33, 255):                       # shift counts are masked to five bits
        p += ["a=b", "a++", ("a<<=", s)] + _fold() + ["a=b", "a!", ("a>>=", s)] + _fold()
    p += ["a=b", "a!", "a*=a"] + _fold() + ["a=b", ("a+=", 200), ("a<<=", 24), ("a*=", 255)] + _fold()
    p += ["a=0", "a!", "d=a"]                            # d = 0xFFFFFFFF: unsigned compares at both ends
    for cmp in ("a<d", "a>d", "a==d", ("a<", 0), ("a>", 0), ("a==", 0)):
        p += ["a=0", cmp] + f + ["a=d", cmp] + f
    p += ["a=b", "a!", ("a&~", 15)] + _fold() + ["a=b", "a!", "a&~b"] + _fold()
    p += ["a=b", ("a+=", 3), "b<>a"] + _fold() + ["a=b", "c<>a", "a++", "c<>a"] + _fold() + ["d<>a"] + _fold()
    p += ["a=b", "*b<>a"] + _fold() + ["*c<>a"] + _fold() + ["d=0", "*d<>a"] + _fold()
    p += ["a!", "b!", "b!", "d!", "*b!", "*c!", "*d!", "a+=*b", "a+=*c", "a+=*d", "a+=d"] + _fold()
    p += ["c!", "c!", "a=c", "hash"] + _fold()           # hash reads *b: a zero where the model has no M
    return p + ["a=c"]


def _all_ops(n):
    """Every defined opcode that is no jump and no halt, once, in order, with an operand from its own number."""
    p = ["b=a"]
    for op in range(256):
        if defined(op) and op not in JUMPS + (56, 255):
            p += [op] + ([(op * 7 + 3) & 255] if oplen(op) == 2 else [])
    return p


def _undefined(n):
    """An undefined opcode of every family, picked by the byte's low four bits, each followed by code that would zero
    the contexts if the run went on."""
    ops = [5, 6, 53, 54, 58, 61, 62, 120, 126, 240, 254]
    p = ["a=b", ("a&=", 15)]
    for i in range(len(ops)):
        p += [("a==", i), ("jt", "u%d" % i)]
    p += ["halt"]
    for i, op in enumerate(ops):
        p += ["u%d:" % i, op, ("jmp", "spoil")]
    return p + ["spoil:", "d=0", "*d=0", "d++", "*d=0", "d++", "*d=0", "halt"]


LOOP_COUNT = ["b=a", ("a&=", 15), "a++", "c=a", "d=0",
              "loop:", "a=b", "hashd", "d++", "a=d", ("a&=", 3), "d=a", "c--", "a=c", ("a>", 0), ("jt", "loop"), "a=b"]


def P(body, tail="acc", end=("halt",), hh=5, hm=8, to_len=False):
    return dict(body=body, tail=tail, end=end if callable(end) else list(end), hh=hh, hm=hm, to_len=to_len)


NAMED = {
    # ---- loops
    # (a) (byte & 15) + 1 iterations of hashd d++, d wrapped by a&= 3; closed by a backward JT
    "loop_count": P(LOOP_COUNT),
    # (b) the count comes from M: scan back over *b until the byte repeats or 32 steps; backward JMP, forward JT exits
    "loop_scan_m": P(["c++", "*c=a", "b=c", "d=0",
                      "loop:", "b--", "d++", "a=d", ("a>", 31), ("jt", "done"), "a=*c", "a==*b", ("jt", "done"), ("jmp", "loop"),
                      "done:", "a=d", ("a<<=", 8), "a+=*c"]),
    # (c) nested: (byte & 3) + 1 times ((byte >> 2) & 7) + 1 hashd; inner loop closed by a backward JF, outer by JT
    "loop_nested": P([("r=a", 5), ("a&=", 3), "a++", "c=a",
                      "outer:", ("a=r", 5), ("a>>=", 2), ("a&=", 7), "a++", "b=a",
                      "inner:", "a=c", "a+=b", "d=a", ("a=r", 5), "hashd", "b--", "a=b", ("a==", 0), ("jf", "inner"),
                      "c--", "a=c", ("a>", 0), ("jt", "outer"), ("a=r", 5)]),
    # (d) the loop of (a) closed by LJ
    "loop_lj": P(["b=a", ("a&=", 15), "a++", "c=a", "d=0",
                  "loop:", "a=b", "hashd", "d++", "a=d", ("a&=", 3), "d=a", "c--", "a=c", ("a==", 0), ("jt", "out"), ("lj", "loop"),
                  "out:", "a=b"]),
    # (e) the first instruction jumps on the F the PREVIOUS run left (byte > 100): the loop runs one byte late
    "loop_on_old_f": P([("jt", "loop"), ("jmp", "join"),
                        "loop:", "b=a", ("a&=", 7), "a++", "c=a", "d=0",
                        "l2:", "a=b", "hashd", "d++", "c--", "a=c", ("a>", 0), ("jt", "l2"), "a=b",
                        "join:", ("a>", 100)]),
    # ---- state carried from run to run
    # (f) d is never reset: n hashd per byte walk all of H and wrap at hlen
    "d_walks_h": P(lambda n: ["c--", "*c=a", "b=c"] + ["hashd", "d++"] * n, tail=None, hh=4),
    # (g) an R delay line over R 0, 1, 127, 255: a byte reaches the contexts again one, two and three runs later
    "r_delay": P(["b=a", ("a=r", 127), ("r=a", 255), ("a=r", 1), ("r=a", 127), ("a=r", 0), ("r=a", 1), "a=b", ("r=a", 0),
                  ("a=r", 255), ("a<<=", 8), ("c=r", 127), "a+=c", ("a<<=", 8), ("c=r", 1), "a+=c", ("a<<=", 8), ("c=r", 0), "a+=c"],
                 tail="set"),
    # (h) b-- from 0 indexes M at 0xFFFFFFFF (masked by mlen - 1) and walks down; *b++ takes a cell from 255 to 0
    "m_wraps": P(["b--", "*b=a", "*b++", "c=0", "c--", "a+=*c", "a+=b"], tail="set", hm=3),
    # (i) F carried over runs that execute no compare: once (byte & 31) == 5 every later run takes the other path
    "f_sticks": P([("jf", "normal"), ("a+=", 77), ("jmp", "tail"),
                   "normal:", "b=a", ("a&=", 31), ("a==", 5), "a=b", "tail:"]),
    # ---- ends of a run other than HALT (the contexts are written before each)
    "end_off_hend": P(["b=a"], end=()),                                              # (j) no HALT: the pc reaches hend
    "end_jmp_fwd": P(["b=a"], end=(("jmp", 100), "d=0", "*d=0")),                    # (k) JMP beyond hend
    "end_jmp_back": P(["b=a"], end=(("jmp", 128), "d=0", "*d=0")),                   # (l) JMP -127: below hbegin
    "end_undefined": P(["b=a"], end=_undefined),                                     # (m) see _undefined
    "end_lj_out": P(["b=a"], end=(("lj", 0x7F00), "d=0", "*d=0")),                   # (n) LJ to a target >= hend
    # (o) r=a as the header's last byte: no operand to fetch, so R[0] = a; the next run reads R[0] back
    "end_cut_operand": P([("a=r", 0), ("a*=", 31), "a+=b", "b=a"], end=(55,), to_len=True),
    # (p) LJ as the header's last byte: the target comes from the two bytes before the pc (the second is the LJ itself)
    "end_cut_lj": P(["b=a"], end=(255,), to_len=True),
    # ---- (q) arithmetic edges, with and without M; every defined non-jump opcode once
    "arith": P(_arith, tail="set"),
    "arith_no_m": P(_arith, tail="set", hm=0),
    "all_ops": P(_all_ops),
    # ---- memory sizes: (a) with no H (every context 0), the least H and M, k_lanes' LDS / slot switch (hh 8 / 9), a large H
    "loop_hh0_hm0": P(LOOP_COUNT, hh=0, hm=0),
    "loop_hh1_hm1": P(LOOP_COUNT, hh=1, hm=1),
    "loop_hh8_hm8": P(LOOP_COUNT, hh=8, hm=8),
    "loop_hh9_hm16": P(LOOP_COUNT, hh=9, hm=16),
    "loop_hh12_hm0": P(LOOP_COUNT, hh=12, hm=0),
}
SEGMENT_PROGRAMS = ("loop_on_old_f", "d_walks_h", "r_delay", "f_sticks")
END_PROGRAMS = {"end_off_hend": "hend", "end_jmp_fwd": "jmp_fwd", "end_jmp_back": "jmp_back", "end_undefined": "undefined",
                "end_lj_out": "lj_out", "end_cut_operand": "cut_operand", "end_cut_lj": "cut_lj"}
GEN_SEED, GEN_COUNT = 33, 16                                # (this seed reaches every hh and hm the generator draws)


def step_cap_program(n):
    """a== 255; jf go; jmp self in front of the shipped hash chain: a run never ends on byte 0xFF, and only there."""
    return asm([("a==", 255), ("jf", "go"), "self:", ("jmp", "self"), "go:"]) + HC_HEAD + HC_LINK * (n - 1) + HC_TAIL


STEP_CAP = dict(body=None, tail=None, end=[], hh=5, hm=8, to_len=False)


def assemble(prog, n):
    """The program's bytes for a model of n contexts."""
    if prog is STEP_CAP:
        return step_cap_program(n)
    body = prog["body"](n) if callable(prog["body"]) else list(prog["body"])
    end = prog["end"](n) if callable(prog["end"]) else list(prog["end"])
    tail = {"acc": tail_acc, "set": tail_set, None: lambda n: []}[prog["tail"]](n)
    return asm(body + tail + end)


# ---------------------------------------------------------------- the generator
RESERVED_R = (249, 250, 251)                             # the saved byte and the two loop counters: no body writes them


def _random_ops(r, count):
    """`count` random defined opcodes, no jump, no halt, no write to a reserved R."""
    out = []
    for _ in range(count):
        op = r.choice([o for o in range(1, 240) if defined(o) and o not in JUMPS + (56,)])
        out.append(op)
        if oplen(op) == 2:
            x = r.choice([0, 1, 2, 3, 7, 31, 32, 255, r.randrange(256), r.randrange(256)])
            out.append(x % 249 if op == 55 else x)
    return out


def _bound(r, top):
    """Loop bound into a: a constant, or (byte & mask) + 1 -- the trip count then follows the data."""
    if r.random() < 0.5:
        return [("a=", r.randint(1, top))]
    return [("a=r", 249), ("a&=", top - 1), "a++"]


def _loop(r, uid, depth):
    k = 250 + depth
    inner = _loop(r, uid + "i", 1) if depth == 0 and r.random() < 0.4 else []
    top = 4 if depth else (8 if inner else 16)
    body = _random_ops(r, r.randint(1, 4 if depth else 6)) + inner + _random_ops(r, r.randint(0, 3))
    return (_bound(r, top) + [("r=a", k), "L%s:" % uid] + body
            + [("a=r", k), "a--", ("r=a", k), ("a>", 0), ("jt", "L%s" % uid)])


def _diamond(r, uid):
    cmp = r.choice([("a>", r.randrange(256)), ("a<", r.randrange(256)), ("a==", r.randrange(8)), "a<d", "a>*b", "a==*c"])
    jmp = r.choice(["jt", "jf"])
    return ([cmp, (jmp, "E%s" % uid)] + _random_ops(r, r.randint(1, 5)) + [("jmp", "X%s" % uid), "E%s:" % uid]
            + _random_ops(r, r.randint(1, 5)) + ["X%s:" % uid])


def _hop(r, uid):
    return [("lj", "H%s" % uid)] + [r.choice([5, 6, 58, 120, 254, 56]) for _ in range(r.randint(1, 4))] + ["H%s:" % uid]


def random_program(r):
    """One structured program from random.Random r that always terminates: blocks drawn from counted loops (the counter
    in a reserved R, bound at most 16, nested at most twice), forward JT / JF diamonds, straight-line runs of random
    defined opcodes and forward LJ hops, then the accumulating tail.  hh / hm on both sides of 8 / 9, and 0 now and then."""
    body = [("r=a", 249)]
    for i in range(r.randint(2, 5)):
        kind = r.choice(["loop", "loop", "diamond", "line", "hop"])
        uid = "%d" % i
        body += (_loop(r, uid, 0) if kind == "loop" else _diamond(r, uid) if kind == "diamond"
                 else _hop(r, uid) if kind == "hop" else _random_ops(r, r.randint(2, 10)))
    body += [("a=r", 249)]
    return P(body, hh=r.choice([0, 3, 5, 8, 8, 9, 9, 10]), hm=r.choice([0, 1, 8, 9, 12]))


def generated(seed=GEN_SEED, count=GEN_COUNT):
    r = random.Random(seed)
    return [random_program(r) for _ in range(count)]


# ---------------------------------------------------------------- model shapes
SHAPES = {
    "chain": [[ICM, 10], [ISSE, 8, 0], [ISSE, 12, 1]],                                   # k_chain, 8 lanes per block
    "chain16": isse_chain(8, bits=(10, 8, 12, 6, 7, 9, 11, 5, 4)),                       # nine links: 16 lanes per block
    "rows": [[CM, 6, 255], [ICM, 7], [ISSE, 6, 1], [MATCH, 8, 9], [MIX, 4, 0, 4, 24, 255]],
    "lanes": isse_chain(8) + cms(9, 4, 8) + [[MIX, 4, 9, 9, 24, 255]],                   # 19 components: k_lanes
    "generic": cms(64, 4, 9) + [[MIX, 4, 56, 8, 24, 255]],                               # 65: k_generic alone
}
KERNEL = {"chain": "k_chain", "chain16": "k_chain", "rows": "k_rows", "lanes": "k_lanes", "generic": "k_generic"}


def embed(prog, shape):
    """(header, (cend, hbegin, hend)) of `prog` behind the components of `shape`."""
    comps = SHAPES[shape]
    code = assemble(prog, len(comps))
    hdr = header(comps, prog["hh"], prog["hm"], code)
    if prog["to_len"]:
        hdr = hdr[:-1]
    cend = 5 + sum(len(c) for c in comps)
    return hdr, (cend, cend + 1, cend + 1 + len(code))


# ---------------------------------------------------------------- inputs
LENGTHS = [0, 1, 2, 17, 64, 65, 300, 1500, 0, 1, 2, 17, 64, 65, 300, 17, 64, 65, 300, 1, 2, 17, 1500]   # 23 blocks


def _data(r, kind, n):
    if kind == 0:
        return bytes(n)
    if kind == 1:
        return bytes(r.getrandbits(8) for _ in range(n))
    if kind == 2:
        return bytes(r.choice(b"etaoin shrdlu\n") for _ in range(n))
    per = bytes(r.getrandbits(8) for _ in range(r.randint(1, 40)))
    return (per * (n // len(per) + 1))[:n]


def batch(seed=7):
    """23 blocks (no multiple of 4, 8 or 16) of 0 .. 1500 bytes: zeros, random, text, periodic."""
    r = random.Random(seed)
    return [_data(r, (i + i // 8) % 4, n) for i, n in enumerate(LENGTHS)]


def divergence_batch(seed=8):
    """Neighbours in a row, group or wave run 1 against 16 iterations of loop_count at every byte."""
    r = random.Random(seed)
    kinds = [b"\x00", b"\x0f", b"\xf0", b"\xff", None]
    return [(_data(r, 1, 200) if kinds[i % 5] is None else kinds[i % 5] * 200) for i in range(23)]


def step_cap_batch(seed=9):
    """12 blocks of at most 40 bytes without 0xFF, except blocks 1, 6 and 7: two, one and two 0xFF bytes."""
    r = random.Random(seed)
    blocks = [bytes(r.randrange(255) for _ in range(n)) for n in (40, 30, 0, 1, 17, 40, 40, 9, 33, 2, 40, 25)]
    for i, at in ((1, (3, 20)), (6, (39,)), (7, (0, 8))):
        b = bytearray(blocks[i])
        for p in at:
            b[p] = 255
        blocks[i] = bytes(b)
    return blocks
