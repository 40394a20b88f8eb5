"""The ZPAQL program corpus (tests/zpaql_programs.py) pinned without a GPU: the C oracle's VM and the independent Python
reference VM agree on every register and every word of H, M and R after every run, on the very blocks the GPU test
codes; every run ends (and how many steps the costliest block takes); what the corpus covers -- every defined opcode,
every kind of jump taken, every way a run can end, neighbours that differ fourfold in steps; the route each embedding
takes on the host; and that the three step caps are one number."""
import array
import ctypes as C
import os
import re
import sys

import pytest

import chain_models as CMOD
import general_models as GM
import oracle_lib as O
import zpaql_programs as ZP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "pyref"))
import zpaq_pyref as PY  # noqa: E402

BLOCK_STEP_BOUND = 1 << 21
ROUTE_SHAPES = ("chain", "chain16", "rows", "lanes")
GENERIC_PROGRAMS = ("loop_count", "r_delay")              # the 65-component shape (its tail alone is 196 bytes long)
PROGRAMS = dict(ZP.NAMED)
PROGRAMS.update(("generated%02d" % i, p) for i, p in enumerate(ZP.generated()))


class Tracer(PY.ZPAQL):
    """The Python reference VM, counting steps and recording which opcodes ran, which jumps were taken and which way,
    and how each run ended."""

    def __init__(self, *a):
        super().__init__(*a)
        self.ops, self.taken, self.ends = set(), set(), set()
        self.steps = 0
        self.last = None

    def execute(self):
        pc0 = self.pc
        if pc0 < self.hbegin or pc0 >= self.hend:
            return super().execute()
        op = self.header[pc0]
        ok = super().execute()
        cut = pc0 + ZP.oplen(op) > len(self.header)       # the operand fetch was refused by the header's length
        if ok or op in (56, 255):
            self.ops.add(op)
        if ok:
            self.steps += 1
            if op in ZP.JUMPS and self.pc != pc0 + (1 if cut else 2):
                self.taken.add(({39: "jt", 47: "jf", 63: "jmp"}[op], "back" if self.pc <= pc0 else "fwd"))
            if op == 255:
                self.taken.add(("lj", "back" if self.pc <= pc0 else "fwd"))
            if cut:
                self.ends.add("cut_operand")
            elif self.pc >= self.hend:
                self.ends.add("jmp_fwd" if op in ZP.JUMPS else "hend")
            elif self.pc < self.hbegin:
                self.ends.add("jmp_back")
        else:
            self.ends.add("halt" if op == 56 else ("cut_lj" if cut else "lj_out") if op == 255 else "undefined")
        return ok

    def run(self, inp):
        self.steps = 0
        try:
            super().run(inp)
        except RuntimeError:
            return False
        return True


def oracle_steps(hdr, offs, blocks):
    """Per block: (steps summed over its runs, the PP byte's included; the longest run; whether a run hit the cap)."""
    L = O.lib()
    out = []
    for b in blocks:
        z = L.zo_vm_new(hdr, len(hdr), *offs)
        total = longest = 0
        for x in b"\0" + b:
            L.zo_vm_run(z, x)
            s = L.zo_vm_steps(z)
            total += s
            longest = max(longest, s)
        out.append((total, longest, bool(L.zo_vm_overflow(z))))
        L.zo_vm_free(z)
    return out


def two_vms(hdr, offs, blocks):
    """Both VMs over PP byte + block, compared after every run; returns the tracers."""
    L = O.lib()
    tracers = []
    for bi, b in enumerate(blocks):
        z = L.zo_vm_new(hdr, len(hdr), *offs)
        t = Tracer(hdr, *offs)
        hlen, mlen = L.zo_vm_hlen(z), L.zo_vm_mlen(z)
        assert (hlen, mlen) == (len(t.h), len(t.m))
        hb, mb, rb = C.create_string_buffer(4 * hlen + 4), C.create_string_buffer(mlen + 1), C.create_string_buffer(1024)
        for i, x in enumerate(b"\0" + b):
            L.zo_vm_run(z, x)
            ended = t.run(x)
            at = (bi, i, x)
            assert [L.zo_vm_reg(z, k) for k in range(5)] == [t.a, t.b, t.c, t.d, t.f], at
            assert L.zo_vm_steps(z) == t.steps and bool(L.zo_vm_overflow(z)) == (not ended), at
            L.zo_vm_dump(z, hb, mb, rb)
            assert hb.raw[:4 * hlen] == array.array("I", t.h).tobytes(), at
            assert mb.raw[:mlen] == bytes(t.m), at
            assert rb.raw == array.array("I", t.r).tobytes(), at
            if not ended:
                break
        L.zo_vm_free(z)
        tracers.append(t)
    return tracers


_TRACE = {}


def trace(name):
    """The corpus program on the `rows` embedding over the GPU test's batch, through both VMs (once per session)."""
    if name not in _TRACE:
        hdr, offs = ZP.embed(PROGRAMS[name], "rows")
        _TRACE[name] = two_vms(hdr, offs, ZP.batch())
    return _TRACE[name]


def test_assembler_follows_the_reference_jump_rule():
    assert ZP.asm(["self:", ("jmp", "self")]) == [63, 0xFD]                      # jumps to itself
    assert ZP.asm([("jf", "x"), "a++", "x:"]) == [47, 0, 1]                       # N = 0 skips one byte
    assert ZP.asm(["a++", "l:", "hashd", ("lj", "l")]) == [1, 60, 255, 1, 0]      # LJ: relative to the first byte
    assert ZP.asm(["b=c", "c--", "*c=a", ("d=", 0)]) == CMOD.HC_HEAD and ZP.asm(["hash", "*d=a", "d++"]) == CMOD.HC_LINK
    assert sorted(set(ZP.ONE.values()) | set(ZP.TWO.values()) | {255}) == [op for op in range(256) if ZP.defined(op)]


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_two_reference_vms_agree(name):
    trace(name)


@pytest.mark.parametrize("name", sorted(ZP.NAMED))
def test_two_reference_vms_agree_behind_every_other_shape(name):
    """The program's bytes depend on the number of contexts (the tail; d_walks_h's body): the named programs as the GPU
    test feeds them to the chain kernels (n = 3, 9), k_lanes (19) and k_generic (65), on the batch's 21 blocks of up to
    300 bytes (the two 1500-byte blocks run through both VMs on the `rows` embedding above)."""
    blocks = [b for b in ZP.batch() if len(b) <= 300]
    assert len(blocks) == 21
    for shape in ("chain", "chain16", "lanes") + (("generic",) if name in GENERIC_PROGRAMS else ()):
        hdr, offs = ZP.embed(ZP.NAMED[name], shape)
        two_vms(hdr, offs, blocks)


def test_step_cap_program_stops_both_vms_after_the_same_step():
    hdr, offs = ZP.embed(ZP.STEP_CAP, "rows")
    tracers = two_vms(hdr, offs, ZP.step_cap_batch())     # (a capped run ends the comparison of its block)
    capped = [i for i, t in enumerate(tracers) if t.steps >= PY.ZPAQL.STEP_CAP]
    assert capped == [1, 6, 7]
    for shape in ROUTE_SHAPES:
        hdr, offs = ZP.embed(ZP.STEP_CAP, shape)
        assert [i for i, s in enumerate(oracle_steps(hdr, offs, ZP.step_cap_batch())) if s[2]] == [1, 6, 7], shape
    assert all(b.count(255) <= 2 and len(b) <= 40 for b in ZP.step_cap_batch()) and len(ZP.step_cap_batch()) == 12


def test_the_three_step_caps_are_one_number():
    text = open(os.path.join(ROOT, "include", "zpaq_hip.h")).read()
    shift = re.search(r"#define ZPQ_VM_STEP_CAP \(1u << (\d+)\)", text)
    assert shift and 1 << int(shift.group(1)) == O.lib().zo_vm_step_cap() == PY.ZPAQL.STEP_CAP == 1 << 20


def test_every_run_ends_and_no_block_costs_more_than_the_bound():
    """No run of any program outside the step-cap group overflows on any test input, and the steps summed over any one
    block stay within 1 << 21 (about two capped runs: what the older step-cap test costs a lane)."""
    worst = {}
    for name, prog in sorted(PROGRAMS.items()):
        shapes = ROUTE_SHAPES + (("generic",) if name in GENERIC_PROGRAMS else ())
        for shape in shapes:
            hdr, offs = ZP.embed(prog, shape)
            batches = [ZP.batch()] + ([ZP.divergence_batch()] if name == "loop_count" else [])
            for blocks in batches:
                for i, (total, longest, over) in enumerate(oracle_steps(hdr, offs, blocks)):
                    assert not over and total <= BLOCK_STEP_BOUND, (name, shape, i, total, longest)
                    if total > worst.get(name, (0,))[0]:
                        worst[name] = (total, longest, shape)
    print("\nmost steps in one block / in one run (pytest -s shows them):")
    for name, (total, longest, shape) in sorted(worst.items()):
        print("  %-16s %8d %6d  (%s)" % (name, total, longest, shape))


def test_the_corpus_covers_every_opcode_jump_and_end():
    ops, taken, ends = set(), set(), {}
    for name in PROGRAMS:
        for t in trace(name):
            ops |= t.ops
            taken |= t.taken
            for e in t.ends:
                ends.setdefault(e, set()).add(name)
    assert sorted(ops) == [op for op in range(256) if ZP.defined(op)], sorted(set(range(256)) - ops)
    assert {("jmp", "back"), ("jt", "back"), ("jf", "back"), ("lj", "back"), ("jmp", "fwd"), ("jt", "fwd"), ("jf", "fwd"),
            ("lj", "fwd")} <= taken, taken
    for name, end in ZP.END_PROGRAMS.items():             # each end kind is reached by the program named for it
        assert name in ends.get(end, ()), (name, end, {k: sorted(v) for k, v in ends.items()})
    assert "halt" in ends


def test_undefined_opcodes_of_every_family_end_a_run():
    """end_undefined reaches each of its eleven undefined opcodes, and none of them lets the run go on (H[0] stays)."""
    hdr, offs = ZP.embed(ZP.NAMED["end_undefined"], "rows")
    code = hdr[offs[1]:offs[2]]
    want = {5, 6, 53, 54, 58, 61, 62, 120, 126, 240, 254}
    seen = set()
    for x in range(16):
        t = Tracer(hdr, *offs)
        pcs = []
        orig = t.execute

        def spy():
            pcs.append(t.pc)
            return orig()
        t.execute = spy
        PY.ZPAQL.run(t, x)
        last = code[pcs[-1] - offs[1]]
        seen.add(last)
        assert t.h[0] != 0 and (last in want or last == 56)
    assert want <= seen


def test_neighbours_in_the_divergence_batch_differ_fourfold_in_steps():
    blocks = ZP.divergence_batch()
    for shape in ("rows", "chain", "chain16"):
        hdr, offs = ZP.embed(ZP.NAMED["loop_count"], shape)
        per_run = [s[0] / (len(b) + 1) for s, b in zip(oracle_steps(hdr, offs, blocks), blocks)]
        assert max(per_run[:4]) >= 4 * min(per_run[:4]), (shape, per_run[:4])   # blocks 0-3 share a row group, hence a wave


def test_generated_programs_reach_both_sides_of_the_memory_switches():
    gen = ZP.generated()
    assert {p["hh"] for p in gen} >= {0, 8, 9} and {p["hm"] for p in gen} >= {0, 8, 9}
    assert ZP.generated() == gen                          # seeded: the same on every machine


def test_routes(zpq):
    """The chain embeddings take k_chain's runtime instantiation with the interpreter, at 8 and 16 lanes per block; the
    others are no hash chain and take the lane kernel their size asks for; the 65-component shape is k_generic's alone."""
    progs = dict(PROGRAMS, step_cap=ZP.STEP_CAP)
    for name, prog in sorted(progs.items()):
        for shape in ROUTE_SHAPES + (("generic",) if name in GENERIC_PROGRAMS else ()):
            hdr, offs = ZP.embed(prog, shape)
            model = zpq.Model(header=hdr, offsets=offs)
            assert model.ncomp == len(ZP.SHAPES[shape])
            if shape in ("chain", "chain16"):
                rt = CMOD.route(zpq, model)
                assert rt is not None and model.has_fast_path, (name, shape)
                assert (rt["nch_spec"], rt["vm_kind"], rt["g"]) == (0, CMOD.VM_GENERIC, 8 if shape == "chain" else 16), (name, rt)
            else:
                assert not GM.is_hashchain(hdr)
                gp, gd, lanes, kernel = GM.route(zpq, model)
                assert (gp, gd) == (0, 0), (name, shape)
                assert (lanes, kernel) == {"rows": (1, GM.ROWS), "lanes": (1, GM.LANES), "generic": (0, GM.LANES)}[shape], (name, shape)
            model.close()


def test_segment_programs_scan_to_their_own_offsets():
    """The block-set tests build their models and oracle codecs from the header alone: the scan must find the offsets
    embed() states (no NOP and no LJ in these programs: either would end or shift the reference's scan)."""
    for name in ZP.SEGMENT_PROGRAMS:
        for shape in ROUTE_SHAPES:
            hdr, offs = ZP.embed(ZP.NAMED[name], shape)
            assert O.scan_header(hdr) == offs, (name, shape)
