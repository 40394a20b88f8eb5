"""Are the kernels two builds share the same code?  Disassembles every gfx950 code object of two libzpaq_hip.so builds
(llvm-objdump, no GPU needed) and compares, per kernel symbol, the list of instructions with their operands.
    python tools/isa_identity.py OLD.so NEW.so [name filter ...]      (default filters: k_chain k_pipe)
A k_chain or k_pipe symbol of OLD that NEW lacks is looked up with one more `false` template argument (a parameter added at
the end with a default: KEEP); a k_lanes / k_rows symbol with `false` in front of its last template argument (KEEP, added before VMH, which
stays last).  What follows a kernel's last s_endpgm is no code -- s_nop fill up to the next symbol's alignment, the
prefetch guard behind the module's last function, objdump's `...` for a run of it -- and depends on which function comes
next, so it is left out of the comparison.  Prints the kernels that differ with their per-opcode count changes, then the totals."""
import collections
import os
import re
import struct
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_stats import LLVM, MAGIC  # noqa: E402


def disassemble(so):
    funcs = {}
    with tempfile.TemporaryDirectory() as td:
        fat = os.path.join(td, "fat.bin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fat])
        d = open(fat, "rb").read()
        for m in re.finditer(re.escape(MAGIC), d):
            base = m.start()
            n = struct.unpack_from("<Q", d, base + len(MAGIC))[0]
            p = base + len(MAGIC) + 8
            for _ in range(n):
                off, size, tlen = struct.unpack_from("<QQQ", d, p)
                triple = d[p + 24:p + 24 + tlen].decode()
                p += 24 + tlen
                if "gfx950" not in triple or size == 0:
                    continue
                co = os.path.join(td, "dev.co")
                open(co, "wb").write(d[base + off:base + off + size])
                txt = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
                cur = None
                for ln in txt.splitlines():
                    mm = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
                    if mm:
                        cur = mm.group(1)
                        funcs[cur] = []
                    elif cur and "\t" in ln:
                        funcs[cur].append(re.sub(r"^\s*[0-9a-f]+:\s*", "", ln.split("//")[0]).strip())
    for name, ins in funcs.items():
        ends = [i for i, x in enumerate(ins) if x.split()[0] == "s_endpgm"]
        if ends and all(x.split()[0] in ("s_nop", "s_code_end", "...") for x in ins[ends[-1] + 1:]):
            del ins[ends[-1] + 1:]
    return funcs


def main():
    old, new = disassemble(sys.argv[1]), disassemble(sys.argv[2])
    filters = sys.argv[3:] or ["k_chain", "k_pipe"]
    same = diff = 0
    for name, ia in sorted(old.items()):
        if not any(f in name for f in filters):
            continue
        if name in new:
            other = name
        elif "k_lanes" in name or "k_rows" in name:
            other = re.sub(r"(Lb[01]E)(Lb[01]EEEv6DBatch)", r"\1Lb0E\2", name)
        else:
            other = name.replace("EEEv6DBatch", "ELb0EEEv6DBatch")
        if other not in new:
            print("missing in the new build:", name)
            diff += 1
            continue
        ib = new[other]
        if ia == ib:
            same += 1
            continue
        diff += 1
        ca, cb = collections.Counter(x.split()[0] for x in ia), collections.Counter(x.split()[0] for x in ib)
        print("differs:", name, len(ia), "->", len(ib), {k: cb[k] - ca[k] for k in set(ca) | set(cb) if cb[k] != ca[k]})
    print("identical: %d   different: %d" % (same, diff))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
