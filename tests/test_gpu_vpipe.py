"""GPU parity of k_vpipe / k_vdec (zpq_gpipe.hip): the wave-per-component pipelines with an interpreter wave, taken on
request (ZPQ_FLAG_VMPIPE / ZPQ_VM_PIPE) for general models whose HCOMP program is not the shipped hash chain.  Every
coded stream is compared byte for byte with the CPU oracle's, every decode with what the same call answers on k_rows, and
the kernel that ran is asserted by name after each call."""
import random

import pytest

import general_models as GM
import offnominal_corpus as OC
import oracle_lib as O
import test_gpu_general_models as TG
import vpipe_models as VM
import zpaql_programs as ZP
from test_gpu_chain_models import BUDGET, knobs
from test_gpu_offnominal import dev_call, raw_decode

pytestmark = pytest.mark.gpu

PROGRAMS = dict(ZP.NAMED)
PROGRAMS.update(("generated%02d" % i, p) for i, p in enumerate(ZP.generated()))
ENC, DEC = "k_vpipe<encode>", "k_vdec<decode>"
E_OVERFLOW, E_VMSTEPS = -7, -8
KNOBS = TG.KNOBS + ("ZPQ_VM_PIPE",)
_WANT = {}


def oracle_streams(hdr, offs, blocks, key):
    """What the sequential coder writes for each block (a fresh model per block), computed once per key."""
    if key not in _WANT:
        _WANT[key] = [O.Codec(hdr, offs).encode(b) for b in blocks]
    return _WANT[key]


class Run(TG.Run):
    """TG.Run (every call checks all it returns and the kernel that ran) for a model that is asked onto the new kernels:
    the kernel a call must run also follows ZPQ_FLAG_VMPIPE and ZPQ_VM_PIPE."""

    def __init__(self, zpq, ctx, mp, hdr, offs=None, inside=True):
        mp.delenv("ZPQ_VM_PIPE", raising=False)
        super().__init__(zpq, ctx, mp, hdr, offs)
        self.inside, self.V = inside, zpq.FLAG_VMPIPE
        assert VM.applies(zpq, self.model) == ((1, 1) if inside else (0, 0))
        self.F = zpq.FLAG_PP | zpq.FLAG_VMPIPE            # for calls made past the helpers: the flag alone, as a user passes it

    def kernel(self, decode, flags, env):
        v = env.get("ZPQ_VM_PIPE", "")
        asked = v[0] == "1" if v[:1] in ("0", "1") else bool(flags & self.V)
        if asked and self.inside and not flags & self.zpq.FLAG_GENERIC:
            return DEC if decode else ENC
        return super().kernel(decode, flags, env)

    def both(self, blocks, want, **env):
        """Encode against the oracle; decode the oracle's streams and compare all outputs with k_rows' for the same call."""
        self.encode(blocks, want, True, flags=self.V, **env)
        res = self.decode(want, blocks, True, flags=self.V, **env)
        assert res == self.decode(want, blocks, True)
        assert {ENC, DEC, "k_rows<decode>"} <= {k.split(" ")[0] for k in self.seen}
        return res

    def budget(self, slots):
        self.zpq.lib().zpq_ctx_set_state_budget(self.ctx.h, slots * self.model.state_bytes + 1000 if slots else BUDGET)


# ---------------------------------------------------------------- 1. every program
@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_every_program(zpq, gpu_ctx, monkeypatch, name):
    """The corpus behind CM, ICM, ISSE, MATCH, MIX on 23 ragged blocks: batched and bit-serial stages, 64 and 16 lanes per
    decoder workgroup (23 blocks = two workgroups of 16)."""
    hdr, offs = ZP.embed(PROGRAMS[name], "rows")
    blocks = ZP.batch()
    assert len(blocks) == 23
    run = Run(zpq, gpu_ctx, monkeypatch, hdr, offs)
    want = oracle_streams(hdr, offs, blocks, (name, "rows"))
    res = run.both(blocks, want)
    run.encode(blocks, want, True, flags=run.V, ZPQ_GPIPE_BATCH="0")
    assert run.decode(want, blocks, True, flags=run.V, ZPQ_GDEC_BPW="16") == res
    run.model.close()


# ---------------------------------------------------------------- 2. slot reuse
@pytest.mark.parametrize("name", ["loop_scan_m", "r_delay", "d_walks_h", "f_sticks"])
def test_seven_slots_for_23_blocks(zpq, gpu_ctx, monkeypatch, name):
    """A lane codes three or four blocks in turn: the registers, M, H and R of the block before must not reach the next."""
    hdr, offs = ZP.embed(ZP.NAMED[name], "rows")
    blocks = ZP.batch()
    run = Run(zpq, gpu_ctx, monkeypatch, hdr, offs)
    want = oracle_streams(hdr, offs, blocks, (name, "rows"))
    run.budget(7)
    try:
        run.encode(blocks, want, True, flags=run.V, slots=7)
        run.decode(want, blocks, True, flags=run.V, slots=7)
        run.encode(blocks, want, True, flags=run.V, slots=7, ZPQ_GPIPE_BATCH="0")
        run.decode(want, blocks, True, flags=run.V, slots=7, ZPQ_GDEC_BPW="16")
        assert {ENC, DEC} == {k.split(" ")[0] for k in run.seen}
    finally:
        run.budget(0)
    run.model.close()


# ---------------------------------------------------------------- 3. more blocks than lanes; divergence
def test_67_blocks_and_neighbours_that_run_sixteen_times_the_steps(zpq, gpu_ctx, monkeypatch):
    hdr, offs = ZP.embed(ZP.NAMED["loop_count"], "rows")
    run = Run(zpq, gpu_ctx, monkeypatch, hdr, offs)
    r = random.Random(67)
    blocks = [ZP._data(r, i % 4, r.choice([0, 1, 2, 17, 64, 65, 150, 300])) for i in range(67)]
    run.both(blocks, oracle_streams(hdr, offs, blocks, "wide67"))       # two workgroups, the second with three lanes
    blocks = ZP.divergence_batch()
    run.both(blocks, oracle_streams(hdr, offs, blocks, "divergence"))   # 1 against 16 loop iterations at every byte
    run.model.close()


# ---------------------------------------------------------------- 4. all nine types, tied to k_gpipe
def test_all_nine_types_equal_the_oracle_and_the_chain_pipeline(zpq, gpu_ctx, monkeypatch):
    """C4b's components behind its hash chain with a=a in front: the same contexts, so the streams equal the oracle's for
    the new header AND what k_gpipe writes for the true C4b."""
    assert not GM.is_hashchain(VM.C4B_VM) and GM.is_hashchain(VM.C4B)
    run = Run(zpq, gpu_ctx, monkeypatch, VM.C4B_VM)
    r = random.Random(70)
    blocks = [TG._block(r, i % 5, 0 if i % 23 == 0 else r.randrange(2601)) for i in range(70)]
    want = O.encode_blocks(VM.C4B_VM, blocks, nthreads=8)
    run.both(blocks, want)
    run.encode(blocks, want, True, flags=run.V, ZPQ_GPIPE_BATCH="0")
    true = zpq.Model(header=VM.C4B)
    coded, status, _ = gpu_ctx.encode_blocks(true, blocks, flags=zpq.FLAG_PP)
    assert gpu_ctx.last_kernel_name == "k_gpipe<encode>" and not status.any()
    assert coded == want
    true.close()
    run.model.close()


# ---------------------------------------------------------------- 5. model edges
@pytest.mark.parametrize("name", ["hh_small", "hm0", "perturbed_rows", "chain14"])
def test_model_edges(zpq, gpu_ctx, monkeypatch, name):
    """H shorter than n (the contexts beyond it are 0), no M, one opcode exchanged, and the most components taken."""
    hdr = VM.chain(14) if name == "chain14" else GM.NAMED[name][0]
    run = Run(zpq, gpu_ctx, monkeypatch, hdr)             # (an ISSE chain is a chain model too: TG.Run's ZPQ_FLAG_LANES keeps k_chain away)
    blocks = ZP.batch()
    run.both(blocks, oracle_streams(hdr, None, blocks, name))
    run.model.close()


def test_the_flag_is_a_request(zpq, gpu_ctx, monkeypatch):
    """Fifteen components: outside the envelope, the call runs as without the flag."""
    hdr = VM.chain(15)
    run = Run(zpq, gpu_ctx, monkeypatch, hdr, inside=False)
    blocks = ZP.batch()
    want = oracle_streams(hdr, None, blocks, "chain15")
    run.encode(blocks, want, True, flags=run.V)
    run.decode(want, blocks, True, flags=run.V)
    assert run.seen == {"k_rows<encode> interpreter", "k_rows<decode> interpreter"}
    run.model.close()


# ---------------------------------------------------------------- 6. the step cap
def test_step_cap_hits_three_blocks_and_their_neighbours_code_on(zpq, gpu_ctx, monkeypatch):
    hdr, offs = ZP.embed(ZP.STEP_CAP, "rows")
    run = Run(zpq, gpu_ctx, monkeypatch, hdr, offs)
    blocks = ZP.step_cap_batch()
    want = [O.Codec(hdr, offs).encode(b) for b in blocks]
    status_want = [E_VMSTEPS if i in (1, 6, 7) else 0 for i in range(12)]
    coded, status, _ = gpu_ctx.encode_blocks(run.model, blocks, flags=run.F)
    assert gpu_ctx.last_kernel_name == ENC
    assert [int(s) for s in status] == status_want
    dec, dstatus, consumed, _, first = gpu_ctx.decode_blocks(run.model, want, cap=48, flags=run.F)
    assert gpu_ctx.last_kernel_name == DEC
    assert [int(s) for s in dstatus] == status_want
    for i in range(12):
        if status_want[i] == 0:
            assert coded[i] == want[i], i
            assert dec[i] == blocks[i] and int(consumed[i]) == len(want[i]) and int(first[i]) == 0, i
    run.model.close()


# ---------------------------------------------------------------- 7. off-nominal, once
def test_damaged_streams_and_a_short_slab(zpq, gpu_ctx, monkeypatch):
    """A stream cut by three bytes and one with a flipped bit in its second byte decode to what the oracle's decode gives
    when stopped where the kernels stop; a slab one byte short overflows, for that block only."""
    hdr, offs = ZP.embed(ZP.NAMED["loop_count"], "rows")
    run = Run(zpq, gpu_ctx, monkeypatch, hdr, offs)
    blocks = ZP.batch()
    streams = list(oracle_streams(hdr, offs, blocks, ("loop_count", "rows")))
    streams[6] = streams[6][:-3]
    flipped = bytearray(streams[22])
    flipped[1] ^= 0x10
    streams[22] = bytes(flipped)
    caps = [1600] * 23

    def check(caps):
        got = raw_decode(zpq, gpu_ctx, run.model, streams, caps, run.F)
        assert gpu_ctx.last_kernel_name == DEC
        out, out_off, out_len, consumed, code, first, status = got
        for i, (s, cap) in enumerate(zip(streams, caps)):
            e = OC.shape(O.Codec(hdr, offs).decode_prefix(s, cap + 1), cap, True)
            o = int(out_off[i])
            have = (int(status[i]), int(out_len[i]), out[o:o + min(int(out_len[i]), cap)].tobytes(), int(consumed[i]), int(code[i]), int(first[i]))
            assert have == tuple(e), (i, cap, have[:2], have[3:], e._replace(data=len(e.data)))
        return status, out_len

    check(caps)
    caps = [len(b) for b in blocks]
    caps[6], caps[22] = 400, 1600                            # (the damaged ones: any slab)
    caps[7] -= 1
    status, out_len = check(caps)
    assert int(status[7]) == E_OVERFLOW and int(out_len[7]) == caps[7] + 1
    assert [int(s) for i, s in enumerate(status) if i not in (6, 7, 22)] == [0] * 20
    run.model.close()


# ---------------------------------------------------------------- 8. device pointers; the knob
def test_device_pointer_form_equals_the_host_form(zpq, gpu_ctx, monkeypatch):
    hdr, offs = ZP.embed(ZP.NAMED["loop_nested"], "rows")
    run = Run(zpq, gpu_ctx, monkeypatch, hdr, offs)
    blocks = ZP.batch()
    want = oracle_streams(hdr, offs, blocks, ("loop_nested", "rows"))
    host = run.both(blocks, want)
    caps = [len(b) * 17 + 4096 for b in blocks]
    out, out_off, out_len, _, _, _, status = dev_call(zpq, gpu_ctx, run.model, False, blocks, caps, run.F)
    assert gpu_ctx.last_kernel_name == ENC and not status.any()
    assert [out[int(out_off[i]):int(out_off[i]) + int(out_len[i])].tobytes() for i in range(23)] == want
    caps = [max(len(b) for b in blocks) + 64] * 23
    out, out_off, out_len, consumed, code, first, status = dev_call(zpq, gpu_ctx, run.model, True, want, caps, run.F)
    assert gpu_ctx.last_kernel_name == DEC and not status.any()
    assert [out[int(out_off[i]):int(out_off[i]) + int(out_len[i])].tobytes() for i in range(23)] == blocks
    assert list(zip([int(x) for x in out_len], [0] * 23, [int(x) for x in consumed], [int(x) for x in code], [int(x) for x in first])) == host
    run.model.close()


def test_the_environment_decides_first(zpq, gpu_ctx, monkeypatch):
    """ZPQ_VM_PIPE=1 without the flag selects the new kernels, ZPQ_VM_PIPE=0 with the flag k_rows; the resident capacity
    answers for the pair that would run, and the hash chain keeps k_gpipe whatever is asked for."""
    hdr, offs = ZP.embed(ZP.NAMED["loop_nested"], "rows")
    run = Run(zpq, gpu_ctx, monkeypatch, hdr, offs)
    blocks = ZP.batch()
    want = oracle_streams(hdr, offs, blocks, ("loop_nested", "rows"))
    run.encode(blocks, want, True, ZPQ_VM_PIPE="1")
    run.decode(want, blocks, True, ZPQ_VM_PIPE="1")
    assert run.seen == {ENC + " interpreter", DEC + " interpreter"}
    run.encode(blocks, want, True, flags=run.V, ZPQ_VM_PIPE="0")
    run.decode(want, blocks, True, flags=run.V, ZPQ_VM_PIPE="0")
    run.encode(blocks, want, True)
    assert run.seen == {ENC + " interpreter", DEC + " interpreter", "k_rows<encode> interpreter", "k_rows<decode> interpreter"}
    run.seen.clear()                                        # a value that starts with neither digit decides nothing
    run.encode(blocks, want, True, flags=run.V, ZPQ_VM_PIPE="yes")
    run.decode(want, blocks, True, ZPQ_VM_PIPE="")
    assert run.seen == {ENC + " interpreter", "k_rows<decode> interpreter"}
    assert gpu_ctx.resident_capacity(run.model, run.F) % 64 == 0
    with knobs(monkeypatch, ZPQ_VM_PIPE="0"):
        assert gpu_ctx.resident_capacity(run.model, run.F) == gpu_ctx.resident_capacity(run.model, zpq.FLAG_PP)
    true = zpq.Model(header=VM.C4B)                         # the hash chain keeps k_gpipe whatever is asked for
    with knobs(monkeypatch, ZPQ_VM_PIPE="1"):
        coded, status, _ = gpu_ctx.encode_blocks(true, blocks[:12], flags=run.F)
        assert gpu_ctx.last_kernel_name == "k_gpipe<encode>" and not status.any()
    true.close()
    run.model.close()
