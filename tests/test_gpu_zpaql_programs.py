"""GPU parity of every kernel's ZPAQL interpreter on programs that loop, carry state and end in every way a run can end
(tests/zpaql_programs.py; the corpus itself is pinned by test_zpaql_programs_cpu.py): k_chain's runtime instantiation at
8 and 16 lanes per block, k_rows, k_lanes with H in LDS and in the slot, k_generic -- each against the CPU oracle, with
fewer slots than blocks, with neighbours in a wave that run sixteen times as many steps, across segments (block sets and
zpq.Block), and with the step cap hitting some blocks of a wave while the others code on."""
import pytest

import chain_models as CMOD
import general_models as GM
import oracle_lib as O
import test_gpu_chain_models as TC
import test_gpu_general_models as TG
import zpaql_programs as ZP
from test_gpu_blockset import check_parity, make_members, oracle_history

pytestmark = pytest.mark.gpu

PROGRAMS = dict(ZP.NAMED)
PROGRAMS.update(("generated%02d" % i, p) for i, p in enumerate(ZP.generated()))
E_VMSTEPS = -8
_WANT = {}


def oracle_streams(hdr, offs, blocks, key):
    """What the sequential coder writes for each block (a fresh model per block), computed once per key."""
    if key not in _WANT:
        _WANT[key] = [O.Codec(hdr, offs).encode(b) for b in blocks]
    return _WANT[key]


def run_general(zpq, ctx, mp, prog, shape, blocks, key, generic=True):
    """Every kernel that takes a `rows` / `lanes` embedding: the default one, one block per wave where four ride a wave,
    one lane per block; then each of them with seven slots for the 23 blocks (a slot's M, H and R of the block before must be
    cleared)."""
    hdr, offs = ZP.embed(prog, shape)
    run = TG.Run(zpq, ctx, mp, hdr, offs)
    want = oracle_streams(hdr, offs, blocks, key)
    run.encode(blocks, want, True)
    res = [run.decode(want, blocks, True)]
    expect = {"k_%s<%s> interpreter" % (shape, d) for d in ("encode", "decode")}
    if shape == "rows":
        run.encode(blocks, want, True, ZPQ_LANES_ROWS="0")
        res.append(run.decode(want, blocks, True, ZPQ_LANES_ROWS="0"))
        expect |= {"k_lanes<encode> interpreter", "k_lanes<decode> interpreter"}
    if generic:
        run.encode(blocks, want, True, flags=zpq.FLAG_GENERIC)
        res.append(run.decode(want, blocks, True, flags=zpq.FLAG_GENERIC))
        expect |= {"k_generic<encode> interpreter", "k_generic<decode> interpreter"}
    assert all(r == res[0] for r in res)
    run.slot_reuse(blocks, want, True, 7)
    if generic:                                           # k_generic too codes several blocks per slot in turn
        L = zpq.lib()
        L.zpq_ctx_set_state_budget(ctx.h, 7 * run.model.state_bytes + 1000)
        try:
            run.encode(blocks, want, True, flags=zpq.FLAG_GENERIC)
            assert 0 < ctx.last_slots < len(blocks), ctx.last_slots
            assert run.decode(want, blocks, True, flags=zpq.FLAG_GENERIC) == res[0]
            assert 0 < ctx.last_slots < len(blocks), ctx.last_slots
        finally:
            L.zpq_ctx_set_state_budget(ctx.h, TC.BUDGET)
    assert run.seen == expect, (run.seen, expect)
    run.model.close()


def run_chain(zpq, ctx, mp, prog, shape, blocks, key):
    hdr, offs = ZP.embed(prog, shape)
    run = TC.Run(zpq, ctx, mp, hdr, offs)
    assert (run.rt["nch_spec"], run.rt["vm_kind"], run.rt["g"]) == (0, CMOD.VM_GENERIC, 8 if shape == "chain" else 16)
    want = oracle_streams(hdr, offs, blocks, key)
    run.encode(blocks, want, True)
    run.decode(want, blocks, True)
    run.slot_reuse(blocks, want, True, slots=7)
    assert run.seen == {"k_chain<encode>", "k_chain<decode>"}
    run.model.close()


@pytest.mark.parametrize("shape", ["chain", "chain16", "rows", "lanes"])
@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_program_on_every_route(zpq, gpu_ctx, monkeypatch, name, shape):
    blocks = ZP.batch()
    assert len(blocks) == 23
    if shape in ("chain", "chain16"):
        run_chain(zpq, gpu_ctx, monkeypatch, PROGRAMS[name], shape, blocks, (name, shape))
    else:                                                 # (one lane per block: the named programs, and every program on `rows`)
        run_general(zpq, gpu_ctx, monkeypatch, PROGRAMS[name], shape, blocks, (name, shape),
                    generic=shape == "rows" or name in ZP.NAMED)


@pytest.mark.parametrize("name", ["loop_count", "r_delay"])
def test_program_behind_65_components(zpq, gpu_ctx, monkeypatch, name):
    """More components than a wave has lanes: k_generic is the default and the only kernel."""
    hdr, offs = ZP.embed(ZP.NAMED[name], "generic")
    run = TG.Run(zpq, gpu_ctx, monkeypatch, hdr, offs)
    blocks = [b for b in ZP.batch() if len(b) <= 300]
    want = oracle_streams(hdr, offs, blocks, (name, "generic"))
    run.encode(blocks, want, True)
    run.decode(want, blocks, True)
    assert run.seen == {"k_generic<encode> interpreter", "k_generic<decode> interpreter"}
    run.model.close()


@pytest.mark.parametrize("name", sorted(ZP.NAMED))
def test_contexts_byte_by_byte(zpq, gpu_ctx, name):
    """The contexts after every byte against the oracle's VM: separates the interpreter from the coder around it."""
    hdr, offs = ZP.embed(ZP.NAMED[name], "rows")
    model = zpq.Model(header=hdr, offsets=offs)
    blocks = ZP.batch()
    data = blocks[7][:300] + blocks[6] + blocks[22][:200]
    got = gpu_ctx.debug_contexts(model, data)
    L = O.lib()
    z = L.zo_vm_new(hdr, len(hdr), *offs)
    hlen = L.zo_vm_hlen(z)
    for i, b in enumerate(data):
        L.zo_vm_run(z, b)
        assert got[i].tolist() == [L.zo_vm_h(z, k) if k < hlen else 0 for k in range(model.ncomp)], (name, i)
    L.zo_vm_free(z)
    model.close()


@pytest.mark.parametrize("shape", ["rows", "chain", "chain16"])
def test_neighbours_that_run_sixteen_times_the_steps(zpq, gpu_ctx, monkeypatch, shape):
    """loop_count on constant blocks of 0x00, 0x0F, 0xF0, 0xFF and random ones: at every byte the blocks that share a
    row group, a lane group or a wave run 1 against 16 iterations of the loop."""
    blocks = ZP.divergence_batch()
    if shape == "rows":
        run_general(zpq, gpu_ctx, monkeypatch, ZP.NAMED["loop_count"], shape, blocks, ("divergence", shape), generic=False)
    else:
        run_chain(zpq, gpu_ctx, monkeypatch, ZP.NAMED["loop_count"], shape, blocks, ("divergence", shape))


# ---------------------------------------------------------------- state from segment to segment
@pytest.fixture()
def clean_env(monkeypatch):
    for k in TC.KNOBS + TG.KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.mark.parametrize("shape", ["chain", "chain16"])
@pytest.mark.parametrize("name", ZP.SEGMENT_PROGRAMS)
def test_block_set_hands_the_vm_from_launch_to_launch(zpq, gpu_ctx, clean_env, name, shape):
    """k_chain<..., KEEP>: a b c d f, M, H and R of 21 members with 1-4 segments each (zero-length ones among them) go
    through the set's slots; expected values from one oracle codec per member."""
    hdr, _ = ZP.embed(ZP.NAMED[name], shape)
    members = make_members(500 + len(name) + len(shape))
    assert any(len(s) == 0 for segs in members for s in segs)
    check_parity(zpq, gpu_ctx, hdr, members, oracle_history(hdr, members))


@pytest.mark.parametrize("name", ZP.SEGMENT_PROGRAMS)
def test_block_set_of_a_general_model_keeps_the_vm(zpq, gpu_ctx, clean_env, name):
    """A block set of a model that is no chain: k_generic, its registers reloaded from and stored to the slot per segment."""
    hdr, _ = ZP.embed(ZP.NAMED[name], "rows")
    members = [[s[:300] for s in segs] for segs in make_members(600 + len(name), nmembers=9)]
    check_parity(zpq, gpu_ctx, hdr, members, oracle_history(hdr, members), "k_generic<encode>", "k_generic<decode>")


@pytest.mark.parametrize("name", ZP.SEGMENT_PROGRAMS)
def test_block_replays_its_first_segment_into_the_lane0_kernel(zpq, gpu_ctx, clean_env, name):
    """zpq.Block on the `rows` embedding: the first segment runs on k_rows, the second replays it into k_generic and goes
    on from the VM state the replay left."""
    hdr, offs = ZP.embed(ZP.NAMED[name], "rows")
    model = zpq.Model(header=hdr, offsets=offs)
    batch = ZP.batch()
    segs = [batch[6], b"", batch[4], batch[7][:400], batch[1]]
    codec = O.Codec(hdr, offs)
    want = [codec.encode(s, pp=True) for s in segs]
    blk = zpq.Block(gpu_ctx, model)
    for i, s in enumerate(segs):
        assert blk.encode_segment(s) == want[i], (name, i)
        assert gpu_ctx.last_kernel_name == ("k_rows<encode>" if i == 0 else "k_generic<encode>"), (i, gpu_ctx.last_kernel_name)
    blk.close()
    dblk = zpq.Block(gpu_ctx, model)
    for i, s in enumerate(segs):
        out, cons, _, first = dblk.decode_segment(want[i], cap=2048)
        assert gpu_ctx.last_kernel_name == ("k_rows<decode>" if i == 0 else "k_generic<decode>"), (i, gpu_ctx.last_kernel_name)
        assert out == s and first == 0 and cons == len(want[i]), (name, i)
    dblk.close()
    model.close()


# ---------------------------------------------------------------- the step cap on some blocks of a wave
@pytest.mark.parametrize("route", ["rows", "lanes", "chain", "generic"])
def test_step_cap_hits_three_blocks_and_their_neighbours_code_on(zpq, gpu_ctx, clean_env, route):
    """a== 255; jf; jmp self before the hash chain: a run never ends on byte 0xFF.  Blocks 1, 6 and 7 of 12 hold one or
    two such bytes: exactly they report ZPQ_E_VMSTEPS, from the encoder and from the decoder; the nine others -- in the
    same row group, lane group or wave -- equal the oracle byte for byte.  (The bytes of a capped block are not asserted:
    the header promises a status for it, not a stream.)"""
    shape = "rows" if route == "generic" else route
    hdr, offs = ZP.embed(ZP.STEP_CAP, shape)
    model = zpq.Model(header=hdr, offsets=offs)
    flags = zpq.FLAG_PP | {"rows": zpq.FLAG_LANES, "lanes": zpq.FLAG_LANES, "chain": 0, "generic": zpq.FLAG_GENERIC}[route]
    blocks = ZP.step_cap_batch()
    want = [O.Codec(hdr, offs).encode(b) for b in blocks]
    status_want = [E_VMSTEPS if i in (1, 6, 7) else 0 for i in range(12)]
    coded, status, _ = gpu_ctx.encode_blocks(model, blocks, flags=flags)
    assert gpu_ctx.last_kernel_name == "k_%s<encode>" % route
    assert [int(s) for s in status] == status_want
    dec, dstatus, consumed, _, first = gpu_ctx.decode_blocks(model, want, cap=48, flags=flags)
    assert gpu_ctx.last_kernel_name == "k_%s<decode>" % route
    assert [int(s) for s in dstatus] == status_want
    for i in range(12):
        if status_want[i] == 0:
            assert coded[i] == want[i], (route, i)
            assert dec[i] == blocks[i] and int(consumed[i]) == len(want[i]) and int(first[i]) == 0, (route, i)
    model.close()
