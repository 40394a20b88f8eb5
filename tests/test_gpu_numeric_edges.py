"""Every kernel family over the edge corpus of tests/numeric_edges.py: inputs that drive ISSE and MIX weights to both
clamp512k bounds, clamp2k to both ends, MIX2 weights to 0 and 65535, CM / SSE counts to their limits, MATCH to 255 and
back, and the coder through ranges below 2^16, multi-byte shifts and the low = 1 repair.  A case has two forms: four segments
with the model carried over (the block-set tests) and one block on a fresh model (every other test); tests/
test_numeric_edges_cpu.py shows on the host, for each form, what it reaches and which mutants of the reference it tells.  Expected bytes,
lengths, consumed, final_code and first_byte come from oracle_lib.Codec; the kernel that ran is asserted by name through
the neighbouring files' helpers."""
import pytest

import general_models as GM
import numeric_edges as NE
import oracle_lib as O
import test_gpu_blockset as TB
import test_gpu_chain_models as TC
import test_gpu_general_models as TG
import test_gpu_set_pipe as TP
import test_gpu_set_vmwaves as TS
import test_gpu_vpipe as TV

pytestmark = pytest.mark.gpu

CHAIN = [n for n, c in NE.EDGE_CASES.items() if c.cls == "chain"]
GENERAL = [n for n, c in NE.EDGE_CASES.items() if c.cls == "general" and not n.endswith("_vm")]
GENERAL_VM = [n for n, c in NE.EDGE_CASES.items() if n.endswith("_vm")]
SET_CHAIN = ["l1", "l2", "l3_mixed", "l4_rate255", "l5_small", "chain9", "chain15_mix2"]
_WANT = {}


def blocks_of(case):
    """The case as a batch of independent blocks: its block form (case.block: the warm-up as ONE block and bytes steered for that
    block's own coder state; tests/test_numeric_edges_cpu.py pins what it reaches and tells in exactly this form) and each of
    the four segments on its own, three times over: 15 blocks, so the pipelines engage."""
    assert len(case.block) <= 4096
    return ([case.block] + list(case.segments)) * 3


def want_of(key, hdr, blocks, pp=True):
    if (key, pp) not in _WANT:
        _WANT[key, pp] = O.encode_blocks(hdr, blocks, pp=pp, nthreads=8)
    return _WANT[key, pp]


def header_and_case(zpq, name):
    if isinstance(name, int):                             # a shipped level with tables beyond pyref: l2's bytes
        return zpq.level_header(name), NE.EDGE_CASES["l2"]
    return NE.EDGE_CASES[name].header, NE.EDGE_CASES[name]


def members_of(case, bystanders=3):
    """The case as member 0, eleven more members that are the case's segments rotated by 1 .. 11 bytes (four segments each:
    twelve live members in every round) and a few ragged bystanders of the block-set tests."""
    rot = [[seg[k:] + seg[:k] for seg in case.segments] for k in range(1, 12)]
    return [list(case.segments)] + rot + TB.make_members(5, nmembers=bystanders)


def history(key, hdr, members, offs=None):
    return TS.oracle_history(("numeric_edges", key), hdr, members, offs)


# ---------------------------------------------------------------- chain class
@pytest.mark.parametrize("name", CHAIN + list(NE.SHIPPED_BIG), ids=str)
def test_chain_class(zpq, gpu_ctx, monkeypatch, name):
    hdr, case = header_and_case(zpq, name)
    run = TC.Run(zpq, gpu_ctx, monkeypatch, hdr)
    assert run.rt is not None
    blocks = blocks_of(case)
    want = want_of(name, hdr, blocks)
    coded = run.encoders(blocks, want, True)
    run.decoders(coded, blocks, True)
    expect = {"k_chain<encode>", "k_chain<decode>"}
    spec, mix2 = run.rt["nch_spec"], run.rt["has_mix2"]
    if spec:
        expect.add("k_pipe<encode>")
    if spec == 2:
        expect.add("k_pipe2<encode>")
    if spec in (2, 3, 5) and not mix2:
        expect.add("k_dpipe<decode>")
    if not isinstance(name, int):                         # (the shipped levels 3 - 5: gigabytes of tables per block)
        store = run.tables(blocks, want, True)
        if max(TC.CM.table_bits(hdr)) >= 14:
            assert store > 0, store
        run.cross_check(blocks, want, True)
        L = zpq.FLAG_LANES                                 # ... and each of the general kernels that takes the model, by name
        run.encode(blocks, want, True, flags=L, names={"k_rows<encode>", "k_lanes<encode>"}, ZPQ_ENC_GPIPE="0")
        run.encode(blocks, want, True, flags=L, names={"k_lanes<encode>"}, ZPQ_ENC_GPIPE="0", ZPQ_LANES_ROWS="0")
        res = [run.decode(coded, blocks, True, flags=L, names=TC.DEC_OTHER),
               run.decode(coded, blocks, True, flags=L, names={"k_rows<decode>", "k_lanes<decode>"}, ZPQ_DEC_GPIPE="0"),
               run.decode(coded, blocks, True, flags=L, names={"k_lanes<decode>"}, ZPQ_DEC_GPIPE="0", ZPQ_LANES_ROWS="0"),
               run.decode(coded, blocks, True, flags=zpq.FLAG_GENERIC, names={"k_generic<decode>"})]
        assert all(r == res[0] for r in res)
        expect |= {"k_generic<encode>", "k_generic<decode>", "k_lanes<encode>", "k_lanes<decode>"}
        general = GM.route(zpq, run.model)                 # (gpipe, gdec, lanes, k_rows | k_lanes) for the same model
        if general[3] == GM.ROWS:
            expect |= {"k_rows<encode>", "k_rows<decode>"}
        if general[0]:
            expect.add("k_gpipe<encode>")
        if general[1]:
            expect.add("k_gdec<decode>")
    raw = want_of(name, hdr, blocks, pp=False)
    run.decode(run.encode(blocks, raw, False), blocks, False)
    print("\nkernels %s (spec %d, g %d, mix2 %d): %s" % (name, spec, run.rt["g"], mix2, sorted(run.seen)))
    assert expect <= run.seen, (expect - run.seen)


# ---------------------------------------------------------------- general class
@pytest.mark.parametrize("name", GENERAL)
def test_general_class(zpq, gpu_ctx, monkeypatch, name):
    case = NE.EDGE_CASES[name]
    run = TG.Run(zpq, gpu_ctx, monkeypatch, case.header)
    assert run.rt == GM.PIPE
    blocks = blocks_of(case)
    for pp in (True, False):
        want = want_of(name, case.header, blocks, pp=pp)
        run.decoders(run.encoders(blocks, want, pp), blocks, pp)
    print("\nkernels %s: %s" % (name, sorted(run.seen)))
    assert run.seen == TG.expected_kernels(run.rt, True)


@pytest.mark.parametrize("name", GENERAL_VM)
def test_general_class_behind_another_program(zpq, gpu_ctx, monkeypatch, name):
    """The same components behind `a=a` and the hash chain: k_vpipe / k_vdec on request, k_rows / k_lanes / k_generic with
    the interpreter otherwise; the streams are those of the hash-chain header."""
    case = NE.EDGE_CASES[name]
    run = TV.Run(zpq, gpu_ctx, monkeypatch, case.header)
    blocks = blocks_of(case)
    want = want_of(name, case.header, blocks)
    assert want == want_of(name[:-3], NE.EDGE_CASES[name[:-3]].header, blocks)
    res = run.both(blocks, want)
    run.encode(blocks, want, True, flags=run.V, ZPQ_GPIPE_BATCH="0")
    assert run.decode(want, blocks, True, flags=run.V, ZPQ_GDEC_BPW="16") == res
    run.decoders(run.encoders(blocks, want, True), blocks, True)
    raw = want_of(name, case.header, blocks, pp=False)
    run.decode(run.encode(blocks, raw, False, flags=run.V), blocks, False, flags=run.V)
    print("\nkernels %s: %s" % (name, sorted(run.seen)))
    assert {TV.ENC + " interpreter", TV.DEC + " interpreter", TV.DEC + " bpw16 interpreter"} | \
        TG.expected_kernels(run.rt, False) == run.seen                    # (k_vpipe ran batched and bit-serial: one name)


# ---------------------------------------------------------------- block sets
@pytest.mark.parametrize("name", SET_CHAIN)
def test_chain_sets(zpq, gpu_ctx, monkeypatch, name):
    """k_chain<KEEP> both ways, then k_pipe<KEEP> (pipe=True, twelve or more live members in every round) with k_chain decoding:
    the weight at the bound is saved at a segment's end and restored at the next one's start."""
    for k in TB.KNOBS + TP.KNOBS:
        monkeypatch.delenv(k, raising=False)
    case = NE.EDGE_CASES[name]
    members = members_of(case)
    want = history(name, case.header, members)
    TB.check_parity(zpq, gpu_ctx, case.header, members, want)
    model = zpq.Model(header=case.header)
    piped = bool(TC.CM.route(zpq, model)["nch_spec"])      # (the runtime-loop chains have no pipelined encoder)
    model.close()
    assert piped == (name not in ("chain9", "chain15_mix2"))
    if piped:
        TP.check_every_round(zpq, gpu_ctx, case.header, members_of(case, bystanders=0))
    print("\nkernels %s: k_chain<encode> k_chain<decode> KEEP%s" % (name, ", k_pipe<encode> KEEP" if piped else ""))


FORMS = {"lanes_rows": ({"lanes": True}, 1, TS.ROWS, {}), "lanes_lanes": ({"lanes": True}, 1, TS.LANES, {"ZPQ_LANES_ROWS": "0"}),
         "waves": ({"waves": True}, 17, TS.WSET, {}), "waves_bit_serial": ({"waves": True}, 17, TS.WSET, {"ZPQ_GPIPE_BATCH": "0"}),
         "generic": ({}, 0, TS.GENERIC, {})}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", GENERAL)
def test_general_sets(zpq, gpu_ctx, monkeypatch, name, form):
    for k in TS.KNOBS:
        monkeypatch.delenv(k, raising=False)
    kw, flags, names, env = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = NE.EDGE_CASES[name]
    members = members_of(case)
    if form == "generic":                                  # (one lane per member: two rounds carry the weights over one boundary)
        members = [segs[:2] for segs in members]
    TS.run_members(zpq, gpu_ctx, case.header, members, history((name, form == "generic"), case.header, members), names=names,
                   flags=flags, kw=kw)
    print("\nkernels %s %s: %s" % (name, form, names))


@pytest.mark.parametrize("batch", ["batched", "bit_serial"])
@pytest.mark.parametrize("name", GENERAL_VM)
def test_general_sets_on_the_interpreter_waves(zpq, gpu_ctx, monkeypatch, name, batch):
    for k in TS.KNOBS:
        monkeypatch.delenv(k, raising=False)
    if batch == "bit_serial":
        monkeypatch.setenv("ZPQ_GPIPE_BATCH", "0")
    case = NE.EDGE_CASES[name]
    members = members_of(case)
    TS.run_members(zpq, gpu_ctx, case.header, members, history(name, case.header, members))
    print("\nkernels %s %s: %s" % (name, batch, TS.VSET))


@pytest.mark.parametrize("name", GENERAL + GENERAL_VM)
def test_the_families_alternate_on_one_set(zpq, gpu_ctx, monkeypatch, name):
    """Rounds 0 and 2 on the wave kernels, round 1 on k_rows, round 3 on k_lanes (ZPQ_ENC_GPIPE=0 / ZPQ_DEC_GPIPE=0 at the call):
    a weight at the bound is written by one family and read by the other."""
    for k in TS.KNOBS:
        monkeypatch.delenv(k, raising=False)
    vm = name.endswith("_vm")
    wave = TS.VSET if vm else TS.WSET
    family = [wave, TS.ROWS, wave, TS.LANES]

    def before_call(r, decode):
        for k in ("ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE", "ZPQ_LANES_ROWS"):
            monkeypatch.delenv(k, raising=False)
        if family[r] is not wave:
            monkeypatch.setenv("ZPQ_DEC_GPIPE" if decode else "ZPQ_ENC_GPIPE", "0")
        if family[r] is TS.LANES:
            monkeypatch.setenv("ZPQ_LANES_ROWS", "0")
        return family[r][decode]

    case = NE.EDGE_CASES[name]
    members = members_of(case)
    TS.run_members(zpq, gpu_ctx, case.header, members, history(name, case.header, members), flags=65 if vm else 17,
                   kw={"vmwaves": True} if vm else {"waves": True}, before_call=before_call)
    print("\nkernels %s: %s" % (name, [f[0] for f in family]))
