"""The edge corpus of tests/numeric_edges.py on the host, from the reference alone: the case list; that every required event is
reached at least FLOOR times per class; that for every required event a pinned case tells the true reference from one whose
edge is moved by one (different coded bytes in a segment at or after the event's first occurrence); that the set cases tell a
component state lost at a segment boundary; that oracle_lib.Codec and pyref agree byte for byte on every case; and the
golden census table (tests/golden/numeric_edges_census.json).

The table is recomputed here only in part, to keep the file near a minute of pure Python: of the old corpora the group
NE.CHEAP_OLD (levels 1 and 2 on the ragged batch), of the edge cases NE.CHEAP_EDGE (l2, g_cm, g_w3).  The floors are checked
on the whole table as committed; NE.write_census() regenerates it."""
import functools
import json

import pytest

import numeric_edges as NE
import oracle_lib as O

P = NE.P
TABLE = json.load(open(NE.CENSUS_JSON))
CASES = sorted(NE.EDGE_CASES)


@functools.lru_cache(maxsize=None)
def true_coded(name):
    c = NE.EDGE_CASES[name]
    return tuple(NE.run(c.header, c.segments, c.offsets)[0])


def test_case_list():
    assert CASES == sorted(
        ["l1", "l2", "l1_sizes", "l3_mixed", "l4_rate255", "l5_small", "chain7", "chain9", "mix2_chain3", "chain15_mix2"]
        + [g + v for g in ("g_all", "g_isse", "g_isse_hi", "g_isse_lo", "g_w1", "g_w2", "g_w3", "g_sse", "g_cm") for v in ("", "_vm")])
    for name, c in NE.EDGE_CASES.items():
        assert c.cls == ("general" if name.startswith("g_") else "chain")
        assert len(c.segments) == 4 and sum(len(s) for s in c.segments) <= 4096, name      # (k_generic runs every case)
        assert all(0 < len(s) <= 1500 for s in c.segments), name                          # (a block set's decode slab)
        if name.endswith("_vm"):
            base = NE.EDGE_CASES[name[:-3]]
            assert c.segments == base.segments and NE.GM.components(c.header) == NE.GM.components(base.header)
            assert NE.GM.program_of(c.header) == [64] + NE.GM.program_of(base.header)
            assert not NE.GM.is_hashchain(c.header) and NE.GM.is_hashchain(base.header)
    assert set(NE.SET_TELLS) <= set(NE.EDGE_CASES)
    assert {cls for cls, _ in NE.TELLS} == set(NE.REQUIRED) and all(set(NE.REQUIRED[c]) == {r for k, r in NE.TELLS if k == c}
                                                                     for c in NE.REQUIRED)


BASE = [n for n in CASES if not n.endswith("_vm")]


@pytest.mark.parametrize("name", BASE)
def test_the_steered_bytes_are_the_generators(name):
    """Every committed blob, both forms: steer() from the case's own warm-up gives exactly these bytes."""
    c = NE.EDGE_CASES[name]
    stored = json.load(open(NE.STEERED_JSON))
    assert sorted(stored) == sorted(BASE + [n + "/block" for n in BASE])
    assert bytes.fromhex(stored[name]) == c.segments[-1] and bytes.fromhex(stored[name + "/block"]) == c.block[-NE.BLOCK_STEER:]
    assert NE.steer(c.header, c.offsets, c.segments[:-1], NE.STEER_BYTES) == c.segments[-1]
    assert NE.steer(c.header, c.offsets, [], NE.BLOCK_STEER, prefix=c.block[:-NE.BLOCK_STEER]) == c.block[-NE.BLOCK_STEER:]


@pytest.mark.parametrize("name", CASES)
def test_oracle_and_pyref_agree(name):
    c = NE.EDGE_CASES[name]
    codec = O.Codec(c.header, c.offsets)
    want = [codec.encode(seg) for seg in c.segments]
    assert list(true_coded(name)) == want
    back = O.Codec(c.header, c.offsets)
    assert [back.decode(w) for w in want] == [(b"\0" + seg, len(w)) for seg, w in zip(c.segments, want)]


def test_the_table_is_the_census():
    """The cheap part of the table, recomputed."""
    old = NE.old_table(only=NE.CHEAP_OLD)
    assert old[NE.CHEAP_OLD] == TABLE["old"][NE.CHEAP_OLD]
    for name, t in NE.edge_table(NE.CHEAP_EDGE).items():
        assert json.loads(json.dumps(t)) == TABLE["edge_cases"][name], name
    for name, t in NE.edge_table(NE.CHEAP_EDGE, block=True).items():
        assert json.loads(json.dumps(t)) == TABLE["edge_blocks"][name], name
    # the rest of the table is tied to the cases by a hash of everything its counts were computed from
    for form in ("edge_cases", "edge_blocks"):
        assert sorted(TABLE[form]) == BASE
        for name, t in TABLE[form].items():
            assert t["hash"] == NE.case_hash(NE.EDGE_CASES[name]), (form, name)
            assert set(NE.EVENTS) <= set(t), (form, name)                     # every event listed, zeros included
    for t in TABLE["old"].values():
        assert set(NE.EVENTS) <= set(t)
    assert sorted(TABLE["edge_cases"]) == [n for n in CASES if not n.endswith("_vm")]
    merged = {cls: {} for cls in NE.REQUIRED}
    for n, t in TABLE["edge_cases"].items():
        NE.merge(merged[NE.EDGE_CASES[n].cls], t)
    assert merged == TABLE["edge"]


def test_reach_floors():
    """Every required event: some case of the class reaches it FLOOR times or more; encoder and decoder see the same coder events."""
    for cls, required in NE.REQUIRED.items():
        for req, events in required.items():
            best = max(sum(t.get(e, 0) for e in events) for n, t in TABLE["edge_cases"].items() if NE.EDGE_CASES[n].cls == cls)
            print("%-8s %-24s %d" % (cls, req, best))
            assert best >= NE.FLOOR, (cls, req, best)
    for n, t in TABLE["edge_cases"].items():
        for e in ("r16", "r8", "s1", "s2", "s3", "s4", "low1"):
            assert t.get("enc." + e, 0) == t.get("dec." + e, 0), (n, e)
    for t in list(TABLE["edge_cases"].values()) + list(TABLE["edge_blocks"].values()) + list(TABLE["old"].values()):
        assert t["c2k.mix2.hi"] == 0 and t["c2k.mix2.lo"] == 0                    # (out of reach: the next test)


@pytest.mark.parametrize("name", ["l4_rate255", "chain15_mix2", "g_all", "g_w1"])
def test_a_mix2_output_never_leaves_clamp2k(name):
    """The chain-class event "clamp2k on a MIX2 output" cannot occur: w * p[j] + (65536 - w) * p[k] with 0 <= w <= 65535 and both
    inputs in -2048 .. 2047 is a weighted mean times 65536.  Checked at the extremes and on what the census saw go in."""
    for w in (0, 1, 32768, 65534, 65535):
        for pj in (-2048, 2047):
            for pk in (-2048, 2047):
                assert -2048 <= (w * pj + (65536 - w) * pk) >> 16 <= 2047
    c = NE.EDGE_CASES[name]
    cs = NE.run(c.header, [c.block], c.offsets, cs=NE.Census(), decode=False)[1]
    lo, hi = cs.range2k["mix2"]
    print(name, "clamp2k argument at the MIX2:", lo, hi)
    assert -2048 <= lo <= hi <= 2047 and (name != "g_all" or (lo, hi) == (-2048, 2031))


def test_block_forms_reach():
    """The form the kernels that code independent blocks run (tests/test_gpu_numeric_edges.py::blocks_of): every chain case's block
    reaches every required chain event FLOOR times or more -- one per specialisation (2: l1, l1_sizes; 3: l2; 5: l3_mixed; 6:
    l4_rate255; 8: l5_small) and the runtime loops at 8 and 16 lanes with and without MIX2 -- and the general class every event."""
    blocks = TABLE["edge_blocks"]
    for n in BASE:
        if NE.EDGE_CASES[n].cls == "chain":
            for req, events in NE.REQUIRED["chain"].items():
                assert sum(blocks[n][e] for e in events) >= NE.FLOOR, (n, req)
            assert blocks[n]["enc.r8"] >= NE.FLOOR and blocks[n]["enc.s3"] >= NE.FLOOR, n
    for req, events in NE.REQUIRED["general"].items():
        best = max(sum(t[e] for e in events) for n, t in blocks.items() if NE.EDGE_CASES[n].cls == "general")
        assert best >= NE.FLOOR, (req, best)
    for n, t in blocks.items():
        for e in ("r16", "r8", "s1", "s2", "s3", "s4", "low1"):
            assert t["enc." + e] == t["dec." + e], (n, e)


def test_sought_events():
    """Reached, or a sentence in the table saying what was tried."""
    for e in NE.SOUGHT:
        reached = max(t.get(e, 0) for t in TABLE["edge_cases"].values())
        print("%-14s %d" % (e, reached))
        assert reached >= 1 or len(TABLE["sought"][e]) > 40, e
    assert {e for e in NE.SOUGHT if max(t.get(e, 0) for t in TABLE["edge_cases"].values()) == 0} == {"match.255_rec", "wrap.cm"}
    assert TABLE["old"]["general: general_models.NAMED (n <= 22), ragged batch"]["wrap.cm"] > 0


def test_mul24_operands():
    """zpq_chain.hip uses __mul24 on err * pin with |err| < 2^15 and |pin| <= 2^11 stated: the largest the census saw."""
    tables = list(TABLE["old"].values()) + list(TABLE["edge_cases"].values())
    assert max(t.get("max.isse.err", 0) for t in tables) == 32767 < 1 << 15
    assert max(t.get("max.isse.pin", 0) for t in tables) == 2048 <= 1 << 11
    assert max(t.get("max.mix.pin", 0) for t in tables) == 2048 and max(t.get("max.mix.err", 0) for t in tables) == 522225 < 1 << 23
    assert max(t.get("max.mix2.err", 0) for t in tables) <= 261120 < 1 << 23 and max(t.get("max.mix2.pdiff", 0) for t in tables) <= 4095
    assert P.DT[0] * 32767 >= 1 << 31 > P.DT[1] * 32767                       # the one wrap site: a CM update at count 0


@pytest.mark.parametrize("cls,req", sorted(NE.TELLS))
def test_a_case_tells_the_edge_moved_by_one(cls, req):
    event, name = NE.TELLS[cls, req]
    c, t = NE.EDGE_CASES[name], TABLE["edge_cases"][name]
    assert c.cls == cls and event in NE.REQUIRED[cls][req] and t[event] >= NE.FLOOR
    true = true_coded(name)
    mutant = NE.mutant_coded(c, event, until=true)
    differ = [s for s in range(len(mutant)) if mutant[s] != true[s]]
    assert differ and differ[0] >= t["first"][event][0], (event, name, differ, t["first"][event])


def test_an_equivalent_mutant_is_known():
    """A MATCH length stopped at 254 instead of 255 changes nothing anywhere: both index the same DT2K entry."""
    assert P.DT2K[254] == P.DT2K[255] and P.STRETCH[1] == P.STRETCH[2]
    c = NE.EDGE_CASES["g_all"]
    with NE.patched(MATCH_MAX_LEN=254):
        assert tuple(NE.run(c.header, c.segments)[0]) == true_coded("g_all")


@pytest.mark.parametrize("name", sorted(NE.SET_TELLS))
def test_set_cases_tell_a_state_lost_at_the_boundary(name):
    """The weight first reaches its bound in segment 0 or 1 and is there again in a later segment; the reference that starts
    the next segment with the component's tables as new writes other bytes."""
    c, t = NE.EDGE_CASES[name], TABLE["edge_cases"][name]
    true = true_coded(name)
    for event in NE.SET_TELLS[name]:
        assert t["first"][event][0] <= 1 and max(t["segs"][event]) > t["first"][event][0], (name, event)
    kinds = {NE.RESETS[e.split(".")[1]]: e for e in NE.SET_TELLS[name]}           # one lost state per component type
    for types, event in sorted(kinds.items()):
        lost = NE.mutant_coded(c, event, reset=True, until=true)
        differ = [s for s in range(len(lost)) if lost[s] != true[s]]
        assert differ and differ[0] >= 1, (name, types, differ)


@functools.lru_cache(maxsize=None)
def true_block(name):
    c = NE.EDGE_CASES[name]
    return tuple(NE.run(c.header, [c.block], c.offsets)[0])


@pytest.mark.parametrize("cls,req", sorted(NE.BLOCK_TELLS))
def test_a_block_tells_the_edge_moved_by_one(cls, req):
    """The same telling check on the block form: a pinned case per required event."""
    event, name = NE.BLOCK_TELLS[cls, req]
    c, t = NE.EDGE_CASES[name], TABLE["edge_blocks"][name]
    assert c.cls == cls and event in NE.REQUIRED[cls][req] and t[event] >= NE.FLOOR
    assert NE.mutant_coded(c, event, until=true_block(name), block=True) != list(true_block(name))


@pytest.mark.parametrize("name", sorted(NE.BLOCK_TELLS_TOP))
def test_chain_blocks_tell_the_top_bound_moved_by_one(name):
    """262143 -> 262142 per specialisation where a block tells it: 2 (l1, l1_sizes), 3 (l2), 5 (l3_mixed), a runtime loop
    (mix2_chain3).  The bottom bound moved by one is told by l1 and l1_sizes alone (the ISSE's wt1 * 64 changes its output once
    in 1024 uses, and the longer chains halve that difference at every further ISSE): measured over all ten chain blocks,
    top told by 5, bottom by 2; the next test holds every chain block to a coarser fault at both bounds."""
    c = NE.EDGE_CASES[name]
    assert NE.mutant_coded(c, "w512.wt1.hi", until=true_block(name), block=True) != list(true_block(name))


@pytest.mark.parametrize("name", [n for n in BASE if NE.EDGE_CASES[n].cls == "chain"])
def test_every_chain_block_tells_a_bound_that_does_not_fit_its_field(name):
    """The chain kernels pack the ISSE's weight pair as 20 + 20 bits.  A field one bit too narrow (or a sign extension lost) gives
    a weight at 262143 back as -1 and one at -262144 as 0: every chain case's block, hence every specialisation, tells either."""
    c = NE.EDGE_CASES[name]
    for event in ("w512.wt1.hi", "w512.wt1.lo"):
        assert TABLE["edge_blocks"][name][event] >= NE.FLOOR
        assert NE.mutant_coded(c, event, until=true_block(name), block=True, wrap=True) != list(true_block(name)), event
