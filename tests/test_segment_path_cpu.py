"""The corpus of the one-block segment path (tests/segment_path.py) on the host: what it holds, that the two reference
implementations agree on every case (the Python one keeps p[] across segments, as Predictor.reset leaves it), at which
segment a coder that zeroed p[] between segments would write other bytes than the oracle -- only those cases see a kernel
that drops p[] -- and that the library's host predicates send a block's first segment to the kernel the GPU file
(test_gpu_segment_path.py) asserts."""
import os
import sys

import pytest

import general_models as GM
import segment_path as SP

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "pyref"))
import zpaq_pyref as P  # noqa: E402

KNOBS = ("ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE", "ZPQ_LANES_ROWS", "ZPQ_VM_PIPE", "ZPQ_CHAIN_G", "ZPQ_CHAIN_BPW", "ZPQ_SPARSE_MODE",
         "ZPQ_SPARSE_FORCE_LOG2")
# must tell at segment 2 of the main sequence, the one-byte segment / must tell somewhere in it / are parity cases only
AT_TWO, SOMEWHERE, SILENT = ("fwd_avg", "fwd_isse", "fwd_mix_self", "fwd_n67"), ("fwd_chain", "fwd_mix2"), ("fwd_sse_self", "isse_stale_input", "fwd_n20")


def test_the_corpus():
    assert 20 <= len(SP.MODELS) <= 24
    for name in ("level1", "level2", "level3", "level4", "level5", "c4b", "match_wrap", "vm_rows", "vm_lanes", "n65", "fwd_n20",
                 "fwd_n67") + AT_TWO + SOMEWHERE + SILENT:
        assert name in SP.MODELS, name
    assert set(SP.FORWARD) == set(SP.TELLS) == set(AT_TWO + SOMEWHERE + SILENT)
    for name in SP.FORWARD:
        assert GM.has_forward_reference(SP.MODELS[name].header), name
    for name, m in SP.MODELS.items():
        n = m.header[4]
        assert (n > 16) == (name in SP.SMALL), (name, n)
        assert (name in SP.FORWARD) == GM.has_forward_reference(m.header) or m.family == "chain", name
    assert SP.MODELS["vm_rows"].header[4] <= 16 < SP.MODELS["vm_lanes"].header[4] <= 64
    assert SP.MODELS["fwd_n67"].header[4] == 67 and GM.components(SP.MODELS["fwd_n67"].header)[0] == [GM.ISSE, 12, 65]
    for which in SP.SEQUENCES:
        for small in (False, True):
            segs = SP.sequence(which, small)
            lens = [len(s.data) for s in segs]
            assert 5 <= len(segs) <= 6 and max(lens) <= 1500 and sum(lens) <= (800 if small else 4096)
            assert 0 in lens and 1 in lens and any(a == 0 and b > 0 for a, b in zip(lens, lens[1:]))
            assert segs is SP.sequence(which, small)                        # computed once
    assert [len(s.data) for s in SP.sequence("main", True)][1] == 1 and len(SP.sequence("main")[1].data) == 1
    assert len(SP.sequence("empty_first")[0].data) == 0
    first = SP.sequence("prog_first")[0]
    assert first.flags == 0 and first.data[0] != 0
    assert {s.flags for s in SP.sequence("prog_first")} == {0, SP.PP}
    # the MATCH buffer of match_wrap (256 bytes) wraps inside every sequence
    assert GM.components(SP.MATCH_WRAP)[1] == [GM.MATCH, 8, 8]
    assert all(sum(len(s.data) for s in SP.sequence(w)) > 2 * 256 for w in SP.SEQUENCES)


@pytest.mark.parametrize("name", list(SP.MODELS))
def test_both_references_agree_and_the_tells_are_pinned(name):
    """The Python reference with p[] kept equals the C oracle on every sequence; with p[] zeroed before every segment it
    first departs exactly where segment_path.TELLS says (a forward-reference model), or never."""
    m = SP.MODELS[name]
    tells = []
    for which in SP.SEQUENCES:
        segs, want = SP.segments(name, which), SP.coded(name, which)
        kept = P.new_model(m.header, m.offsets)
        assert tuple(P.encode_segment(kept, s.data, pp=bool(s.flags & SP.PP)) for s in segs) == want, which
        del kept
        if name not in SP.FORWARD:
            continue
        zeroed, tell = P.new_model(m.header, m.offsets), None
        for i, s in enumerate(segs):
            zeroed.p = [0] * len(zeroed.p)
            if P.encode_segment(zeroed, s.data, pp=bool(s.flags & SP.PP)) != want[i]:
                tell = i + 1                                # (from here on the tables differ too: the first one is what is pinned)
                break
        tells.append(tell)
    if name in SP.FORWARD:
        assert tuple(tells) == SP.TELLS[name], (name, tells)


def test_the_required_tellers_tell():
    main = SP.SEQUENCES.index("main")
    for name in AT_TWO:
        assert SP.TELLS[name][main] == 2, name
    for name in SOMEWHERE:
        assert SP.TELLS[name][main] is not None, name
    for name in SILENT:
        assert SP.TELLS[name] == (None, None, None), name
    # every telling case tells after the first segment (the first one starts from a fresh p[] either way)
    assert all(t is None or t >= 2 for ts in SP.TELLS.values() for t in ts)


def test_decode_expectations_round_trip():
    """What the GPU file expects of a decoder is the sequence itself, the PP byte apart."""
    for name in ("level2", "fwd_isse"):
        for which in SP.SEQUENCES:
            segs = SP.segments(name, which)
            for s, stream, e, a in zip(segs, SP.coded(name, which), SP.decoded(name, which), SP.decoded(name, which, all_pp=True)):
                assert e.status == 0 and e.data == s.data and e.consumed == len(stream)
                assert e.first_byte == (0 if s.flags & SP.PP else SP.OC.NO_BYTE)
                assert a.status == 0 and a.consumed == len(stream) and a.final_code == e.final_code
                if s.flags & SP.PP:
                    assert a == e
                else:
                    assert a.first_byte == (s.data[0] if s.data else SP.OC.NO_BYTE) and a.data == s.data[1:]
    assert SP.decoded("level2", "prog_first", all_pp=True)[0].first_byte == 1


@pytest.mark.parametrize("name", list(SP.MODELS))
def test_first_segment_routes(zpq, monkeypatch, name):
    """zpq_chain_route, zpq_gpipe_applies, zpq_gdec_applies, zpq_lanes_supported and zpq_lanes_kernel_name give the kernel of a
    block's first segment that the GPU file asserts; every later segment is k_generic's."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    assert SP.first_kernels(zpq, name) == SP.expected_first_kernels(name), name
    if name in SP.FORWARD:                                 # no wave pipeline takes a forward reference: its p[] is the lanes' to keep
        assert not SP.first_kernels(zpq, name)[0].startswith("k_gpipe")
    model = zpq.Model(header=SP.MODELS[name].header, offsets=SP.MODELS[name].offsets)
    lanes = zpq.lib().zpq_blockset_lanes_applies(model.h) == 1
    assert lanes == (SP.MODELS[name].family == "general"), name          # which sets may ask for ZPQ_SET_LANES
    model.close()


def _zeroed_departs(name, segs):
    """Does the Python reference with p[] zeroed before every segment write other bytes than the oracle for `segs` (coded with
    ZPQ_FLAG_PP throughout)?  The kept one must not."""
    m = SP.MODELS[name]
    c = SP.codec(name)
    want = [c.encode(s, pp=True) for s in segs]
    del c
    kept, zeroed = P.new_model(m.header, m.offsets), P.new_model(m.header, m.offsets)
    assert [P.encode_segment(kept, s) for s in segs] == want
    other = []
    for s in segs:
        zeroed.p = [0] * len(zeroed.p)
        other.append(P.encode_segment(zeroed, s))
    assert other[0] == want[0]
    return other != want


@pytest.mark.parametrize("name", AT_TWO + SOMEWHERE)
def test_the_set_members_tell(name):
    """Each of the three members test_gpu_segment_path.py puts into its block sets tells a dropped p[]."""
    members = SP.set_members(name)
    assert len(members) == 3
    for segs in members:
        assert _zeroed_departs(name, segs), name


@pytest.mark.parametrize("name", SP.ARCHIVE_MODELS)
def test_the_archive_blocks_tell(name):
    """Blocks of 2, 4 and 5 segments, an empty file among them: every block of the archives tells a dropped p[]."""
    blocks = SP.archive_blocks(name)
    assert [len(b) for b in blocks] == [2, 4, 5] and blocks[1][0][2] == b"" and name in AT_TWO
    for files in blocks:
        assert _zeroed_departs(name, [d for _, _, d in files]), (name, len(files))
