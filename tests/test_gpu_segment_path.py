"""The one-block segment path against the oracle (the corpus: tests/segment_path.py; what it tells: test_segment_path_cpu.py).

A zpq.Block codes its first segment on the batch kernels and every later one on k_generic with ZB_KEEP_STATE, behind a
replay of the first segment's symbols into the block's slot; a default-route block set of a general model, any model with
more than 64 components and the sequential front end code their later segments with the same launches.  Every model of
the corpus goes through three sequences of segments in both directions; expected values come from oracle_lib.Codec, one
codec per block.  The forward-reference models tell whether p[], the last bit's predictions, went from segment to segment."""
import pytest

import segment_path as SP
from test_gpu_blockset import check_parity, make_members, oracle_history
from test_gpu_set_lanes import requesting
from test_gpu_set_lanes_archive import solid_block
from test_gpu_solid_archive import sequential_extract, triples

pytestmark = pytest.mark.gpu

KNOBS = ("ZPQ_SET_LANES", "ZPQ_SET_PIPE", "ZPQ_SET_WAVES", "ZPQ_SET_VMWAVES", "ZPQ_LANES_ROWS", "ZPQ_ENC_GPIPE", "ZPQ_DEC_GPIPE",
         "ZPQ_GPIPE_BATCH", "ZPQ_GDEC_BPW", "ZPQ_VM_PIPE", "ZPQ_ENC_PIPE", "ZPQ_ENC_SPLIT", "ZPQ_DEC_PIPE", "ZPQ_DEC_HYP16",
         "ZPQ_SPARSE_MODE", "ZPQ_SPARSE_FORCE_LOG2", "ZPQ_CHAIN_G", "ZPQ_CHAIN_BPW")
E_OVERFLOW = -7
GENERIC = ("k_generic<encode>", "k_generic<decode>")
CASES = [(name, which) for name in SP.MODELS for which in SP.SEQUENCES]


@pytest.fixture()
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _model(zpq, name):
    m = SP.MODELS[name]
    return zpq.Model(header=m.header, offsets=m.offsets)


def encode_block(zpq, ctx, model, name, which, generic, first_cap=None):
    """The sequence through one Block: (the segments whose bytes differ from the oracle's, the kernels seen)."""
    segs, want = SP.segments(name, which), SP.coded(name, which)
    blk = zpq.Block(ctx, model)
    bad, kernels = [], []
    try:
        if first_cap is not None:                         # a first call whose slab is too small: the block stays fresh
            with pytest.raises(zpq.ZpqError) as e:
                blk.encode_segment(segs[0].data, flags=segs[0].flags, cap=first_cap)
            assert e.value.code == E_OVERFLOW
        for i, s in enumerate(segs):
            got = blk.encode_segment(s.data, flags=s.flags | (zpq.FLAG_GENERIC if generic else 0))
            kernels.append(ctx.last_kernel_name)
            if got != want[i]:
                bad.append(i + 1)
    finally:
        blk.close()
    return bad, kernels


def decode_block(zpq, ctx, model, name, which, generic, all_pp=False):
    """A fresh Block decodes the oracle's streams without ever encoding: (the segments that differ in any of data, out_len,
    consumed, first_byte, final_code; the kernels seen)."""
    segs, streams, want = SP.segments(name, which), SP.coded(name, which), SP.decoded(name, which, all_pp)
    blk = zpq.Block(ctx, model)
    bad, kernels = [], []
    try:
        for i, (s, stream, w) in enumerate(zip(segs, streams, want)):
            assert w.status == 0
            flags = (zpq.FLAG_PP if all_pp else s.flags) | (zpq.FLAG_GENERIC if generic else 0)
            out, consumed, code, first = blk.decode_segment(stream, SP.CAP + 8, flags=flags)
            kernels.append(ctx.last_kernel_name)
            if (out, len(out), consumed, first, code) != (w.data, w.out_len, w.consumed, w.first_byte, w.final_code):
                bad.append(i + 1)
    finally:
        blk.close()
    return bad, kernels


@pytest.mark.parametrize("name,which", CASES)
def test_block_encode(zpq, gpu_ctx, clean_env, name, which):
    """The first segment on its batch kernel, the later ones on k_generic behind the replay; then the same sequence on
    k_generic from the first segment on, which needs no replay."""
    model = _model(zpq, name)
    first = SP.expected_first_kernels(name)[0]
    n = len(SP.segments(name, which))
    try:
        bad, kernels = encode_block(zpq, gpu_ctx, model, name, which, generic=False)
        assert kernels == [first] + [GENERIC[0]] * (n - 1), kernels
        assert not bad, ("coded bytes differ from segment %d on" % bad[0], name, which, bad)
        bad, kernels = encode_block(zpq, gpu_ctx, model, name, which, generic=True)
        assert kernels == [GENERIC[0]] * n, kernels
        assert not bad, ("k_generic from the first segment: coded bytes differ from segment %d on" % bad[0], name, which, bad)
    finally:
        model.close()


@pytest.mark.parametrize("name,which", CASES)
def test_block_decode_first(zpq, gpu_ctx, clean_env, name, which):
    """A block that only ever decodes: its replay feeds [PP byte] + output of the first segment -- nothing at all after
    an empty first segment, the first byte literally where it is not 0 (prog_first, read with and without ZPQ_FLAG_PP)."""
    model = _model(zpq, name)
    first = SP.expected_first_kernels(name)[1]
    n = len(SP.segments(name, which))
    try:
        for all_pp in ((False, True) if which == "prog_first" else (False,)):
            bad, kernels = decode_block(zpq, gpu_ctx, model, name, which, generic=False, all_pp=all_pp)
            assert kernels == [first] + [GENERIC[1]] * (n - 1), kernels
            assert not bad, ("decoded segment %d differs" % bad[0], name, which, all_pp, bad)
        bad, kernels = decode_block(zpq, gpu_ctx, model, name, which, generic=True)
        assert kernels == [GENERIC[1]] * n, kernels
        assert not bad, ("k_generic from the first segment: decoded segment %d differs" % bad[0], name, which, bad)
    finally:
        model.close()


@pytest.mark.parametrize("name", ["level2", "c4b", "vm_rows", "fwd_isse", "fwd_n67"])
def test_a_first_segment_that_fails_then_succeeds(zpq, gpu_ctx, clean_env, name):
    """The first call's slab is too small: ZPQ_E_OVERFLOW, nothing persisted, the block is still fresh.  The same segment
    coded again with room runs on the batch kernel and the later segments equal the oracle."""
    model = _model(zpq, name)
    try:
        assert len(SP.coded(name, "main")[0]) > 8
        bad, kernels = encode_block(zpq, gpu_ctx, model, name, "main", generic=False, first_cap=8)
        assert kernels == [SP.expected_first_kernels(name)[0]] + [GENERIC[0]] * 4, kernels
        assert not bad, ("coded bytes differ from segment %d on" % bad[0], name, bad)
    finally:
        model.close()


def _set_members(name):
    """test_gpu_blockset.make_members's, eight of them, three replaced by the telling sequences; the segments of the others
    cut to 120 bytes where one lane walks more than 16 components."""
    members = make_members(4000 + len(name), nmembers=8)
    if name in SP.SMALL:
        members = [[s[:120] for s in segs] for segs in members]
    for at, segs in zip((1, 4, 6), SP.set_members(name)):
        members[at] = segs
    return members


@pytest.mark.parametrize("name", SP.FORWARD)
def test_default_route_sets(zpq, gpu_ctx, clean_env, name):
    """BlockSet without flags: k_generic per member, ZB_KEEP_STATE from a member's second segment on.  The same members with
    lanes=True (k_rows / k_lanes<..., KEEP>, at most 64 components): both routes equal the oracle, so each other."""
    m = SP.MODELS[name]
    assert m.offsets is None
    members = _set_members(name)
    want = oracle_history(m.header, members)
    check_parity(zpq, gpu_ctx, m.header, members, want, *GENERIC)
    if m.family == "general":
        check_parity(requesting(zpq), gpu_ctx, m.header, members, want, *SP.expected_first_kernels(name))


@pytest.mark.parametrize("name", SP.ARCHIVE_MODELS)
def test_archives_of_a_forward_reference_model(zpq, gpu_ctx, clean_env, name):
    """Blocks of 2, 4 and 5 segments, assembled from the oracle as test_gpu_set_lanes_archive.py does it.  The sequential
    Decompresser reads every file; archive_extract accepts every file (SHA-1) on k_generic<decode> and, for a model of at
    most 64 components, on k_rows<decode> under ZPQ_SET_LANES=1, with equal results.  (No block is written through the
    sequential Compressor: start_block_hcomp reproduces the reference's quirk Q14 -- no block header is written and every
    component stays type 0, compressor.v:191-209 -- so it cannot carry such a model.)"""
    header = SP.MODELS[name].header
    files = SP.archive_files(name)
    arc = b"".join(solid_block(header, b) for b in SP.archive_blocks(name))
    got = sequential_extract(zpq, gpu_ctx, arc)
    assert [(nm, d, st) for nm, d, st in got] == [(nm, d, 0) for nm, _, d in files]
    plain = zpq.archive_extract(gpu_ctx, arc)
    assert gpu_ctx.last_kernel_name == GENERIC[1]
    assert triples(plain) == files
    assert all(g["sha1_ok"] and g["status"] == 0 for g in plain)
    clean_env.setenv("ZPQ_SET_LANES", "1")
    lanes = zpq.archive_extract(gpu_ctx, arc)
    assert gpu_ctx.last_kernel_name == (SP.expected_first_kernels(name)[1] if SP.MODELS[name].family == "general" else GENERIC[1])
    assert lanes == plain
