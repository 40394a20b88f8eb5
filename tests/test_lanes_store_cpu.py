"""The line-store request of the lane-per-component kernels (ZPQ_FLAG_LINESTORE), host side: the two predicates that need no
device -- would the request be honoured for a model at a capacity, and how large is a slot under the store -- and the
arithmetic the GPU test's blocks stand on: every block meant to fit touches at most 202 lines of any table, the block meant
to be refused more than twice the store's limit of 240."""
import pytest

import lanes_store as LS

NO_HASHED = LS.H([[LS.CM, 12, 255], [LS.MATCH, 10, 12], [LS.MIX2, 4, 0, 1, 24, 255]], 2, 8, LS.GM.hashchain(3))
N65 = LS.GM.NAMED["n65"][0]
N65_BIG = LS.H([[LS.ICM, 16]] + LS.GM.cms(63, 0, 9) + [[LS.MIX, 2, 56, 8, 24, 255]], 7, 8, LS.GM.hashchain(65))


def test_the_request_applies_by_the_models_shape(zpq):
    for name, hdr in LS.MODELS.items():
        m = zpq.Model(header=hdr)
        assert LS.compact(hdr), name
        assert m.lanes_store_applies(LS.CAP), name
        assert not m.lanes_store_applies(LS.DENSE_CAP), name       # a store larger than every hashed table
        assert not LS.compact(hdr, LS.DENSE_CAP), name
        for cap in (0, 4, 12, 15, 17, 258, 1023):                   # below 16, or no multiple of 4
            assert not m.lanes_store_applies(cap), (name, cap)
        assert m.lanes_store_applies(16) and m.lanes_store_applies(260), name
    assert not zpq.Model(header=N65).lanes_store_applies(LS.CAP)      # more than 64 components: no lane kernel
    assert not zpq.Model(header=N65_BIG).lanes_store_applies(LS.CAP)  # ... also with a table that would go on the store
    assert not zpq.Model(header=NO_HASHED).lanes_store_applies(LS.CAP)  # no ICM / ISSE
    assert zpq.FLAG_LINESTORE == 32


def test_a_slot_on_the_store_is_smaller(zpq):
    for name, hdr in LS.MODELS.items():
        m = zpq.Model(header=hdr)
        small = m.lanes_store_slot_bytes(LS.CAP)
        assert 0 < small < m.state_bytes, (name, small, m.state_bytes)
        # what leaves the slot: the dense tables of the compact components; what comes: a store each (and alignment)
        gone = sum(64 << b for _, b in LS.compact(hdr))
        come = len(LS.compact(hdr)) * LS.STORE_BYTES
        assert abs((m.state_bytes - small) - (gone - come)) <= 512 * len(LS.compact(hdr)), (name, small, m.state_bytes)
        assert m.lanes_store_slot_bytes(LS.DENSE_CAP) == 0 and m.lanes_store_slot_bytes(10) == 0, name
    for hdr in (N65, N65_BIG, NO_HASHED):
        assert zpq.Model(header=hdr).lanes_store_slot_bytes(LS.CAP) == 0
    big = zpq.Model(header=LS.H([[LS.ICM, 22], [LS.ISSE, 22, 0], [LS.CM, 16, 255], [LS.MIX2, 8, 0, 1, 24, 255]], 2, 8, LS.GM.hashchain(4)))
    assert big.state_bytes > 512 << 20 and big.lanes_store_slot_bytes(146824) < 21 << 20   # two tables of 256 MiB against two stores


@pytest.mark.parametrize("name", sorted(LS.MODELS))
def test_every_fitting_block_stays_below_the_limit(name):
    hdr = LS.MODELS[name]
    blocks = LS.fitting_blocks()
    assert len(blocks) == 21 and max(len(b) for b in blocks) == 100 and sorted(len(b) for b in blocks)[:3] == [0, 1, 2]
    for b in blocks:
        for comp, count in LS.distinct_lines(hdr, b).items():
            assert count <= 2 * (len(b) + 1) <= 202 < LS.LIMIT, (name, comp, len(b), count)


def test_the_overflowing_block_needs_twice_the_limit():
    hdr = LS.MODELS[LS.OVERFLOW_MODEL]
    counts = LS.distinct_lines(hdr, LS.overflow_block())
    on_store = {i: counts[i] for i, _ in LS.compact(hdr)}
    assert LS.LIMIT == 240 and max(on_store.values()) > 2 * LS.LIMIT, on_store
    # ... under a context of order two: the hash chain's first link already mixes the byte with the one before it
    assert all(b >= 9 for _, b in LS.compact(hdr)) and (2, 8) in LS.hashed(hdr) and (2, 8) not in LS.compact(hdr)
