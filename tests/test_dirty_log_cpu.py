"""What test_gpu_dirty_log_paths.py assumes about its inputs, as far as it can be decided without a GPU (tests/dirty_log.py):
that the blocks it calls short cannot overflow a log of 64 entries while the ones beside them can, that every batch run on
fewer slots than blocks puts clean-table data directly behind dirty data on a slot, that the empty and the one-byte blocks
sit where the sequences say, and that the oracle's streams fit and overflow the slabs as the GPU tests expect."""
import pytest

import dirty_log as DL
import oracle_lib as O

ROUND_BATCHES = [(83, 1), (19, 2), (45, 3), (83, 4)]      # (blocks, seed) of seq_rounds, each run on 19, 13 and 5 slots
ROUND_SLOTS = (19, 13, 5)
HOST_BATCHES = [(83, 5), (83, 6)]                         # of the host rounds, on 16 slots


def test_short_blocks_cannot_overflow_64_entries_and_the_uniform_ones_can():
    assert DL.write_back_bound(DL.SHORT, True) < 64 and DL.write_back_bound(2048, False) < DL.DEFAULT_CAP
    assert DL.write_back_bound(1, True) < 8 and DL.write_back_bound(4, True) < 13
    for nb, seed in ((40, 1), (16, 3)):                   # the "mixed" batches: a launch at full residency
        plan = DL.mixed_plan(nb, seed)
        short = [n for kind, n in plan if kind != "uniform"]
        assert short and all(n <= DL.SHORT for n in short) and 0 in short and 1 in short
        assert sum(1 for kind, n in plan if kind == "uniform" and n == 2048) >= nb // 2
        assert all(len(b) == n for b, (_, n) in zip(DL.blocks_of("mixed", nb, seed), plan))
    # 2 KiB of uniform data touch far more than 64 lines of a table of 2^22 lines and more: nearly every nibble's context is new
    data = DL.make("uniform", 7, 2048)
    assert len({data[i:i + 2] for i in range(len(data) - 1)}) > 1900


@pytest.mark.parametrize("nb,seed", ROUND_BATCHES)
def test_round_batches_put_clean_data_behind_dirty_data_on_every_slot_count(nb, seed):
    plan = DL.round_plan(nb, seed)
    assert all(0 <= n <= 2048 for _, n in plan)
    for slots in ROUND_SLOTS:
        if nb > slots:
            assert DL.clean_behind_dirty(plan, slots), (nb, slots)
        last = [plan[i] for i in DL.last_of_slot(nb, slots)]
        # the last block of a slot: an empty one, a one-byte one, a short one and a 2 KiB uniform one -- "mixed" at 8, 13, 64
        assert ("zeros", 0) in last and ("periodic", 1) in last and ("text", DL.SHORT) in last and ("uniform", 2048) in last
        if nb == 83:                                      # ... an empty and a one-byte block in a later round that is not the last
            assert plan[22][1] == 0 and plan[29][1] == 1 and 22 >= slots and 29 + slots < nb
            assert nb % slots != 0                        # the last round leaves slots idle


def test_round_launches_follow_each_other_with_clean_data_behind_dirty_data():
    """From one launch to the next: a slot whose last block was 2 KiB uniform begins the next launch with zeros or periodic data."""
    order = [ROUND_BATCHES[i] for i in (0, 1, 2, 0, 3, 1, 2, 3, 1)]        # seq_rounds
    for slots in ROUND_SLOTS:
        hits = 0
        for (nb0, s0), (nb1, s1) in zip(order, order[1:]):
            p0, p1 = DL.round_plan(nb0, s0), DL.round_plan(nb1, s1)
            for slot, i in enumerate(DL.last_of_slot(nb0, slots)):
                if p0[i] == ("uniform", 2048) and slot < nb1 and p1[slot][0] in DL.CLEAN:
                    hits += 1
        assert hits >= 3, slots


@pytest.mark.parametrize("nb,seed", HOST_BATCHES)
def test_host_round_batches(nb, seed):
    plan = DL.round_plan(nb, seed, shift=16)
    assert DL.clean_behind_dirty(plan, 16) and (nb - 1) % 16 + 1 == 3 and (nb + 15) // 16 == 6
    last = [plan[i] for i in DL.last_of_slot(nb, 16)]
    assert ("uniform", 2048) in last and ("periodic", 1) in last


def test_batches_of_the_old_sequences_hold_an_empty_and_a_one_byte_block():
    for kind in ("uniform", "zeros", "text", "periodic"):
        for nb in (16, 40):
            lens = [len(b) for b in DL.batch(kind, nb, 1)]
            assert lens[3] == 0 and lens[7] == 1 and max(lens) <= 8192
    assert all(len(b) > 0 for b in DL.batch("uniform", 11, 5))


def test_capacity_variable_as_the_library_reads_it():
    assert [DL.parse_cap(v) for v in (None, "", "-5", "abc", "3", "1048577", "0", "64", "13x")] == \
        [16384, 16384, 0, 0, 3, 1 << 20, 0, 64, 13]


def test_streams_fit_and_overflow_as_the_gpu_tests_assume():
    # seq_error_status: slabs of 2100 bytes hold some of the 40 uniform blocks and streams and not all of them
    blocks, want = DL.oracle("small", "uniform", 40, 0, True)
    assert 0 < sum(len(w) <= 2100 for w in want) < 40 and 0 < sum(len(b) <= 2100 for b in blocks) < 40
    # the variants' and the rounds' decoders get slabs of 2100 bytes: every block fits
    assert all(len(b) <= 2048 for b in DL.blocks_of("uniform2k", 40, 2) + DL.blocks_of("rounds16", 83, 5))
    # the damaged batch: a third damaged, some members overflow the slab, damaged ones end inside it, one stream is empty
    for pp in (True, False):
        batch, caps, want = DL.damaged_batch(pp, 1531)
        bad = [c for c in batch if c.kind != "exact"]
        assert len(batch) == 39 and len(bad) == 13 and any(not c.stream for c in bad)
        assert {c.what.split()[1][:5] for c in bad} >= {"trunc", "flip-"}
        assert any(w.status == -7 for w in want) and any(w.status == 0 and c.kind != "exact" for w, c in zip(want, batch))
        assert all(w.status == (0 if c.nominal <= 1531 else -7) for w, c in zip(want, batch) if c.kind == "exact")
        assert any(w.out_len != c.nominal for w, c in zip(want, batch) if c.kind != "exact")


def test_the_small_header_is_level_2_with_16_line_tables():
    h2, hs = O.level_header(2), DL.HEADERS["small"]
    assert len(h2) == len(hs) and h2 != hs and sum(a != b for a, b in zip(h2, hs)) <= 3
