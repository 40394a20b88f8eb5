"""The corpus of three-round members for the block sets (tests/offnominal_sets.py) on the host: its counts and layout; that
enough members survive their damaged segment, come out of it somewhere else than the original, and decode a follow-on
segment that tells the state they kept from the state an undamaged segment would have left (only those see a kernel that
kept the wrong state); the slab policies; and the checker of test_gpu_offnominal_sets.py fed such a wrong state."""
import collections
import time

import numpy as np
import pytest

import offnominal_corpus as OC
import offnominal_sets as OS
from test_gpu_offnominal import PAD, SENTINEL, check_decode

# conditions, not measurements (measured: survivors 341-360, diverged 147-181, telling 119-176 over OS.STATEFUL)
MIN_SURVIVORS, MIN_DIVERGED, MIN_TELLING = 330, 140, 100


def as_got(caps, exps):
    """What a kernel that computed `exps` would hand back: check_decode's tuple, on a sentinel-filled buffer."""
    off = np.zeros(len(caps) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(caps, dtype=np.uint64))
    out = np.full(int(off[-1]) + PAD, SENTINEL, dtype=np.uint8)
    for i, e in enumerate(exps):
        out[int(off[i]):int(off[i]) + len(e.data)] = np.frombuffer(e.data, dtype=np.uint8)
    u32 = [np.asarray(col, dtype=np.uint32) for col in ([e.out_len for e in exps], [e.consumed for e in exps],
                                                        [e.final_code for e in exps], [e.first_byte for e in exps])]
    return (out, off) + tuple(u32) + (np.asarray([e.status for e in exps], dtype=np.int32),)


def census(model):
    """Indices of the mutated members of layout(model, True) that survive round 1 under roomy slabs, of those that come out
    of it with other bytes than the original's, and of those whose round 2 tells the kept state from the undamaged one's."""
    batch = OS.layout(model, True)
    want, wrong = OS.expectations(model, True, "roomy"), OS.expectations(model, True, "roomy", undamaged=True)
    mutated = [i for i, m in enumerate(batch) if m.kind not in ("junk", "filler")]
    survivors = [i for i in mutated if want[1][i].status == 0]
    diverged = [i for i in survivors if want[1][i].data != batch[i].data]
    telling = [i for i in diverged if want[2][i] != wrong[2][i]]
    return batch, want, wrong, mutated, survivors, diverged, telling


@pytest.mark.parametrize("model", OS.STATEFUL + OS.STATELESS)
def test_counts_and_layout(model):
    for pp in (True, False):
        ms = OS.members(model, pp)
        mutated = [m for m in ms if m.kind != "junk"]
        assert len(mutated) == 360 and len(ms) == 375
        per = collections.Counter(m.what.split(" ")[0] for m in mutated)
        assert len(per) == 24 and set(per.values()) == {15}
        assert {m.kind for m in ms} == set(OC.MUTATIONS)
        assert collections.Counter(m.kind for m in mutated) == {"exact": 24, "trail": 72, "trunc": 192, "flip": 72}
        batch = OS.layout(model, pp)
        assert batch is OS.layout(model, pp)                                # one order for all three rounds
        assert sorted(m for m in batch if m.kind != "filler") == sorted(ms)
        assert batch[0].kind == batch[-1].kind == "filler"
        buf, off = b"".join(m.streams[1] for m in batch), OS.offsets(batch)
        for i, m in enumerate(batch):
            if m.kind != "filler":
                assert buf[off[i] - 1] != 0 and buf[off[i + 1]] != 0, (model, i, m.what)
        trunc = [i for i, m in enumerate(batch) if m.kind == "trunc"]
        assert {off[i + 1] % 4 for i in trunc if batch[i].streams[1]} == set(range(4))
        assert {off[i] % 16 for i in trunc} == set(range(16))


@pytest.mark.parametrize("model", OS.STATEFUL)
def test_enough_members_tell_a_wrong_kept_state(model):
    t0 = time.perf_counter()
    batch, want, wrong, mutated, survivors, diverged, telling = census(model)
    fresh = OS.fresh_round2(model, True)
    spent = time.perf_counter() - t0
    assert len(mutated) == 360
    assert all(e.status == 0 and e.consumed == len(m.streams[0]) for e, m in zip(want[0], batch))     # the warm-up is good
    differs = [i for i in survivors if want[2][i] != fresh[i]]
    print("\n%s: survivors %d, diverged %d, telling %d, differ from a fresh model %d; oracle %.1f s"
          % (model, len(survivors), len(diverged), len(telling), len(differs), spent))
    assert len(survivors) >= MIN_SURVIVORS and len(diverged) >= MIN_DIVERGED and len(telling) >= MIN_TELLING
    assert len(differs) >= len(survivors) - (1 if model == "hm0" else 0)
    # an undamaged round 1 is the original, and the follow-on segment then decodes to its end
    for i in mutated:
        if batch[i].kind == "exact":
            assert want[1][i] == wrong[1][i] and want[2][i] == wrong[2][i]
        assert wrong[1][i].status == 0 and wrong[1][i].data == batch[i].data
        assert wrong[2][i].status == 0 and wrong[2][i].consumed == len(batch[i].streams[2])
    # failed members report without coding
    for i in mutated:
        if want[1][i].status:
            assert want[2][i] == OC.Expected(want[1][i].status, 0, b"", 0, 0, OC.NO_BYTE)


@pytest.mark.parametrize("model", OS.STATELESS)
def test_stateless_models_tell_nothing(model):
    """Their coded streams do not depend on the state a segment leaves: no member can show a wrong kept state, so they must
    not stand in for a model of OS.STATEFUL in test_gpu_offnominal_sets.py."""
    assert model not in OS.STATEFUL
    telling = census(model)[-1]
    assert len(telling) == 0


@pytest.mark.parametrize("model", OS.STATEFUL)
def test_tight_slabs(model):
    for pp in (True, False):
        batch = OS.layout(model, pp)
        tight, short = OS.expectations(model, pp, "tight"), OS.expectations(model, pp, "tight-1")
        caps = OS.slabs(batch, "tight-1")
        assert {e.status for e in tight[1]} == {0, -7} == {e.status for e in short[1]}
        assert sum(1 for c, m in zip(caps, batch) if c == 0 and m.nominal == 64) == 1
        for i, m in enumerate(batch):
            if m.kind in ("exact", "trail"):
                assert tight[1][i].status == 0 and tight[1][i].out_len == m.nominal == len(tight[1][i].data), (model, m.what)
            if m.kind == "exact" and m.nominal:
                assert short[1][i].status == -7 and short[1][i].out_len == caps[i] + 1, (model, m.what)
                assert short[1][i].data == m.data[:caps[i]]
            for want in (tight, short):
                assert want[0][i].status == 0
                if want[1][i].status:
                    assert want[2][i] == OC.Expected(want[1][i].status, 0, b"", 0, 0, OC.NO_BYTE)
        # round 2 has failed members and live ones side by side: the call that copies only the live members' stored bytes
        assert 0 < sum(1 for e in tight[1] if e.status) < len(batch)


@pytest.mark.parametrize("model", OS.STATEFUL)
def test_the_checker_rejects_a_wrong_kept_state(model):
    """The stand-in for a kernel that leaves in the slot the state of the undamaged segment's end: the expectations computed
    with the undamaged round 1.  check_decode takes the true round 2, rejects the stand-in's as a whole and for every
    telling member on its own; round 1 itself it rejects for every diverged member."""
    batch, want, wrong, mutated, survivors, diverged, telling = census(model)
    caps = [OS.ROOMY] * len(batch)
    cases = [OS.as_case(m, 2) for m in batch]
    check_decode(model, cases, caps, want[2], as_got(caps, want[2]), whole=True)
    with pytest.raises(AssertionError):
        check_decode(model, cases, caps, want[2], as_got(caps, wrong[2]))
    for rnd, which in ((2, telling), (1, diverged)):
        for i in which:
            for whole in (False, True):
                with pytest.raises(AssertionError):
                    check_decode(model, [OS.as_case(batch[i], rnd)], [OS.ROOMY], [want[rnd][i]], as_got([OS.ROOMY], [wrong[rnd][i]]), whole=whole)
    quiet = [i for i in mutated if want[2][i] == wrong[2][i]]
    for i in quiet[:5]:
        check_decode(model, [OS.as_case(batch[i], 2)], [OS.ROOMY], [want[2][i]], as_got([OS.ROOMY], [wrong[2][i]]), whole=True)
