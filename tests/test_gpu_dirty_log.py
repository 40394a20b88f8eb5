"""The pool's dirty-line logs (ZPQ_DIRTY_LOG_CAP; DBatch::dlog): level 2's k_pipe<encode> and two-hypothesis k_chain<decode>
note the 64-byte table lines a launch made non-zero, and the next launch of theirs on the pool zeroes those lines instead
of every slot.  A line that was dirtied and not logged, or logged and not cleared, is stale state under the next block: the
sequences below put a block whose result depends on clean tables behind one that dirtied them, on one ctx, and compare every
launch with the C oracle stream for stream.  Each sequence runs twice per log capacity: once as it is (the kernels' own
clear), once with zpq_debug_pool_residue after every launch that keeps the log (it must find nothing left)."""
import pytest

from dirty_log import Run

pytestmark = pytest.mark.gpu


def seq_classes(r):
    for i, kind in enumerate(("uniform", "zeros", "text", "uniform")):
        r.both(kind, 40 if i % 2 == 0 else 16, i, pp=i != 2)


def seq_decode_only(r):
    for i, kind in enumerate(("uniform", "zeros", "text", "periodic", "uniform", "zeros")):
        r.dec(kind, 16 if i == 3 else 40, i, pp=i != 1)


def seq_slot_counts(r):
    r.both("uniform", 40, 0)
    r.both("text", 16, 2, pp=False)
    r.both("zeros", 40, 1)                                # slots 16 .. 39 still hold the first launch's lines
    r.enc("uniform", 11, 5)                               # below twelve blocks the encoder is k_chain<encode>: no log
    r.both("zeros", 40, 1)
    r.dec("uniform", 11, 5)
    r.both("periodic", 16, 3)
    r.both("zeros", 40, 1)


def seq_other_launches(r):
    r.both("uniform", 40, 0)
    r.other(1)
    r.both("zeros", 40, 1)
    r.both("uniform", 16, 4, pp=False)
    r.other(3)
    r.both("text", 40, 2)
    r.blockset()
    r.both("zeros", 40, 1)


def seq_error_status(r):
    r.both("uniform", 40, 0)
    r.enc("uniform", 40, 0, cap=2100)                     # the larger blocks' coded streams do not fit: status per block
    r.both("zeros", 40, 1)
    r.dec("uniform", 40, 0, cap=2100)                     # ... and the larger blocks do not fit the decoder's slab
    r.both("zeros", 40, 1)
    r.both("text", 16, 2)


SEQUENCES = {"classes": seq_classes, "decode_only": seq_decode_only, "slot_counts": seq_slot_counts,
             "other_launches": seq_other_launches, "error_status": seq_error_status}


@pytest.mark.parametrize("cap_env", [None, "8", "64"])      # the default; every table overflows; some do and some do not
@pytest.mark.parametrize("name", ["level2", "small"])
@pytest.mark.parametrize("seq", sorted(SEQUENCES))
def test_sequences_against_the_oracle(zpq, gpu_ctx, monkeypatch, seq, name, cap_env):
    for v in ("ZPQ_ENC_PIPE", "ZPQ_ENC_SPLIT", "ZPQ_DEC_PIPE", "ZPQ_SPARSE_MODE", "ZPQ_SPARSE_FORCE_LOG2"):
        monkeypatch.delenv(v, raising=False)
    if cap_env is None:
        monkeypatch.delenv("ZPQ_DIRTY_LOG_CAP", raising=False)
    else:
        monkeypatch.setenv("ZPQ_DIRTY_LOG_CAP", cap_env)
    for residue in (False, True):
        r = Run(zpq, gpu_ctx, name, cap_env, residue)
        SEQUENCES[seq](r)
        r.model.close()


def test_cap_zero_switches_the_mechanism_off(zpq, gpu_ctx, monkeypatch):
    monkeypatch.setenv("ZPQ_DIRTY_LOG_CAP", "0")
    r = Run(zpq, gpu_ctx, "small", "0", True)
    seq_classes(r)
    r.model.close()


def test_cap_changes_between_launches(zpq, gpu_ctx, monkeypatch):
    """The capacity is read per call: logs kept at one capacity are not read at another."""
    r = Run(zpq, gpu_ctx, "small", None, False)
    for i, cap in enumerate(("64", "8", None, "0", "16384", "64")):
        if cap is None:
            monkeypatch.delenv("ZPQ_DIRTY_LOG_CAP", raising=False)
        else:
            monkeypatch.setenv("ZPQ_DIRTY_LOG_CAP", cap)
        r.both("uniform" if i % 2 == 0 else "zeros", 40, i % 2)
    r.model.close()
