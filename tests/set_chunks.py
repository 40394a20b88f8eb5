"""Chunked coding on block sets (zpq_blockset_{encode,decode}_chunks): a deterministic plan of members, segments, chunks
and calls, and the host-side bookkeeping the GPU tests share.  CPU-only; test_set_chunks_cpu.py checks the plan alone,
test_gpu_set_chunks.py holds the library to the oracle on it.

Encode plan: 21 members (no multiple of any blocks-per-workgroup) of 1-3 segments; every segment is cut into chunks whose
lengths come from CHUNK_LENGTHS -- shorter than, equal to and just past the longest chain's skew (16 lanes), around the
64-byte line, and zero.  The chunks are dealt into ROUNDS (one encode_chunks call each): members begin in different rounds
and sit some rounds out, so that single calls mix members that start a segment, go on with one and end one.
Decode schedule: every call lists all members that still have a stream to decode; member m gets in call t the capacity
DECODE_CAPS[(t + m) % 8], so caps cycle per call and differ between neighbours.  What a call must report follows from the
plaintext lengths alone (simulate_decode): a decoder pauses with its slab full, in front of the next EOF flag.
"""
import collections
import random

CHUNK_LENGTHS = [0, 1, 2, 3, 15, 16, 17, 64, 65, 300]
DECODE_CAPS = [0, 1, 2, 3, 17, 64, 65, 300]
NMEMBERS = 21
SEED = 1907

# one chunk of one call: member, segment index, chunk index inside the segment, its bytes, more (the segment goes on),
# opens (the member is closed when the call begins)
Chunk = collections.namedtuple("Chunk", "member seg idx data more opens")
Plan = collections.namedtuple("Plan", "members cuts rounds")
# one member's part of one decode call: member, segment, capacity, window start in the coded stream is the caller's to keep;
# expected bytes, out_len, open, opening (first call on the segment), closing_empty (the call that only finds the EOF)
Step = collections.namedtuple("Step", "member seg cap begin take open opening exact")


def _data(r, kind, n):
    if kind == 0:
        return bytes(n)
    if kind == 1:
        return bytes(r.getrandbits(8) for _ in range(n))
    if kind == 2:
        return bytes(r.choice(b"etaoin shrdlu\n") for _ in range(n))
    per = bytes(r.getrandbits(8) for _ in range(r.randint(1, 40)))
    return (per * (n // len(per) + 1))[:n]


def _cut(r, m, s, L):
    """chunk lengths of segment s of member m: the forced shapes first (so that every count the plan promises is met by
    construction), random cuts of one to five chunks for the rest"""
    shape = (m + 2 * s) % 7
    if shape == 0:
        return [0] + [r.choice(L[1:]) for _ in range(r.randint(1, 3))]      # opened by an empty chunk
    if shape == 1:
        return [r.choice(L[1:]) for _ in range(r.randint(1, 3))] + [0]      # ended by an empty chunk
    if shape == 2:
        return [r.choice(L)]                                                # one chunk: more = 0 on a closed member
    if shape == 3:
        return [0, 0] if s else [0]                                                     # nothing but empty chunks
    return [r.choice(L) for _ in range(r.randint(2, 5))]


def counts(plan):
    """the shapes the issue names, counted over the plan's segments"""
    c = collections.Counter()
    for m, segs in enumerate(plan.cuts):
        for s, cut in enumerate(segs):
            c["opened_by_empty"] += len(cut) > 1 and cut[0] == 0
            c["ended_by_empty"] += len(cut) > 1 and cut[-1] == 0
            c["one_chunk"] += len(cut) == 1
            c["second_after_chunked"] += s == 1 and len(segs[0]) > 1
    for rnd in plan.rounds:
        kinds = {(ch.opens, ch.more) for ch in rnd}
        c["mixed_rounds"] += len(kinds) == 4            # starts-and-goes-on, one-chunk, goes on, ends: all in ONE call
    return c


SHORT_LENGTHS = [0, 1, 2, 3, 15, 16, 17]


def make_plan(seed=SEED, nmembers=NMEMBERS, lengths=CHUNK_LENGTHS):
    """lengths=SHORT_LENGTHS: the same plan with no chunk beyond 17 bytes, for a line store forced small -- a member is then
    at most 3 segments x 5 chunks x 17 = 255 bytes and claims at most 2 (255 + 2) = 514 lines per table (predictor.v:495-532,
    558-560: two nibble rows per byte), below the 960 at which a 1024-line store refuses."""
    r = random.Random(seed)
    cuts = [[_cut(r, m, s, lengths) for s in range(1 + m % 3)] for m in range(nmembers)]
    members = [[_data(r, (m + s) % 4, sum(cut)) for s, cut in enumerate(segs)] for m, segs in enumerate(cuts)]
    # every member's chunks in order, then the rounds
    queues = []
    for m, segs in enumerate(cuts):
        q = []
        for s, cut in enumerate(segs):
            pos = 0
            for i, n in enumerate(cut):
                q.append(Chunk(m, s, i, members[m][s][pos:pos + n], i + 1 < len(cut), i == 0))
                pos += n
        queues.append(q)
    rounds, t = [], 0
    while any(queues):
        rnd = []
        for m in range(nmembers):
            if queues[m] and t >= m % 4 and (t + m) % 5 != 0:       # staggered starts, a round out of five sat out
                rnd.append(queues[m].pop(0))
        if rnd:
            if t % 2:
                rnd.reverse()                                       # member lists in either order
            rounds.append(rnd)
        t += 1
    plan = Plan(members, cuts, rounds)
    c = counts(plan)
    assert len(members) == nmembers and all(1 <= len(s) <= 3 for s in members)
    assert all(n in lengths for segs in cuts for cut in segs for n in cut)
    if nmembers >= NMEMBERS:
        for k in ("opened_by_empty", "ended_by_empty", "one_chunk", "second_after_chunked", "mixed_rounds"):
            assert c[k] >= 3, (k, c[k])
    return plan


def simulate_decode(members, nmembers=None):
    """The calls that decode every segment of every member, and what each must report.  calls[t] = [Step, ...]."""
    nm = len(members) if nmembers is None else nmembers
    seg = [0] * nm
    done = [0] * nm                      # plaintext bytes of the current segment decoded so far
    opened = [False] * nm
    calls, t = [], 0
    while any(seg[m] < len(members[m]) for m in range(nm)):
        call = []
        for m in range(nm):
            if seg[m] >= len(members[m]):
                continue
            cap = DECODE_CAPS[(t + m) % len(DECODE_CAPS)]
            left = len(members[m][seg[m]]) - done[m]
            take = min(cap, left)
            still = left >= cap                                     # a full slab pauses, whether or not bytes remain
            call.append(Step(m, seg[m], cap, done[m], take, still, not opened[m], still and left == cap and cap > 0))
            opened[m] = still
            done[m] += take
            if not still:
                seg[m] += 1
                done[m] = 0
        calls.append(call)
        t += 1
        assert t < 4000
    return calls
