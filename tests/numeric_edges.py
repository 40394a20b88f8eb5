"""Which numeric edges of the predictor and the coder a corpus reaches, and a small corpus that reaches each of them.

census(header, segments, offsets) runs the pure-Python reference (oracle/pyref/zpaq_pyref.py) over one member's segments,
the model kept from segment to segment as in a block, and counts the events below.  It instruments by wrapping: clamp2k and
clamp512k are replaced for the run by counting wrappers that know the calling component from the order of the calls (a
model's components call them in a fixed order per predict / update), everything else is read from the predictor's state
before and after each predict and update.  predict and update themselves are pyref's.

Events (per component type where one applies; `hi` / `lo` = the top / bottom bound):
  w512.{mix,wt0,wt1}.{hi,lo}   a weight at clamp512k's bound (262143 / -262144) after an update
  w512.wt1.init.{hi,lo}        an ISSE's wt1 at the bound straight from Predictor.__init__
  c2k.{mix2,mix,isse_j,isse_n}.{hi,lo}   clamp2k changed its argument (isse_j: j < n, isse_n: j >= n)
  mix2.w0 / mix2.w65535        a MIX2 weight stored as 0 / 65535
  cm.limit, cm.p0, cm.p32767   count == limit != 0 at an update; cm >> 17 == 0 / 32767 at a predict
  sse.limit, sse.pq0, sse.pq1983, sse.row_in, sse.row_out
  states.{icm,isse}            number of distinct bit-history states written (of the 253 the table can reach)
  match.255_inc, match.255_rec, match.reset, match.wrap, match.skip
  squash.out                   the last component's stretch outside +-2047 going into squash (CONST 0 gives -2048)
  {enc,dec}.r16, .r8           range below 2^16 / 2^8 before a bit;  .s1 .. .s4: a bit shifted out 1 .. 4 bytes;
  {enc,dec}.low1               low << 8 == 0 replaced by 1 (seen as low == 1 after a shift; not the segment's first bit)
  wrap.cm                      the one i32 site of predict / update that really wraps, see below
  max.*                        largest operands at the sites where the kernels use __mul24

Wrap sites of predict / update (every i32(...) / u32(...) there), with the bound that keeps each from wrapping.  |p| <= 2048
(stretch gives +-2047, clamp2k -2048 .. 2047, CONST (c - 128) * 16 in -2048 .. 2032), |err| <= 32767 as y * 32767 - squash(.):
  CM     i32(cr.cxt), u32(h ^ hmap4): reinterpretations of a 32-bit context, no arithmetic.
         i32(err * DT[count]): DT[0] = 87380, 32767 * 87380 > 2^31: WRAPS when count == 0 and |err| > 24576, which needs
         a CM whose count stays 0 (limit 0) and a probability beyond 1/4 from the bit.  Counted as wrap.cm.  DT[1] = 52428:
         32767 * 52428 < 2^31, so no other count wraps.  u32(i32(pn) + upd + inc): the probability stays in 0 .. 2^32 - 1
         by construction of upd (|upd| <= distance to the end), a reinterpretation.
  ICM    u32(h + 16 * c8): context arithmetic mod 2^32 by definition.  u32(v + ((y * 32767 - (v >> 8)) >> 2)): v < 2^23.
  MATCH  i32(limit - b), i32(limit - cm): |.| < 2^32 differences of buffer positions, masked before use.
  AVG    i32(p[j] * wt + p[k] * (256 - wt)): 2048 * 256 < 2^31.
  MIX2   i32(w * p[j] + (65536 - w) * p[k]): 65536 * 2048 = 2^27.  i32((y * 32767 - squash) * rate): 32767 * 255 < 2^23.
         i32(err * (p[j] - p[k])): |err| <= 32767 * 255 >> 5 = 261119, |p[j] - p[k]| <= 4095: 261119 * 4095 + 2^12 < 2^31.
  MIX    i32(wt * p): |wt| = |w >> 8| <= 1024, 1024 * 2048 = 2^21 per input, at most 255 inputs: < 2^29.
         i32(err * p): |err| <= 32767 * 255 >> 4 = 522225 (rounded down), * 2048 + 2^12 < 2^31.  i32(w + ...): 2^18 + 2^17 < 2^31.
  ISSE   i32(wt0 * p[j]) + i32(wt1 * 64): 262144 * 2048 + 262144 * 64 = 2^29 + 2^24 < 2^31.
         i32(err * p[j]): 32767 * 2048 + 2^12 < 2^26.  i32(w + ...): 2^18 + 2^13 < 2^31.
  SSE    u32((h + c8) * 32), i32(cxt) + pq: context arithmetic mod 2^32 by definition; the row test catches what falls outside.
         i32(p1 * (64 - wt) + p2 * wt): p < 2^22, * 64 = 2^28.  i32(err * (limit - count)): 32767 * 1020 + 2^12 < 2^25.
The kernels use __mul24 (operands must fit 24 bits signed) on the ISSE's products only: w0 * pin in predict (|w0| <= 2^18 by
clamp512k, |pin| <= 2^11), err * pin in update (zpq_chain.hip states |err| < 2^15, |pin| <= 2^11), and the a * pin forms of
zpq_dpipe.hip (a is a w0).  The census records max.isse.err and max.isse.pin (and, for the same sites of MIX and MIX2, which
the kernels multiply in 32 bits, max.mix.err, max.mix.pin, max.mix2.err after the rate and the shift, max.mix2.pdiff): the
golden table shows 32767 and 2048 reached exactly and never exceeded; w0 is at +-2^18 wherever w512.wt0.* is counted.

What the suite reached before EDGE_CASES (tests/golden/numeric_edges_census.json, "old"; old_corpora() says what was counted
and what the pure-Python reference had to leave out):
  levels 1-2 on the ragged batch       no weight at a bound, no clamp2k, range below 2^16 69 times, no low = 1 repair
  chain_models.NAMED, ragged batch     wt1 at 262143 / -262144 70799 / 57479 times (wt0 never), range below 2^16 421, no repair
  block-set members on chain models    wt1 at the bounds 1304 / 1012 times, no repair
  general_models.NAMED (n <= 22)       every general-class event except an ISSE's wt0 at a bound and clamp2k on an ISSE output
  members_of on C4B                    MIX weights at both bounds, clamp2k on the MIX, no ISSE weight at a bound
So the weight bounds were reached on the chain kernels only by whichever named model met a long constant block, never on
the shipped levels' small inputs, and the repair of low never on a chain model.  "edge" / "edge_cases" in the same table are
the counts over EDGE_CASES: every required event at least FLOOR = 8 times per class (REQUIRED), each told by a pinned case
(TELLS), the sought events under SOUGHT / "sought".

EDGE_CASES: name -> Case(cls, header, offsets, segments, block).  segments: four of at most 1200 bytes, 4 KiB or less in all, the
model carried from one to the next (what a block set codes).  block: the same warm-up as one block of 4 KiB or less on a fresh
model with its own steered tail (what every kernel that codes independent blocks runs); "edge_blocks" in the table.
  chain class    two segments of a flip pattern (flips), one that goes on with fresh order-3 contexts (varied), one steered
                 (steer): levels 1 and 2 and chain_models' chains (the level 1 / 3 / 4 / 5 specialisations at small tables, the
                 runtime-loop kernels at 8 and 16 lanes, with and without the MIX2 tail).  The shipped levels 3 - 5 take l2's
                 bytes on the GPU (SHIPPED_BIG).
  general class  three segments of runs (runs) and a steered one on nine small models: g_all holds every component type, the
                 others keep the path from one edge to the coder short, because most models saturate behind a weight at its
                 bound and then tell nothing.  Each also stands behind `a=a` + the hash chain (<name>_vm) for the
                 interpreter-wave kernels.
The data come from seeded generators; the steered segments are steer()'s output, committed as
tests/golden/numeric_edges_steered.json (write_steered() regenerates it).  The flip pattern, the run lengths and the small
models are the result of searches on the census counts and on the mutants (random small models over fixed data, seeded);
the searches are not committed, only what they found.
"""
import collections
import contextlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "pyref"))
import zpaq_pyref as P  # noqa: E402

import chain_models as CMD  # noqa: E402
import general_models as GM  # noqa: E402

HI512, LO512 = 262143, -262144
CM_T, ICM_T, MATCH_T, AVG_T, MIX2_T, MIX_T, ISSE_T, SSE_T = 2, 3, 4, 5, 6, 7, 8, 9


# ---------------------------------------------------------------- patching pyref for the duration of a run
@contextlib.contextmanager
def patched(**names):
    """pyref's module-level functions / constants replaced for the duration (the suite's mutants are built this way)."""
    old = {k: getattr(P, k) for k in names}
    try:
        for k, v in names.items():
            setattr(P, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(P, k, v)


def schedules(pr):
    """The order in which a model's components call clamp2k in predict and clamp512k in update: [(component, site)]."""
    n = len(pr.comp)
    pred, upd = [], []
    for i, cr in enumerate(pr.comp):
        t = cr.ctype
        if t == MIX2_T and cr.cm[0] < n and cr.cm[1] < n:
            pred.append((i, "mix2"))
        elif t == MIX_T:
            pred.append((i, "mix"))
            upd += [(i, "mix")] * max(0, min(cr.limit, n - cr.b))
        elif t == ISSE_T:
            pred.append((i, "isse_j" if cr.b < n else "isse_n"))
            if cr.b < n:
                upd += [(i, "wt0"), (i, "wt1")]
    return pred, upd


class Census:
    """Counts events while pyref codes; see the module docstring.  first[event] = (segment, bit index in the segment)."""

    def __init__(self):
        self.n = collections.Counter()
        self.first = {}
        self.segs = collections.defaultdict(set)           # event -> the segments it occurred in
        self.max = collections.Counter()
        self.states = {"icm": set(), "isse": set()}
        self.range2k = {}                                  # site -> [least, largest] argument of clamp2k (for searches)
        self.seg = 0
        self.bit = 0
        self.phase = None
        self.k = 0

    def hit(self, ev, count=1):
        self.n[ev] += count
        self.first.setdefault(ev, (self.seg, self.bit))
        self.segs[ev].add(self.seg)

    def top(self, name, v):
        if abs(v) > self.max[name]:
            self.max[name] = abs(v)

    # -- wrappers around pyref's clamps (the true functions are kept in self.true2k / self.true512k)
    def clamp2k(self, x):
        r = self.true2k(x)
        if self.phase == "predict":
            site = self.sched_p[self.k][1]
            self.k += 1
            lohi = self.range2k.setdefault(site, [x, x])
            lohi[0], lohi[1] = min(lohi[0], x), max(lohi[1], x)
            if x > 2047:
                self.hit("c2k.%s.hi" % site)
            elif x < -2048:
                self.hit("c2k.%s.lo" % site)
        return r

    def clamp512k(self, x):
        r = self.true512k(x)
        if self.phase == "update":
            site = self.sched_u[self.k][1]
            self.k += 1
            if r == HI512:
                self.hit("w512.%s.hi" % site)
            elif r == LO512:
                self.hit("w512.%s.lo" % site)
        return r

    # -- state reading around predict / update
    def after_init(self, pr):
        self.sched_p, self.sched_u = schedules(pr)
        for cr in pr.comp:
            if cr.ctype == ISSE_T:
                for k in range(256):
                    w = P.i32(cr.cm[2 * k + 1])
                    if w == HI512:
                        self.hit("w512.wt1.init.hi")
                    elif w == LO512:
                        self.hit("w512.wt1.init.lo")

    def predict(self, pr):
        old = list(pr.p)
        self.phase, self.k = "predict", 0
        p = self.true_predict(pr)
        self.phase = None
        assert self.k == len(self.sched_p)
        n = len(pr.comp)
        for i, cr in enumerate(pr.comp):
            t = cr.ctype
            if t == CM_T:
                v = cr.cm[P.i32(cr.cxt) & (len(cr.cm) - 1)] >> 17
                if v == 0:
                    self.hit("cm.p0")
                elif v == 32767:
                    self.hit("cm.p32767")
            elif t == SSE_T:
                j = cr.b
                pq = 992
                if j < n:
                    pq = (pr.p[j] if j < i else old[j]) + 992
                if pq < P.SSE_PQ_MIN:
                    self.hit("sse.pq0")
                    pq = P.SSE_PQ_MIN
                if pq > P.SSE_PQ_MAX:
                    self.hit("sse.pq1983")
                    pq = P.SSE_PQ_MAX
                idx = P.i32(P.i32(P.u32((pr.h[i] + pr.c8) * 32)) + (pq >> 6))
                self.hit("sse.row_in" if idx >= 0 and P.i32(idx + 1) < len(cr.cm) else "sse.row_out")
        if n and not -2047 <= pr.p[n - 1] <= 2047:
            self.hit("squash.out")
        return p

    def update(self, pr, y):
        n = len(pr.comp)
        pre = []
        for i, cr in enumerate(pr.comp):
            t = cr.ctype
            if t == CM_T:
                pn = cr.cm[P.i32(cr.cxt) & (len(cr.cm) - 1)]
                count = pn & 0x3ff
                if cr.limit and count == cr.limit:
                    self.hit("cm.limit")
                if abs((y * 32767 - (pn >> 17)) * P.DT[count]) >= 1 << 31:
                    self.hit("wrap.cm")
                pre.append(None)
            elif t == SSE_T:
                v = cr.cm[P.i32(cr.cxt) & (len(cr.cm) - 1)]
                if (P.i32(v) & 1023) == cr.limit:
                    self.hit("sse.limit")
                pre.append(None)
            elif t in (ICM_T, ISSE_T):
                pre.append(cr.c + (pr.hmap4 & 15))
                if t == ISSE_T and cr.b < n:
                    self.top("max.isse.err", y * 32767 - P.squash(pr.p[i]))
                    self.top("max.isse.pin", pr.p[cr.b])
            elif t == MATCH_T:
                pre.append((cr.a, cr.c, cr.cxt, cr.limit))
            elif t == MIX2_T:
                pre.append(None)
                j, k = cr.cm[0], cr.cm[1]
                if j < n and k < n:
                    self.top("max.mix2.err", P.i32((y * 32767 - P.squash(pr.p[i])) * cr.cm[2]) >> 5)
                    self.top("max.mix2.pdiff", pr.p[j] - pr.p[k])
            elif t == MIX_T:
                pre.append(None)
                self.top("max.mix.err", P.i32((y * 32767 - P.squash(pr.p[i])) * cr.ht[0]) >> 4)
                for l in range(max(0, min(cr.limit, n - cr.b))):
                    self.top("max.mix.pin", pr.p[cr.b + l])
            else:
                pre.append(None)
        self.phase, self.k = "update", 0
        self.true_update(pr, y)
        self.phase = None
        assert self.k == len(self.sched_u)
        for i, cr in enumerate(pr.comp):
            t = cr.ctype
            if t == ICM_T:
                self.states["icm"].add(cr.ht[pre[i]])
            elif t == ISSE_T:
                self.states["isse"].add(cr.ht[pre[i]])
            elif t == MIX2_T and cr.cm[0] < n and cr.cm[1] < n:
                w = cr.a16[cr.cxt]
                if w == 0:
                    self.hit("mix2.w0")
                elif w == 65535:
                    self.hit("mix2.w65535")
            elif t == MATCH_T:
                a0, c0, cxt0, lim0 = pre[i]
                if a0 > 0 and c0 != y:
                    self.hit("match.reset")
                    a0 = 0
                if cxt0 == 7:
                    if cr.limit == 0 and lim0 != 0:
                        self.hit("match.wrap")
                    if a0 == 0:
                        if (cr.b & (len(cr.ht) - 1)) == 0:
                            self.hit("match.skip")
                        elif cr.a == 255:
                            self.hit("match.255_rec")
                    elif a0 < 255 and cr.a == 255:
                        self.hit("match.255_inc")
        self.bit += 1

    def coder(self, who, true, coder, *args):
        """Encoder.encode(y, p) / Decoder.decode(p): the range before the bit, the bytes shifted out by it, and whether one
        of those shifts left low == 0 (replayed from the interval after the bit: low is shifted as often as bytes went)."""
        low, high = coder.low, coder.high
        rng = P.u32(high - low)
        before = len(coder.out) if who == "enc" else coder.shifts
        r = true(coder, *args)
        shifted = (len(coder.out) if who == "enc" else coder.shifts) - before
        if rng < 1 << 16:
            self.hit(who + ".r16")
        if rng < 1 << 8:
            self.hit(who + ".r8")
        if shifted:
            self.hit("%s.s%d" % (who, shifted))
            y, p = (args[0], args[1]) if who == "enc" else (r, args[0])
            if y == 0:
                low = P.u32(low + ((rng * min(max(p, 0), 65535)) >> 16) + 1)
            for _ in range(shifted):
                low = P.u32(low << 8)
                if low == 0:
                    low = 1
                    if not (p == 0 and y == 1):            # (not the end-of-segment bit: nothing is coded after it)
                        self.hit(who + ".low1")
            assert low == coder.low
        return r

    def table(self):
        out = dict(self.n)
        out["states.icm"] = len(self.states["icm"])
        out["states.isse"] = len(self.states["isse"])
        out.update(self.max)
        return out


REACHABLE_STATES = None


def reachable_states():
    """How many bit-history states ns can reach from 0 (what states.icm / states.isse are out of)."""
    global REACHABLE_STATES
    if REACHABLE_STATES is None:
        seen, todo = {0}, [0]
        while todo:
            s = todo.pop()
            for y in (0, 1):
                t = P.ns_next(s, y)
                if t not in seen:
                    seen.add(t)
                    todo.append(t)
        REACHABLE_STATES = len(seen)
    return REACHABLE_STATES


class _CountingDecoder(P.Decoder):
    shifts = -4                                            # (the four bytes the constructor reads are no bit's)

    def _shift(self):
        self.shifts += 1
        P.Decoder._shift(self)


def run(header, segments, offsets=None, pp=True, cs=None, decode=True, prepare=None, between=None, until=None):
    """pyref over one member's segments, state kept between them.  Returns (coded segments, Census or None).  cs: a Census
    to count into (None: no instrumentation, for mutants).  prepare(pr): changes the fresh Predictor (a mutant's limits);
    between(pr, s): called before segment s >= 1 (a mutant that drops state at the boundary).  until: the true coded
    segments; a mutant's run ends with the first segment that differs from them."""
    if cs is None:
        pr = P.new_model(header, offsets)
        if prepare:
            prepare(pr)
        coded = []
        for s, seg in enumerate(segments):
            if s and between:
                between(pr, s)
            coded.append(P.encode_segment(pr, seg, pp=pp))
            if until is not None and coded[s] != until[s]:
                break
        return coded, None

    cs.true2k, cs.true512k = P.clamp2k, P.clamp512k
    cs.true_predict, cs.true_update = P.Predictor.predict, P.Predictor.update
    true_enc, true_dec = P.Encoder.encode, P.Decoder.decode
    with patched(clamp2k=cs.clamp2k, clamp512k=cs.clamp512k):
        pr = P.new_model(header, offsets)
    cs.after_init(pr)
    pr.predict = lambda: cs.predict(pr)
    pr.update = lambda y: cs.update(pr, y)
    coded = []
    with patched(clamp2k=cs.clamp2k, clamp512k=cs.clamp512k):
        P.Encoder.encode = lambda e, y, p: cs.coder("enc", true_enc, e, y, p)
        try:
            for s, seg in enumerate(segments):
                cs.seg, cs.bit = s, 0
                coded.append(P.encode_segment(pr, seg, pp=pp))
                if until is not None and coded[s] != until[s]:
                    break
        finally:
            P.Encoder.encode = true_enc
    if decode:                                             # the decoder's coder events, on a model of its own, uncounted
        pr2 = P.new_model(header, offsets)
        P.Decoder.decode = lambda d, p: cs.coder("dec", true_dec, d, p)
        try:
            for s, (seg, c) in enumerate(zip(segments, coded)):
                cs.seg, cs.bit = s, 0
                pr2.reset()
                d = _CountingDecoder(pr2, c)
                out = bytearray()
                while True:
                    ch = d.decompress()
                    if ch < 0:
                        break
                    out.append(ch)
                assert bytes(out) == (b"\0" if pp else b"") + bytes(seg) and d.pos == len(c)
        finally:
            P.Decoder.decode = true_dec
    return coded, cs


def census(header, segments, offsets=None, pp=True, decode=True):
    """{event: count} of one member (see the module docstring), with "first" = {event: [segment, bit]}."""
    coded, cs = run(header, segments, offsets, pp, Census(), decode)
    out = cs.table()
    out["first"] = {k: list(v) for k, v in cs.first.items()}
    out["segs"] = {k: sorted(v) for k, v in cs.segs.items()}
    out["coded"] = coded
    return out


def merge(total, one):
    """Adds one census to a running table: counts add, max.* and states.* take the maximum."""
    for k, v in one.items():
        if k in ("first", "coded", "segs", "hash"):
            continue
        if k.startswith("max.") or k.startswith("states."):
            total[k] = max(total.get(k, 0), v)
        else:
            total[k] = total.get(k, 0) + v
    return total


# ---------------------------------------------------------------- data that steers the coder
def steer(header, offsets, warm, nbytes, goals=("low1", "s2", "low1", "s3"), pp=True, prefix=b""):
    """`nbytes` bytes for a segment that follows the segments `warm`, chosen bit by bit from the reference's own
    predictions so that the coder's interval keeps straddling a multiple B of 2^24 while it narrows (no byte can be shifted
    out, so the range falls below 2^16 and 2^8), and then leaves the straddle the way the current goal asks:
      "low1"  at the last step, where mid == B - 1, code a 0: low becomes B, B << 8 == 0, the repair sets low = 1
      "s2"    leave as soon as the range is below 2^16: the two top bytes agree, two bytes are shifted out (or three)
      "s3"    leave once the range is below 2^8
    The goals are taken in turn.  A deterministic construction, no search: the same bytes on every machine."""
    pr = P.new_model(header, offsets)
    for seg in warm:
        P.encode_segment(pr, seg, pp=pp)
    pr.reset()
    e = P.Encoder(pr)
    if pp:
        e.compress(0)
    for b in prefix:                                       # (the same segment's bytes before the steered ones)
        e.compress(b)
    out, g = bytearray(), 0
    for _ in range(nbytes):
        e.encode(0, 0)
        c = 0
        for _ in range(8):
            p16 = pr.predict() * 2 + 1
            low, high = e.low, e.high
            rng = P.u32(high - low)
            edge = ((low >> 24) + 1) << 24
            mid = low + ((rng * p16) >> 16)
            if edge > high:                                # (no multiple of 2^24 inside: cannot happen after a shift)
                y = 1 if p16 >= 32768 else 0
            elif mid >= edge:
                y = 1
            elif mid <= edge - 2:
                y = 0
            else:
                y = 0 if goals[g % len(goals)] == "low1" else 1
                g += 1
            if edge <= high and mid != edge - 1:
                goal = goals[g % len(goals)]
                if (goal == "s2" and rng < 1 << 16) or (goal == "s3" and rng < 1 << 8):
                    y ^= 1
                    g += 1
            e.encode(y, p16)
            pr.update(y)
            c = (c << 1) | y
        out.append(c)
    return bytes(out)


# ---------------------------------------------------------------- mutants: the reference with one edge moved by one
class SiteMutant(Census):
    """A Census whose clamp at one site (see schedules) has one bound moved by one; it counts nothing of interest."""

    def __init__(self, fn, site, hi, wrap=False):
        Census.__init__(self)
        self.fn, self.site, self.hi, self.wrap = fn, site, hi, wrap

    def _moved(self, true, x, sched, lo_b, hi_b):
        site = sched[self.k][1]
        self.k += 1
        if site != self.site:
            return true(x)
        if self.wrap:                                      # a packed field one bit too narrow: the bound comes back wrapped
            r = true(x)
            return r - (hi_b + 1) if self.hi and r == hi_b else (0 if not self.hi and r == lo_b else r)
        if self.hi:
            return hi_b - 1 if x > hi_b - 1 else true(x)
        return lo_b + 1 if x < lo_b + 1 else true(x)

    def clamp2k(self, x):
        if self.fn != "clamp2k" or self.phase != "predict":
            return Census.clamp2k(self, x)
        return self._moved(self.true2k, x, self.sched_p, -2048, 2047)

    def clamp512k(self, x):
        if self.fn != "clamp512k" or self.phase != "update":
            return Census.clamp512k(self, x)
        return self._moved(self.true512k, x, self.sched_u, LO512, HI512)


def _stretch_mutant(at):
    true = P.stretch

    def stretch(p):                                        # 0: the entry below the clamp (a stretch without its idx < 1 test);
        if p == at:                                        # 32767: the table's neighbour.  (Entries 1 and 2 are equal: the
            return P.STRETCH[0 if at == 0 else 32766]      # reference's ln series is cut off there.)
        return true(p)
    return stretch


def _squash_mutant(d):
    """squash whose lower clamp takes -2048 to entry 1 instead of entry 0 (entries 0 and 1 differ in no shipped table, so the
    mutant moves the value itself: one more than the true table's)."""
    idx = P.i32(d + 2047)
    if idx < 0:
        return P.SQUASH[0] + 1
    if idx >= 4094:
        idx = 4093
    return P.SQUASH[idx]


def _encode_mutant(kind):
    """Encoder.encode with one thing wrong: "r16": the probability is one unit off while the range is below 2^16;
    "s2": at most one byte is shifted out per bit (the rest waits for the next bit)."""
    def encode(self, y, p):
        pr = 0 if p < 0 else (65535 if p > 65535 else p)
        rng = P.u32(self.high - self.low)
        if kind == "r16" and rng < 1 << 16 and pr:
            pr ^= 2
        mid = P.u32(self.low + ((rng * pr) >> 16))
        if y != 0:
            self.high = mid
        else:
            self.low = P.u32(mid + 1)
        shifts = 0
        while (self.high ^ self.low) < 0x1000000 and not (kind == "s2" and shifts == 1 and pr):
            self.out.append(self.high >> 24)
            self.low = P.u32(self.low << 8)
            self.high = P.u32(self.high << 8) | 0xFF
            if self.low == 0:
                self.low = P.LOW_REPAIR
            shifts += 1
    return encode


def _limits(ctype):
    def prepare(pr):
        for cr in pr.comp:
            if cr.ctype == ctype and cr.limit:
                cr.limit -= 1
    return prepare


def _sse_rows(more):
    """more: every SSE table four times as long (rows beyond the true table exist); else: every entry's probability moved."""
    def prepare(pr):
        for cr in pr.comp:
            if cr.ctype == SSE_T:
                cr.cm = cr.cm * 4 if more else [P.u32(v ^ (1 << 24)) for v in cr.cm]
    return prepare


def _match_buffer(pr):
    for cr in pr.comp:
        if cr.ctype == MATCH_T:
            cr.ht = bytearray(2 * len(cr.ht))


def _fresh(types):
    """between(): the components of these types as a new model has them (a KEEP form that lost them at the boundary)."""
    def between(pr, s):
        new = P.new_model(pr.z.header, (pr.z.cend, pr.z.hbegin, pr.z.hend))
        for cr, nr in zip(pr.comp, new.comp):
            if cr.ctype in types:
                cr.cm, cr.a16 = nr.cm, nr.a16
    return between


# event -> how its mutant is built: ("site", function, site, hi) | ("const", name, value) | ("fn", name, function)
# | ("prepare", function) | ("encode", kind)
MUTANTS = {
    "w512.mix.hi": ("site", "clamp512k", "mix", True), "w512.mix.lo": ("site", "clamp512k", "mix", False),
    "w512.wt0.hi": ("site", "clamp512k", "wt0", True), "w512.wt0.lo": ("site", "clamp512k", "wt0", False),
    "w512.wt1.hi": ("site", "clamp512k", "wt1", True), "w512.wt1.lo": ("site", "clamp512k", "wt1", False),
    "c2k.mix.hi": ("site", "clamp2k", "mix", True), "c2k.mix.lo": ("site", "clamp2k", "mix", False),
    "c2k.isse_j.hi": ("site", "clamp2k", "isse_j", True), "c2k.isse_j.lo": ("site", "clamp2k", "isse_j", False),
    "mix2.w0": ("const", "MIX2_W_MIN", 1), "mix2.w65535": ("const", "MIX2_W_MAX", 65534),
    "cm.limit": ("prepare", _limits(CM_T)), "sse.limit": ("prepare", _limits(SSE_T)),
    "cm.p0": ("fn", "stretch", _stretch_mutant(0)), "cm.p32767": ("fn", "stretch", _stretch_mutant(32767)),
    # (MATCH_MAX_LEN = 254 changes no byte of any input: the length only indexes DT2K, and DT2K[254] == DT2K[255]; a length
    # that is not stopped at 255 indexes DT2K[256 & 255] = 0 on the next byte.)
    "match.255_inc": ("const", "MATCH_MAX_LEN", 256), "match.reset": ("const", "MATCH_RESET_LEN", 1),
    "match.wrap": ("prepare", _match_buffer),
    "sse.pq0": ("const", "SSE_PQ_MIN", 1), "sse.pq1983": ("const", "SSE_PQ_MAX", 1982),
    "sse.row_in": ("prepare", _sse_rows(False)), "sse.row_out": ("prepare", _sse_rows(True)),
    "squash.out": ("fn", "squash", _squash_mutant),
    "enc.r16": ("encode", "r16"), "enc.s2": ("encode", "s2"), "enc.low1": ("const", "LOW_REPAIR", 0),
}
RESETS = {"mix": (MIX_T,), "wt0": (ISSE_T,), "wt1": (ISSE_T,)}       # w512.<site>: what a lost state would reset


def mutant_coded(case, event, reset=False, until=None, block=False, wrap=False):
    """The coded segments of `case` (block: its block form, one segment) from the reference with `event`'s edge moved by one; reset: from the true reference
    that loses the event's component state at every segment boundary instead."""
    a = (case.header, [case.block] if block else case.segments, case.offsets)
    if wrap:                                               # (the weight at the bound as a 19-bit field would hold it: -1 / 0)
        m = MUTANTS[event]
        return run(*a, cs=SiteMutant(*m[1:], wrap=True), decode=False, until=until)[0]
    if reset:
        return run(*a, between=_fresh(RESETS[event.split(".")[1]]), until=until)[0]
    m = MUTANTS[event]
    if m[0] == "site":
        return run(*a, cs=SiteMutant(*m[1:]), decode=False, until=until)[0]
    if m[0] == "const":
        with patched(**{m[1]: m[2]}):
            return run(*a, until=until)[0]
    if m[0] == "fn":
        with patched(**{m[1]: m[2]}):
            return run(*a, until=until)[0]
    if m[0] == "prepare":
        return run(*a, prepare=m[1], until=until)[0]
    true = P.Encoder.encode
    P.Encoder.encode = _encode_mutant(m[1])
    try:
        return run(*a, until=until)[0]
    finally:
        P.Encoder.encode = true


# ---------------------------------------------------------------- the edge corpus
Case = collections.namedtuple("Case", "cls header offsets segments block")
GOLDEN = os.path.join(ROOT, "tests", "golden")
STEERED_JSON = os.path.join(GOLDEN, "numeric_edges_steered.json")
_STEERED = None
# write_steered() alone computes; everyone else reads the file.  (NUMERIC_EDGES_GENERATE=1 in the environment: the first
# generation, when the file does not yet hold what the import needs.)
_GENERATE = os.environ.get("NUMERIC_EDGES_GENERATE") == "1"
BLOCK_STEER = 500                                         # steered bytes at the end of a case's block form
SEG, STEER_BYTES = 1200, 600                              # (a block set's decode slab in test_gpu_blockset.py takes 1500)


def steered(name, header, offsets, warm, prefix=b"", nbytes=STEER_BYTES):
    """A case's steered bytes: steer()'s result as committed in tests/golden/numeric_edges_steered.json under `name` (the CPU
    test regenerates every one of them).  A missing file or name is an error."""
    global _STEERED
    if _GENERATE:
        return steer(header, offsets, warm, nbytes, prefix=prefix)
    if _STEERED is None:
        import json
        _STEERED = json.load(open(STEERED_JSON))
    return bytes.fromhex(_STEERED[name])


def flips(pattern, n):
    """`pattern` repeated to n bytes.  With b"a\\xffa\\x00" the order-1 context `a` is followed by 0xff and 0x00 in turn (the ICM
    stays undecided), the order-2 contexts are deterministic: the first ISSE's bias weights wt1 of the two deterministic
    bit-history states walk to 262143 and -262144 within 1.8 KiB (found by trying periods and alphabets; level 1 hashes two
    more bytes, hence its longer pattern)."""
    return (pattern * (n // len(pattern) + 1))[:n]


def varied(seed, n, a=0x61):
    """R 00 a ff S ff a 00 with seeded random R, S: the order-2 contexts of the flip pattern go on (the weights at the bound
    are used), the order-3 contexts are new every time, so the next component starts from its initial weights and the
    last prediction is far from saturated: a weight one off shows in the coded bytes."""
    r = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += bytes([r.randrange(256), 0, a, 0xff, r.randrange(256), 0xff, a, 0])
    return bytes(out[:n])


def runs(seed, n):
    """Runs of 0x00 and 0xff, the flip pattern and four-symbol noise, 300 bytes each in a seeded order: constant runs drive
    the CONST-fed mixers' weights to both clamp512k bounds and the MATCH length to 255, the noise resets it."""
    r = random.Random(seed)
    parts = [bytes(300), b"\xff" * 300, flips(b"a\xffa\x00", 300), bytes(r.choice(b"ab\x00\xff") for _ in range(300))]
    r.shuffle(parts)
    return b"".join(parts)[:n]


G = GM
# every required general-class event in one model of fourteen components (the most the interpreter-wave kernels take): CONST inputs
# that are always wrong on one kind of run, a CM that saturates, a rate-255 MIX feeding an ISSE, a MATCH with a long buffer and
# one with an 8-byte buffer under a slow MIX of their own, a MIX2 between the two CONSTs with a weight per partial byte (each
# weight runs to 0 or to 65535 and stays), an SSE fed by it whose context stays 0 (eight hash links: its rows are c8 * 32,
# inside a 5-bit table for c8 < 32 only), AVGs that bring every branch to the last component, and a second such SSE as the
# last component.  (squash's table is the wrong way round beyond +-1280, the reference's quirk: a model whose last
# component saturates there codes every bit at its worst and tells nothing about the components before it; an SSE maps the
# saturated input back.)
EDGE_GENERAL = [[G.CONST, 255], [G.CONST, 0], [G.CM, 4, 1], [G.ICM, 6], [G.MIX, 0, 0, 4, 255, 0], [G.ISSE, 6, 4],
                [G.MATCH, 6, 10], [G.MATCH, 2, 3], [G.MIX2, 8, 0, 1, 255, 255], [G.SSE, 5, 8, 0, 1], [G.MIX, 0, 6, 2, 4, 0],
                [G.AVG, 5, 9, 128], [G.AVG, 11, 10, 128], [G.SSE, 5, 12, 0, 255]]
# the ISSE's own edges with little else around: CONST 0, a CM, a rate-255 MIX over both, the ISSE fed by the MIX.  As the
# last component it feeds squash -2048.  With an AVG against a CONST behind it the clamped value lands where squash is steep
# and the division by 256 tells 2047 from 2046 (CONST 88: (2047 * 65 - 640 * 191) >> 8 = 42, one less for 2046) and -2048 from
# -2047 (CONST 164: (-2048 * 65 + 576 * 191) >> 8 = -91, one more for -2047).
EDGE_ISSE = [[G.CONST, 0], [G.CM, 4, 4], [G.MIX, 0, 0, 2, 255, 0], [G.ISSE, 8, 2]]
EDGE_ISSE_HI = EDGE_ISSE + [[G.CONST, 88], [G.AVG, 3, 4, 65]]
EDGE_ISSE_LO = EDGE_ISSE + [[G.CONST, 164], [G.AVG, 3, 4, 65]]
# found by a seeded random search over small models for ones whose coded bytes tell a weight at the bound from one moved by
# one (most models saturate behind such a weight): (components, hash links)
EDGE_SMALL = {
    "g_w1": ([[G.CM, 8, 1], [G.CM, 4, 255], [G.MIX2, 8, 0, 1, 255, 255], [G.ISSE, 8, 2], [G.SSE, 5, 3, 32, 1]], 4),
    "g_w2": ([[G.CONST, 64], [G.CONST, 192], [G.CM, 0, 255], [G.MIX, 8, 0, 3, 4, 0], [G.ISSE, 4, 3]], 5),
    "g_sse": ([[G.CM, 8, 1], [G.CONST, 74], [G.MIX, 8, 0, 2, 24, 255], [G.SSE, 5, 2, 0, 4], [G.SSE, 5, 3, 0, 255]], 2),
    "g_w3": ([[G.CONST, 206], [G.CONST, 64], [G.CM, 8, 4], [G.MIX, 4, 0, 3, 100, 0], [G.SSE, 5, 3, 32, 255]], 3),
    "g_cm": ([[G.CM, 4, 1]], 1),                          # a CM alone: its probability of 0 goes straight to the coder
}


def _vm(hdr):
    """The same components behind `a=a` and the same hash chain: the same contexts from a program no recogniser takes."""
    return G.H(G.components(hdr), hdr[0], hdr[1], [64] + G.program_of(hdr))


def _case(name, cls, header, pattern=None, seeds=None, offsets=None, order=(0, 1, 2)):
    if pattern is not None:
        segs = [flips(pattern, SEG), flips(pattern, SEG), varied(7, SEG // 2) if len(pattern) == 4 else flips(pattern, SEG // 2)]
    else:
        segs = [runs(s, SEG - 50) for s in seeds]
    segs.append(steered(name, header, offsets, segs))
    assert sum(len(s) for s in segs) <= 4096
    # The block form, for kernels that code independent blocks (a fresh model, one coder from the first byte to the last): the
    # same warm-up as ONE block, long enough for the weights to arrive at their bounds and to be used there, then bytes steered
    # for exactly that coder state.  (The segments' steered bytes steer nothing here: the coder is in another state.)
    if pattern is None:
        pre = b"".join(segs[i] for i in order)
    elif len(pattern) == 4:
        pre = flips(pattern, 2000) + varied(7, 1500)
    else:
        pre = flips(pattern, 3500)
    block = pre + steered(name + "/block", header, offsets, [], prefix=pre, nbytes=BLOCK_STEER)
    assert len(block) <= 4096
    return Case(cls, header, offsets, segs, block)


def _build():
    flip, flip1 = b"a\xffa\x00", b"aaa\xffaaa\x00"
    cases = {"l1": _case("l1", "chain", P.level_header(1), flip1), "l2": _case("l2", "chain", P.level_header(2), flip)}
    # chain_models' chains: the level-1 / 3 / 4 / 5 specialisations at small tables, the runtime-loop kernels at 8 and 16 lanes,
    # with and without the MIX2 tail
    for name in ("l1_sizes", "l3_mixed", "l4_rate255", "l5_small", "chain7", "chain9", "mix2_chain3", "chain15_mix2"):
        cases[name] = _case(name, "chain", CMD.NAMED[name][0], flip1 if name == "l1_sizes" else flip)
    g = G.H(EDGE_GENERAL, 3, 8, CMD.hashchain(8))
    i = G.H(EDGE_ISSE, 3, 8, CMD.hashchain(4))
    cases["g_all"] = _case("g_all", "general", g, seeds=(1, 2, 3))
    cases["g_isse"] = _case("g_isse", "general", i, seeds=(4, 5, 6))
    cases["g_isse_hi"] = _case("g_isse_hi", "general", G.H(EDGE_ISSE_HI, 3, 8, CMD.hashchain(4)), seeds=(4, 5, 6))
    cases["g_isse_lo"] = _case("g_isse_lo", "general", G.H(EDGE_ISSE_LO, 3, 8, CMD.hashchain(4)), seeds=(4, 5, 6))
    for name, (comps, links) in EDGE_SMALL.items():
        # (g_w1's block takes the runs in another order: that one tells its MIX2 weight at 65535 from 65534)
        cases[name] = _case(name, "general", G.H(comps, 3, 8, CMD.hashchain(links)), seeds=(1, 2, 3),
                            order=(1, 0, 2) if name == "g_w1" else (0, 1, 2))
    for name in [n for n, c in cases.items() if c.cls == "general"]:               # (the same bytes: the same contexts)
        cases[name + "_vm"] = Case("general", _vm(cases[name].header), None, cases[name].segments, cases[name].block)
    return cases


EDGE_CASES = _build()
# the shipped levels 3 - 5 take l2's segments on the GPU (their tables, 2^18 .. 2^22 slots of 64 bytes per component, are
# beyond what the pure-Python census can hold; the first ISSE sees the same contexts at every level)
SHIPPED_BIG = (3, 4, 5)


def write_steered(path=STEERED_JSON):
    """Regenerates tests/golden/numeric_edges_steered.json (run by hand when a case's model or warm-up changes)."""
    import json
    global _GENERATE, _STEERED
    _GENERATE = True
    try:
        out = {}
        for name, c in _build().items():
            if not name.endswith("_vm"):
                out[name] = c.segments[-1].hex()
                out[name + "/block"] = c.block[-BLOCK_STEER:].hex()
    finally:
        _GENERATE = False
    json.dump(out, open(path, "w"), indent=0, sort_keys=True)
    _STEERED = None


# ---------------------------------------------------------------- what the corpus must reach
# class -> {required event: the census events that count for it}.  "An ISSE weight" is wt0 or wt1.  clamp2k on a MIX2 output
# (asked for in the chain class) cannot change its argument: w * p[j] + (65536 - w) * p[k] with 0 <= w <= 65535 and both
# inputs in -2048 .. 2047 is a weighted mean times 65536, so after >> 16 it lies in -2048 .. 2047; c2k.mix2.* is 0 everywhere.
_BOTH = {"isse weight at 262143": ("w512.wt0.hi", "w512.wt1.hi"), "isse weight at -262144": ("w512.wt0.lo", "w512.wt1.lo"),
         "range below 2^16": ("enc.r16",), "2-byte shift": ("enc.s2",), "low = 1 repair": ("enc.low1",)}
_GENERAL = {e: (e,) for e in ("w512.mix.hi", "w512.mix.lo", "c2k.mix.hi", "c2k.mix.lo", "c2k.isse_j.hi", "c2k.isse_j.lo",
                              "mix2.w0", "mix2.w65535", "cm.limit", "cm.p0", "cm.p32767", "match.255_inc", "match.reset",
                              "match.wrap", "sse.limit", "sse.pq0", "sse.pq1983", "sse.row_in", "sse.row_out", "squash.out")}
REQUIRED = {"chain": dict(_BOTH), "general": dict(_BOTH, **_GENERAL)}
SOUGHT = ("enc.r8", "enc.s3", "w512.wt1.hi", "w512.wt1.lo", "match.255_rec", "wrap.cm")
FLOOR = 8

# (class, required event) -> the census event and the case pinned to tell its mutant (tests/test_numeric_edges_cpu.py)
TELLS = {
    ("chain", "isse weight at 262143"): ("w512.wt1.hi", "l1"), ("chain", "isse weight at -262144"): ("w512.wt1.lo", "l1"),
    ("chain", "range below 2^16"): ("enc.r16", "l2"), ("chain", "2-byte shift"): ("enc.s2", "l2"),
    ("chain", "low = 1 repair"): ("enc.low1", "l2"),
    ("general", "isse weight at 262143"): ("w512.wt0.hi", "g_w2"), ("general", "isse weight at -262144"): ("w512.wt1.lo", "g_w2"),
    ("general", "range below 2^16"): ("enc.r16", "g_w3"), ("general", "2-byte shift"): ("enc.s2", "g_cm"),
    ("general", "low = 1 repair"): ("enc.low1", "g_cm"),
    ("general", "w512.mix.hi"): ("w512.mix.hi", "g_w3"), ("general", "w512.mix.lo"): ("w512.mix.lo", "g_w3"),
    ("general", "c2k.mix.hi"): ("c2k.mix.hi", "g_isse"), ("general", "c2k.mix.lo"): ("c2k.mix.lo", "g_isse"),
    ("general", "c2k.isse_j.hi"): ("c2k.isse_j.hi", "g_isse_hi"), ("general", "c2k.isse_j.lo"): ("c2k.isse_j.lo", "g_isse_lo"),
    ("general", "mix2.w0"): ("mix2.w0", "g_w1"), ("general", "mix2.w65535"): ("mix2.w65535", "g_w1"),
    ("general", "cm.limit"): ("cm.limit", "g_cm"), ("general", "cm.p0"): ("cm.p0", "g_cm"),
    ("general", "cm.p32767"): ("cm.p32767", "g_cm"),
    ("general", "match.255_inc"): ("match.255_inc", "g_all"), ("general", "match.reset"): ("match.reset", "g_all"),
    ("general", "match.wrap"): ("match.wrap", "g_all"),
    ("general", "sse.limit"): ("sse.limit", "g_w3"), ("general", "sse.pq0"): ("sse.pq0", "g_w3"),
    ("general", "sse.pq1983"): ("sse.pq1983", "g_sse"), ("general", "sse.row_in"): ("sse.row_in", "g_w3"),
    ("general", "sse.row_out"): ("sse.row_out", "g_w3"), ("general", "squash.out"): ("squash.out", "g_isse"),
}
# the same for the block form; the top bound moved by one is told by one block per specialisation 2, 3, 5 and a runtime loop
BLOCK_TELLS = dict(TELLS)
BLOCK_TELLS["chain", "isse weight at 262143"] = ("w512.wt1.hi", "l2")
BLOCK_TELLS_TOP = ("l1", "l1_sizes", "l2", "l3_mixed", "mix2_chain3")
# the cases that stand in block sets, with the weight events a KEEP form has to carry over a segment boundary
_WT1 = ("w512.wt1.hi", "w512.wt1.lo")
SET_TELLS = {"l1": _WT1, "l2": _WT1, "l3_mixed": _WT1, "l4_rate255": _WT1, "l5_small": _WT1, "chain9": _WT1, "chain15_mix2": _WT1,
             "g_all": ("w512.mix.hi", "w512.mix.lo", "w512.wt0.hi", "w512.wt1.lo"), "g_w2": ("w512.mix.hi", "w512.wt0.hi", "w512.wt1.lo"),
             "g_w3": ("w512.mix.hi", "w512.mix.lo"), "g_w1": ("w512.wt0.hi", "w512.wt1.hi"), "g_isse": ("w512.mix.lo", "w512.wt0.hi")}


# ---------------------------------------------------------------- the census table (tests/golden/numeric_edges_census.json)
CENSUS_JSON = os.path.join(GOLDEN, "numeric_edges_census.json")
CHEAP_OLD = "chain: levels 1-2, ragged batch"             # the group of the old corpora the CPU test recomputes
CHEAP_EDGE = ("l2", "g_cm", "g_w3")                       # ... and the edge cases


def old_corpora():
    """(group, header, segments) for what the suite ran before EDGE_CASES: the ragged batches of the chain and general model
    tests without their blocks beyond 4 KiB, the block-set members, members_of on C4B.  Left out, because the pure-Python
    reference cannot hold or finish them: tables beyond 2^16 slots (the shipped levels 3 - 5, big_next_to_tiny), models of
    more than 22 components, and the 16 / 64 KiB blocks (the issue's probe of a 64 KiB periodic block stands for those)."""
    sys.path.insert(0, GOLDEN)
    import test_gpu_blockset as TB
    import test_gpu_chain_models as TC
    import test_gpu_general_models as TG
    import test_gpu_set_waves as TW
    from inputs import C4B
    sets = "sets: make_members, levels 1-2 and chain models"
    for lvl in (1, 2):
        for b in TC.ragged_blocks(lvl, big=False):
            yield CHEAP_OLD, P.level_header(lvl), [b]
        for segs in TB.make_members(1000 + lvl):
            yield sets, P.level_header(lvl), segs
    for name, (hdr, _) in CMD.NAMED.items():
        if max(CMD.table_bits(hdr)) <= 16:
            for b in TC.ragged_blocks(sum(name.encode()), big=False):
                yield "chain: chain_models.NAMED, ragged batch", hdr, [b]
    for k, name in enumerate(TB.NAMES):
        if max(CMD.table_bits(CMD.NAMED[name][0])) <= 16:
            for segs in TB.make_members(1000 + k + 10):
                yield sets, CMD.NAMED[name][0], segs
    for name, (hdr, _) in GM.NAMED.items():
        if hdr[4] <= 22 and name != "big_next_to_tiny":
            for b in TG.general_blocks(sum(name.encode()), big=False):
                yield "general: general_models.NAMED (n <= 22), ragged batch", hdr, [b]
    for segs in TW.members_of(41, 7):
        yield "sets: members_of(41, 7) on C4B", C4B, segs


EVENTS = tuple("w512.%s.%s" % (s, e) for s in ("mix", "wt0", "wt1", "wt1.init") for e in ("hi", "lo")) + tuple(
    "c2k.%s.%s" % (s, e) for s in ("mix2", "mix", "isse_j", "isse_n") for e in ("hi", "lo")) + (
    "mix2.w0", "mix2.w65535", "cm.limit", "cm.p0", "cm.p32767", "sse.limit", "sse.pq0", "sse.pq1983", "sse.row_in", "sse.row_out",
    "states.icm", "states.isse", "match.255_inc", "match.255_rec", "match.reset", "match.wrap", "match.skip", "squash.out",
    "wrap.cm") + tuple("%s.%s" % (w, e) for w in ("enc", "dec") for e in ("r16", "r8", "s1", "s2", "s3", "s4", "low1")) + (
    "max.isse.err", "max.isse.pin", "max.mix2.err", "max.mix2.pdiff", "max.mix.err", "max.mix.pin")


def zeros(t):
    """A census with every event of EVENTS listed, 0 where it never occurred."""
    return dict({e: 0 for e in EVENTS}, **t)


def case_hash(c):
    """What a case's counts in the table were computed from: header, offsets, segments and block."""
    import hashlib
    h = hashlib.sha256(repr((bytes(c.header), c.offsets, [bytes(s) for s in c.segments], bytes(c.block))).encode())
    return h.hexdigest()[:16]


def _count(job):
    group, hdr, segs, offs = job
    t = census(hdr, segs, offs) if any(len(s) for s in segs) else {}
    return group, zeros({k: v for k, v in t.items() if k not in ("coded", "first", "segs")}), t.get("first", {}), t.get("segs", {})


def old_table(only=None, pool=None):
    out = {}
    jobs = [(g, h, s, None) for g, h, s in old_corpora() if only is None or g == only]
    for g, t, _, _ in (pool.imap_unordered(_count, jobs, 4) if pool else map(_count, jobs)):
        merge(out.setdefault(g, {}), t)
    return out


def edge_table(names=None, pool=None, block=False):
    """{case: its census, with "first", "segs" and "hash"} for the edge cases as four segments, or (block) in their block form,
    which is what the kernels that code independent blocks run (the _vm cases code the same bytes: left out)."""
    names = [n for n in EDGE_CASES if not n.endswith("_vm")] if names is None else names
    jobs = [(n, EDGE_CASES[n].header, [EDGE_CASES[n].block] if block else EDGE_CASES[n].segments, EDGE_CASES[n].offsets) for n in names]
    return {n: dict(t, first=f, segs=s, hash=case_hash(EDGE_CASES[n])) for n, t, f, s in (pool.imap(_count, jobs) if pool else map(_count, jobs))}


SOUGHT_NOTES = {
    "match.255_rec": "not in EDGE_CASES (the old corpora reach it: constant runs against an 8-byte buffer jump to 255 inside the "
                     "recovery loop); tried in g_all: its short-buffer MATCH recovers onto the flip pattern and the noise, where the "
                     "loop stops at the first differing byte.",
    "wrap.cm": "not in EDGE_CASES: it needs a CM with limit 0, which the old general corpora have (cms() cycles through limit 0) and "
               "reach 416366 times; the edge models' CMs have limits of 1 and more so that cm.limit is reached.",
    "w512.wt0.lo": "never: wt0 falls only while the input's sign is wrong, and the steps shrink with the error; tried: ISSEs fed by "
                   "CONST 0 / CONST 255, by a rate-255 MIX and by a MIX2, runs of 0x00 / 0xff of 300 bytes.",
    "c2k.mix2": "cannot be reached: a MIX2's output is a weighted mean of two values in -2048 .. 2047 (see REQUIRED's comment).",
}


def write_census(path=CENSUS_JSON, procs=8):
    """Regenerates the golden table (a few minutes on 8 cores)."""
    import json
    import multiprocessing as mp
    with mp.Pool(procs) as pool:
        old, cases, blocks = old_table(pool=pool), edge_table(pool=pool), edge_table(pool=pool, block=True)
    edge = {cls: {} for cls in REQUIRED}
    for n, t in cases.items():
        merge(edge[EDGE_CASES[n].cls], t)
    json.dump({"old": old, "edge": edge, "edge_cases": cases, "edge_blocks": blocks, "sought": SOUGHT_NOTES}, open(path, "w"),
              indent=1, sort_keys=True)
