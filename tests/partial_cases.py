"""Inputs of the window-record tests (TEST INFRASTRUCTURE; stage_model and pyref only, nothing of the engine).

The bucket reduction (csrc/kernels/reduce.hpp) runs over all 2^L buckets of a window whatever the input, so what a case
chooses is WHICH buckets are occupied.  A case is built from digits: scalar_from_digits puts a chosen digit into chosen
windows of a geometry and checks with the model's recode that the scalar gives exactly those digits back.

    planted(g, ...)        one point alone in bucket index 2^b of window w, for as many (w, b) as the geometry has; index 0,
                           index 2^L - 1 (the digit -2^L), an empty window, P and -P in two buckets of one window
    ladder(g, ...)         a window's only two entries at bucket indices 0 and 2^L >> (r + 1): they first meet at level r, in
                           the running block -- a different level in every window of one call of two scalars; with age > 0
                           the pair inside the list an earlier level left behind: indices lo + k and lo + k + half

Every case states what it promises as `occupied` -- per record the bucket indices that hold something -- and `meet` -- per
record the (level, array) pairs at which its two entries are first added; tests/test_stage_model_host.py asserts both from
the model (stage_model.csr, stage_model.meetings) with no GPU, tests/test_partial_records_gpu.py runs the cases.
Points are [a]G with known a (Edwards-BLS12: [a]G of its subgroup, or a low-order point with no logarithm), so that an
expected record point is one scalar multiplication."""
from typing import Dict, List, NamedTuple, Optional, Tuple

import pyref as R
import stage_model as M


class Case(NamedTuple):
    name: str
    g: M.Geometry
    scalars: List[int]
    points: list                      # affine points of the call's curve
    logs: List[Optional[int]]         # logs[i]: points[i] = [logs[i]] generator, or None
    occupied: Dict[int, set]          # record -> bucket indices that hold entries (records not named: empty)
    meet: Dict[int, List[Tuple[int, int]]]  # record -> [(level, array)] of its pair's first addition
    ed: bool = False
    fold: bool = False                # the sixteen slots of the 16-bit table added into one record


def positions(g):
    """Digit positions of a scalar under g: one per slot; 16 behind the GLV front end (8 of k1, then 8 of k2)."""
    return 16 if g.name == "glv8" else len(g.slots)


def record_of(g, pos, fold=False):
    """The record a digit position feeds."""
    if g.name == "wide13" or fold:
        return 0
    return pos % 8 if g.name == "glv8" else pos


def scalar_from_digits(g, digits: Dict[int, int]):
    """The scalar whose recode under g is exactly `digits` (position -> digit, 0 elsewhere), or None if there is none:
    the digit does not fit the window (an unsigned window, the narrow top window of a short call, lambda's top bits)."""
    full = [0] * positions(g)
    for pos, d in digits.items():
        full[pos] = d
    k = M.rebuild(full, g)
    if not 0 <= k < (1 << 253) or (g.name == "short" and k >> g.bits):
        return None
    rec = M.recode(k, g)
    return k if rec.flags == 0 and rec.digits == full else None


def digit_of_index(t):
    return t + 1  # bucket index t holds key t + 1


class Points:
    """Points with known logarithms, one new one per call of new(); neg(i) / same(i) reuse point i."""

    def __init__(self, seed, ed=False):
        import random

        self.rnd = random.Random("partial records/%s" % seed)
        self.ed = ed
        _, _, self.mul, _, self.gen, self.order = M.group(ed)
        self.points, self.logs = [], []

    def add_log(self, a):
        self.points.append(self.mul(self.gen, a % self.order))
        self.logs.append(a % self.order)
        return len(self.points) - 1

    def new(self):
        return self.add_log(self.rnd.randrange(2, self.order))

    def neg(self, i):
        return self.add_log(-self.logs[i])

    def same(self, i):
        return self.add_log(self.logs[i])

    def raw(self, pt):
        """A point without a known logarithm (low-order points of Edwards-BLS12, sums with them)."""
        self.points.append(pt)
        self.logs.append(None)
        return len(self.points) - 1


def _case(name, g, entries, pts, meet=None, ed=False, fold=False):
    """entries: [(position, bucket index, point number)], one scalar each."""
    scalars, occupied = [], {}
    for pos, t, _ in entries:
        k = scalar_from_digits(g, {pos: digit_of_index(t)})
        assert k is not None, (name, pos, t)
        scalars.append(k)
        occupied.setdefault(record_of(g, pos, fold), set()).add(t)
    order = [i for _, _, i in entries]
    return Case(name, g, scalars, [pts.points[i] for i in order], [pts.logs[i] for i in order], occupied, meet or {}, ed, fold)


def planted(g, ed=False, fold=False, use=None):
    """Call "planes": position w holds one point in bucket index 2^b, b = w mod L, and nothing else (every position where such
    a digit fits; `use`: only these positions, e.g. one half of the GLV positions per call).  Behind one record (the wide
    table, the folded table) that is one call per plane instead, the position rotating through the digit columns."""
    L = g.bucket_log
    single = g.name == "wide13" or fold
    pts = Points("planted/%s/%s" % (g.name, fold), ed)
    cases = []
    if single:
        for b in range(L):
            pos = b % positions(g)
            if scalar_from_digits(g, {pos: digit_of_index(1 << b)}) is None:
                pos = 0
            cases.append(_case("plane %d" % b, g, [(pos, 1 << b, pts.new())], pts, ed=ed, fold=fold))
        return cases
    entries = []
    for w in (range(positions(g)) if use is None else use):
        b = w % L
        if scalar_from_digits(g, {w: digit_of_index(1 << b)}) is not None:
            entries.append((w, 1 << b, pts.new()))
    return [_case("planes", g, entries, pts, ed=ed, fold=fold)]


def extras(g, ed=False, fold=False):
    """Index 0 alone; index 2^L - 1 (the digit -2^L, whose carry puts the same point into index 0 of the next window); a
    wholly empty window; a window whose total is the identity while its planes are not (P at index 5, -P at index
    2^(L-1) + 2).  One call where the geometry has the windows for it, else one call each (a single record)."""
    L = g.bucket_log
    single = g.name == "wide13" or fold
    pts = Points("extras/%s/%s" % (g.name, fold), ed)
    top = (1 << L) - 1

    def top_index_scalar(pos):
        return scalar_from_digits(g, {pos: -(1 << L), pos + 1: 1})

    cases = []
    if single:
        p = pts.new()
        cases.append(_case("index 0", g, [(1, 0, p)], pts, ed=ed, fold=fold))
        k = top_index_scalar(0)
        assert k is not None
        i = pts.new()
        # window 0: -P in index 2^L - 1; the carry: [2^offset(1)] P in index 0 -- one record holds both
        cases.append(Case("index 2^L - 1", g, [k], [pts.points[i]], [pts.logs[i]], {0: {top, 0}}, {}, ed, fold))
        cases.append(Case("empty", g, [0], [pts.points[i]], [pts.logs[i]], {}, {}, ed, fold))
        a = pts.new()
        cases.append(_case("P and -P", g, [(0, 5, a), (0, (1 << (L - 1)) + 2, pts.neg(a))], pts, ed=ed, fold=fold))
        return cases
    k = top_index_scalar(0)
    assert k is not None and positions(g) >= 5, g.name
    i = pts.new()
    a = pts.new()
    rest = [(3, 5, a), (3, (1 << (L - 1)) + 2, pts.neg(a))]
    if positions(g) > 5 and scalar_from_digits(g, {5: 1}) is not None:
        rest.append((5, 0, pts.new()))
    c = _case("extras", g, rest, pts, ed=ed)
    occupied = dict(c.occupied)
    occupied[record_of(g, 0)] = {top}
    occupied.setdefault(record_of(g, 1), set()).add(0)
    # record 2 (and 4): wholly empty
    return [Case("extras", g, [k] + c.scalars, [pts.points[i]] + c.points, [pts.logs[i]] + c.logs, occupied, {}, ed)]


SECOND = ("same", "negative", "other")  # the ladder's second operand; Edwards-BLS12 also "order2", "order4"


def _second(pts, first, kind):
    if kind == "same":
        return pts.same(first)
    if kind == "negative":
        return pts.neg(first)
    if kind == "other":
        return pts.new()
    from check_vectors import ed_low_order_points

    t2, t4, _ = ed_low_order_points()
    return pts.raw(t2 if kind == "order2" else t4)


def ladder_pairs(L, levels, age=0):
    """level r -> (x, y, where they meet).  age = 0: bucket indices 0 and half = 2^L >> (r + 1), the running block.  age > 0:
    inside the list that level r' = r - age left behind (lo = 2^L >> (r' + 1)): lo + k and lo + k + half with k = half / 2;
    such a pair sits in the block's upper half at level r' too, so it meets again in the block at level r."""
    out = {}
    for r in levels:
        half = (1 << L) >> (r + 1)
        if age == 0:
            out[r] = (0, half, [(r, 0)])
        elif r - age >= 0:
            rp = r - age
            lo, k = (1 << L) >> (rp + 1), half // 2
            out[r] = (lo + k, lo + k + half, [(r, 0), (r, rp + 1)])
    return out


def ladder(g, kind, ed=False, age=0, use=None, levels=None, fold=False):
    """One call: position use[j] carries level levels[j] -- its only two entries are the pair of ladder_pairs -- the first
    operand the same point in every window (one scalar), the second one `kind` of it (a second scalar).  Defaults: every
    level of the geometry's tree, in the first L positions where both digits fit."""
    L = g.bucket_log
    pts = Points("ladder/%s/%s/%d" % (g.name, kind, age), ed)
    pairs = ladder_pairs(L, range(L) if levels is None else levels, age)
    free = list(range(8 if g.name == "glv8" else positions(g))) if use is None else list(use)  # (GLV: k1's windows; k2's are range(8, 16))
    first, second = {}, {}
    occupied, meet = {}, {}
    for r, (x, y, where) in pairs.items():
        for pos in free:
            if scalar_from_digits(g, {pos: digit_of_index(x)}) is not None and scalar_from_digits(g, {pos: digit_of_index(y)}) is not None:
                free.remove(pos)
                first[pos], second[pos] = digit_of_index(x), digit_of_index(y)
                occupied[record_of(g, pos, fold)] = {x, y}
                meet[record_of(g, pos, fold)] = where
                break
    assert first, (g.name, kind, age, levels)
    a = pts.new()
    b = _second(pts, a, kind)
    ks = [scalar_from_digits(g, first), scalar_from_digits(g, second)]
    assert None not in ks, (g.name, kind, age)
    name = "ladder %s age %d levels %s" % (kind, age, sorted({r for ms in meet.values() for r, _ in ms}))
    return Case(name, g, ks, [pts.points[a], pts.points[b]], [pts.logs[a], pts.logs[b]], occupied, meet, ed, fold)


def levels_in(case):
    return sorted({r for ms in case.meet.values() for r, _ in ms})


def wire(case):
    """(points, scalars) as the engine takes them."""
    enc = R.ed_encode_points if case.ed else R.encode_points
    return enc(case.points), R.encode_scalars(case.scalars)


def model_records(case):
    """The records the call must leave: stage_model.partial_points over the case's digit matrix."""
    cols, flags = M.digit_matrix(case.scalars, case.g)
    assert flags == 0
    return M.partial_points(case.points, cols, case.g, len(case.scalars), logs=case.logs, ed=case.ed, fold=case.fold)


def expected_result(case):
    add, _, mul, ident, gen, order = M.group(case.ed)
    acc, total = ident, 0
    for k, pt, a in zip(case.scalars, case.points, case.logs):
        if a is None:
            acc = add(acc, mul(pt, k))
        else:
            total += k * a
    if total % order:
        acc = add(acc, mul(gen, total % order))
    return R.ed_encode_result(acc) if case.ed else R.encode_result(acc)
