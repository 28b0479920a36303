"""The cases of tests/test_walk_stash_gpu.py (TEST INFRASTRUCTURE): inputs, crafted lanes and the events each case promises.

A case is a dict:
    call      "batch_mul" | "multi" | "commit" | "var" | "lincomb2" | "ed"
    name      its test id
    c         the width the walk runs: 8 or 16 (set_mul_window, or the generator set's); 4 for var and lincomb2
    n         outputs
    bases     the fixed bases / generators (points)                       -- batch_mul, multi, commit, ed
    points    per lane, a tuple of one (var) or two (lincomb2) points; None is a flagged input
    rows      per lane, the tuple of scalars THE WALK SEES (after the Montgomery import where scalar_form is "mont")
    crafted   the lanes whose walk the model replays (walk_model.walk_events) and whose value is compared with pyref
    promises  the events the crafted lanes must contain: asserted from the model on the CPU and again before the GPU runs
and whatever the call needs beside (layout, forms, strides).  tests/test_walk_model_host.py asserts every promise with no
GPU; nothing here calls the engine's device code.
"""
import functools

import batch_mul_multi_vectors as MV
import batch_mul_var_vectors as VV
import batch_mul_vectors as V
import check_vectors as CV
import commit_rows_vectors as CR
import ed_batch_mul_vectors as EV
import pyref as R
import walk_model as WM

r = R.R_ORDER
SIZES = (1, 64, 65, 255, 257, 1025, 3079)  # wave, workgroup and BM_BLOCK boundaries; 3079: the normalisation tests' size
SEAMS = (0, 63, 64, 255, 256)
M = MV.M
ALL_G1_EVENTS = frozenset(WM.EVENTS)


def small_order_extras(c):
    """Scalars that steer a base of order 2, 3, 4 or 6 through the exits: [2]T = O (a flagged entry), acc = entry
    (2^c = 1 mod 3: digits (1, 1) on order 3), acc = -entry (digits (2, 1)), then a digit behind the O that leaves."""
    return [2, 3, 4, 5, 6, (1 << c) + 1, (1 << c) + 2, (1 << 2 * c) + (1 << c) + 2, (1 << 2 * c) + (1 << c) + 1, 12 * r + 7]


def place(n, crafted_rows, filler_rows, zero_row, single=6):
    """n rows: the crafted rows on lanes 0, 63, 64, 255, 256, n - 1 and then 1, 2, ..; from n = 255 on the whole wave
    128..191 holds zero scalars and wave 64..127 holds zero scalars beside its one crafted lane 64 (the wave-uniform skip);
    every other lane a filler row.  Returns (rows, crafted lanes)."""
    rows = [filler_rows[i % len(filler_rows)] for i in range(n)]
    if n >= 255:
        for i in range(64, 192):
            rows[i] = zero_row
    lanes = []
    for i in list(SEAMS) + [n - 1] + list(range(1, 64)):
        if i < n and i not in lanes:
            lanes.append(i)
    lanes = lanes[: len(crafted_rows)]
    if n == 1:
        crafted_rows = crafted_rows[single : single + 1]  # n = 1: the row with 2^256 - 1, the carry through every window
    for lane, row in zip(lanes, crafted_rows):
        rows[lane] = row
    if n >= 255:
        assert any(rows[64]) and not any(any(rows[i]) for i in range(65, 192))
    return rows, sorted(lanes)


def rows_of(scalars, k=1):
    """k columns out of one scalar list: row t = (s_t, s_(t+1), ..)."""
    return [tuple(scalars[(t + j) % len(scalars)] for j in range(k)) for t in range(len(scalars))]


def _filler(seed, count, k=1, bits=256):
    flat = V.random_scalars(seed, count * k, bits)
    return [tuple(flat[k * i : k * i + k]) for i in range(count)]


def _case(call, name, c, bases, rows, crafted, promises=(), placed=True, **extra):
    """placed: the rows are place()'s as they stand -- crafted rows on the seam lanes, the zero waves; False where a case
    overrides them (one scalar for all lanes, a list of relation rows)."""
    case = dict(call=call, name=name, c=c, n=len(rows), bases=tuple(bases) if bases is not None else None, rows=rows, crafted=crafted, promises=frozenset(promises), placed=placed)
    case.update(extra)
    return case


def lanes_of(case):
    """[(points of the lane, scalars of the lane)] over the crafted lanes, as walk_model.lane_events takes them; a row
    commitment: one lane per segment of a crafted row (each segment's walk starts from O)."""
    if case["call"] in ("var", "lincomb2"):
        return [(tuple(case["points"][i]), tuple(case["rows"][i])) for i in case["crafted"]]
    if case["call"] == "commit":
        return [(case["bases"][j0:j1], tuple(case["rows"][i][j0:j1])) for i in case["crafted"] for j0, j1 in segments_of(len(case["bases"]))]
    return [(case["bases"], tuple(case["rows"][i])) for i in case["crafted"]]


def events_of(case):
    """walk_model.walk_events over the crafted lanes of a case."""
    if case["call"] == "ed":
        out = set()
        for i in case["crafted"]:
            out |= WM.ed_events(case["rows"][i], case["c"])
        return out
    kind = "var" if case["call"] in ("var", "lincomb2") else "fixed"
    out = WM.walk_events(dict(kind=kind, c=case["c"], lanes=lanes_of(case)))
    if case["call"] == "commit":  # a segment that is O says nothing about the row: the fold's events are fold_events
        out -= {WM.EV_ZERO_O, WM.EV_SMALL_O}
    return out


_lane = WM.lane_events


def expected_point(case, i):
    kind = "var" if case["call"] in ("var", "lincomb2") else "fixed"
    if case["call"] == "ed":
        return WM.ed_expected(case["bases"], case["rows"][i])
    pts = case["points"][i] if kind == "var" else case["bases"]
    if case["call"] == "commit":
        return commit_partial(case, i, 0, len(case["bases"]))
    return _lane(kind, case["c"], tuple(pts), tuple(case["rows"][i]))[0]


def segments_of(k):
    s, per, _ = CR.plan(k)
    return [(g * per, min(k, g * per + per)) for g in range(s)]


def commit_partial(case, i, j0, j1):
    """The model's sum over generators j0 .. j1 - 1 of row i: through the logarithms where the set has them."""
    row = case["rows"][i]
    if case.get("logs"):
        return R.mul(R.G, sum(s * g for s, g in zip(row[j0:j1], case["logs"][j0:j1])) % r)
    acc = None
    for gen, s in zip(case["bases"][j0:j1], row[j0:j1]):
        if s:
            acc = R.add(acc, R.mul(gen, s))
    return acc


# ------------------------------------------------------------------ k_bm_accumulate ----

@functools.lru_cache(maxsize=None)
def batch_mul_cases():
    out = []
    named = dict(V.bases())
    subgroup = R.mul(R.G, 0x5AB6)
    for c in V.WIDTHS:
        crafted = [s for _, s in WM.crafted_scalars(c)]
        for n in SIZES:
            rows, lanes = place(n, rows_of(crafted), _filler(0xB300 + n, min(n, 1024)), (0,))
            promises = {WM.EV_CARRY} if n == 1 else {WM.EV_ZERO_O, WM.EV_CARRY, WM.EV_HALF}
            out.append(_case("batch_mul", "G-c%d-n%d" % (c, n), c, [R.G], rows, lanes, promises, scalar_form="wire"))
        values = [s for _, s in WM.crafted_scalars(c)]
        dev_rows, lanes = place(257, rows_of(values), _filler(0xB3AA, 257), (0,))
        seen = [tuple(VV.mont_scalars(row)) for row in dev_rows]
        out.append(_case("batch_mul", "G-c%d-mont" % c, c, [R.G], seen, lanes, {WM.EV_ZERO_O}, scalar_form="mont", device_rows=dev_rows))
        extras = crafted + small_order_extras(c)
        for name in ("small_0", "small_1", "small_2", "small_3", "small_4", "small_5", "small_6", "G_plus_torsion"):
            rows, lanes = place(65, rows_of(extras), _filler(0xB3BB, 65, bits=40), (0,))
            promises = {WM.EV_ZERO_O}
            if name.startswith("small"):
                promises |= {WM.EV_SMALL_O}
            if name == "small_0":
                promises |= {WM.EV_FLAGGED}
            if name == "small_3":
                promises |= {WM.EV_EQUAL, WM.EV_OPPOSITE, WM.EV_MID_O}
            out.append(_case("batch_mul", "%s-c%d" % (name, c), c, [named[name]], rows, lanes, promises, scalar_form="wire"))
        rows, lanes = place(65, rows_of(crafted), _filler(0xB3CC, 65), (0,))
        out.append(_case("batch_mul", "subgroup-c%d" % c, c, [subgroup], rows, lanes, {WM.EV_ZERO_O, WM.EV_CARRY, WM.EV_HALF}, scalar_form="wire"))
    return tuple(out)


MULTI_PASS = {"batch_mul": ((1 << 20) + 300, 8, 1 << 20), "var": ((1 << 17) + 257, 4, 1 << 17), "lincomb2": ((1 << 16) + 257, 4, 1 << 16)}  # n, width, pass length


# ------------------------------------------------------------------ k_bmm_accumulate ----

@functools.lru_cache(maxsize=None)
def multi_cases():
    out = []
    tuples = dict(MV.tuples())
    for c, layout in ((8, "rows"), (16, "columns")):
        crafted = [s for _, s in WM.crafted_scalars(c)]
        for name in ("G_G", "G_negG", "G_mG"):
            special = rows_of(crafted, 2) + MV.cancelling_rows() + MV.ZERO_ROWS
            rows, lanes = place(65, special, _filler(0xB400, 65, 2), (0, 0))
            promises = {WM.EV_ZERO_O, WM.EV_CARRY, WM.EV_HALF}
            promises |= {"G_G": {WM.EV_EQUAL, WM.EV_OPPOSITE}, "G_negG": {WM.EV_OPPOSITE, WM.EV_EQUAL}, "G_mG": {WM.EV_OPPOSITE}}[name]
            out.append(_case("multi", "%s-c%d-%s" % (name, c, layout), c, tuples[name], rows, lanes, promises, layout=layout, cancels=True))
        for n in SIZES:  # k = 2 at every size (65 is the relation case above)
            if n != 65:
                rows, lanes = place(n, special, _filler(0xB410 + n, min(n, 512), 2), (0, 0))
                promises = {WM.EV_CARRY} if n == 1 else {WM.EV_ZERO_O, WM.EV_CARRY, WM.EV_HALF, WM.EV_OPPOSITE}
                out.append(_case("multi", "G_mG-c%d-%s-n%d" % (c, layout, n), c, tuples["G_mG"], rows, lanes, promises, layout=layout, cancels=n > 1))
        special = rows_of(crafted + small_order_extras(c), 2) + MV.ZERO_ROWS
        rows, lanes = place(65, special, _filler(0xB401, 65, 2, bits=40), (0, 0))
        out.append(_case("multi", "order2_GplusT-c%d-%s" % (c, layout), c, tuples["order2_GplusT"], rows, lanes, {WM.EV_FLAGGED, WM.EV_ZERO_O}, layout=layout))
        out.append(_case("multi", "small3_small3-c%d-%s" % (c, layout), c, tuples["small3_small3"], rows, lanes, {WM.EV_EQUAL, WM.EV_OPPOSITE, WM.EV_MID_O, WM.EV_SMALL_O}, layout=layout))
        t2 = dict(V.bases())["small_0"]  # B_1 = B_0 of order 2: (1, 1) doubles T -- madd's doubling exit leaves ZZ = 0 beside arbitrary X, Y
        rows, lanes = place(65, [(1, 1), (1, 3), (3, 1), (2, 1)] + special, _filler(0xB402, 65, 2, bits=40), (0, 0))
        out.append(_case("multi", "order2_order2-c%d-%s" % (c, layout), c, (t2, t2), rows, lanes, {WM.EV_EQUAL, WM.EV_SMALL_O, WM.EV_FLAGGED}, layout=layout))
        bases16 = [R.mul(R.G, 100 + j) for j in range(16)]
        for n in (257, 1025):
            rows, lanes = place(n, rows_of(crafted, 16), _filler(0xB416 + n, 64, 16), (0,) * 16)
            out.append(_case("multi", "k16-c%d-%s-n%d" % (c, layout, n), c, bases16, rows, lanes, {WM.EV_CARRY, WM.EV_HALF}, layout=layout))
    return tuple(out)


# ------------------------------------------------------------------ k_cr_accumulate / k_cr_fold ----

@functools.lru_cache(maxsize=None)
def commit_cases():
    out = []
    crafted = [s for _, s in WM.crafted_scalars(8)]
    for k in (16, 17, 33, 257):
        logs, gens = CR.known_logs(k)
        bases = R.decode_points(gens)
        for n in (1, 255, 300):
            special = rows_of(crafted, k)[:3]  # dense rows: every table walked
            sparse = []
            for t in range(6):  # one full-width scalar per segment, all other tables skipped
                row = [0] * k
                for j0, j1 in segments_of(k):
                    row[min(j1 - 1, j0 + t % 3)] = crafted[6 + t]
                sparse.append(tuple(row))
            rows, lanes = place(n, special + sparse, _filler(0xC0 + k, 16, k), (0,) * k, single=3)
            out.append(_case("commit", "k%d-rows%d" % (k, n), 8, bases, rows, lanes, {WM.EV_CARRY} if n == 1 else {WM.EV_CARRY, WM.EV_HALF}, logs=logs, gens=gens))
    rel = [row for _, row in CR.relation_rows()]
    names = [name for name, _ in CR.relation_rows()]
    out.append(_case("commit", "relations-k48", 8, CR.relation_generators(), rel, list(range(len(rel))),
                     {WM.EV_CARRY, WM.EV_FLAGGED, WM.EV_EQUAL, WM.EV_OPPOSITE}, gens=R.encode_points(list(CR.relation_generators())), names=names, placed=False))
    return tuple(out)


FOLD_EVENTS = ("a partial of O", "two equal partials", "two opposite partials", "a total of O from partials that are not O")


def fold_events(case):
    """What k_cr_fold meets over the crafted rows of a commit case, from the model: the running sum against each next partial."""
    out = set()
    segs = segments_of(len(case["bases"]))
    for i in case["crafted"]:
        parts = [commit_partial(case, i, j0, j1) for j0, j1 in segs]
        acc = parts[0]
        if len(parts) > 1 and any(p is None for p in parts):
            out.add(FOLD_EVENTS[0])
        for p in parts[1:]:
            if acc is not None and p is not None:
                if acc == p:
                    out.add(FOLD_EVENTS[1])
                elif acc == R.neg(p):
                    out.add(FOLD_EVENTS[2])
            acc = R.add(acc, p)
        if acc is None and len(parts) > 1 and sum(p is not None for p in parts) >= 2:
            out.add(FOLD_EVENTS[3])
    return out


# ------------------------------------------------------------------ k_bmv_table / k_bmv_accumulate, k_bl2_accumulate ----

def var_crafted():
    """[(point, scalar)]: the generator and a subgroup point under every crafted scalar of width 4, every point of small
    order and P + T under the scalars that steer them through the exits."""
    named = dict(V.bases())
    out = [((R.G, R.mul(R.G, 0x5AB6))[t % 2], s) for t, (_, s) in enumerate(WM.crafted_scalars(4))]
    for t, pt in enumerate(CV.g1_small_order_points()):
        for s in (1, 2, 3, 0x11, 0x12, 0x121, 0x81, 2**256 - 1)[t % 2 :: 2] + (5 + t,):
            out.append((pt, s))
    out += [(named["G_plus_torsion"], 2**256 - 1), (named["torsion"], r + 1), (named["small_3"], 0x11), (named["small_3"], 0x12), (named["small_3"], 0x121), (named["small_0"], 2)]
    return out


@functools.lru_cache(maxsize=None)
def var_cases():
    out = []
    crafted = var_crafted()
    G1_VAR = {WM.EV_ZERO_O, WM.EV_SMALL_O, WM.EV_MID_O, WM.EV_EQUAL, WM.EV_OPPOSITE, WM.EV_FLAGGED, WM.EV_CARRY, WM.EV_HALF}

    def build(name, n, point_form="wire", flagged=(), stride=32, scalar=None, seed=0xD0):
        pts = list(VV.mixed_points(max(n, 8)))[:n]
        fill = _filler(seed + n, min(n, 512), bits=256)
        rows, lanes = place(n, [(s,) for _, s in crafted], fill, (0,))
        points = [(p,) for p in pts]
        order = crafted[6:7] if n == 1 else crafted
        for lane, (pt, _) in zip(lanes_in_order(n, len(order)), order):
            points[lane] = (pt,)
        for i in flagged:
            if i < n:
                points[i] = (None,)
        if scalar is not None:
            rows = [(scalar,)] * n
        promises = G1_VAR if n >= 64 and scalar is None else ({WM.EV_CARRY} if (scalar or 2**256 - 1) >> 255 else set())
        if flagged:
            promises = set(promises) | {WM.EV_FLAGGED}
        return _case("var", name, 4, None, rows, sorted(set(lanes) | {i for i in flagged if i < n}), promises, points=points, point_form=point_form, stride=stride, placed=scalar is None)

    for n in SIZES:
        out.append(build("wire-n%d" % n, n))
    out.append(build("mont-n257", 257, "mont"))
    out.append(build("mont_flag-n257", 257, "mont_flag", flagged=(0, 63, 64, 255, 256)))
    out.append(build("stride0-carry", 257, stride=0, scalar=2**256 - 1))
    out.append(build("stride0-64bit", 257, stride=0, scalar=0xF123456789ABCDE7))
    return tuple(out)


def lanes_in_order(n, count):
    lanes = []
    for i in list(SEAMS) + [n - 1] + list(range(1, 64)):
        if i < n and i not in lanes:
            lanes.append(i)
    return lanes[:count]


@functools.lru_cache(maxsize=None)
def lincomb2_cases():
    out = []
    k_mul = 0x1D3F
    g, h = R.G, R.mul(R.G, 0x5AB6)
    t3 = dict(V.bases())["small_3"]
    t2 = dict(V.bases())["small_0"]
    sc = [s for _, s in WM.crafted_scalars(4)]
    t = V.random_scalars(0xE2, 1, bits=200)[0]
    special = [((g, h), (a, b)) for a, b in zip(sc, sc[1:] + sc[:1])]
    special += [((g, g), (t, t)), ((g, g), (t, r - t)), ((g, R.neg(g)), (t, t)), ((g, R.neg(g)), (t, t + 1)),  # Q = P, Q = -P
                ((g, R.mul(g, k_mul)), ((-k_mul * t) % r, t)), ((g, R.mul(g, k_mul)), (t, t)),              # Q = [m]P: O with no term O
                ((t3, t3), (0x11, 0)), ((t3, t3), (0x12, 0)), ((t3, t3), (1, 2)), ((t3, t3), (0x121, 0)), ((t2, h), (2, 0)), ((t2, t2), (1, 1)),
                ((None, h), (5, 7)), ((g, None), (2**256 - 1, 3)), ((None, None), (1, 1)), ((g, h), (0, 0))]

    def build(name, n, a_stride=32, b_stride=32, ab=None, in_place=False, point_form="wire"):
        p, q = list(VV.random_subgroup_points(0x11C0B2, min(n, 300))), list(VV.random_subgroup_points(0x22C0B2, min(n, 300)))
        points = [(p[i % len(p)], q[i % len(q)]) for i in range(n)]
        rows, lanes = place(n, [s for _, s in special], _filler(0xE3 + n, min(n, 512), 2), (0, 0))
        order = special[6:7] if n == 1 else special
        for lane, (pts, _) in zip(lanes_in_order(n, len(order)), order):
            points[lane] = pts
        if point_form != "mont_flag":  # a flagged input needs the form that can say so: the lane takes the generator
            points = [tuple(g if x is None else x for x in pts) for pts in points]
        if ab is not None:
            rows = [tuple(ab[j] if (a_stride, b_stride)[j] == 0 else row[j] for j in range(2)) for row in rows]
        promises = {WM.EV_ZERO_O, WM.EV_EQUAL, WM.EV_OPPOSITE, WM.EV_MID_O, WM.EV_CARRY, WM.EV_HALF, WM.EV_SMALL_O} if n >= 64 and ab is None else set()
        if point_form == "mont_flag" and n >= 64:
            promises |= {WM.EV_FLAGGED}
        return _case("lincomb2", name, 4, None, rows, lanes, promises, points=points, point_form=point_form, a_stride=a_stride, b_stride=b_stride, in_place=in_place, placed=ab is None)

    for n in SIZES:
        out.append(build("wire-n%d" % n, n))
    out.append(build("mont_flag-n257", 257, point_form="mont_flag"))
    out.append(build("a=b=1", 257, 0, 0, (1, 1)))
    out.append(build("a-stride0", 257, 0, 32, (2**256 - 1, 0)))
    out.append(build("b-stride0", 257, 32, 0, (0, 0xF123456789ABCDE7)))
    out.append(build("out=p", 257, in_place=True))
    return tuple(out)


# ------------------------------------------------------------------ k_edbm_accumulate ----

@functools.lru_cache(maxsize=None)
def ed_cases():
    out = []
    named = dict(EV.bases())
    classes = [named[x] for x in ("identity", "order2", "order4_a", "order4_b", "P_plus_order2", "P_plus_order4_a")]
    for c in EV.WIDTHS:
        crafted = [s for _, s in WM.crafted_scalars(c)] + [EV.ORD - 1, EV.ORD, EV.ORD + 1, 4 * EV.ORD]
        for n in SIZES if c == 8 else (257,):
            rows, lanes = place(n, rows_of(crafted), _filler(0xED0 + n, min(n, 1024)), (0,))
            out.append(_case("ed", "G-c%d-n%d" % (c, n), c, [R.ED_G], rows, lanes, {WM.EV_CARRY} if n == 1 else {WM.EV_CARRY, WM.EV_HALF}))
        for t, pt in enumerate(classes):
            rows, lanes = place(65, rows_of(crafted + [2, 3, 4, 5]), _filler(0xED1, 65, bits=40), (0,))
            out.append(_case("ed", "class%d-c%d" % (t, c), c, [pt], rows, lanes, {WM.EV_CARRY, WM.EV_HALF}))
        for n in (65, 257):
            rows, lanes = place(n, rows_of(crafted, 2) + EV.relation_rows(2), _filler(0xED2 + n, 64, 2), (0, 0))
            out.append(_case("ed", "G_mG-c%d-n%d" % (c, n), c, dict(EV.tuples())["G_mG"], rows, lanes, {WM.EV_CARRY, WM.EV_HALF}))
        bases16 = [R.ED_G] + classes + [R.ed_mul(R.ED_G, 77 + j) for j in range(9)]
        rows, lanes = place(257, rows_of(crafted, 16), _filler(0xED3, 64, 16), (0,) * 16)
        out.append(_case("ed", "k16-c%d" % c, c, bases16, rows, lanes, {WM.EV_CARRY, WM.EV_HALF}))
        rows = [(2**256 - 1,) * 16] * 1025  # the longest chain: 16 x (W + 1) lazy additions in every lane
        out.append(_case("ed", "k16-all-ones-c%d" % c, c, bases16, rows, [0, 63, 64, 255, 256, 1024], {WM.EV_CARRY}, placed=False))
    return tuple(out)


def all_cases():
    return batch_mul_cases() + multi_cases() + commit_cases() + var_cases() + lincomb2_cases() + ed_cases()
