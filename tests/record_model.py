"""Record model for the base-record and window-table read-backs (TEST INFRASTRUCTURE; Python integers and NumPy, nothing of
the engine).

What a conversion must leave in a base record and what a batch operation must leave in a window-table record, written
from the descriptions in csrc/te377.hpp, csrc/curves.hpp and kernels/batch_mul.hpp, not from their code:

    te_affine(pt)          the affine twisted Edwards point (xe, ye) of a Weierstrass point: u = s (x + 1), v = s y,
                           xe = c u / v, ye = (u - 1) / (u + 1); None where the map is undefined (orders 2 and 4)
    te_projective(pt)      (X, Y, T, Z) = (c u (u + 1), (u - 1) v, c u (u - 1), v (u + 1)): the scale Te377::from_wire fixes
    *_words(...)           the words of one record of each form; an entry is a list of limbs where the contract says
                           canonical, Lazy(value mod p) where it says "a stored lazy product"
    Box                    limb box and value bound of a coordinate class, from tools/check_lazy_bounds.py shapes()
    window_points(...)     [2^offset_w] P for the windows of a precomputed table
    table_point(...)       [d 2^(c w)] B of a batch window table

tests/test_record_model_host.py pins this module on the CPU; tests/test_base_records_gpu.py compares the GPU with it.
"""
import functools
import os
import sys
from typing import List, NamedTuple, Optional

import numpy as np

import pyref as R
import stage_model as M
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_lazy_bounds as B  # noqa: E402

LB = 29
MASK = (1 << LB) - 1
RADIX_FP = 1 << 406  # Montgomery radix of the 13-limb field (14 reduction steps of 29 bits)
RADIX_FQ = 1 << 261  # ... of the 9-limb field (9 steps)

FORM_TE_PROJECTIVE, FORM_TE_AFFINE, FORM_WEIERSTRASS, FORM_ED = 0, 1, 2, 3  # MSM377_BASES_*
RECORD_WORDS = {FORM_TE_PROJECTIVE: 64, FORM_TE_AFFINE: 40, FORM_WEIERSTRASS: 32, FORM_ED: 32}
LIMBS = {FORM_TE_PROJECTIVE: 13, FORM_TE_AFFINE: 13, FORM_WEIERSTRASS: 13, FORM_ED: 9}
COORDS = {FORM_TE_PROJECTIVE: 4, FORM_TE_AFFINE: 3, FORM_WEIERSTRASS: 2, FORM_ED: 3}
COORD_NAMES = {
    FORM_TE_PROJECTIVE: ("Y - X", "Y + X", "2d T", "2 Z"),
    FORM_TE_AFFINE: ("y - x", "y + x", "2d x y"),
    FORM_WEIERSTRASS: ("x", "y"),
    FORM_ED: ("y - x", "y + x", "2d x y"),
}
# the coordinate the contract stores as a lazy product (every other one is canonical)
LAZY_COORDS = {FORM_TE_PROJECTIVE: (), FORM_TE_AFFINE: (2,), FORM_WEIERSTRASS: (), FORM_ED: ()}

TABLE_RECORD_WORDS, TABLE_FLAG_WORD = 32, 26
WINDOWS16 = (16,) * 16
WIDE_WIDTHS = M.WIDE_WIDTHS


class Lazy(NamedTuple):
    """A coordinate the contract fixes mod p only: any limbs inside the `stored` box with this residue."""

    value: int  # the Montgomery residue mod p the limbs must stand for


# ---- fields ----
def limbs_of(v: int, n: int) -> List[int]:
    return [(v >> (LB * j)) & MASK for j in range(n - 1)] + [v >> (LB * (n - 1))]


def value_of(limbs) -> int:
    return sum(int(x) << (LB * j) for j, x in enumerate(limbs))


def fp_mont(v: int) -> int:
    return v % R.P * RADIX_FP % R.P


def fq_mont(v: int) -> int:
    return v % R.Q * RADIX_FQ % R.Q


def fp_limbs(v: int) -> List[int]:
    """canonical residue -> the 13 limbs of v 2^406 mod p"""
    return limbs_of(fp_mont(v), 13)


def fq_limbs(v: int) -> List[int]:
    return limbs_of(fq_mont(v), 9)


# ---- boxes: tools/check_lazy_bounds.py shapes() ----
class Box(NamedTuple):
    name: str
    limbs: tuple  # inclusive per-limb maxima
    hi: int       # exclusive value bound

    def accepts(self, arr: np.ndarray) -> np.ndarray:
        """arr: (m, N) limbs -> (m,) bool: every limb inside the box and the value below the bound."""
        arr = np.asarray(arr, dtype=np.uint64)
        n = len(self.limbs)
        assert arr.ndim == 2 and arr.shape[1] == n
        inside = np.ones(arr.shape[0], dtype=bool)
        for j in range(n):
            inside &= arr[:, j] <= np.uint64(self.limbs[j])
        # the lower limbs of every box here are carry-normalised, so the value compares limb by limb from the top
        assert all(x == MASK for x in self.limbs[:-1])
        top = limbs_of(self.hi - 1, n)
        below = np.zeros(arr.shape[0], dtype=bool)
        equal = np.ones(arr.shape[0], dtype=bool)
        for j in reversed(range(n)):
            below |= equal & (arr[:, j] < np.uint64(top[j]))
            equal &= arr[:, j] == np.uint64(top[j])
        return inside & (below | equal)

    def corner(self) -> List[int]:
        """The largest value of the box, as limbs."""
        return limbs_of(self.hi - 1, len(self.limbs))


@functools.lru_cache(maxsize=None)
def boxes(field: str):
    """{"canonical": Box, "stored": Box} of Fp or Fq, read from the proof's shape table under use_field(field)."""
    B.use_field(field)
    try:
        t = B.shapes()
        return {k: Box(k, tuple(t[k].limbs), t[k].hi) for k in ("canonical", "stored")}
    finally:
        B.use_field("Fp")


def coord_box(form: int, coord: int) -> Box:
    t = boxes("Fq" if form == FORM_ED else "Fp")
    return t["stored" if coord in LAZY_COORDS[form] else "canonical"]


# ---- the Weierstrass -> twisted Edwards map (csrc/te377.hpp, constants of tools/gen_consts.py) ----
def _uv(pt):
    te = util.te_params()
    return te["s"] * (pt[0] + 1) % R.P, te["s"] * pt[1] % R.P


def te_representable(pt) -> bool:
    """False for the curve points the map does not cover: v (u + 1) = 0, the points of order 2 and 4."""
    u, v = _uv(pt)
    return v * (u + 1) % R.P != 0


def te_projective(pt):
    """(X, Y, T, Z) of the inversion-free conversion: X = c u (u + 1), Y = (u - 1) v, T = c u (u - 1), Z = v (u + 1)."""
    c = util.te_params()["c"]
    u, v = _uv(pt)
    return c * u * (u + 1) % R.P, (u - 1) * v % R.P, c * u * (u - 1) % R.P, v * (u + 1) % R.P


def te_affine(pt):
    """(xe, ye) = (c u / v, (u - 1) / (u + 1)); the identity (None) is (0, 1); None where the map is undefined."""
    if pt is None:
        return (0, 1)
    if not te_representable(pt):
        return None
    X, Y, _, Z = te_projective(pt)
    zi = pow(Z, -1, R.P)
    return X * zi % R.P, Y * zi % R.P


def te_add(a, b):
    """The a = -1 twisted Edwards law on affine points (used by the homomorphism pin only)."""
    d = util.te_params()["d"]
    x1, y1 = a
    x2, y2 = b
    t = d * x1 * x2 * y1 * y2 % R.P
    return (x1 * y2 + y1 * x2) * pow(1 + t, -1, R.P) % R.P, (y1 * y2 + x1 * x2) * pow(1 - t, -1, R.P) % R.P


def te_to_weierstrass(e):
    """Inverse of te_affine on its image (the identity comes back as None)."""
    te = util.te_params()
    xe, ye = e
    if xe == 0:
        assert ye == 1, "(0, -1) stands for the 2-torsion point the forward map does not produce"
        return None
    u = (1 + ye) * pow(1 - ye, -1, R.P) % R.P
    v = te["c"] * u * pow(xe, -1, R.P) % R.P
    si = pow(te["s"], -1, R.P)
    return (u * si - 1) % R.P, v * si % R.P


def beta() -> int:
    return M.glv_consts()[1]


# ---- expected words of one record ----
def te_projective_words(pt):
    """64 words: Y - X, Y + X, 2d T, 2 Z, all canonical (Te377::from_wire), 12 pad."""
    d = util.te_params()["d"]
    X, Y, T, Z = te_projective(pt)
    return [fp_limbs(Y - X), fp_limbs(Y + X), fp_limbs(2 * d * T), fp_limbs(2 * Z)]


def te_affine_words(pt):
    """40 words: y - x, y + x canonical; 2d x y a stored lazy product; 1 pad.  pt is a representable Weierstrass point."""
    d = util.te_params()["d"]
    xe, ye = te_affine(pt)
    return [fp_limbs(ye - xe), fp_limbs(ye + xe), Lazy(fp_mont(2 * d * xe * ye))]


def weierstrass_words(pt, phi=False):
    """32 words: x, y canonical (phi: BETA x, y), 6 pad."""
    x, y = pt
    return [fp_limbs(beta() * x if phi else x), fp_limbs(y)]


def ed_make_base(pt):
    """Edwards-BLS12 (ed_ext.hpp make_base): y - x, y + x, 2 d x y over Fq, all canonical."""
    x, y = pt
    return [fq_limbs(y - x), fq_limbs(y + x), fq_limbs(2 * R.ED_D * x * y)]


def record_words(form: int, pt, phi=False):
    if form == FORM_TE_PROJECTIVE:
        return te_projective_words(pt)
    if form == FORM_TE_AFFINE:
        return te_affine_words(pt)
    if form == FORM_WEIERSTRASS:
        return weierstrass_words(pt, phi)
    return ed_make_base(pt)


def table_record_words(pt):
    """A window-table record: x[13], y[13], flag, 5 pad; the identity is all zero but the flag."""
    if pt is None:
        return [0] * 26 + [1] + [0] * 5
    return fp_limbs(pt[0]) + fp_limbs(pt[1]) + [0] * 6


# ---- which points the records of a table stand for ----
def window_offsets(widths):
    return [sum(widths[:w]) for w in range(len(widths))]


def window_points(pt, widths):
    """[2^offset_w] pt for every window, by one chain of doublings (pyref's Jacobian doubling, one inversion per window).
    tests/test_record_model_host.py pins it to R.mul(pt, 2^offset_w)."""
    out = [pt]
    X, Y, Z = pt[0], pt[1], 1
    for w in range(1, len(widths)):
        for _ in range(widths[w - 1]):
            X, Y, Z = R._jac_dbl(X, Y, Z)
        if Z == 0:
            out.append(None)
            continue
        zi = pow(Z, -1, R.P)
        out.append((X * zi * zi % R.P, Y * zi * zi * zi % R.P))
    return out


def table_windows(c: int) -> int:
    return (256 + c - 1) // c


def table_records(c: int) -> int:
    return table_windows(c) * (1 << (c - 1)) + 1


def table_index(c: int, w: int, d: int) -> int:
    return w * (1 << (c - 1)) + d - 1


def table_point(base, c: int, t: int):
    """The point record t of the width-c table of `base` stands for: [d 2^(c w)] base, w = t >> (c - 1), d = (t mod 2^(c-1)) + 1."""
    w, d = t >> (c - 1), (t & ((1 << (c - 1)) - 1)) + 1
    return R.mul(base, d << (c * w))


def table_rows(base, c: int):
    """Every record's point of a narrow table, row by row: the row base by doublings, then d = 1 .. 2^(c-1) by additions
    (R.add follows every exceptional case).  Pinned to table_point on the CPU."""
    out = []
    rb = base
    for w in range(table_windows(c)):
        acc = None
        for _ in range(1 << (c - 1)):
            acc = R.add(acc, rb)
            out.append(acc)
        for _ in range(c):
            rb = R.add(rb, rb)
    out.append(rb)
    return out


# ---- comparison of a read-back with the model ----
def split(words: np.ndarray, form: int):
    """(m, record_words) -> list of (m, limbs) arrays, one per coordinate, and the (m, pad) array."""
    n, k = LIMBS[form], COORDS[form]
    return [words[:, n * c : n * c + n] for c in range(k)], words[:, n * k :]


def check_boxes(words: np.ndarray, form: int, where="", stride=None) -> None:
    """Over ALL records of a read: every pad word zero, every limb inside its box, every value below its bound.
    stride: records per window, to name the window of a record."""
    coords, pad = split(words, form)
    stride = stride or max(len(words), 1)
    bad = np.flatnonzero(pad.any(axis=1))
    assert bad.size == 0, "%srecord %d of window %d: pad words not zero: %s" % (where, bad[0] % stride, bad[0] // stride, pad[bad[0]].tolist())
    for c, arr in enumerate(coords):
        box = coord_box(form, c)
        ok = box.accepts(arr)
        bad = np.flatnonzero(~ok)
        assert bad.size == 0, "%srecord %d of window %d, coordinate %s: outside the %s box (limbs %s); %d of %d records are" % (
            where, bad[0] % stride, bad[0] // stride, COORD_NAMES[form][c], box.name, [hex(int(x)) for x in arr[bad[0]]], bad.size, len(arr))


def check_record(row, expected, form: int, where: str) -> None:
    """One record against record_words(): exact limbs, or the residue of a lazy coordinate."""
    n = LIMBS[form]
    mod = R.Q if form == FORM_ED else R.P
    for c, exp in enumerate(expected):
        got = [int(x) for x in row[n * c : n * c + n]]
        name = COORD_NAMES[form][c]
        if isinstance(exp, Lazy):
            assert value_of(got) % mod == exp.value, "%s, coordinate %s: residue differs from the model" % (where, name)
        else:
            assert got == exp, "%s, coordinate %s: limbs %s, model %s" % (where, name, [hex(x) for x in got], [hex(x) for x in exp])


def check_table_boxes(words: np.ndarray, where="") -> None:
    """Over ALL records of a window table: pad zero, flag 0 or 1, x and y canonical, a flagged record all zero."""
    canonical = boxes("Fp")["canonical"]
    pad = words[:, TABLE_FLAG_WORD + 1 :]
    bad = np.flatnonzero(pad.any(axis=1))
    assert bad.size == 0, "%srecord %d: pad words not zero" % (where, bad[0])
    flag = words[:, TABLE_FLAG_WORD]
    bad = np.flatnonzero(flag > 1)
    assert bad.size == 0, "%srecord %d: flag word %d" % (where, bad[0], flag[bad[0]])
    for c, name in enumerate(("x", "y")):
        arr = words[:, 13 * c : 13 * c + 13]
        bad = np.flatnonzero(~canonical.accepts(arr))
        assert bad.size == 0, "%srecord %d, coordinate %s: not canonical (limbs %s)" % (where, bad[0], name, [hex(int(x)) for x in arr[bad[0]]])
    bad = np.flatnonzero((flag == 1) & words[:, :26].any(axis=1))
    assert bad.size == 0, "%srecord %d: an identity record with non-zero coordinates" % (where, bad[0])


def check_table_record(row, pt, c: int, t: int, where: str) -> None:
    w, d = t >> (c - 1), (t & ((1 << (c - 1)) - 1)) + 1
    got = [int(x) for x in row]
    exp = table_record_words(pt)
    if got == exp:
        return
    for name, lo, hi in (("x", 0, 13), ("y", 13, 26), ("flag", 26, 27), ("pad", 27, 32)):
        assert got[lo:hi] == exp[lo:hi], "%srecord %d (row %d, d = %d), %s: %s, model %s" % (
            where, t, w, d, name, [hex(x) for x in got[lo:hi]], [hex(x) for x in exp[lo:hi]])


def sample_indices(n: int, windows: int, stride: int, extra: int, seed) -> List[int]:
    """The records the big-integer comparison visits where it cannot visit all: indices 0, 255, 256, 2047, 2048, n - 1 of
    every window, every record of windows 0, 1 and the last, and `extra` seeded others."""
    import random

    if n <= 2049 and windows == 1:
        return list(range(n))
    pick = set()
    for w in range(windows):
        for i in (0, 255, 256, 2047, 2048, n - 1):
            if i < n:
                pick.add(w * stride + i)
    for w in {0, min(1, windows - 1), windows - 1}:
        pick.update(range(w * stride, w * stride + n))
    rnd = random.Random("record sample/%s" % (seed,))
    total = windows * stride
    want = min(len(pick) + extra, windows * n)
    while len(pick) < want:
        t = rnd.randrange(total)
        if t % stride < n:
            pick.add(t)
    return sorted(pick)
