"""Model and operand families for the batch calls' normalisation kernels (TEST INFRASTRUCTURE, pure Python).

k_bm_up / k_bm_across / k_bm_down<form> (kernels/batch_mul.hpp) and k_edbm_up / k_edbm_across / k_edbm_down<form>
(kernels/ed_batch_mul.hpp) turn a stash of projective points into output records.  tests/test_normalise_gpu.py writes the
stash itself -- through primtest_normalise_g1 / _ed of tests/native/primitives_device.hip, which launch the product's own
kernels -- and compares every output byte with what this module computes on Python integers.

The model is a polynomial map on residues, not a map on curve points:
    G1   x = X ZZ^2 ZZZ^-2,  y = Y ZZZ^-1   (never X / ZZ: the kernels do not assume ZZ^3 = ZZZ^2, and neither do the operands)
         a row is the identity exactly when ZZZ is zero limb by limb -- the one test the kernels make
    Ed   x = X / Z,  y = Y / Z
The operand shapes come from tools/check_lazy_bounds.py NORMALISATION_OPERANDS and shapes(), the table its interval replay
normalisation_formulas() starts from (tests/test_primitives_host.py pins the two together).
"""
import random

import numpy as np

import lazy_model as M
import pyref as R

B = M.B
LB, MASK = M.LB, M.MASK

# around a wave, a thread's four outputs, a workgroup tree, and several workgroups into k_bm_across
SIZES = (1, 2, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 7)
THREADS, PER_THREAD = 256, 4  # BM_THREADS, BM_K
BLOCK = THREADS * PER_THREAD  # BM_BLOCK
G1_FORMS = {"wire": 0, "mont_flag": 1, "table": 2}  # the form numbers of primtest_normalise_g1
ED_FORMS = {"wire": 0, "table": 1}
REC_WORDS, REC_FLAG = 32, 26  # BM_REC_WORDS, BM_REC_FLAG
MONT64 = 1 << 384  # the radix of MSM377_POINTS_MONT_FLAG coordinates


def stash_shapes(fm):
    """coordinate -> lazy_model.Shape, in stash order, from the proof's table."""
    return [(c, fm.shapes[s]) for c, s in B.NORMALISATION_OPERANDS[fm.name].items()]


# ------------------------------------------------------------------ the model ----

def _le_words(v, nbytes):
    return np.frombuffer(v.to_bytes(nbytes, "little"), dtype=np.uint8)


class G1Expect:
    """What the three forms hold for a stash of XYZZ rows ((n, 52) raw limbs)."""

    def __init__(self, fm, rows):
        p, Ri = fm.P, fm.Rinv
        self.fm, self.pts = fm, []
        for row in np.asarray(rows).tolist():
            X, Y, ZZ, ZZZ = (M.value(row[13 * c : 13 * c + 13]) for c in range(4))
            if not any(row[39:52]):
                self.pts.append(None)
                continue
            assert ZZZ % p, "a stash row with ZZZ = 0 mod p that is not the limb-zero identity has no image"
            zi = pow(ZZZ * Ri, -1, p)
            zz = ZZ * Ri % p
            self.pts.append((X * Ri * zz * zz * zi * zi % p, Y * Ri * zi % p))
        self.inf = np.array([1 if pt is None else 0 for pt in self.pts], dtype=np.uint8)

    def records(self, form):
        p, Rm = self.fm.P, self.fm.R
        out = []
        for pt in self.pts:
            x, y = (0, 1) if pt is None else pt
            if form == "wire":
                out.append(np.concatenate([_le_words(x, 48), _le_words(y, 48)]))
            elif form == "mont_flag":
                flag = np.zeros(8, dtype=np.uint8)
                flag[0] = 1 if pt is None else 0
                out.append(np.concatenate([_le_words(x * MONT64 % p, 48), _le_words(y * MONT64 % p, 48), flag]))
            else:
                w = [0] * REC_WORDS
                if pt is None:
                    w[REC_FLAG] = 1
                else:
                    w[0:13], w[13:26] = M.nform_limbs(x * Rm % p, 13), M.nform_limbs(y * Rm % p, 13)
                out.append(np.array(w, dtype=np.uint32).view(np.uint8))
        return np.stack(out)


class EdExpect:
    """What both forms hold for a stash of extended Edwards rows ((n, 36) raw limbs, canonical, Z != 0)."""

    def __init__(self, fm, rows):
        q = fm.P
        self.fm, self.pts = fm, []
        for row in np.asarray(rows).tolist():
            X, Y, _, Z = (M.value(row[9 * c : 9 * c + 9]) for c in range(4))
            assert max(X, Y, Z) < q and Z, "the Edwards stash holds canonical coordinates and no Z = 0"
            zi = pow(Z, -1, q)
            self.pts.append((X * zi % q, Y * zi % q))

    def records(self, form):
        q, Rm = self.fm.P, self.fm.R
        out = []
        for x, y in self.pts:
            if form == "wire":
                out.append(np.concatenate([_le_words(x, 32), _le_words(y, 32)]))
            else:
                w = [0] * REC_WORDS
                for c, v in enumerate(((y - x) % q, (y + x) % q, 2 * R.ED_D * x * y % q)):
                    w[9 * c : 9 * c + 9] = M.nform_limbs(v * Rm % q, 9)
                out.append(np.array(w, dtype=np.uint32).view(np.uint8))
        return np.stack(out)


# ------------------------------------------------------------------ operand rows ----

def _row(fm, vals):
    return [x for v in vals for x in (v if isinstance(v, list) else M.nform_limbs(v, fm.N))]


def _in_box(fm, shapes, row):
    n = fm.N
    return all(sh.holds(row[n * c : n * c + n]) for c, (_, sh) in enumerate(shapes))


def random_rows(fm, count, seed, nonzero_last=True):
    """Seeded random in-box rows: every limb of every coordinate from {0, its maximum, uniform} (lazy_model's generator);
    the last coordinate (ZZZ, Z) never 0 mod p."""
    shapes = stash_shapes(fm)
    cols = []
    for c, (_, sh) in enumerate(shapes):
        v = fm.vectors(sh, 1000 * seed + c, count + 64)[fm.n_edges :]
        if c == len(shapes) - 1 and nonzero_last:
            v = [x for x in v if M.value(x) % fm.P]
        cols.append(v[:count])
    rows = [sum((cols[c][i] for c in range(len(shapes))), []) for i in range(count)]
    assert len(rows) == count and all(_in_box(fm, shapes, r) for r in rows)
    return rows


def tile(rows, n, offset=0):
    """n stash rows: the family's rows over and over, from `offset` on."""
    return np.array([rows[(offset + i) % len(rows)] for i in range(n)], dtype=np.uint32)


def g1_corner_rows(fm):
    """[(label, row)]: every coordinate at the inclusive per-limb maxima of its box -- all at once, and each alone beside
    random in-box coordinates -- and the value-maximal representatives x + k p (k = 0 .. 5 for X, 0 .. 1 for the others)
    while below the box bound."""
    shapes = stash_shapes(fm)
    assert [c for c, _ in shapes] == ["X", "Y", "ZZ", "ZZZ"]
    p, e = fm.P, fm.E
    fill = random_rows(fm, 64, 7)
    out = [("all corners", sum((sh.box for _, sh in shapes), []))]
    k = 0

    def beside(c, limbs, label):
        nonlocal k
        row = list(fill[k % len(fill)])
        k += 1
        row[13 * c : 13 * c + 13] = limbs
        out.append((label, row))

    for c, (name, sh) in enumerate(shapes):
        beside(c, sh.box, name + " corner")
        reps = [(v, kk) for v in (p - 1, e - 1) for kk in range(6 if c == 0 else 2) if v + kk * p < sh.hi]
        assert (e - 1, 5 if c == 0 else 1) in reps  # hi - 1 itself
        for v, kk in reps:
            beside(c, M.nform_limbs(v + kk * p, 13), "%s = %s + %d p" % (name, "p - 1" if v == p - 1 else "e - 1", kk))
    out.append(("all value maxima", _row(fm, [sh.hi - 1 for _, sh in shapes])))
    for label, row in out:
        assert _in_box(fm, shapes, row) and M.value(row[39:52]) % p, label
    return out


def g1_zero_rows(fm):
    """[(label, row)]: every representative of a zero coordinate the boxes admit -- X in {0, p, .., 5p} (a point with
    x = 0), Y in {0, p} (y = 0): the outputs must be THE canonical 0 -- and identities: ZZ = ZZZ = 0 limb by limb beside
    arbitrary X and Y, corners included.  Last, the two rows that say WHICH coordinate the kernels test: ZZZ = 0 with
    ZZ != 0 is an identity, ZZ = 0 (or p) with ZZZ != 0 is not (x = 0, y = Y / ZZZ)."""
    shapes = stash_shapes(fm)
    p = fm.P
    fill = random_rows(fm, 32, 11)
    out = []
    for i, f in enumerate(fill[:6]):
        out.append(("X = %d p" % i, _row(fm, [i * p]) + f[13:]))
    for i, y in enumerate((0, p)):
        out.append(("Y = %s" % ("p" if y else "0"), fill[6 + i][:13] + _row(fm, [y]) + fill[6 + i][26:]))
        out.append(("X = %d p, Y = %s" % (3 * i, "p" if y else "0"), _row(fm, [3 * i * p, y]) + fill[8 + i][26:]))
    zero = [0] * 13
    for i in range(4):
        out.append(("identity, random X, Y", fill[10 + i][:26] + zero + zero))
    out.append(("identity, X, Y at their corners", shapes[0][1].box + shapes[1][1].box + zero + zero))
    out.append(("identity()", _row(fm, [0, fm.R % p, 0, 0])))
    out.append(("ZZZ = 0, ZZ != 0: an identity", fill[14][:39] + zero))
    out.append(("ZZ = 0, ZZZ != 0: not an identity", fill[15][:26] + zero + fill[15][39:]))
    out.append(("ZZ = p, ZZZ != 0: not an identity", fill[16][:26] + _row(fm, [p]) + fill[16][39:]))
    for label, row in out:
        assert _in_box(fm, shapes, row), label
    return out


def identity_placements(n):
    """[(label, lanes)]: where identities sit among n outputs -- the wave, thread and workgroup seams and the last lane;
    all four outputs of one thread; one whole workgroup; every output of the call.  Only placements that fit n."""
    out = [("seams", sorted({i for i in (0, 63, 64, 255, 256, n - 1) if i < n})), ("all", list(range(n)))]
    for blk, tid in ((0, 5), ((n - 1) // BLOCK, 0)):
        lanes = [blk * BLOCK + j * THREADS + tid for j in range(PER_THREAD)]
        if lanes[-1] < n:
            out.append(("all four outputs of thread %d of workgroup %d" % (tid, blk), lanes))
    if n > BLOCK:
        out.append(("workgroup 0", list(range(BLOCK))))
        if n > 2 * BLOCK:
            out.append(("workgroup 1", list(range(BLOCK, 2 * BLOCK))))
    return out


def with_identities(fm, rows, lanes):
    rows = np.array(rows, dtype=np.uint32)
    w = rows.shape[1] // 2
    rows[lanes, w:] = 0  # ZZ = ZZZ = 0 limb by limb; X and Y stay whatever they were
    return rows


def steered_values(fm):
    """[(label, a)]: residues the chunk product -- the operand of the ONE inversion in k_bm_across / k_edbm_across -- is
    steered to: the Montgomery 1, 2, p - 1, 2^j, and the inputs with the smallest and the largest k of the whole
    inverse_mont case list (lazy_model.inverse_cases, the k-model)."""
    p, Rm = fm.P, fm.R
    top = 376 if fm.name == "Fp" else 252
    out = [("R", Rm % p), ("2 R", 2 * Rm % p), ("(p - 1) R", (p - 1) * Rm % p)] + [("2^%d R" % j, (1 << j) * Rm % p) for j in (1, 29, top)]
    cases = [(a % p, k) for a, k, _ in M.inverse_cases(fm)]
    for which, (a, k) in (("smallest", min(cases, key=lambda t: t[1])), ("largest", max(cases, key=lambda t: t[1]))):
        out.append(("%s k = %d" % (which, k), a))
    out += [(label, a % p) for a, _, label in M.inverse_cases(fm) if "of the scan" in label]  # and the extremes among random residues
    assert len(out) == 10
    return out


def chunk_product(fm, rows):
    """The residue the inversion sees for these stash rows: the Montgomery-form product of the last coordinate of every
    row that is no identity (every 1 the kernels put in leaves it unchanged)."""
    n = fm.N
    t = 1
    for row in np.asarray(rows).tolist():
        if any(row[3 * n : 4 * n]):
            t = t * M.value(row[3 * n : 4 * n]) * fm.Rinv % fm.P
    return t * fm.R % fm.P


def steered_rows(fm, a, n, seed):
    """n random in-box rows whose last coordinates multiply to the stored residue a (row n - 1 takes what is missing)."""
    rows = random_rows(fm, n, seed)
    w = fm.N
    rest = chunk_product(fm, rows[: n - 1]) if n > 1 else fm.R % fm.P
    last = a * fm.R * pow(rest, -1, fm.P) % fm.P  # a / R = (rest / R) (last / R)
    rows[n - 1][3 * w :] = M.nform_limbs(last, w)
    assert chunk_product(fm, rows) == a % fm.P
    return np.array(rows, dtype=np.uint32)


def ed_value_rows(fm):
    """[(label, row)] for the Edwards stash: coordinates from {0, 1, q - 1, the canonical corner}, Z never 0; identities
    as (0 : c : 0 : c)."""
    q = fm.P
    corner = M.value(fm.shapes["canonical"].box)
    assert corner < q
    rnd = random.Random("ed-stash")
    vals = [0, 1, q - 1, corner, fm.R % q]
    out = []
    for x in vals:
        for y in vals:
            for z in vals[1:]:
                out.append(("X = %#x Y = %#x Z = %#x" % (x, y, z), _row(fm, [x, y, rnd.randrange(q), z])))
    for c in (1, q - 1, corner, rnd.randrange(1, q)):
        out.append(("identity (0 : c : 0 : c)", _row(fm, [0, c, 0, c])))
    out.append(("all corners", _row(fm, [corner] * 4)))
    return out
