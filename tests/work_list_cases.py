"""Skewed inputs for tests/test_work_list_gpu.py (TEST INFRASTRUCTURE; the model is tests/stage_model.py): scalars drawn from
eleven distinct values whose multiplicities are the row lengths at which the accumulation work list changes shape for a
work-item length S -- 1, S - 1, S, S + 1, 2S, 2S + 1, 3S - 1, 31S + 1, 32S, 32S + 1, 33S + 5: 138 S + 8 points.  The values
have pairwise different non-zero sort keys in every window slot of the case's geometry, so EVERY slot holds rows of
exactly these lengths (behind the GLV front end each twice, on the wide table thirteen times in its one slot).
tests/test_stage_model_host.py pins what a case promises on the CPU; the GPU test asserts it again before it launches."""
import random
from typing import List, NamedTuple

import numpy as np

import pyref as R
import stage_model as M


def multiplicities(S: int) -> List[int]:
    return [1, S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S - 1, 31 * S + 1, 32 * S, 32 * S + 1, 33 * S + 5]


def slot_keys(k: int, g: M.Geometry):
    """Per window slot, the sort keys |digit| one scalar contributes; None if the scalar does not fit the geometry."""
    rec = M.recode(k, g)
    if rec.flags:
        return None
    if g.name == "glv8":
        return [[abs(rec.digits[w]), abs(rec.digits[8 + w])] for w in range(8)]
    if g.name == "wide13":
        return [[abs(d) for d in rec.digits]]
    return [[abs(d)] for d in rec.digits]


def distinct_values(g: M.Geometry, count: int, seed, bound: int) -> List[int]:
    """`count` scalars below `bound` whose keys are non-zero and pairwise different in every slot."""
    rnd = random.Random("work list values/%s/%s" % (g.name, seed))
    taken = None
    out = []
    while len(out) < count:
        k = rnd.randrange(1, bound)
        keys = slot_keys(k, g)
        if keys is None:
            continue
        taken = taken if taken is not None else [set() for _ in keys]
        if any(0 in ks or len(set(ks)) != len(ks) or taken[s] & set(ks) for s, ks in enumerate(keys)):
            continue
        for s, ks in enumerate(keys):
            taken[s] |= set(ks)
        out.append(k)
    return out


class Case(NamedTuple):
    S: int
    g: M.Geometry
    scalars: List[int]
    other: List[int]      # for the call before, on the same context: same size, other values
    lengths: List[int]    # the row lengths every slot holds


def skewed(g: M.Geometry, S: int, seed=0, bound: int = R.R_ORDER) -> Case:
    mult = multiplicities(S)
    out = []
    for which in ("case", "other"):
        values = distinct_values(g, len(mult), "%s/%d/%s" % (which, S, seed), bound)
        ks = [v for v, m in zip(values, mult) for _ in range(m)]
        random.Random("work list order/%s/%d/%s" % (which, S, seed)).shuffle(ks)
        out.append(ks)
    return Case(S, g, out[0], out[1], mult)


def row_lengths(g: M.Geometry, cols):
    """Entries per row of every window slot of a pass, rows in the work list's numbering: row = slot 2^L + t for bucket t
    (key t + 1).  Key 0 (digit 0) is no row."""
    count = 1 if g.name == "wide13" else len(g.slots)
    lens = []
    for slot in range(count):
        s = g.slots[-1] if g.name == "wide13" else g.slots[slot]
        lens.append(M.csr(cols[slot], g.bucket_log, s.bias, s.key_unsigned).counts[1:])
    return np.concatenate(lens)


def check_promises(case: Case, row_lens, wl: M.WorkList, slots):
    """What the issue asks of every slot read, from the model alone: a row at each of the case's lengths, rows of 32 and of
    33 work items, and (S > 16) at least three occupied histogram bins above 16."""
    NB = 1 << case.g.bucket_log
    for slot in slots:
        lens = row_lens[slot * NB : (slot + 1) * NB]
        have = sorted(int(x) for x in lens[lens > 0])
        per = {"glv8": 2, "wide13": 13}.get(case.g.name, 1)
        assert have == sorted(case.lengths * per), (case.S, case.g.name, slot, have)
        nsegs = {M.row_split(x, case.S).nseg for x in have}
        assert {32, 33} <= nsegs, (case.S, case.g.name, slot, sorted(nsegs))
    if case.S > 16:
        assert sum(1 for b in range(17, M.SEG_BINS) if wl.hist[b]) >= 3, (case.S, wl.hist)
