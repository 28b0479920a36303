"""The launch plan of the bucket reduction's column kernel (csrc/kernels/reduce.hpp k_tree_columns, sequencer.hip
enqueue_reduce) as a plain model: lanes, their (lower, upper) pairs and the exchanges between steps, exactly as the kernel
indexes them, against the per-level plan of k_tree_step.  For every bucket_log the stage serves and every tail_from:

  * the multiset of (level, lower index, upper index) additions of the column plan equals the per-level plan's;
  * every index the next stage reads -- the next column launch, the per-level tail, or the gather kernel -- is among the
    ones the column launch stores, and a launch stores nothing else;
  * run on values (a non-commutative stand-in for the addition; empty buckets under k_tree_step's identity rule below
    the level from which the per-level launches use k_tree_step_quad, which adds them like any other bucket), the
    buckets every later stage reads come out the same as from the per-level plan.

No GPU: tests/test_reduce_columns_gpu.py runs the kernel itself."""
import numpy as np
import pytest

COLUMN_LEVELS_MAX = 4  # reduce.hpp
COOP_THREADS = 131072  # knobs.hpp
MASK = (1 << 64) - 1


def coop_from(L, windows):
    """sequencer.hip: the first level whose additions, four lanes each, fit COOP_THREADS."""
    r = 0
    while r < L and 4 * (r + 1) * ((1 << L) >> (r + 1)) * windows > COOP_THREADS:
        r += 1
    return r


def add_rule(lo, up, rule=True):
    """k_tree_step's rule on uint64 stand-ins (0 = a stored identity): upper empty -> lower unchanged, lower empty ->
    the upper one, else an 'addition' that is neither commutative nor associative, so operand order and versions count."""
    with np.errstate(over="ignore"):
        mixed = (lo * np.uint64(0x9E3779B97F4A7C15) + up * np.uint64(0xC2B2AE3D27D4EB4F) + np.uint64(0x165667B19E3779F9)) | np.uint64(1)
    return np.where(up == 0, lo, np.where(lo == 0, up, mixed)) if rule else mixed


def level_pairs(L, r):
    """(lower, upper) bucket indices of level r, k_tree_step's index scheme."""
    NB = 1 << L
    half = NB >> (r + 1)
    g = np.arange((r + 1) * half, dtype=np.int64)
    oi, kk = g // half, g % half
    lo = np.where(oi == 0, 0, NB >> np.maximum(oi, 1))
    x = lo + kk
    return x, x + half


def per_level(b, L, first, last, log=None, quad_from=99):
    for r in range(first, last):
        x, y = level_pairs(L, r)
        b[x] = add_rule(b[x], b[y], r < quad_from)
        if log is not None:
            log.append(np.stack([np.full_like(x, r), x, y], axis=1))


def column_launch(b, L, r0, k, log, quad_from=99):
    """One k_tree_columns launch on bucket values b (in place); returns the indices it stored."""
    NB = 1 << L
    H, stride = 1 << (k - 1), NB >> (r0 + k)
    threads = (r0 + 1) * (NB >> (r0 + 1))  # per window, as the sequencer computes it
    assert threads % H == 0 and 64 % H == 0, "whole groups inside a wave"
    g = np.arange(threads, dtype=np.int64)
    i, col = g & (H - 1), g >> (k - 1)
    arr, c = col // stride, col % stride
    assert arr.max() == r0
    base = np.where(arr == 0, 0, NB >> np.maximum(arr, 1)) + c
    row_lo, row_up = i.copy(), i + H
    lo, up = b[base + row_lo * stride].copy(), b[base + row_up * stride].copy()
    live = np.ones(threads, dtype=bool)
    for s in range(k):
        if s:
            m = H >> s
            low = (i & m) == 0
            src = g ^ m  # the partner lane: same group, same wave
            assert np.array_equal(src >> (k - 1), col)
            got, got_row = np.where(low, up, lo)[src], np.where(low, row_up, row_lo)[src]
            keep, keep_row = np.where(low, lo, up), np.where(low, row_lo, row_up)
            lo, up = np.where(low, keep, got), np.where(low, got, keep)
            row_lo, row_up = np.where(low, keep_row, got_row), np.where(low, got_row, keep_row)
            live = live & (low | ((arr == 0) & (i < 2 * m)))
        lo = np.where(live, add_rule(lo, up, r0 + s < quad_from), lo)
        log.append(np.stack([np.full(int(live.sum()), r0 + s), (base + row_lo * stride)[live], (base + row_up * stride)[live]], axis=1))
    heads = (arr == 0) & (i == 0)
    stored = np.concatenate([(base + row_lo * stride)[live], (base + row_up * stride)[heads]])
    assert len(np.unique(stored)) == len(stored), "no bucket is stored twice"
    b[(base + row_lo * stride)[live]] = lo[live]
    b[(base + row_up * stride)[heads]] = up[heads]
    return stored


def reads_after(L, r):
    """Bucket indices the stage behind level r - 1 reads: both operands of level r, or the gather kernel's heads."""
    if r < L:
        x, y = level_pairs(L, r)
        return np.concatenate([x, y])
    return np.array([0] + [1 << l for l in range(L)], dtype=np.int64)


def sorted_rows(chunks):
    a = np.concatenate(chunks)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


def plan(tail_from):
    r, out = 0, []
    while r < tail_from:
        k = min(tail_from - r, COLUMN_LEVELS_MAX)
        out.append((r, k))
        r += k
    return out


def cases():
    """(bucket_log, tail_from, windows): the window count decides from which level the per-level launches use lane quads"""
    out = []
    for L, windows in ((11, 22), (15, 16)):  # narrow and main path: MSM377_NARROW_TAIL_FROM / MSM377_TAIL_FROM accept 1..15, capped at L
        out += [(L, t, windows) for t in range(1, L + 1)]
    out += [(15, 7, 1), (15, 7, 2)]  # a folded table (wc_out = 1), a shard of two windows
    out.append((19, 11, 1))  # the wide window: tail_from = L - 8, not a setting
    return out


def test_plans_the_code_uses():
    assert (coop_from(15, 16), coop_from(11, 22), coop_from(15, 1), coop_from(19, 1)) == (6, 0, 0, 6)
    assert plan(7) == [(0, 4), (4, 3)]  # main path
    assert plan(4) == [(0, 4)]  # narrow path
    assert plan(11) == [(0, 4), (4, 4), (8, 3)]  # wide window


@pytest.mark.parametrize("L,tail_from,windows", cases())
def test_column_plan_equals_per_level_plan(L, tail_from, windows):
    NB = 1 << L
    qf = coop_from(L, windows)
    rng = np.random.default_rng(L * 100 + tail_from)
    start = rng.integers(1, MASK, size=NB, dtype=np.uint64)
    start[rng.random(NB) < 0.3] = 0  # empty buckets: both identity branches
    start[NB - NB // 8 :] = 0  # ... and whole waves of them, like the top window
    ref, ref_log = start.copy(), []
    per_level(ref, L, 0, tail_from, ref_log, qf)
    got, got_log = start.copy(), []
    for r0, k in plan(tail_from):
        assert 1 <= k <= COLUMN_LEVELS_MAX and r0 + k <= L
        stored = column_launch(got, L, r0, k, got_log, qf)
        needed = np.unique(reads_after(L, r0 + k))
        assert np.array_equal(np.sort(stored), needed), (r0, k)  # stores exactly what is read later
        assert np.array_equal(got[needed], per_level_prefix(start, L, r0 + k, qf)[needed]), (r0, k)
    assert np.array_equal(sorted_rows(got_log), sorted_rows(ref_log))
    # the rest of the stage (the single-launch tail does the per-level additions) and what the gather kernel reads
    per_level(ref, L, tail_from, L, None, 0)
    per_level(got, L, tail_from, L, None, 0)
    heads = reads_after(L, L)
    assert np.array_equal(got[heads], ref[heads])
    assert ref[0] != 0


def per_level_prefix(start, L, upto, quad_from):
    b = start.copy()
    per_level(b, L, 0, upto, None, quad_from)
    return b
