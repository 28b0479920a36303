"""Crafted scalars for the GLV front end k -> (k1, k2), k = k1 + lambda k2 (TEST INFRASTRUCTURE; Python integers only).

Shared by tests/test_stage_model_host.py (csrc/glv_split.hpp compiled for the host) and tests/test_glv_front_end_gpu.py
(k_decompose_glv as run), so that both see the same multiples of lambda, the same half-digit boundaries and the same edge
of the GLV range.  floor(k MU / 2^384) is one less than k // lambda exactly for k = m lambda, m >= 1: those are the only
inputs that reach the correction arm of the Barrett quotient."""
import random

import stage_model as M

LAM = M.glv_consts()[0]
BOUNDARY_WORDS = (0x0000, 0x0001, 0x7FFF, 0x8000, 0xFFFF)  # stored limbs that give the digits 0, +1, 2^15 - 1, -2^15, -1
# The largest half the digit chain takes: digits in [-2^15, 2^15 - 1] below a non-negative top digit reach at most
# sum (2^15 - 1) 2^(16 w); anything above carries into a top digit of 2^15.
HALF_MAX = sum(0x7FFF << (16 * w) for w in range(8))
# ... and the largest half whose window 6 carries into window 7: top limb 0x7FFE + 1.
HALF_MAX_CARRIED = (0x7FFE << 112) | ((1 << 112) - 1)
EDGE = (LAM - 1) + LAM * HALF_MAX          # the largest scalar that splits
EDGE_CARRIED = (LAM - 1) + LAM * HALF_MAX_CARRIED
BEYOND = EDGE + 1                          # = lambda (HALF_MAX + 1): the smallest step that does not


def lambda_factors(rnd, count):
    """m for k = m lambda + t: 0, 1, 2; 2^j - 1, 2^j, 2^j + 1 for every j up to 129; lambda - 1, lambda, lambda + 1; the
    largest m with k < 2^256; factors whose low words are all ones or all zeros (the increment of q = m - 1 carries
    across words exactly for the zeros; the ones see no carry at all); `count` random ones of every length."""
    ms = [0, 1, 2]
    for j in range(130):
        ms += [(1 << j) - 1, 1 << j, (1 << j) + 1]
    ms += [LAM - 1, LAM, LAM + 1, ((1 << 256) - 1) // LAM]
    for words in (1, 2, 3, 4):
        for _ in range(8):
            hi = rnd.getrandbits(126 - 32 * words + 3) << (32 * words)
            ms += [hi | ((1 << (32 * words)) - 1), hi, hi + (1 << (32 * words))]
    ms += [1 + rnd.getrandbits(rnd.randrange(1, 130)) for _ in range(count)]  # 1 .. 2^129: m lambda < 2^256
    return ms


def around_multiples(ms):
    """m lambda + t for t in -2 .. 2, as far as it is a 256-bit scalar."""
    return [m * LAM + t for m in ms for t in (-2, -1, 0, 1, 2) if 0 <= m * LAM + t < (1 << 256)]


def half_with(rnd, win, word, top_below=1 << 16):
    """A 128-bit half with `word` in window `win` and random words elsewhere (window 7 below top_below)."""
    v = 0
    for w in range(8):
        limb = word if w == win else rnd.randrange(top_below) if w == 7 else rnd.getrandbits(16)
        v |= limb << (16 * w)
    return v


def boundary_halves(rnd, per):
    """k = k1 + lambda k2 with every boundary word in every window of k2 (k1 random below lambda) and of k1 (reduced mod
    lambda; its top window kept below lambda's where the planted window is another one, so the word stays where it is;
    k2 random below 2^127).  `per` scalars per (half, window, word)."""
    ks = []
    for win in range(8):
        for word in BOUNDARY_WORDS:
            for _ in range(per):
                ks.append(rnd.randrange(LAM) + LAM * half_with(rnd, win, word))
                ks.append(half_with(rnd, win, word, top_below=LAM >> 112) % LAM + LAM * rnd.getrandbits(127))
    return [k for k in ks if k < (1 << 256)]


BOUNDARY_DIGITS = (0, 1, -1, (1 << 15) - 1, -(1 << 15))


def half_with_digit(rnd, win, digit, below):
    """A half below `below` whose signed digit in window `win` is `digit`: random digits elsewhere, the top one
    non-negative.  None where no such half exists (a negative top digit; a top digit beyond the bound's)."""
    if win == 7 and (digit < 0 or digit << 112 >= below):
        return None
    while True:
        ds = [rnd.randrange(-(1 << 15), 1 << 15) for _ in range(7)] + [rnd.randrange(min(1 << 15, below >> 112))]
        ds[win] = digit
        v = sum(d << (16 * w) for w, d in enumerate(ds))
        if 0 <= v < below:
            return v


def boundary_digits(rnd):
    """[(k, position, digit)]: k = k1 + lambda k2 with `digit` at `position` (0..7 in k1, 8..15 in k2) of its sixteen
    signed digits, for every position and every boundary digit that position can hold."""
    out = []
    for pos in range(16):
        for d in BOUNDARY_DIGITS:
            if pos < 8:
                k1, k2 = half_with_digit(rnd, pos, d, LAM), half_with_digit(rnd, 0, rnd.randrange(-(1 << 15), 1 << 15), HALF_MAX + 1)
            else:
                k1, k2 = rnd.randrange(LAM), half_with_digit(rnd, pos - 8, d, HALF_MAX + 1)
            if k1 is not None and k2 is not None:
                out.append((k1 + LAM * k2, pos, d))
    return out


def rng(tag):
    return random.Random("glv-cases/" + tag)
