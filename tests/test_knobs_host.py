"""Knobs::from_env() (csrc/knobs.hpp): the one table that turns the MSM377_* environment into a context's tunables.
tests/native/knobs_host.cpp is compiled with g++ and the address / undefined-behaviour sanitizers against the header (a
stand-alone program: nothing is loaded into python) and prints every field under the environment it is started in.  The
expected values are written out here by hand, from the getenv lines msm377_ctx_create had before the table existed
(atoi / atoll / strtoull with the clamp each line carried inline), not from the table.  CPU only."""
import os
import subprocess

import pytest

import util

ROOT = util.ROOT
CSRC = os.path.join(ROOT, "webgpu-msm-bls12-377_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "knobs_host.cpp")
OUT = os.path.join(ROOT, "tests", "native", "_build")

DEFAULTS = {
    "glv_mode": 0, "g1_form": 1, "conv_wave_prio": 1, "aff_prewake_us": 600, "upload_chunks": 4, "upload_split_pct": 30,
    "upload_chunk_min": 1 << 18, "tail_threads": 6, "tail_wait_ms": 2000, "tail_spin_us": 1000, "tail_trace": 0, "tail_numa": 1,
    "te_affine_msm": 1, "narrow_max_points": 1 << 16, "precomp_bits": 16, "affine_min_points": 1 << 20, "seg_plain": 0, "seg_glv": 0,
    "zc_out": 1, "narrow_seg": 0, "narrow_quad_items": 100000, "coop_threads": 131072, "narrow_tail_from": 4, "tail_lds": 1,
    "reduce_columns": 1, "even_windows": 1, "sort_elem": 8, "twin_batches": 1, "base_checks": 0, "tail_from": 7,
}  # fmt: skip

# variable -> the field it writes
FIELD = {
    "MSM377_GLV": "glv_mode", "MSM377_G1_FORM": "g1_form", "MSM377_CONV_WAVE_PRIO": "conv_wave_prio", "MSM377_AFF_PREWAKE_US": "aff_prewake_us",
    "MSM377_UPLOAD_CHUNKS": "upload_chunks", "MSM377_UPLOAD_SPLIT": "upload_split_pct", "MSM377_UPLOAD_CHUNK_MIN": "upload_chunk_min",
    "MSM377_TAIL_THREADS": "tail_threads", "MSM377_TAIL_WAIT_MS": "tail_wait_ms", "MSM377_TAIL_SPIN_US": "tail_spin_us", "MSM377_TAIL_TRACE": "tail_trace",
    "MSM377_TAIL_NUMA": "tail_numa", "MSM377_TE_AFFINE_MSM": "te_affine_msm", "MSM377_NARROW_MAX": "narrow_max_points", "MSM377_PRECOMP_BITS": "precomp_bits",
    "MSM377_AFFINE_MIN": "affine_min_points", "MSM377_SEG_PLAIN": "seg_plain", "MSM377_SEG_GLV": "seg_glv", "MSM377_ZERO_COPY_OUT": "zc_out",
    "MSM377_NARROW_SEG": "narrow_seg", "MSM377_NARROW_QUAD_ITEMS": "narrow_quad_items", "MSM377_COOP_THREADS": "coop_threads",
    "MSM377_NARROW_TAIL_FROM": "narrow_tail_from", "MSM377_TAIL_LDS": "tail_lds", "MSM377_REDUCE_COLUMNS": "reduce_columns", "MSM377_EVEN_WINDOWS": "even_windows",
    "MSM377_SORT_ELEM": "sort_elem", "MSM377_TWIN_BATCH": "twin_batches", "MSM377_BASE_CHECKS": "base_checks", "MSM377_TAIL_FROM": "tail_from",
}  # fmt: skip
assert sorted(FIELD.values()) == sorted(DEFAULTS)

# every variable at an ordinary value: (text, value read)
ORDINARY = {
    "MSM377_GLV": ("1", 1), "MSM377_G1_FORM": ("0", 0), "MSM377_CONV_WAVE_PRIO": ("0", 0), "MSM377_AFF_PREWAKE_US": ("250", 250),
    "MSM377_UPLOAD_CHUNKS": ("5", 5), "MSM377_UPLOAD_SPLIT": ("40", 40), "MSM377_UPLOAD_CHUNK_MIN": ("524288", 524288),
    "MSM377_TAIL_THREADS": ("3", 3), "MSM377_TAIL_WAIT_MS": ("500", 500), "MSM377_TAIL_SPIN_US": ("0", 0), "MSM377_TAIL_TRACE": ("1", 1),
    "MSM377_TAIL_NUMA": ("0", 0), "MSM377_TE_AFFINE_MSM": ("0", 0), "MSM377_NARROW_MAX": ("1024", 1024), "MSM377_PRECOMP_BITS": ("20", 20),
    "MSM377_AFFINE_MIN": ("4096", 4096), "MSM377_SEG_PLAIN": ("32", 32), "MSM377_SEG_GLV": ("64", 64), "MSM377_ZERO_COPY_OUT": ("0", 0),
    "MSM377_NARROW_SEG": ("16", 16), "MSM377_NARROW_QUAD_ITEMS": ("5000", 5000), "MSM377_COOP_THREADS": ("1048576", 1048576),
    "MSM377_NARROW_TAIL_FROM": ("3", 3), "MSM377_TAIL_LDS": ("0", 0), "MSM377_REDUCE_COLUMNS": ("0", 0), "MSM377_EVEN_WINDOWS": ("0", 0),
    "MSM377_SORT_ELEM": ("4", 4), "MSM377_TWIN_BATCH": ("0", 0), "MSM377_BASE_CHECKS": ("4", 7), "MSM377_TAIL_FROM": ("6", 6),
}  # fmt: skip

# the ranged variables: (text below, value read, text above, value read).  SEG_MIN..SEG_MAX = 16..128, NARROW_SEG..SEG_BINS - 1
# = 8..128, TREE_LEVELS = 15, TailPool::WORKERS + 1 = 8; MSM377_TAIL_WAIT_MS has a lower end only.
RANGED = {
    "MSM377_UPLOAD_CHUNKS": ("1", 2, "8", 7), "MSM377_UPLOAD_SPLIT": ("4", 5, "91", 90), "MSM377_TAIL_THREADS": ("0", 1, "9", 8),
    "MSM377_TAIL_WAIT_MS": ("0", 1, "100000", 100000), "MSM377_SEG_PLAIN": ("15", 16, "129", 128), "MSM377_SEG_GLV": ("-3", 16, "1000", 128),
    "MSM377_NARROW_SEG": ("7", 8, "129", 128), "MSM377_NARROW_TAIL_FROM": ("0", 1, "16", 15), "MSM377_TAIL_FROM": ("-1", 1, "99", 15),
}  # fmt: skip

# what every variable reads from text that atoi / atoll / strtoull / strtoul turn into 0
ZERO_TEXT = dict(DEFAULTS, glv_mode=0, g1_form=0, conv_wave_prio=0, aff_prewake_us=0, upload_chunks=2, upload_split_pct=5, upload_chunk_min=0,
                 tail_threads=1, tail_wait_ms=1, tail_spin_us=0, tail_trace=0, tail_numa=0, te_affine_msm=0, narrow_max_points=0, precomp_bits=16,
                 affine_min_points=0, seg_plain=16, seg_glv=16, zc_out=0, narrow_seg=8, narrow_quad_items=0, coop_threads=0, narrow_tail_from=1,
                 tail_lds=0, reduce_columns=0, even_windows=0, sort_elem=8, twin_batches=0, base_checks=0, tail_from=1)  # fmt: skip


@pytest.fixture(scope="module")
def exe():
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "knobs_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I", CSRC, "-o", path, SRC]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return path


def knobs(exe, **env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MSM377_")}
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(clean, **env))
    assert res.returncode == 0, res.stderr
    got = {}
    for line in res.stdout.splitlines():
        name, value = line.split()
        got[name] = int(value)
    assert list(got) == list(DEFAULTS)  # every field, once, in the struct's order
    return got


def test_defaults(exe):
    assert knobs(exe) == DEFAULTS


def test_every_variable_at_an_ordinary_value(exe):
    env = {var: text for var, (text, _) in ORDINARY.items()}
    assert set(env) == set(FIELD)
    assert knobs(exe, **env) == {FIELD[var]: value for var, (_, value) in ORDINARY.items()}
    for var, (text, value) in ORDINARY.items():  # and each one alone moves its own field only
        assert knobs(exe, **{var: text}) == dict(DEFAULTS, **{FIELD[var]: value}), var


def test_ranged_variables_clamp(exe):
    below = knobs(exe, **{var: r[0] for var, r in RANGED.items()})
    above = knobs(exe, **{var: r[2] for var, r in RANGED.items()})
    assert below == dict(DEFAULTS, **{FIELD[var]: r[1] for var, r in RANGED.items()})
    assert above == dict(DEFAULTS, **{FIELD[var]: r[3] for var, r in RANGED.items()})
    ends = {"MSM377_UPLOAD_CHUNKS": (2, 7), "MSM377_UPLOAD_SPLIT": (5, 90), "MSM377_TAIL_THREADS": (1, 8), "MSM377_SEG_PLAIN": (16, 128), "MSM377_SEG_GLV": (16, 128),
            "MSM377_NARROW_SEG": (8, 128), "MSM377_NARROW_TAIL_FROM": (1, 15), "MSM377_TAIL_FROM": (1, 15)}  # fmt: skip
    for k in (0, 1):  # the ends themselves are inside
        got = knobs(exe, **{var: str(e[k]) for var, e in ends.items()})
        assert got == dict(DEFAULTS, **{FIELD[var]: e[k] for var, e in ends.items()})


@pytest.mark.parametrize(
    "var, text, value",
    [
        ("MSM377_PRECOMP_BITS", "19", 16),  # 20, or else 16
        ("MSM377_PRECOMP_BITS", "21", 16),
        ("MSM377_SORT_ELEM", "5", 8),  # 4, or else 8
        ("MSM377_SORT_ELEM", "0", 8),
        ("MSM377_BASE_CHECKS", "0x9", 0),  # a bit outside MSM377_CHECK_ALL: an invalid mask reads as 0
        ("MSM377_BASE_CHECKS", "8", 0),
        ("MSM377_BASE_CHECKS", "010", 0),  # strtoul base 0: octal 8
        ("MSM377_BASE_CHECKS", "0x2", 3),  # normalised: the curve check needs the canonical one
        ("MSM377_BASE_CHECKS", "1", 1),
        ("MSM377_BASE_CHECKS", "0x5", 7),
        ("MSM377_GLV", "2", 2),  # a raw atoi (the setter maps 2 to 0, the environment does not)
        ("MSM377_GLV", "-1", -1),
        ("MSM377_G1_FORM", "7", 1),  # != 0
        ("MSM377_ZERO_COPY_OUT", "5", 5),  # a raw atoi
        ("MSM377_COOP_THREADS", "-1", 0xFFFFFFFF),  # (uint32_t)atoi
        ("MSM377_NARROW_MAX", "12abc", 12),  # strtoull stops at the first non-digit
        ("MSM377_UPLOAD_CHUNKS", "3.9", 3),
        ("MSM377_AFF_PREWAKE_US", "-7", -7),  # atoll, no clamp
        ("MSM377_TAIL_WAIT_MS", "-5", 1),
    ],
)
def test_odd_cases(exe, var, text, value):
    assert knobs(exe, **{var: text}) == dict(DEFAULTS, **{FIELD[var]: value})


@pytest.mark.parametrize("text", ["", "abc", " ", "x20"])
def test_text_that_reads_as_zero(exe, text):
    assert knobs(exe, **{var: text for var in FIELD}) == ZERO_TEXT
    for var in FIELD:
        if text == "":  # one at a time, once
            assert knobs(exe, **{var: text}) == dict(DEFAULTS, **{FIELD[var]: ZERO_TEXT[FIELD[var]]}), var
