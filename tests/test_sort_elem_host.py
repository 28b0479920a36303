"""csrc/common.hpp, host-only: the packed 4-byte sort_temp element (SortElem4: sign | sub | column index) and the rule that
chooses between it and the 8-byte SortElem (sort_elem_bytes).  tests/native/sort_elem_host.cpp is compiled with g++ against
the header and asked for single values.  CPU only; the kernels that use the element: tests/test_sort_elem_gpu.py."""
import itertools
import os
import subprocess

import pytest

import util

ROOT = util.ROOT
CSRC = os.path.join(ROOT, "webgpu-msm-bls12-377_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "sort_elem_host.cpp")
OUT = os.path.join(ROOT, "tests", "native", "_build")
KRANGE, NRANGE, NB = 128, 256, 32768


@pytest.fixture(scope="module")
def exe():
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "sort_elem_host")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", path, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def ask(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return [int(x) for x in r.stdout.split()]


@pytest.mark.parametrize("idx,sub,sign", list(itertools.product([0, (1 << 23) - 1], [0, 127, 128], [0, 1])))
def test_pack_round_trips_at_the_corners(exe, idx, sub, sign):
    v, sub_back, idx_sign = ask(exe, "pack", idx, sign, sub)
    assert v == (sign << 31) | (sub << 23) | idx  # bit 31 the sign, bits 30..23 sub, bits 22..0 the column index
    assert sub_back == sub
    assert idx_sign == idx | (sign << 31)  # a val_idx entry


def test_neighbouring_fields_do_not_bleed(exe):
    """An index one bit away from the sub field, and sub = 255 (all eight bits), each beside zeros and ones."""
    for idx, sub, sign in [(1 << 22, 0, 0), (1 << 22, 255, 1), (0, 255, 0), ((1 << 23) - 1, 0, 1), (0x2AAAAA, 0x55, 1), (0x555555, 0xAA, 0)]:
        v, sub_back, idx_sign = ask(exe, "pack", idx, sign, sub)
        assert (v, sub_back, idx_sign) == ((sign << 31) | (sub << 23) | idx, sub, idx | (sign << 31))


def test_sort_elem_bytes(exe):
    assert ask(exe, "bytes", 1, 0) == [4]
    assert ask(exe, "bytes", 65537, 0) == [4]
    assert ask(exe, "bytes", 1 << 23, 0) == [4]  # indices 0 .. 2^23 - 1
    assert ask(exe, "bytes", (1 << 23) + 1, 0) == [8]
    assert ask(exe, "bytes", 1 << 26, 0) == [8]
    assert ask(exe, "bytes", 1 << 33, 0) == [8]  # a 64-bit column count is not truncated
    assert ask(exe, "bytes", 1000, 1) == [8]  # the wide table: indices run to 13 n
    assert ask(exe, "bytes", 1 << 23, 1) == [8]


def test_first_key_of_a_range(exe):
    """sub = key - first key of the range: at full width ranges of 128 keys, the last one also owning key NB (sub 128);
    narrowed by shift s, ranges of 128 >> s keys."""
    assert ask(exe, "first", 0, 0) == [0]
    assert ask(exe, "first", 1, 0) == [KRANGE]
    assert ask(exe, "first", NRANGE - 1, 0) == [NB - KRANGE]
    assert NB - ask(exe, "first", NRANGE - 1, 0)[0] == KRANGE  # key NB in the last range: sub = KRANGE
    for s in range(1, 6):
        assert ask(exe, "first", 1, s) == [KRANGE >> s]
        assert ask(exe, "first", NRANGE - 1, s) == [(NRANGE - 1) * (KRANGE >> s)]
