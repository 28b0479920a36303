"""Short-scalar G1 MSM, the parts that need no GPU: the new symbols, the window-count rule, a Python model of the recode
that pins the geometry the kernel implements (kernels/decompose.hpp k_decompose_short), the host width call and the
compact scalar codec."""
import ctypes
import os
import random
import re

import pytest

import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host import codecs
from webgpu_msm_bls12_377_amd.host import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = (
    "msm377_g1_msm_short_device",
    "msm377_g1_msm_short",
    "msm377_g1_msm_fixed_base_short_device",
    "msm377_scalars_width_device",
    "msm377_scalars_width_host",
    "msm377_short_windows",
    "msm377_ctx_get_last_geometry",
)
LOGS = (11, 15)  # bucket_log of the narrow and of the main path


def test_header_declares_and_library_exports_the_new_symbols():
    with open(os.path.join(ROOT, "include", "msm377.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(msm377_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(msm.library_path())
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name


# ---- the window count ----
def test_short_windows_rule():
    for L in LOGS:
        last = 0
        for bits in range(1, 254):
            w = msm.short_windows(bits, L)
            assert w == bits // (L + 1) + 1, (bits, L, w)
            assert w >= last, "the window count never decreases as bits grows"
            last = w
    assert msm.short_windows(253, 15) == 16
    assert msm.short_windows(253, 11) == 22
    assert msm.short_windows(64, 15) == 5 and msm.short_windows(128, 15) == 9


def test_short_windows_rejects_what_no_call_accepts():
    for bits, L in ((0, 15), (254, 15), (64, 0), (64, 16)):
        assert msm.short_windows(bits, L) == 0


# ---- Python model of the recode (written here, imported from nowhere) ----
def recode(k: int, bits: int, L: int):
    """W = floor(bits / (L + 1)) + 1 digits of k < 2^bits: W - 1 signed digits of L + 1 bits (v = field + carry; v >= 2^L
    becomes v - 2^(L+1) and carries), then the unsigned rest plus the carry.  Returns (digits, carry out of the top)."""
    c = L + 1
    W = bits // c + 1
    digits, carry = [], 0
    for w in range(W - 1):
        v = ((k >> (c * w)) & ((1 << c) - 1)) + carry
        carry = 1 if v >= (1 << L) else 0
        digits.append(v - (carry << c))
    top = (k >> (c * (W - 1))) + carry
    out = top >> (L + 1)  # what a top digit beyond the bucket range would have to hand on
    digits.append(top)
    return digits, out


def edge_scalars(bits: int, L: int, rng: random.Random):
    c = L + 1
    mask = (1 << bits) - 1
    fields = (bits + c - 1) // c
    all_half = sum((1 << L) << (c * f) for f in range(fields)) & mask  # every (L + 1)-bit field 2^L
    all_below = sum(((1 << L) - 1) << (c * f) for f in range(fields)) & mask  # every field 2^L - 1
    ks = [0, 1, mask, 1 << (bits - 1), all_half, all_below]
    ks += [rng.getrandbits(bits) for _ in range(200)]
    return ks


@pytest.mark.parametrize("L", LOGS)
def test_recode_model_covers_every_width(L):
    rng = random.Random(0x5C0DE + L)
    c = L + 1
    for bits in range(1, 254):
        W = bits // c + 1
        assert W == msm.short_windows(bits, L)
        for k in edge_scalars(bits, L, rng):
            assert 0 <= k < (1 << bits)
            digits, out = recode(k, bits, L)
            assert len(digits) == W
            assert sum(d << (c * w) for w, d in enumerate(digits)) == k, (bits, L, hex(k))
            for d in digits[:-1]:
                assert -(1 << L) <= d <= (1 << L), (bits, L, hex(k), d)
            assert 0 <= digits[-1] <= (1 << L), (bits, L, hex(k), digits[-1])
            assert out == 0, "no carry out of the top window"


def test_recode_model_top_digit_reaches_its_bound():
    """bits = 31 at L = 15: the top window holds 15 bits and a carry, 2^31 - 1 drives it to exactly 2^15 -- the digit the
    main path stores unsigned (common.hpp KEY_UNSIGNED)."""
    digits, out = recode((1 << 31) - 1, 31, 15)
    assert digits == [-1, 1 << 15] and out == 0


# ---- msm377_scalars_width_host ----
@pytest.mark.parametrize("stride", (4, 8, 16, 32))
def test_scalars_width_host_matches_bit_length(stride):
    rng = random.Random(0xB17 + stride)
    top = min(8 * stride, 256)
    for trial in range(40):
        width = rng.randrange(0, top + 1)
        n = rng.randrange(1, 70)
        ks = [rng.getrandbits(width) if width else 0 for _ in range(n)]
        buf = b"".join(k.to_bytes(stride, "little") for k in ks)
        assert msm.scalars_width_host(buf, stride) == max(k.bit_length() for k in ks), (stride, trial)
    for bit in range(8 * stride):  # every single bit position, somewhere in the middle of the array
        ks = [0, 0, 1 << bit, 0]
        buf = b"".join(k.to_bytes(stride, "little") for k in ks)
        assert msm.scalars_width_host(buf, stride) == bit + 1


def test_scalars_width_host_zero_and_empty():
    for stride in (4, 8, 16, 32):
        assert msm.scalars_width_host(bytes(stride * 17), stride) == 0
        assert msm.scalars_width_host(b"", stride) == 0


def test_scalars_width_host_bad_arguments():
    lib = msm.load_library()
    bits = ctypes.c_uint32(77)
    buf = bytes(64)
    assert lib.msm377_scalars_width_host(None, 2, 32, ctypes.byref(bits)) == E.EINVAL
    assert lib.msm377_scalars_width_host(buf, 2, 32, None) == E.EINVAL
    for stride in (0, 1, 5, 12, 64):
        assert lib.msm377_scalars_width_host(buf, 2, stride, ctypes.byref(bits)) == E.EINVAL, stride
    assert lib.msm377_scalars_width_host(None, 0, 8, ctypes.byref(bits)) == E.OK and bits.value == 0  # n = 0 needs no buffer


# ---- codecs.encode_scalars ----
def test_encode_scalars_round_trips_at_every_stride():
    rng = random.Random(0xC0DEC)
    for stride in (4, 8, 16, 32):
        ks = [0, 1, (1 << (8 * stride)) - 1] + [rng.getrandbits(8 * stride) for _ in range(50)]
        buf = codecs.encode_scalars(ks, scalar_bytes=stride)
        assert len(buf) == stride * len(ks)
        assert codecs.readBigIntsFromBufferLE(buf, 8 * stride) == ks
    ks = [rng.getrandbits(253) for _ in range(20)]
    assert codecs.encode_scalars(ks) == codecs.bigIntsToBufferLE(ks, 256), "the default stays the 32-byte wire format"
    assert msm.encode_scalars is codecs.encode_scalars


def test_encode_scalars_rejects_what_does_not_fit():
    with pytest.raises(ValueError):
        codecs.encode_scalars([1 << 64], scalar_bytes=8)
    with pytest.raises(ValueError):
        codecs.encode_scalars([-1], scalar_bytes=8)
    with pytest.raises(ValueError):
        codecs.encode_scalars([1], scalar_bytes=5)
