"""Wire codecs of the test harness, mirrored name for name.

Reference: src/reference/webgpu/utils.ts:41-99 (bigIntsToU32Array, bigIntToU32Array,
bigIntBufferLE, bigIntsToBufferLE, readBigIntsFromBufferLE, u32ArrayToBigInts); vectors in
src/reference/webgpu/utils.test.ts:4-14.  These define the buffers compute_msm receives
(src/ui/AllBenchmarks.tsx:57-68): points as x||y 384-bit little-endian, scalars 256-bit
little-endian.
"""
from typing import Iterable, List


def bigIntToU32Array(beBigInt: int, bigIntSize: int = 256) -> List[int]:
    """Most-significant-first u32 words (utils.ts:49-61)."""
    num = bigIntSize // 32
    return [(beBigInt >> (32 * (num - 1 - i))) & 0xFFFFFFFF for i in range(num)]


def bigIntsToU32Array(beBigInts: Iterable[int], bigIntSize: int = 256) -> List[int]:
    """Concatenation of bigIntToU32Array (utils.ts:41-46)."""
    out: List[int] = []
    for v in beBigInts:
        out.extend(bigIntToU32Array(v, bigIntSize))
    return out


def u32ArrayToBigInts(u32Array: Iterable[int], bigIntSize: int = 256) -> List[int]:
    """Inverse of bigIntsToU32Array (utils.ts:87-103)."""
    words = list(u32Array)
    chunk = bigIntSize // 32
    out = []
    for i in range(0, len(words), chunk):
        v = 0
        for w in words[i : i + chunk]:
            v = (v << 32) | (int(w) & 0xFFFFFFFF)
        if len(words[i : i + chunk]) < chunk:  # the reference tolerates a short tail
            v <<= 32 * (chunk - len(words[i : i + chunk]))
        out.append(v)
    return out


def bigIntBufferLE(bigInt: int, bigIntSize: int = 256) -> bytes:
    """Little-endian bytes of one integer (utils.ts:63-67)."""
    return int(bigInt).to_bytes(bigIntSize // 8, "little")


def bigIntsToBufferLE(bigInts: Iterable[int], bigIntSize: int = 256) -> bytes:
    """Concatenated little-endian integers (utils.ts:69-72)."""
    return b"".join(bigIntBufferLE(v, bigIntSize) for v in bigInts)


def readBigIntsFromBufferLE(buffer: bytes, bigIntSize: int = 256) -> List[int]:
    """Inverse of bigIntsToBufferLE (utils.ts:74-85).  Unlike the reference (whose
    Buffer.reverse() on a slice view reverses the caller's buffer in place, utils.ts:78-79)
    the input is left untouched."""
    step = bigIntSize // 8
    buf = bytes(buffer)
    return [int.from_bytes(buf[i : i + step], "little") for i in range(0, len(buf) - step + 1, step)]


def encode_scalars(scalars: Iterable[int], scalar_bytes: int = 32) -> bytes:
    """Scalars as the engine reads them: little-endian integers of ``scalar_bytes`` bytes each -- 32 for the harness's
    wire format (the default), 4, 8 or 16 for the short-scalar entry points (include/msm377.h).  A value that is negative
    or does not fit the stride raises ValueError."""
    if scalar_bytes not in (4, 8, 16, 32):
        raise ValueError("scalar_bytes must be 4, 8, 16 or 32")
    out = bytearray()
    for k in scalars:
        k = int(k)
        if k < 0 or k >> (8 * scalar_bytes):
            raise ValueError("scalar %d does not fit %d bytes" % (k, scalar_bytes))
        out += k.to_bytes(scalar_bytes, "little")
    return bytes(out)


# ---- native input forms (include/msm377.h "native input forms") ----
# What a prover built on arkworks or snarkVM keeps in memory: G1 coordinates as x * 2^384 mod p, scalars as
# s * 2^256 mod r, an affine point as x, y and an infinity flag byte padded to 104 bytes.  Plain Python integers: a
# third implementation beside the engine's import pass and its host helpers, for tests and for users.
G1_P = 0x01AE3A4617C510EAC63B05C06CA1493B1A22D9F300F5138F1EF3622FBA094800170B5D44300000008508C00000000001
G1_R = 8444461749428370424248824938781546531375899335154063827935233455917409239041
POINT_FORMS = {"wire": 0, "mont": 1, "mont_flag": 2}
SCALAR_FORMS = {"wire": 0, "mont": 1}
POINT_STRIDE = {"wire": 96, "mont": 96, "mont_flag": 104}
_INV384 = pow(1 << 384, -1, G1_P)
_INV256 = pow(1 << 256, -1, G1_R)


def encode_points_native(points, form: str = "mont_flag") -> bytes:
    """Affine points (x, y) -- None for the identity, ``mont_flag`` only -- in the named form."""
    if form not in POINT_FORMS:
        raise ValueError("point form must be one of %s" % sorted(POINT_FORMS))
    out = bytearray()
    for pt in points:
        if pt is None:
            if form != "mont_flag":
                raise ValueError("only the mont_flag form can express the identity")
            out += bytes(96) + b"\x01" + bytes(7)
            continue
        x, y = int(pt[0]), int(pt[1])
        if form != "wire":
            x, y = (x << 384) % G1_P, (y << 384) % G1_P
        out += x.to_bytes(48, "little") + y.to_bytes(48, "little")
        if form == "mont_flag":
            out += bytes(8)
    return bytes(out)


def decode_points_native(buf: bytes, form: str = "mont_flag") -> list:
    """Inverse of encode_points_native: (x, y) tuples, None for a flagged point (whatever its coordinate bytes hold).
    A Montgomery value v decodes to v * 2^-384 mod p."""
    stride = POINT_STRIDE[form]
    buf = bytes(buf)
    if len(buf) % stride:
        raise ValueError("points buffer length must be a multiple of %d" % stride)
    out = []
    for i in range(0, len(buf), stride):
        if form == "mont_flag" and buf[i + 96]:
            out.append(None)
            continue
        x, y = int.from_bytes(buf[i : i + 48], "little"), int.from_bytes(buf[i + 48 : i + 96], "little")
        if form != "wire":
            x, y = x * _INV384 % G1_P, y * _INV384 % G1_P
        out.append((x, y))
    return out


def encode_scalars_native(scalars: Iterable[int], form: str = "mont") -> bytes:
    """Scalars as 32 little-endian bytes each: canonical (``wire``) or s * 2^256 mod r (``mont``)."""
    if form not in SCALAR_FORMS:
        raise ValueError("scalar form must be one of %s" % sorted(SCALAR_FORMS))
    return b"".join(((int(k) << 256) % G1_R if form == "mont" else int(k)).to_bytes(32, "little") for k in scalars)


def decode_scalars_native(buf: bytes, form: str = "mont") -> List[int]:
    """Inverse of encode_scalars_native.  Every 32-byte Montgomery value v is accepted and decodes to
    v * 2^-256 mod r, fully reduced."""
    vals = readBigIntsFromBufferLE(buf, 256)
    return [v * _INV256 % G1_R for v in vals] if form == "mont" else vals
