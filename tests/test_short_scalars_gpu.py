"""Short-scalar G1 MSM on the GPU (include/msm377.h msm377_g1_msm_short*): compact scalars of a declared bit width run
W = floor(bits / (L + 1)) + 1 windows.  Every expected value comes from the CPU oracle on the same scalars zero-extended
to 32 bytes or from the closed form over oracle_gen_points (P_i = [a0 + i d]G); none from the engine's own full-width
call.  After every short call last_geometry() must read (short_windows(bits, L), L): the short geometry ran."""
import ctypes
import random

import pytest

import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import EINVAL, ESCALAR, ESTATE

pytestmark = pytest.mark.gpu

A0, D = 0x1234567890ABCDEF1234567890ABCDEF, 0xFEDCBA0987654321FEDCBA
WIDTHS = (1, 2, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 252, 253)
SIZES = (1, 2, 33, 1000, 4097, 65536, 65537, 1 << 18)
NARROW_MAX = 1 << 16  # msm377_ctx_set_narrow_max default: L = 11 up to here, L = 15 above


def dev(buf: bytes):
    import torch

    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


def stride_for(bits):
    return 4 if bits <= 32 else 8 if bits <= 64 else 16 if bits <= 128 else 32


def path_log(n):
    return 11 if n <= NARROW_MAX else 15


def edge_patterns(bits, L):
    c = L + 1
    mask = (1 << bits) - 1
    fields = (bits + c - 1) // c
    return [
        0,
        1,
        mask,
        1 << (bits - 1),
        sum((1 << L) << (c * f) for f in range(fields)) & mask,
        sum(((1 << L) - 1) << (c * f) for f in range(fields)) & mask,
    ]


def short_scalars(bits, n, seed):
    """Seeded scalars below 2^bits, the edge patterns of both geometries in front, one scalar with bit bits - 1 set."""
    rng = random.Random(seed)
    ks = [rng.getrandbits(bits) for _ in range(n)]
    edges = edge_patterns(bits, 15) + edge_patterns(bits, 11)
    ks[: min(n, len(edges))] = edges[: min(n, len(edges))]
    ks[n - 1] |= 1 << (bits - 1)
    return ks


@pytest.fixture(scope="module")
def pool(oracle):
    """2^20 points P_i = [A0 + i D]G; every case takes a prefix."""
    return util.oracle_gen_points(oracle, 1 << 20, A0, D)


def expected(oracle, pool, ks):
    n = len(ks)
    if n <= 1000:
        return util.oracle_msm(oracle, pool[: 96 * n], R.encode_scalars(ks))
    return util.closed_form(oracle, sum(k * (A0 + i * D) for i, k in enumerate(ks)))


# ---- parity ----
@pytest.mark.parametrize("n", SIZES)
def test_parity_every_width(engine, oracle, pool, n):
    d_p = dev(pool[: 96 * n])
    L = path_log(n)
    for bits in WIDTHS:
        ks = short_scalars(bits, n, 0x5A0000 + 1000 * bits + n % 997)
        exp = expected(oracle, pool, ks)
        strides = [stride_for(bits)] + ([32] if bits in (64, 128) else [])
        for sb in strides:
            d_s = dev(msm.encode_scalars(ks, sb))
            with util.edwards_only(engine):
                got = engine.msm_short_device(d_p.data_ptr(), d_s.data_ptr(), n, sb, bits)
            assert got == exp, (n, bits, sb)
            assert engine.last_geometry() == (msm.short_windows(bits, L), L), (n, bits, sb)


def test_empty_input_is_the_identity(engine):
    assert engine.msm_short_device(0, 0, 0, 8, 64) == bytes(48) + b"\x01" + bytes(47)
    assert engine.msm_short(b"", b"", 8, 64) == bytes(48) + b"\x01" + bytes(47)


# ---- full size ----
@pytest.mark.parametrize("bits, windows", [(64, 5), (128, 9)])
def test_full_size_2_20(engine, oracle, pool, bits, windows):
    n = 1 << 20
    ks = short_scalars(bits, n, 0xF00 + bits)
    sb = stride_for(bits)
    d_p, d_s = dev(pool), dev(msm.encode_scalars(ks, sb))
    with util.edwards_only(engine, products=7):  # the per-call affine records
        got = engine.msm_short_device(d_p.data_ptr(), d_s.data_ptr(), n, sb, bits)
    assert got == expected(oracle, pool, ks)
    assert engine.last_geometry() == (windows, 15)


# ---- skew: one window with few rows ----
def test_one_bit_scalars_half_set(engine, oracle, pool):
    n = 1 << 18
    rng = random.Random(0xB17)
    ks = [rng.getrandbits(1) for _ in range(n)]
    ks[0], ks[1], ks[n - 1] = 0, 1, 1
    d_p, d_s = dev(pool[: 96 * n]), dev(msm.encode_scalars(ks, 4))
    with util.edwards_only(engine):
        got = engine.msm_short_device(d_p.data_ptr(), d_s.data_ptr(), n, 4, 1)
    assert got == expected(oracle, pool, ks)
    assert engine.last_geometry() == (1, 15)


def test_byte_scalars_one_window(engine, oracle, pool):
    n = (1 << 16) + 1
    ks = short_scalars(8, n, 0xB8)
    d_p, d_s = dev(pool[: 96 * n]), dev(msm.encode_scalars(ks, 4))
    with util.edwards_only(engine):
        got = engine.msm_short_device(d_p.data_ptr(), d_s.data_ptr(), n, 4, 8)
    assert got == expected(oracle, pool, ks)
    assert engine.last_geometry() == (1, 15)


# ---- form 0 ----
def test_weierstrass_form(engine, oracle, pool):
    n, bits = 4097, 64
    ks = short_scalars(bits, n, 0xF0)
    d_p, d_s = dev(pool[: 96 * n]), dev(msm.encode_scalars(ks, 8))
    engine.set_g1_form("weierstrass")
    try:
        got = engine.msm_short_device(d_p.data_ptr(), d_s.data_ptr(), n, 8, bits)
        assert engine.accumulate_products() == 10
        assert engine.last_geometry() == (msm.short_windows(bits, 15), 15)  # form 0 runs 2^15 buckets at every size
    finally:
        engine.set_g1_form("edwards")
    assert got == expected(oracle, pool, ks)


# ---- points outside the prime-order subgroup ----
def test_points_outside_the_prime_order_subgroup(engine, oracle, pool):
    """The construction of test_g1_parity_gpu.test_points_outside_the_prime_order_subgroup, with 64-bit scalars: the
    Edwards form meets an exceptional case, the short call reruns on the Weierstrass path and says so."""
    t2 = (R.P - 1, 0)
    rnd_pts = R.decode_points(pool[: 96 * 40])
    shifted = [R.add(p, t2) for p in rnd_pts[:10]]
    for a in shifted:
        assert (a[1] * a[1] - a[0] ** 3 - 1) % R.P == 0
    te = util.te_params()
    x4 = (-1 - pow(te["s"], -1, R.P)) % R.P
    import gen_consts  # tools/ (put on sys.path by util.te_params)

    t4 = (x4, gen_consts._sqrt_p((x4 ** 3 + 1) % R.P))
    assert R.add(t4, t4) == t2
    cases = {
        "order-4 input": rnd_pts[:3] + [t4] + rnd_pts[3:6] + [R.neg(t4)],
        "two-torsion input": rnd_pts[:5] + [t2] + rnd_pts[5:9],
        "P and P + T2 in one bucket": [rnd_pts[0], shifted[0]] + rnd_pts[1:4],
        "cofactor points only": shifted,
    }
    bits = 64
    for name, pts in cases.items():
        n = len(pts)
        rng = random.Random(len(name))
        ks = [rng.getrandbits(bits) for _ in range(n)]
        if name.startswith("P and"):
            ks[0], ks[1] = 5, 5  # same digits, same buckets: P + (P + T2)
        pb, sb = R.encode_points(pts), msm.encode_scalars(ks, 8)
        exp = R.encode_result(R.msm_naive(pts, ks))  # pyref: complete affine arithmetic, torsion points included
        # points of order 2 and 4 have no Edwards record: the conversion flags them, a rerun is certain; the other two sets
        # are valid Edwards points, for which an exceptional case is possible and not certain
        must = name in ("order-4 input", "two-torsion input")
        d_p, d_s = dev(pb), dev(sb)

        def reruns(call):
            before = engine.fallback_info()[0]
            assert call() == exp, name
            return engine.fallback_info()[0] - before

        r = reruns(lambda: engine.msm_short_device(d_p.data_ptr(), d_s.data_ptr(), n, 8, bits))
        assert r == 1 if must else r <= 1, (name, r)
        if r:
            assert engine.fallback_info()[1] != 0
            assert engine.last_geometry() == (msm.short_windows(bits, 15), 15), name  # the rerun: W windows of XYZZ
        r = reruns(lambda: engine.msm_short(pb, sb, 8, bits))
        assert r == 1 if must else r <= 1, (name, r)
        engine.set_bases(pb)
        r = reruns(lambda: engine.msm_fixed_base_short_device(d_s.data_ptr(), n, 8, bits))
        assert r == 1 if must else r <= 1, (name, r)
        if r:  # the table stays in the form it fell back to
            assert reruns(lambda: engine.msm_fixed_base_short_device(d_s.data_ptr(), n, 8, bits)) == 0, name


# ---- fixed base ----
@pytest.mark.parametrize("table", ["plain", "precomputed16", "precomputed20"])
def test_fixed_base(engine, oracle, pool, table):
    for n in (4097, 1 << 17):
        pts = pool[: 96 * n]
        if table == "plain":
            engine.set_bases(pts)
        else:
            engine.set_precompute_window(16 if table == "precomputed16" else 20)
            try:
                engine.set_bases_precomputed(pts)
            finally:
                engine.set_precompute_window(16)
        L = 11 if table == "plain" and n <= NARROW_MAX else 15
        for bits in (8, 64, 128):
            sb = stride_for(bits)
            ks = short_scalars(bits, n, 0xF1B + bits + n)
            d_s = dev(msm.encode_scalars(ks, sb))
            with util.edwards_only(engine, products=7):
                got = engine.msm_fixed_base_short_device(d_s.data_ptr(), n, sb, bits)
            assert got == expected(oracle, pool, ks), (table, n, bits)
            assert engine.last_geometry() == (msm.short_windows(bits, L), L), (table, n, bits)
            # the resident set is intact: a full-width call on it still gives its own answer
            full = R.rand_scalars(0xFB + bits, n)
            with util.edwards_only(engine, products=7):
                got = engine.msm_fixed_base(R.encode_scalars(full))
            assert got == expected(oracle, pool, full), (table, n, bits, "full width after short")


def test_fixed_base_needs_bases(oracle, pool):
    with msm.MsmEngine(1 << 12) as eng:
        d_s = dev(msm.encode_scalars([1, 2, 3, 4], 8))
        with pytest.raises(msm.MsmError) as e:
            eng.msm_fixed_base_short_device(d_s.data_ptr(), 4, 8, 64)
        assert e.value.code == ESTATE
        eng.set_bases(pool[: 96 * 2])
        with pytest.raises(msm.MsmError) as e:  # more scalars than resident bases
            eng.msm_fixed_base_short_device(d_s.data_ptr(), 4, 8, 64)
        assert e.value.code == ESTATE


# ---- host buffers ----
@pytest.mark.parametrize("n", [1000, 1 << 18])
def test_host_buffers(engine, oracle, pool, n):
    ks = short_scalars(64, n, 0x405 + n)
    with util.edwards_only(engine):
        got = engine.msm_short(pool[: 96 * n], msm.encode_scalars(ks, 8), 8, 64)
    assert got == expected(oracle, pool, ks)
    L = path_log(n)
    assert engine.last_geometry() == (msm.short_windows(64, L), L)


def test_compute_msm_with_a_declared_width(oracle, pool):
    n = 1024
    ks = short_scalars(64, n, 0xC0)
    exp = R.decode_result(util.oracle_msm(oracle, pool[: 96 * n], R.encode_scalars(ks)))
    got = msm.compute_msm(pool[: 96 * n], ks, log_result=False, scalar_bits=64, scalar_bytes=8)
    assert (got["x"], got["y"]) == exp
    got = msm.compute_msm(pool[: 96 * n], msm.encode_scalars(ks, 8), log_result=False, scalar_bits=64, scalar_bytes=8)
    assert (got["x"], got["y"]) == exp


# ---- errors ----
@pytest.mark.parametrize("bits", [1, 16, 64, 128])
def test_broken_promise(engine, oracle, pool, bits):
    """A scalar equal to 2^bits: MSM377_ESCALAR, the width in the message, out_xy untouched, no rerun, context usable."""
    sb = {1: 4, 16: 4, 64: 16, 128: 32}[bits]  # the smallest stride that can hold 2^bits
    for n, where in ((1000, 0), (1000, 999), (70000, 34567)):
        ks = short_scalars(bits, n, 0xBAD + bits + n)
        bad = list(ks)
        bad[where] = 1 << bits
        d_p, d_good, d_bad = dev(pool[: 96 * n]), dev(msm.encode_scalars(ks, sb)), dev(msm.encode_scalars(bad, sb))
        out = ctypes.create_string_buffer(bytes(range(96)), 96)
        before = engine.fallback_info()
        with pytest.raises(msm.MsmError) as e:
            engine.msm_short_device(d_p.data_ptr(), d_bad.data_ptr(), n, sb, bits, out=out)
        assert e.value.code == ESCALAR
        assert ("%d bits" % bits) in str(e.value), str(e.value)
        assert out.raw == bytes(range(96)), "out_xy is left untouched"
        assert engine.fallback_info() == before, "no rerun"
        L = path_log(n)
        assert engine.last_geometry() == (msm.short_windows(bits, L), L), "one pass, at the declared width"
        with util.edwards_only(engine):
            assert engine.msm_short_device(d_p.data_ptr(), d_good.data_ptr(), n, sb, bits) == expected(oracle, pool, ks)
    with pytest.raises(msm.MsmError) as e:  # host buffers and resident bases answer the same
        engine.msm_short(pool[: 96 * 4], msm.encode_scalars([1, 2, 1 << bits, 3], sb), sb, bits)
    assert e.value.code == ESCALAR
    engine.set_bases(pool[: 96 * 4])
    d_bad = dev(msm.encode_scalars([1, 2, 1 << bits, 3], sb))
    with pytest.raises(msm.MsmError) as e:
        engine.msm_fixed_base_short_device(d_bad.data_ptr(), 4, sb, bits)
    assert e.value.code == ESCALAR


def test_argument_errors(engine, pool):
    n = 64
    d_p, d_s = dev(pool[: 96 * n]), dev(bytes(32 * n + 16))
    p, s = d_p.data_ptr(), d_s.data_ptr()
    bad = [
        (p, s, n, 8, 0),  # bits = 0
        (p, s, n, 32, 254),  # beyond 253
        (p, s, n, 4, 33),  # above 8 x stride
        (p, s, n, 8, 65),
        (p, s, n, 16, 129),
        (p, s, n, 5, 32),  # no such stride
        (p, s, n, 0, 1),
        (p, s + 4, n, 8, 64),  # misaligned device pointers
        (p + 8, s, n, 8, 64),
        (p, s, engine.max_points + 1, 8, 64),  # over capacity
    ]
    for args in bad:
        with pytest.raises(msm.MsmError) as e:
            engine.msm_short_device(*args)
        assert e.value.code == EINVAL, args
    engine.set_bases(pool[: 96 * n])
    for sb, bits in ((8, 0), (8, 65), (5, 32), (32, 254)):
        with pytest.raises(msm.MsmError) as e:
            engine.msm_fixed_base_short_device(s, n, sb, bits)
        assert e.value.code == EINVAL, (sb, bits)
    with pytest.raises(msm.MsmError) as e:
        engine.msm_fixed_base_short_device(s + 4, n, 8, 64)
    assert e.value.code == EINVAL
    with pytest.raises(msm.MsmError) as e:
        engine.msm_short(pool[: 96 * n], bytes(8 * n), 8, 0)
    assert e.value.code == EINVAL
    with pytest.raises(msm.MsmError) as e:
        engine.scalars_width_device(s, n, 5)
    assert e.value.code == EINVAL
    with pytest.raises(msm.MsmError) as e:
        engine.scalars_width_device(s + 4, n, 8)
    assert e.value.code == EINVAL


# ---- width on the device ----
@pytest.mark.parametrize("stride", [4, 8, 16, 32])
def test_scalars_width_device(engine, stride):
    rng = random.Random(0x71D + stride)
    for n in (1, 3, 255, 257, 1000, 100003, 1 << 20):
        for width in (0, 1, 8 * stride, rng.randrange(2, 8 * stride)):
            if n == 1 << 20:
                ks_bytes = bytearray(stride * n)  # zeros but for a few scalars, one of them the widest
                for i in (0, n // 3, n - 1):
                    ks_bytes[stride * i : stride * (i + 1)] = rng.getrandbits(max(width - 1, 0)).to_bytes(stride, "little")
                if width:
                    i = rng.randrange(n)
                    ks_bytes[stride * i : stride * (i + 1)] = (1 << (width - 1)).to_bytes(stride, "little")
                buf = bytes(ks_bytes)
            else:
                buf = msm.encode_scalars([rng.getrandbits(width) if width else 0 for _ in range(n)], stride)
            d_s = dev(buf)
            host = msm.scalars_width_host(buf, stride)
            assert engine.scalars_width_device(d_s.data_ptr(), n, stride) == host, (stride, n, width)
            if n == 1 << 20:
                assert host == width
    assert engine.scalars_width_device(0, 0, stride) == 0
