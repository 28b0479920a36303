"""What an Edwards-BLS12 row-commitment pass leaves in the stash (include/msm377.h "the stash of a batch call";
csrc/kernels/ed_commit_rows.hpp): msm377_read_walk_stash after msm377_ed_commit_rows_device at k = 273 (18 segments: the
two-level fold), 48 (three segments: one fold launch) and 16 (one segment: no fold), n = 257.  The contract:
  - segment 0 holds the row's sum;
  - when S > 16, a segment g > 0 with g % 16 == 0 holds the sum of segments g .. min(S, g + 16) - 1;
  - every other segment holds its own partial sum;
  - running products exist for segment 0 only.
Every segment is read back, checked against the ED stash contract (tests/walk_model.py: canonical coordinates, Z non-zero,
T Z = X Y) and decoded as (X / Z, Y / Z); the expected sums come from generators with known logarithms
(tests/ed_commit_rows_vectors.py), never from the device call."""
import pytest

import ed_commit_rows_vectors as ECR
import pyref as R
import walk_model as WM
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host import engine as E

pytestmark = pytest.mark.gpu

ORD = R.ED_SUBGROUP
N = 257


def dev(buf: bytes):
    import torch

    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


def case_rows(k, logs):
    """N rows of k scalars: sliding rows of the mixed buffer, then crafted ones -- all zero; the first generator alone; the
    last generator alone; a sum of O from two terms that are not O (the first and the last generator: in different fold
    groups at k = 273, in different segments at k = 48); its neighbour."""
    crafted = [[0] * k for _ in range(5)]
    crafted[1][0] = ECR.MASK256
    crafted[2][k - 1] = 2**255 + 5
    crafted[3][0], crafted[3][k - 1] = logs[k - 1], ORD - logs[0]  # g_0 g_(k-1) + g_(k-1) (l - g_0) = 0 mod l
    crafted[4][0], crafted[4][k - 1] = logs[k - 1], ORD - logs[0] + 1
    m = N - len(crafted)
    return ECR.sliding_rows(ECR.mixed_buffer(m + k - 1, 0x57A5 + k), m, k) + [tuple(row) for row in crafted]


@pytest.mark.parametrize("k", [273, 48, 16])
def test_stash_after_a_pass(engine, k):
    import torch

    logs, gens = ECR.known_logs(k)
    rows = case_rows(k, logs)
    S, per, _ = msm.commit_rows_plan(k)
    assert S == {273: 18, 48: 3, 16: 1}[k]
    stride = -(-N // 256) * 256
    d_s = dev(ECR.pack(rows)[0])
    d_out = torch.full((64 * N,), 0xEE, dtype=torch.uint8, device="cuda")
    try:
        engine.ed_set_generators(gens)
        with pytest.raises(msm.MsmError) as e:  # the build went through the stash
            engine.read_walk_stash(info_only=True)
        assert e.value.code == E.ESTATE
        engine.ed_commit_rows_device(d_s.data_ptr(), N, k, d_out.data_ptr())
        out = bytes(d_out.cpu().numpy())

        def segment_sum(g0, g1):
            """Records of sum over generators of segments g0 .. g1 - 1, per row."""
            j0, j1 = g0 * per, min(k, g1 * per)
            return ECR.multiples_of_g([sum(s * lg for s, lg in zip(row[j0:j1], logs[j0:j1])) for row in rows])

        for g in range(S):
            info, pts, prod = engine.read_walk_stash(segment=g)
            want = dict(kind=E.WALK_ED_COMMIT_ROWS, form=E.WALK_FORM_ED, point_words=36, product_words=9, product_pad=3, n=N, pass_offset=0, m=N, width=8, k=k, segments=S, stride=stride)
            assert info.kind == 9 and info._asdict() == want, (info, want)
            assert pts.shape == (N, 36)
            where = "ed_commit_rows k = %d, segment %d: " % (k, g)
            decoded = WM.check_ed_stash(pts, where)  # every Z non-zero, every coordinate canonical, T Z = X Y
            if g == 0:
                exp, what = segment_sum(0, S), "the row's sum"
                assert prod is not None and prod.shape == (N, 12)
                WM.check_products("Fq", pts, prod, where)
                assert b"".join(R.ed_encode_result(p) for p in decoded) == out, where + "the outputs are not the points of segment 0"
            elif S > 16 and g % 16 == 0:
                exp, what = segment_sum(g, min(S, g + 16)), "the sum of its fold group"
                assert prod is None
            else:
                exp, what = segment_sum(g, g + 1), "its own partial sum"
                assert prod is None
            bad = [i for i in range(N) if R.ed_encode_result(decoded[i]) != exp[64 * i : 64 * i + 64]]
            assert not bad, "%srows %s do not hold %s" % (where, bad[:6], what)
        # the crafted rows did what they were made for
        assert out[64 * (N - 5) : 64 * (N - 4)] == ECR.IDENTITY_WIRE and out[64 * (N - 2) : 64 * (N - 1)] == ECR.IDENTITY_WIRE
        assert out[64 * (N - 1) :] == R.ed_encode_result(R.ed_mul(R.ED_G, logs[k - 1]))
        if S > 1:  # ... from partial sums that are not O
            _, last, _ = engine.read_walk_stash(segment=S - 1, first=N - 2, count=1)
            assert WM.check_ed_stash(last)[0] != R.ED_ID
        with pytest.raises(msm.MsmError) as e:
            engine.read_walk_stash(segment=S)
        assert e.value.code == E.EINVAL
        if S > 1:  # running products: segment 0 only
            assert engine._lib.msm377_read_walk_stash(engine._ctx, None, 1, 0, 1, None, pts.ctypes.data) == E.EINVAL
    finally:
        engine.ed_set_generators(None)
    assert engine.ed_generators() == (0, 0)
