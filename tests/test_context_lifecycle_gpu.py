"""The life cycle of a context (csrc/context.hip): every buffer, event and stream a context takes on demand goes through
its one owner and goes back with msm377_ctx_destroy; a twin runs with its owner's knobs, not with the environment of the
moment it is made; a refused create leaves nothing behind.  Contexts of 2^12 points, made and closed by the tests
themselves.  Answers are checked against the CPU oracle or the host twins, as in the tests of the calls themselves."""
import os

import pytest

import batch_mul_vectors as V
import pyref as R
import util
import webgpu_msm_bls12_377_amd as msm
from webgpu_msm_bls12_377_amd.host.engine import EINVAL

pytestmark = pytest.mark.gpu

CAP = 1 << 12
A0, D = 0xC0FFEE0123456789ABCDEF, 0x1D5EED


def dev(buf: bytes):
    import torch

    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


@pytest.fixture(scope="module")
def inputs(oracle):
    """Points, scalar sets and the oracle's answers, computed once and read by every test below."""
    pts = util.oracle_gen_points(oracle, CAP, A0, D)
    sets = [R.encode_scalars(R.rand_scalars(0xC7C1E + b, CAP)) for b in range(5)]

    def msm_of(n, b=0, skip=()):
        keep = [i for i in range(n) if i not in set(skip)]
        p = b"".join(pts[96 * i : 96 * i + 96] for i in keep)
        s = b"".join(sets[b][32 * i : 32 * i + 32] for i in keep)
        return util.oracle_msm(oracle, p, s)

    flagged = (0, 31, 32, 63)
    want = {
        "flagged64": msm_of(64, 0, flagged),
        "n300": [msm_of(300, b) for b in range(5)],
        "n64": [msm_of(64, b) for b in range(4)],
        "n4096": [msm_of(4096, b) for b in range(5)],
    }
    bm_scalars = R.encode_scalars([0, 1, R.R_ORDER - 1, 0x1234567, 2**255 + 12345])
    want["batch_mul"] = msm.batch_mul_host(pts[:96], bm_scalars)
    want["batch_mul_var"] = msm.batch_mul_var_host(pts[: 96 * 5], bm_scalars)
    return {"points": pts, "sets": sets, "flagged": flagged, "bm_scalars": bm_scalars, "want": want}


def one_cycle(inputs):
    """Every resource a context allocates on demand, then close().  Returns what the calls answered."""
    pts, sets, want = inputs["points"], inputs["sets"], inputs["want"]
    got = {}
    eng = msm.MsmEngine(CAP)
    try:
        # the import buffers and the native staging: a host call with infinity flags
        native = bytearray(msm.encode_points_native(R.decode_points(pts[: 96 * 64]), "mont_flag"))
        for i in inputs["flagged"]:
            native[104 * i : 104 * i + 96] = b"\xff" * 96
            native[104 * i + 96] = 1
        eng.set_input_format("mont_flag", "mont")
        got["flagged64"] = eng.msm(bytes(native), msm.encode_scalars_native(R.decode_scalars(sets[0][: 32 * 64]), "mont"))
        eng.set_input_format("wire", "wire")
        eng.reserve_host_staging()
        eng.reserve_host_staging()
        # the bucket snapshot
        eng.set_stage_capture(2)
        d_p, d_s = dev(pts[: 96 * 300]), dev(sets[0][: 32 * 300])
        got["n300"] = eng.msm_device(d_p.data_ptr(), d_s.data_ptr(), 300)
        info, _ = eng.read_stage_ex(0, want=("row_ptr",))
        got["columns"] = info.columns
        eng.set_stage_capture(0)
        # the batch multiplication scratch, its window table and the per-point tables
        eng.set_mul_window(8)
        got["batch_mul"] = eng.batch_mul(pts[:96], inputs["bm_scalars"])
        got["mul_window"] = eng.last_mul_window()
        eng.set_mul_window(0)
        got["batch_mul_var"] = eng.batch_mul_var(pts[: 96 * 5], inputs["bm_scalars"])
        # the precomputed table and the wide buffers; then the twin and the twin's wide buffers
        eng.set_precompute_window(20)
        eng.set_bases_precomputed(pts[: 96 * 64])
        d_b = dev(b"".join(s[: 32 * 64] for s in sets[:4]))
        got["n64"] = eng.msm_fixed_base_batch_device(d_b.data_ptr(), 64, 4)
        # a plain table on top: the precomputed one and the wide buffers go back early
        eng.set_bases(pts[: 96 * 64])
        got["n64 plain"] = eng.msm_fixed_base_batch_device(d_b.data_ptr(), 64, 4)
        got["fallbacks"] = eng.fallback_info()[0]
    finally:
        eng.close()
    return got


def test_every_on_demand_resource_then_destroy_three_times(inputs):
    want = inputs["want"]
    runs = [one_cycle(inputs) for _ in range(3)]
    first = runs[0]
    assert first["flagged64"] == want["flagged64"]
    assert first["n300"] == want["n300"][0] and first["columns"] == 300
    assert first["batch_mul"] == want["batch_mul"] and first["mul_window"] == 8
    assert first["batch_mul_var"] == want["batch_mul_var"]
    assert first["n64"] == want["n64"] and first["n64 plain"] == want["n64"]
    assert first["fallbacks"] == 0
    assert runs[1] == first and runs[2] == first


def test_knobs_outlive_the_environment(inputs, monkeypatch):
    """A context made under MSM377_COOP_THREADS / MSM377_TAIL_FROM keeps them, and so does the twin its first large batch
    makes after the variables are gone.  (Which launch shapes the twin chose is not visible here: tools/route_calls.py
    under a kernel trace shows them, profiles/context_owner/.)"""
    pts, sets, want = inputs["points"], inputs["sets"], inputs["want"]
    monkeypatch.setenv("MSM377_COOP_THREADS", "1048576")
    monkeypatch.setenv("MSM377_TAIL_FROM", "6")
    eng = msm.MsmEngine(CAP)
    try:
        monkeypatch.delenv("MSM377_COOP_THREADS")
        monkeypatch.delenv("MSM377_TAIL_FROM")
        assert "MSM377_COOP_THREADS" not in os.environ and "MSM377_TAIL_FROM" not in os.environ
        eng.set_narrow_max(0)
        eng.set_bases(pts)
        for n in (300, 4096):
            d_b = dev(b"".join(s[: 32 * n] for s in sets))
            with util.edwards_only(eng):
                assert eng.msm_fixed_base_batch_device(d_b.data_ptr(), n, 5) == want["n%d" % n], n
            assert eng.last_geometry() == (16, 15)
    finally:
        eng.close()


def test_a_failed_create_leaves_nothing_behind(inputs):
    for bad in (0, (1 << 30) + 1):
        with pytest.raises(msm.MsmError) as e:
            msm.MsmEngine(bad)
        assert e.value.code == EINVAL
    with msm.MsmEngine(CAP) as eng:
        assert eng.msm(inputs["points"][: 96 * 300], inputs["sets"][1][: 32 * 300]) == inputs["want"]["n300"][1]
