"""ctypes binding of the C ABI in include/msm377.h (csrc/libmsm377.so).

Replaces the reference's device runtime wrappers (src/submission/implementation/cuzk/gpu.ts:2-170:
get_device, create_and_write_sb, create_compute_pipeline, execute_pipeline, read_from_gpu):
a context owns the HIP stream and every HBM buffer, and one call runs the whole pipeline.
No CPU fallback exists: a missing library raises at import-use time, a missing GPU raises
MsmError(MSM377_EHIP) at context creation.
"""
import ctypes
import os
import re
import sys
from typing import List, NamedTuple, Optional, Sequence, Tuple

NUM_WINDOWS = 16
WINDOW_BITS = 16
PARTIAL_POINTS = 16
POINT_WORDS = 52  # a bucket point in the device format (stage read-backs)
ED_POINT_WORDS = 36  # ... of an Edwards-BLS12 call: four coordinates of 9 limbs
STAGE_FORM_XYZZ, STAGE_FORM_TE, STAGE_FORM_ED = 0, 1, 2  # MSM377_STAGE_FORM_*: StageInfo.form
RECORD_POINT_WORDS = 48  # a point of a window partial record (host-tail format)
WINDOW_PARTIAL_BYTES = PARTIAL_POINTS * RECORD_POINT_WORDS * 4
NUM_BUCKETS = 32768
STAGE_NAMES = ("convert", "decompose", "sort", "accumulate", "reduce", "tail", "accumulate_kernel")

OK, EINVAL, EHIP, ESCALAR, ENOMEM, ESTATE, EGLVRANGE, EEXCEPTIONAL, EPOINT = 0, -1, -2, -3, -4, -5, -6, -7, -8
# input validation (include/msm377.h): a cascade, so a mask normalises to 1, 3 or 7
CHECK_CANONICAL, CHECK_CURVE, CHECK_SUBGROUP, CHECK_ALL = 1, 2, 4, 7
# msm377_ctx_get_fallback_info: where an exceptional case of the twisted Edwards law surfaced (include/msm377.h)
FB_ACCUMULATE, FB_MERGE, FB_TREE, FB_TAIL, FB_CONVERT = 4, 8, 16, 32, 64
GLV_WINDOWS = 8
# msm377_ctx_set_input_format (include/msm377.h "native input forms")
POINTS_WIRE, POINTS_MONT, POINTS_MONT_FLAG = 0, 1, 2
SCALARS_WIRE, SCALARS_MONT = 0, 1
_POINT_FORMS = {"wire": POINTS_WIRE, "mont": POINTS_MONT, "mont_flag": POINTS_MONT_FLAG}
_SCALAR_FORMS = {"wire": SCALARS_WIRE, "mont": SCALARS_MONT}
_POINT_STRIDE = {POINTS_WIRE: 96, POINTS_MONT: 96, POINTS_MONT_FLAG: 104}

_LIB = None


class _CheckReportStruct(ctypes.Structure):  # msm377_check_report
    _fields_ = [
        ("checked", ctypes.c_uint64),
        ("noncanonical", ctypes.c_uint64),
        ("off_curve", ctypes.c_uint64),
        ("outside_subgroup", ctypes.c_uint64),
        ("first_bad", ctypes.c_uint64),
        ("first_bad_reason", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


STAGE_MAX_SLOTS = 22


class _StageInfoStruct(ctypes.Structure):  # msm377_stage_info
    _fields_ = [
        ("slots", ctypes.c_uint32),
        ("bucket_log", ctypes.c_uint32),
        ("columns", ctypes.c_uint64),
        ("digit_bytes", ctypes.c_uint32),
        ("row_ptr_len", ctypes.c_uint32),
        ("bucket_records", ctypes.c_uint32),
        ("form", ctypes.c_int32),
        ("table_stride", ctypes.c_uint64),
        ("geometry_reruns", ctypes.c_uint64),
        ("bias", ctypes.c_uint32 * STAGE_MAX_SLOTS),
        ("key_unsigned", ctypes.c_uint32 * STAGE_MAX_SLOTS),
        ("key_max", ctypes.c_uint32 * STAGE_MAX_SLOTS),
    ]


class StageInfo(NamedTuple):
    """msm377_stage_info: the layout of the last call's last pass as its kernels were launched (include/msm377.h);
    ``bias``, ``key_unsigned`` and ``key_max`` hold one entry per window slot."""

    slots: int
    bucket_log: int
    columns: int
    digit_bytes: int
    row_ptr_len: int
    bucket_records: int
    form: int
    table_stride: int
    geometry_reruns: int
    bias: Tuple[int, ...]
    key_unsigned: Tuple[int, ...]
    key_max: Tuple[int, ...]


class _PartialsInfoStruct(ctypes.Structure):  # msm377_partials_info
    _fields_ = [(name, ctypes.c_int32 if name == "form" else ctypes.c_uint32) for name in (
        "records", "points", "planes", "coord_words", "form", "folded_slots", "tail_kind", "tail_windows", "tail_cbits", "tail_planes", "tail_short_from",
        "coop_from", "tail_from", "columns", "tail_lds", "reserved")]


class PartialsInfo(NamedTuple):
    """msm377_partials_info: the window records of the last call's last pass, the geometry the host tail combined them
    with and the schedule the bucket reduction ran (include/msm377.h)."""

    records: int
    points: int
    planes: int
    coord_words: int
    form: int
    folded_slots: int
    tail_kind: int
    tail_windows: int
    tail_cbits: int
    tail_planes: int
    tail_short_from: int
    coop_from: int
    tail_from: int
    columns: int
    tail_lds: int


TAIL_TE, TAIL_XYZZ, TAIL_ED = 0, 1, 2  # PartialsInfo.tail_kind

WORK_HIST_BINS = 129           # MSM377_WORK_HIST_BINS
WORK_ROW_FOLDED = 0x80000000   # MSM377_WORK_ROW_FOLDED: the fold mark in a word of row_ovf_base


class _WorkListInfoStruct(ctypes.Structure):  # msm377_work_list_info
    _fields_ = [
        ("seg", ctypes.c_uint32),
        ("rows", ctypes.c_uint32),
        ("max_items", ctypes.c_uint64),
        ("quad", ctypes.c_uint32),
        ("fold_slot", ctypes.c_int32),
        ("record_words", ctypes.c_uint32),
        ("form", ctypes.c_int32),
        ("bucket_log", ctypes.c_uint32),
        ("items", ctypes.c_uint32),
        ("split_rows", ctypes.c_uint32),
        ("overflow_slots", ctypes.c_uint32),
        ("hist", ctypes.c_uint32 * WORK_HIST_BINS),
        ("reserved", ctypes.c_uint32),
    ]


class WorkListInfo(NamedTuple):
    """msm377_work_list_info: the accumulation work list of the last call's last pass (include/msm377.h); ``hist[b]`` is
    the number of work items of b entries."""

    seg: int
    rows: int
    max_items: int
    quad: int
    fold_slot: int
    record_words: int
    form: int
    bucket_log: int
    items: int
    split_rows: int
    overflow_slots: int
    hist: Tuple[int, ...]
BASES_TE_PROJECTIVE, BASES_TE_AFFINE, BASES_WEIERSTRASS, BASES_ED = 0, 1, 2, 3  # MSM377_BASES_*: BasesInfo.form
MUL_TABLE_SINGLE, MUL_TABLE_MULTI, MUL_TABLE_GENERATOR = 0, 1, 2  # MSM377_MUL_TABLE_*
_MUL_TABLES = {"single": MUL_TABLE_SINGLE, "multi": MUL_TABLE_MULTI, "generator": MUL_TABLE_GENERATOR}
MUL_TABLE_RECORD_WORDS = 32


class _BasesInfoStruct(ctypes.Structure):  # msm377_bases_info
    _fields_ = [
        ("form", ctypes.c_uint32),
        ("record_words", ctypes.c_uint32),
        ("limbs", ctypes.c_uint32),
        ("coords", ctypes.c_uint32),
        ("n", ctypes.c_uint64),
        ("windows", ctypes.c_uint32),
        ("glv", ctypes.c_uint32),
        ("window_stride", ctypes.c_uint64),
        ("records", ctypes.c_uint64),
        ("flagged", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("window_bits", ctypes.c_uint32 * 16),
    ]


class BasesInfo(NamedTuple):
    """msm377_bases_info: the base records the last conversion left (include/msm377.h); ``window_bits`` holds one entry
    per window of a precomputed table and is empty otherwise."""

    form: int
    record_words: int
    limbs: int
    coords: int
    n: int
    windows: int
    glv: int
    window_stride: int
    records: int
    flagged: int
    window_bits: Tuple[int, ...]


class _MulTableInfoStruct(ctypes.Structure):  # msm377_mul_table_info
    _fields_ = [("width", ctypes.c_uint32), ("rows", ctypes.c_uint32), ("records", ctypes.c_uint64), ("key", ctypes.c_uint8 * 96)]


class MulTableInfo(NamedTuple):
    """msm377_mul_table_info: width c, rows W + 1, records W 2^(c-1) + 1 and the 96 key bytes of a window table."""

    width: int
    rows: int
    records: int
    key: bytes


class _WalkStashInfoStruct(ctypes.Structure):  # msm377_walk_stash_info
    _fields_ = [(f, ctypes.c_uint32) for f in ("kind", "form", "point_words", "product_words")] + [(f, ctypes.c_uint64) for f in ("n", "pass_offset", "m")] + [
        (f, ctypes.c_uint32) for f in ("width", "k", "segments", "product_pad")] + [("stride", ctypes.c_uint64)]


class WalkStashInfo(NamedTuple):
    """msm377_walk_stash_info: the last pass of the last batch call -- the call (WALK_*), the record form (WALK_FORM_*) and
    its word counts, the call's n, the pass (pass_offset, m), the width it walked, k, and the row commitments' segments
    and stride."""

    kind: int
    form: int
    point_words: int
    product_words: int
    n: int
    pass_offset: int
    m: int
    width: int
    k: int
    segments: int
    product_pad: int
    stride: int


class _WalkTablesInfoStruct(ctypes.Structure):  # msm377_walk_tables_info
    _fields_ = [("m", ctypes.c_uint64), ("tables", ctypes.c_uint32), ("entries", ctypes.c_uint32)]


class WalkTablesInfo(NamedTuple):
    """msm377_walk_tables_info: points of the pass, tables (1: variable-base, 2: pairwise), entries per point (8)."""

    m: int
    tables: int
    entries: int


WALK_BATCH_MUL, WALK_BATCH_MUL_MULTI, WALK_COMMIT_ROWS, WALK_BATCH_MUL_VAR, WALK_BATCH_LINCOMB2, WALK_ED_BATCH_MUL_MULTI = 1, 2, 3, 4, 5, 6
WALK_ED_BATCH_MUL_VAR = 7
WALK_ED_BATCH_LINCOMB2 = 8
WALK_ED_COMMIT_ROWS = 9
WALK_ED_BATCH_LINCOMB = 10
WALK_FORM_XYZZ, WALK_FORM_ED = 0, 1


class CheckReport(NamedTuple):
    """msm377_check_report: a point is counted once, in the first class it fails; ``first_bad`` is the lowest failing
    index (None if every point passed) and ``first_bad_reason`` the CHECK_* bit it failed (0 if none)."""

    checked: int
    noncanonical: int
    off_curve: int
    outside_subgroup: int
    first_bad: Optional[int]
    first_bad_reason: int

    @property
    def ok(self) -> bool:
        return self.first_bad is None


def _report(r: _CheckReportStruct) -> CheckReport:
    none = r.first_bad == 2**64 - 1
    return CheckReport(int(r.checked), int(r.noncanonical), int(r.off_curve), int(r.outside_subgroup), None if none else int(r.first_bad), int(r.first_bad_reason))


class MsmError(RuntimeError):
    """Raised for any non-zero return of the C ABI (the reference throws Error /
    AssertionError, src/submission/implementation/cuzk/gpu.ts:7-10, submission.ts:405)."""

    def __init__(self, code: int, what: str, detail: str = "", index=None):
        self.code = code
        # EPOINT: the lowest failing index -- given by the caller, or the "point <i>" of msm377_last_error's text
        found = re.search(r"\bpoint (\d+)\b", detail) if code == EPOINT and index is None else None
        self.index = int(found.group(1)) if found else index
        # ed_batch_lincomb2*: the array that index counts in, "p" or "q" ("point <i> of q ..."); None for every other call
        of = re.search(r"\bpoint \d+ of ([pq])\b", detail) if code == EPOINT else None
        self.array = of.group(1) if of else None
        # ed_batch_lincomb*: the term that index counts in ("point <i> of term <j> ..."); None for every other call
        term = re.search(r"\bof term (\d+)\b", detail) if code == EPOINT else None
        self.term = int(term.group(1)) if term else None
        msg = "%s failed: %s (%d)" % (what, _strerror(code), code)
        if detail:
            msg += ": " + detail
        super().__init__(msg)


def library_path() -> str:
    """csrc/libmsm377.so next to this package.  MSM377_LIB points tools/ab_libs.sh at another BUILD of the same
    library (an A/B of two engine versions on one box); it is never a different implementation."""
    override = os.environ.get("MSM377_LIB")
    if override:
        return os.path.abspath(override)
    here = os.path.dirname(os.path.abspath(__file__))
    return os.path.normpath(os.path.join(here, "..", "csrc", "libmsm377.so"))


def load_library():
    """Load csrc/libmsm377.so (built by __graft_entry__.build() / make -C csrc)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(
            "msm377: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C webgpu-msm-bls12-377_amd/csrc`; there is no CPU fallback" % path
        )
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64 with the same
    # SONAME as /opt/rocm's.  If this library pulled in the system copy first, a later `import torch`
    # would bind to it and fail ("No HIP GPUs are available"); loading torch's first makes both share
    # one runtime (measured working on the MI355X box).  Hosts without torch (node, C) use /opt/rocm's.
    if "torch" not in sys.modules and os.environ.get("MSM377_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except Exception:  # torch is optional plumbing
            pass
    lib = ctypes.CDLL(path)
    u8p, vp, u64, u32, i32 = ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    sigs = {
        "msm377_version": (ctypes.c_char_p, []),
        "msm377_strerror": (ctypes.c_char_p, [i32]),
        "msm377_ctx_create": (i32, [i32, u64, ctypes.POINTER(vp)]),
        "msm377_ctx_destroy": (None, [vp]),
        "msm377_last_error": (ctypes.c_char_p, [vp]),
        "msm377_g1_msm": (i32, [vp, u8p, u8p, u64, vp]),
        "msm377_g1_msm_device": (i32, [vp, vp, vp, u64, vp]),
        "msm377_g1_set_bases": (i32, [vp, u8p, u64]),
        "msm377_g1_set_bases_device": (i32, [vp, vp, u64]),
        "msm377_g1_set_bases_precomputed": (i32, [vp, u8p, u64]),
        "msm377_g1_set_bases_precomputed_device": (i32, [vp, vp, u64]),
        "msm377_g1_msm_fixed_base": (i32, [vp, u8p, u64, vp]),
        "msm377_g1_msm_fixed_base_device": (i32, [vp, vp, u64, vp]),
        "msm377_g1_msm_fixed_base_batch_device": (i32, [vp, vp, u64, u32, vp]),
        "msm377_g1_window_partials_device": (i32, [vp, vp, vp, u64, u32, u32, vp]),
        "msm377_g1_window_partials_resident": (i32, [vp, vp, vp, u64, u32, u32, vp]),
        "msm377_g1_combine_partials": (i32, [vp, vp]),
        "msm377_g1_combine_partials_split": (i32, [vp, ctypes.c_uint32, vp]),
        "msm377_g1_combine_partials_ctx": (i32, [vp, vp, vp]),
        "msm377_ctx_get_fallback_info": (i32, [vp, ctypes.POINTER(u64), ctypes.POINTER(u32)]),
        "msm377_g1_glv_window_partials_device": (i32, [vp, vp, vp, u64, u32, u32, vp]),
        "msm377_g1_combine_window_partials": (i32, [vp, u32, vp]),
        "msm377_g1_generate_bases_device": (i32, [vp, u64, u64, vp]),
        "msm377_ed_msm": (i32, [vp, u8p, u8p, u64, vp]),
        "msm377_ed_msm_device": (i32, [vp, vp, vp, u64, vp]),
        "msm377_ed_generate_bases_device": (i32, [vp, u64, u64, vp]),
        "msm377_ctx_set_stage_capture": (i32, [vp, i32]),
        "msm377_g1_read_stage": (i32, [vp, u32, vp, vp, vp, vp]),
        "msm377_g1_read_stage_ex": (i32, [vp, u32, vp, vp, vp, vp, vp]),
        "msm377_g1_read_bases": (i32, [vp, vp, u64, u64, vp]),
        "msm377_g1_read_partials": (i32, [vp, vp, vp]),
        "msm377_g1_read_work_list": (i32, [vp, vp, vp, vp, vp, u64, u64, vp]),
        "msm377_g1_read_mul_table": (i32, [vp, u32, u32, vp, u64, u64, vp]),
        "msm377_read_walk_stash": (i32, [vp, vp, u32, u64, u64, vp, vp]),
        "msm377_g1_read_walk_tables": (i32, [vp, vp, u32, u64, u64, vp]),
        "msm377_g1_xyzz_to_affine": (i32, [vp, vp]),
        "msm377_g1_fold_window_partials": (i32, [vp, ctypes.c_uint32]),
        "msm377_ctx_set_glv": (i32, [vp, i32]),
        "msm377_ctx_set_g1_form": (i32, [vp, i32]),
        "msm377_ctx_set_timing": (i32, [vp, i32]),
        "msm377_ctx_get_stage_ms": (i32, [vp, vp]),
        "msm377_ctx_get_products_per_addition": (i32, [vp]),
        "msm377_ctx_set_precompute_window": (i32, [vp, i32]),
        "msm377_g1_add_points": (i32, [vp, u32, vp]),
        "msm377_ctx_reserve_host_staging": (i32, [vp]),
        "msm377_ctx_get_stage_form": (i32, [vp]),
        "msm377_ctx_set_narrow_max": (i32, [vp, u64]),
        "msm377_g1_check_points_device": (i32, [vp, vp, u64, u32, vp]),
        "msm377_g1_check_points": (i32, [vp, u8p, u64, u32, vp]),
        "msm377_ed_check_points_device": (i32, [vp, vp, u64, u32, vp]),
        "msm377_ed_check_points": (i32, [vp, u8p, u64, u32, vp]),
        "msm377_g1_check_points_host": (i32, [u8p, u64, u32, vp]),
        "msm377_ed_check_points_host": (i32, [u8p, u64, u32, vp]),
        "msm377_ctx_set_base_checks": (i32, [vp, u32]),
        "msm377_ctx_get_last_check": (i32, [vp, vp]),
        "msm377_g1_msm_short": (i32, [vp, u8p, u8p, u64, u32, u32, vp]),
        "msm377_g1_msm_short_device": (i32, [vp, vp, vp, u64, u32, u32, vp]),
        "msm377_g1_msm_fixed_base_short_device": (i32, [vp, vp, u64, u32, u32, vp]),
        "msm377_scalars_width_device": (i32, [vp, vp, u64, u32, ctypes.POINTER(u32)]),
        "msm377_scalars_width_host": (i32, [u8p, u64, u32, ctypes.POINTER(u32)]),
        "msm377_short_windows": (u32, [u32, u32]),
        "msm377_ctx_get_last_geometry": (i32, [vp, ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "msm377_ctx_get_last_sort_elem_bytes": (u32, [vp]),
        "msm377_ctx_set_input_format": (i32, [vp, u32, u32]),
        "msm377_ctx_get_input_format": (i32, [vp, ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "msm377_g1_import_points_host": (i32, [u8p, u64, u32, vp, vp]),
        "msm377_import_scalars_host": (i32, [u8p, u64, u32, vp]),
        "msm377_g1_result_to_native": (i32, [u8p, vp]),
        "msm377_g1_batch_mul_device": (i32, [vp, u8p, vp, u64, u32, vp, vp]),
        "msm377_g1_batch_mul": (i32, [vp, u8p, u8p, u64, u32, vp, vp]),
        "msm377_g1_batch_mul_host": (i32, [u8p, u8p, u64, u32, vp, vp]),
        "msm377_g1_batch_mul_multi_device": (i32, [vp, u8p, u32, vp, u64, u64, u64, u32, vp, vp]),
        "msm377_g1_batch_mul_multi": (i32, [vp, u8p, u32, u8p, u64, u64, u64, u32, vp, vp]),
        "msm377_g1_batch_mul_multi_host": (i32, [u8p, u32, u8p, u64, u64, u64, u32, vp, vp]),
        "msm377_ctx_get_mul_multi_table_builds": (u64, [vp]),
        "msm377_g1_set_generators": (i32, [vp, u8p, u32, i32]),
        "msm377_ctx_get_generators": (i32, [vp, vp, vp]),
        "msm377_g1_commit_rows_device": (i32, [vp, vp, u64, u32, u64, u64, u32, vp, vp]),
        "msm377_g1_commit_rows": (i32, [vp, u8p, u64, u32, u64, u64, u32, vp, vp]),
        "msm377_g1_commit_rows_host": (i32, [u8p, u32, u8p, u32, u64, u64, u64, u32, vp, vp]),
        "msm377_commit_rows_plan": (None, [u32, vp, vp, vp]),
        "msm377_g1_batch_mul_var_device": (i32, [vp, vp, vp, u64, u32, u32, vp, vp]),
        "msm377_g1_batch_mul_var": (i32, [vp, u8p, u8p, u64, u32, u32, vp, vp]),
        "msm377_g1_batch_mul_var_host": (i32, [u8p, u32, u8p, u32, u64, u32, u32, vp, vp]),
        "msm377_g1_batch_lincomb2_device": (i32, [vp, vp, vp, vp, vp, u64, u32, u32, u32, vp, vp]),
        "msm377_g1_batch_lincomb2": (i32, [vp, u8p, u8p, u8p, u8p, u64, u32, u32, u32, vp, vp]),
        "msm377_g1_batch_lincomb2_host": (i32, [u8p, u8p, u32, u8p, u8p, u32, u64, u32, u32, u32, vp, vp]),
        "msm377_ed_batch_mul_multi_device": (i32, [vp, u8p, u32, vp, u64, u64, u64, vp]),
        "msm377_ed_batch_mul_multi": (i32, [vp, u8p, u32, u8p, u64, u64, u64, vp]),
        "msm377_ed_batch_mul_multi_host": (i32, [u8p, u32, u8p, u64, u64, u64, vp]),
        "msm377_ed_batch_mul_var_device": (i32, [vp, vp, vp, u64, u32, vp]),
        "msm377_ed_batch_mul_var": (i32, [vp, u8p, u8p, u64, u32, vp]),
        "msm377_ed_batch_mul_var_host": (i32, [u8p, u8p, u64, u32, vp]),
        "msm377_ed_read_walk_tables": (i32, [vp, vp, u64, u64, vp]),
        "msm377_ed_batch_lincomb2_device": (i32, [vp, vp, vp, vp, vp, u64, u32, u32, u32, u32, vp]),
        "msm377_ed_batch_lincomb2": (i32, [vp, u8p, u8p, u8p, u8p, u64, u32, u32, u32, u32, vp]),
        "msm377_ed_batch_lincomb2_host": (i32, [u8p, u8p, u8p, u8p, u64, u32, u32, u32, u32, vp]),
        "msm377_ed_read_walk_table": (i32, [vp, vp, u32, u64, u64, vp]),
        "msm377_ed_batch_lincomb_device": (i32, [vp, vp, u32, u64, vp]),
        "msm377_ed_batch_lincomb": (i32, [vp, vp, u32, u64, vp]),
        "msm377_ed_batch_lincomb_host": (i32, [vp, u32, u64, vp]),
        "msm377_ed_ctx_get_mul_table_builds": (u64, [vp]),
        "msm377_ed_read_mul_table": (i32, [vp, u32, vp, u64, u64, vp]),
        "msm377_ed_set_generators": (i32, [vp, u8p, u32, i32]),
        "msm377_ed_ctx_get_generators": (i32, [vp, vp, vp]),
        "msm377_ed_commit_rows_device": (i32, [vp, vp, u64, u32, u64, u64, vp]),
        "msm377_ed_commit_rows": (i32, [vp, u8p, u64, u32, u64, u64, vp]),
        "msm377_ed_commit_rows_host": (i32, [u8p, u32, u8p, u64, u64, u64, vp]),
        "msm377_ed_read_generator_table": (i32, [vp, u32, vp, u64, u64, vp]),
        "msm377_ctx_set_mul_window": (i32, [vp, i32]),
        "msm377_ctx_get_last_mul_window": (i32, [vp]),
        "msm377_ctx_get_mul_table_builds": (u64, [vp]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def _strerror(code: int) -> str:
    try:
        return load_library().msm377_strerror(code).decode()
    except Exception:  # pragma: no cover
        return "error"


def _check_host(fn: str, points: bytes, point_bytes: int, flags: int) -> CheckReport:
    if len(points) % point_bytes:
        raise ValueError("points buffer length must be a multiple of %d" % point_bytes)
    lib = load_library()
    rep = _CheckReportStruct()
    rc = getattr(lib, fn)(bytes(points), len(points) // point_bytes, int(flags), ctypes.addressof(rep))
    if rc:
        raise MsmError(rc, fn)
    return _report(rep)


def check_points_host(points: bytes, flags: int = CHECK_ALL) -> CheckReport:
    """Canonical / on-curve / subgroup report of G1 wire points on the calling thread (msm377_g1_check_points_host): no
    context, no device -- small sets, and the yardstick of MsmEngine.check_points."""
    return _check_host("msm377_g1_check_points_host", points, 96, flags)


def ed_check_points_host(points: bytes, flags: int = CHECK_ALL) -> CheckReport:
    """The same for Edwards-BLS12 wire points, 64 bytes each (msm377_ed_check_points_host)."""
    return _check_host("msm377_ed_check_points_host", points, 64, flags)


def scalars_width_host(scalars: bytes, scalar_bytes: int = 32) -> int:
    """Largest bit length among little-endian scalars of ``scalar_bytes`` bytes each (msm377_scalars_width_host; 0 for
    all-zero scalars and for an empty buffer): what a short-scalar call takes as ``scalar_bits``.  No device."""
    if scalar_bytes in (4, 8, 16, 32) and len(scalars) % scalar_bytes:
        raise ValueError("scalars buffer length must be a multiple of %d" % scalar_bytes)
    lib = load_library()
    bits = ctypes.c_uint32()
    rc = lib.msm377_scalars_width_host(bytes(scalars), len(scalars) // max(1, int(scalar_bytes)), int(scalar_bytes), ctypes.byref(bits))
    if rc:
        raise MsmError(rc, "msm377_scalars_width_host")
    return int(bits.value)


def _form(table, form, what):
    if form in table:
        return table[form]
    if isinstance(form, str):
        raise ValueError("%s form must be one of %s" % (what, sorted(table)))
    return int(form)  # a raw value: the library validates it


def import_points_host(points: bytes, form="mont_flag") -> Tuple[bytes, List[int]]:
    """Native-form G1 points -> (wire records, infinity mask words) on the calling thread
    (msm377_g1_import_points_host): no context, no device.  A flagged point's record is the generator's and its mask
    bit (bit i % 32 of word i // 32) is set."""
    f = _form(_POINT_FORMS, form, "point")
    stride = _POINT_STRIDE.get(f, 96)
    if len(points) % stride:
        raise ValueError("points buffer length must be a multiple of %d" % stride)
    n = len(points) // stride
    out = ctypes.create_string_buffer(max(1, 96 * n))
    mask = (ctypes.c_uint32 * max(1, (n + 31) // 32))()
    rc = load_library().msm377_g1_import_points_host(bytes(points), n, f, ctypes.addressof(out), ctypes.addressof(mask))
    if rc:
        raise MsmError(rc, "msm377_g1_import_points_host")
    return out.raw[: 96 * n], list(mask)[: (n + 31) // 32]


def import_scalars_host(scalars: bytes, form="mont") -> bytes:
    """Native-form scalars -> canonical 32-byte scalars (msm377_import_scalars_host): every Montgomery value v gives
    v * 2^-256 mod r."""
    if len(scalars) % 32:
        raise ValueError("scalars buffer length must be a multiple of 32")
    n = len(scalars) // 32
    out = ctypes.create_string_buffer(max(1, 32 * n))
    rc = load_library().msm377_import_scalars_host(bytes(scalars), n, _form(_SCALAR_FORMS, form, "scalar"), ctypes.addressof(out))
    if rc:
        raise MsmError(rc, "msm377_import_scalars_host")
    return out.raw[: 32 * n]


def result_to_native(xy: bytes) -> bytes:
    """A 96-byte wire result as a 104-byte mont_flag record; the wire identity (0, 1) sets the flag
    (msm377_g1_result_to_native)."""
    if len(xy) != 96:
        raise ValueError("a result is 96 bytes")
    out = ctypes.create_string_buffer(104)
    rc = load_library().msm377_g1_result_to_native(bytes(xy), ctypes.addressof(out))
    if rc:
        raise MsmError(rc, "msm377_g1_result_to_native")
    return out.raw


def _batch_mul_out_form(out_form) -> int:
    """Output forms of the batch_mul calls: "wire" or "mont_flag" (plain "mont" cannot say "identity": the library
    refuses it)."""
    return _form(_POINT_FORMS, out_form, "output")


def batch_mul_host(base: bytes, scalars: bytes, out_form="wire") -> Tuple[bytes, bytes]:
    """out[i] = [s_i]B on the calling thread (msm377_g1_batch_mul_host): no context, no device.  ``base``: 96 wire
    bytes; ``scalars``: 32-byte little-endian integers, any value below 2^256.  Returns (records, identity flags): 96-byte
    wire or 104-byte mont_flag records and one byte per output, 1 for the identity."""
    if len(base) != 96:
        raise ValueError("a base is 96 bytes")
    if len(scalars) % 32:
        raise ValueError("scalars buffer length must be a multiple of 32")
    f = _batch_mul_out_form(out_form)
    n = len(scalars) // 32
    stride = _POINT_STRIDE.get(f, 96)
    out = ctypes.create_string_buffer(max(1, stride * n))
    inf = ctypes.create_string_buffer(max(1, n))
    rc = load_library().msm377_g1_batch_mul_host(bytes(base), bytes(scalars), n, f, ctypes.addressof(out), ctypes.addressof(inf))
    if rc:
        raise MsmError(rc, "msm377_g1_batch_mul_host")
    return out.raw[: stride * n], inf.raw[:n]


MUL_MAX_BASES = 16  # MSM377_MUL_MAX_BASES


def _multi_shape(bases: bytes, scalars: bytes, layout: str) -> Tuple[int, int, int, int]:
    """(k, n, out_stride, base_stride) of a dense k x n scalar matrix: ``layout`` "rows" (the k scalars of an output side by
    side) or "columns" (the n scalars of a base side by side)."""
    if len(bases) % 96 or not 1 <= len(bases) // 96 <= MUL_MAX_BASES:
        raise ValueError("bases: 1 to %d records of 96 bytes" % MUL_MAX_BASES)
    k = len(bases) // 96
    if len(scalars) % (32 * k):
        raise ValueError("scalars buffer length must be a multiple of 32 k")
    n = len(scalars) // (32 * k)
    if layout == "rows":
        return k, n, 32 * k, 32
    if layout == "columns":
        return k, n, 32, 32 * max(n, 1)
    raise ValueError('layout is "rows" or "columns"')


def batch_mul_multi_host(bases: bytes, scalars: bytes, out_form="wire", layout="rows") -> Tuple[bytes, bytes]:
    """out[i] = sum_j [s_ij]B_j on the calling thread (msm377_g1_batch_mul_multi_host): no context, no device.  ``bases``:
    k records of 96 wire bytes; ``scalars``: the k x n matrix of 32-byte little-endian integers in ``layout``.  Returns
    (records, identity flags) as batch_mul_host does."""
    k, n, out_stride, base_stride = _multi_shape(bases, scalars, layout)
    f = _batch_mul_out_form(out_form)
    stride = _POINT_STRIDE.get(f, 96)
    out = ctypes.create_string_buffer(max(1, stride * n))
    inf = ctypes.create_string_buffer(max(1, n))
    rc = load_library().msm377_g1_batch_mul_multi_host(bytes(bases), k, bytes(scalars), n, out_stride, base_stride, f, ctypes.addressof(out), ctypes.addressof(inf))
    if rc:
        raise MsmError(rc, "msm377_g1_batch_mul_multi_host")
    return out.raw[: stride * n], inf.raw[:n]


def _ed_multi_shape(bases: bytes, scalars: bytes, layout: str) -> Tuple[int, int, int, int]:
    """_multi_shape for Edwards-BLS12 bases, 64 wire bytes each."""
    if len(bases) % 64 or not 1 <= len(bases) // 64 <= MUL_MAX_BASES:
        raise ValueError("bases: 1 to %d records of 64 bytes" % MUL_MAX_BASES)
    return _multi_shape(b"\0" * (96 * (len(bases) // 64)), scalars, layout)


def ed_batch_mul_multi_host(bases: bytes, scalars: bytes, layout="rows") -> bytes:
    """out[i] = sum_j [s_ij]B_j on Edwards-BLS12 on the calling thread (msm377_ed_batch_mul_multi_host): no context, no
    device.  ``bases``: k records of 64 wire bytes, every one a curve point; ``scalars``: the k x n matrix of 32-byte
    little-endian integers in ``layout``, any value below 2^256.  Returns n 64-byte wire records; the identity is (0, 1)."""
    k, n, out_stride, base_stride = _ed_multi_shape(bases, scalars, layout)
    out = ctypes.create_string_buffer(max(1, 64 * n))
    rc = load_library().msm377_ed_batch_mul_multi_host(bytes(bases), k, bytes(scalars), n, out_stride, base_stride, ctypes.addressof(out))
    if rc:
        raise MsmError(rc, "msm377_ed_batch_mul_multi_host")
    return out.raw[: 64 * n]


def _ed_var_shape(points: bytes, scalars: bytes) -> Tuple[int, int]:
    """(n, scalar_stride) of n 64-byte Edwards-BLS12 points and their scalars."""
    if len(points) % 64:
        raise ValueError("an Edwards-BLS12 point is 64 bytes")
    n = len(points) // 64
    return n, _var_scalar_stride(scalars, n)


def ed_batch_mul_var_host(points: bytes, scalars: bytes) -> bytes:
    """out[i] = [s_i]P_i on Edwards-BLS12 on the calling thread (msm377_ed_batch_mul_var_host): no context, no device.
    ``points``: n records of 64 wire bytes, every one a curve point; ``scalars``: 32 bytes per point, or 32 bytes for all of
    them, any value below 2^256.  Returns n 64-byte wire records; the identity is (0, 1).  A point that is not on the
    curve raises MsmError(EPOINT) whose ``index`` is the lowest failing one (msm377_ed_check_points_host names it)."""
    n, stride = _ed_var_shape(points, scalars)
    out = ctypes.create_string_buffer(max(1, 64 * n))
    rc = load_library().msm377_ed_batch_mul_var_host(bytes(points), bytes(scalars), n, stride, ctypes.addressof(out))
    if rc == EPOINT:
        rep = ed_check_points_host(points, CHECK_CANONICAL | CHECK_CURVE)
        why = "has a coordinate that is not below q" if rep.first_bad_reason == CHECK_CANONICAL else "is not on the curve"
        raise MsmError(rc, "msm377_ed_batch_mul_var_host", "point %d %s" % (rep.first_bad, why), index=rep.first_bad)
    if rc:
        raise MsmError(rc, "msm377_ed_batch_mul_var_host")
    return out.raw[: 64 * n]


def _ed_lincomb2_shape(p: bytes, q: bytes, a: bytes, b: bytes) -> Tuple[int, int, int, int, int]:
    """(n, p_stride, q_stride, a_stride, b_stride) of the four arrays of an Edwards-BLS12 linear combination: n is the
    largest element count; an argument of exactly one element, with n > 1, is the stride-0 form (one for all pairs)."""
    if len(p) % 64 or len(q) % 64 or len(a) % 32 or len(b) % 32:
        raise ValueError("an Edwards-BLS12 point is 64 bytes, a scalar 32")
    counts = (len(p) // 64, len(q) // 64, len(a) // 32, len(b) // 32)
    n = max(counts)
    strides = []
    for count, size in zip(counts, (64, 64, 32, 32)):
        if count != n and not (count == 1 and n > 1):
            raise ValueError("p, q, a and b: one element per pair, or exactly one element for all pairs")
        strides.append(size if count == n else 0)
    return (n, *strides)


def ed_batch_lincomb2_host(p: bytes, q: bytes, a: bytes, b: bytes) -> bytes:
    """out[i] = [a_i]P_i + [b_i]Q_i on Edwards-BLS12 on the calling thread (msm377_ed_batch_lincomb2_host): no context, no
    device.  ``p``, ``q``: 64-byte wire records, every one a curve point; ``a``, ``b``: 32-byte scalars, any value below
    2^256.  n is the largest element count; an argument of exactly one element with n > 1 stands for all pairs.  Returns n
    64-byte wire records; the identity is (0, 1).  A point that is not on the curve raises MsmError(EPOINT) with its
    ``array`` ("p" or "q") and ``index``: the lower index of the two arrays' findings, p where they are equal."""
    n, ps, qs, sa, sb = _ed_lincomb2_shape(p, q, a, b)
    out = ctypes.create_string_buffer(max(1, 64 * n))
    rc = load_library().msm377_ed_batch_lincomb2_host(bytes(p), bytes(q), bytes(a), bytes(b), n, ps, qs, sa, sb, ctypes.addressof(out))
    if rc == EPOINT:
        reps = [ed_check_points_host(pts, CHECK_CANONICAL | CHECK_CURVE) for pts in (p, q)]
        bad = [n if r.first_bad is None else r.first_bad for r in reps]
        t = 1 if bad[1] < bad[0] else 0
        why = "has a coordinate that is not below q" if reps[t].first_bad_reason == CHECK_CANONICAL else "is not on the curve"
        raise MsmError(rc, "msm377_ed_batch_lincomb2_host", "point %d of %s %s" % (bad[t], "pq"[t], why), index=bad[t])
    if rc:
        raise MsmError(rc, "msm377_ed_batch_lincomb2_host")
    return out.raw[: 64 * n]


LINCOMB_MAX_TERMS = 8  # MSM377_LINCOMB_MAX_TERMS


class _LincombTermStruct(ctypes.Structure):
    """msm377_lincomb_term"""

    _fields_ = [("points", ctypes.c_void_p), ("scalars", ctypes.c_void_p), ("point_stride", ctypes.c_uint32), ("scalar_stride", ctypes.c_uint32)]


def _lincomb_terms(terms):
    """The C array of msm377_lincomb_term for ``terms``, a sequence of (points, scalars, point_stride, scalar_stride) with the
    two pointers as integers (0: NULL); None for an empty sequence (the NULL ``terms`` of the C call)."""
    if not terms:
        return None
    arr = (_LincombTermStruct * len(terms))()
    for slot, (pts, scs, ps, ss) in zip(arr, terms):
        slot.points, slot.scalars, slot.point_stride, slot.scalar_stride = pts or None, scs or None, int(ps), int(ss)
    return arr


def _ed_lincomb_shape(points_list, scalars_list) -> Tuple[int, list]:
    """(n, [(point_stride, scalar_stride)] per term) of the k terms of an Edwards-BLS12 linear combination: n is the largest
    element count; an argument of exactly one element, with n > 1, is the stride-0 form (one for all outputs)."""
    if len(points_list) != len(scalars_list):
        raise ValueError("one array of scalars per array of points")
    if any(len(p) % 64 for p in points_list) or any(len(s) % 32 for s in scalars_list):
        raise ValueError("an Edwards-BLS12 point is 64 bytes, a scalar 32")
    counts = [(len(p) // 64, len(s) // 32) for p, s in zip(points_list, scalars_list)]
    n = max((c for pair in counts for c in pair), default=0)
    if any(c != n and not (c == 1 and n > 1) for pair in counts for c in pair):
        raise ValueError("every term: one element per output, or exactly one element for all outputs")
    return n, [(64 if cp == n else 0, 32 if cs == n else 0) for cp, cs in counts]


def _lincomb_host_terms(points_list, scalars_list, strides):
    """(C array, the buffers it points into) for host-buffer terms."""
    keep = [(ctypes.create_string_buffer(bytes(p), max(1, len(p))), ctypes.create_string_buffer(bytes(s), max(1, len(s)))) for p, s in zip(points_list, scalars_list)]
    return _lincomb_terms([(ctypes.addressof(p), ctypes.addressof(s), ps, ss) for (p, s), (ps, ss) in zip(keep, strides)]), keep


def ed_batch_lincomb_host(points_list, scalars_list) -> bytes:
    """out[i] = sum_j [s_ij]P_ij on Edwards-BLS12 on the calling thread (msm377_ed_batch_lincomb_host): no context, no
    device.  ``points_list``: k buffers of 64-byte wire records, every one a curve point; ``scalars_list``: k buffers of
    32-byte scalars, any value below 2^256; 1 <= k <= 8.  n is the largest element count; a buffer of exactly one element
    with n > 1 stands for all outputs.  Returns n 64-byte wire records; the identity is (0, 1).  A point that is not on the
    curve raises MsmError(EPOINT) with its ``term`` and ``index``: the lowest index of all findings, the lowest term where
    indices are equal."""
    n, strides = _ed_lincomb_shape(points_list, scalars_list)
    terms, keep = _lincomb_host_terms(points_list, scalars_list, strides)
    out = ctypes.create_string_buffer(max(1, 64 * n))
    rc = load_library().msm377_ed_batch_lincomb_host(terms, len(points_list), n, ctypes.addressof(out))
    if rc == EPOINT:
        reps = [ed_check_points_host(bytes(p), CHECK_CANONICAL | CHECK_CURVE) for p in points_list]
        bad = [n if r.first_bad is None else r.first_bad for r in reps]
        t = bad.index(min(bad))
        why = "has a coordinate that is not below q" if reps[t].first_bad_reason == CHECK_CANONICAL else "is not on the curve"
        raise MsmError(rc, "msm377_ed_batch_lincomb_host", "point %d of term %d %s" % (bad[t], t, why), index=bad[t])
    if rc:
        raise MsmError(rc, "msm377_ed_batch_lincomb_host")
    del keep
    return out.raw[: 64 * n]


GEN_MAX = 4096  # MSM377_GEN_MAX
GEN_WIDE_MAX = 64  # MSM377_GEN_WIDE_MAX


def _rows_shape(k: int, scalars: bytes, layout: str) -> Tuple[int, int, int]:
    """(n, out_stride, base_stride) of a dense k x n scalar matrix in ``layout`` ("rows" or "columns")."""
    if not 1 <= k <= GEN_MAX:
        raise ValueError("k: 1 to %d generators" % GEN_MAX)
    if len(scalars) % (32 * k):
        raise ValueError("scalars buffer length must be a multiple of 32 k")
    n = len(scalars) // (32 * k)
    if layout == "rows":
        return n, 32 * k, 32
    if layout == "columns":
        return n, 32, 32 * max(n, 1)
    raise ValueError('layout is "rows" or "columns"')


def commit_rows_host(gens: bytes, scalars: bytes, out_form="wire", layout="rows", scalar_form="wire") -> Tuple[bytes, bytes]:
    """out[i] = sum_j [s_ij]G_j on the calling thread (msm377_g1_commit_rows_host): no context, no device.  ``gens``: k
    records of 96 wire bytes, k up to 4 096; ``scalars``: the k x n matrix of 32-byte values in ``layout`` and
    ``scalar_form`` ("wire" or "mont").  Returns (records, identity flags) as batch_mul_host does."""
    if len(gens) % 96:
        raise ValueError("a generator is 96 bytes")
    k = len(gens) // 96
    n, out_stride, base_stride = _rows_shape(k, scalars, layout)
    f = _batch_mul_out_form(out_form)
    stride = _POINT_STRIDE.get(f, 96)
    out = ctypes.create_string_buffer(max(1, stride * n))
    inf = ctypes.create_string_buffer(max(1, n))
    rc = load_library().msm377_g1_commit_rows_host(
        bytes(gens), k, bytes(scalars), _form(_SCALAR_FORMS, scalar_form, "scalar"), n, out_stride, base_stride, f, ctypes.addressof(out), ctypes.addressof(inf)
    )
    if rc:
        raise MsmError(rc, "msm377_g1_commit_rows_host")
    return out.raw[: stride * n], inf.raw[:n]


def ed_commit_rows_host(gens: bytes, scalars: bytes, layout="rows") -> bytes:
    """out[i] = sum_j [s_ij]G_j on Edwards-BLS12 on the calling thread (msm377_ed_commit_rows_host): no context, no device.
    ``gens``: k records of 64 wire bytes, k up to 4 096, every one a curve point; ``scalars``: the k x n matrix of 32-byte
    little-endian integers in ``layout``, any value below 2^256.  Returns n 64-byte wire records; the identity is (0, 1).
    A generator that is not on the curve raises MsmError(EPOINT) whose ``index`` is the lowest failing one
    (msm377_ed_check_points_host names it)."""
    if len(gens) % 64:
        raise ValueError("an Edwards-BLS12 generator is 64 bytes")
    k = len(gens) // 64
    n, out_stride, base_stride = _rows_shape(k, scalars, layout)
    out = ctypes.create_string_buffer(max(1, 64 * n))
    rc = load_library().msm377_ed_commit_rows_host(bytes(gens), k, bytes(scalars), n, out_stride, base_stride, ctypes.addressof(out))
    if rc == EPOINT:
        rep = ed_check_points_host(gens, CHECK_CANONICAL | CHECK_CURVE)
        why = "has a coordinate that is not below q" if rep.first_bad_reason == CHECK_CANONICAL else "is not on the curve"
        raise MsmError(rc, "msm377_ed_commit_rows_host", "point %d of the generators %s" % (rep.first_bad, why), index=rep.first_bad)
    if rc:
        raise MsmError(rc, "msm377_ed_commit_rows_host")
    return out.raw[: 64 * n]


def commit_rows_plan(k: int) -> Tuple[int, int, int]:
    """(segments, generators per segment, rows per pass) of a row-commitment call over k generators
    (msm377_commit_rows_plan); (0, 0, 0) for k outside 1 .. 4 096."""
    seg, bps, rows = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    load_library().msm377_commit_rows_plan(int(k), ctypes.addressof(seg), ctypes.addressof(bps), ctypes.addressof(rows))
    return seg.value, bps.value, rows.value


def _var_scalar_stride(scalars: bytes, n: int) -> int:
    """32 (a scalar per point), or 0 when ONE 32-byte scalar stands for all n > 1 points."""
    if len(scalars) == 32 and n > 1:
        return 0
    if len(scalars) != 32 * n:
        raise ValueError("scalars: 32 bytes per point, or 32 bytes for all points")
    return 32


def batch_mul_var_host(points: bytes, scalars: bytes, out_form="wire", point_form="wire", scalar_form="wire") -> Tuple[bytes, bytes]:
    """out[i] = [s_i]P_i on the calling thread (msm377_g1_batch_mul_var_host): no context, no device.  ``points``:
    records of ``point_form``; ``scalars``: 32 bytes per point, or 32 bytes for all of them.  Returns (records, identity
    flags) as batch_mul_host does."""
    pf = _form(_POINT_FORMS, point_form, "point")
    in_stride = _POINT_STRIDE.get(pf, 96)
    if len(points) % in_stride:
        raise ValueError("points buffer length must be a multiple of %d" % in_stride)
    n = len(points) // in_stride
    f = _batch_mul_out_form(out_form)
    stride = _POINT_STRIDE.get(f, 96)
    out = ctypes.create_string_buffer(max(1, stride * n))
    inf = ctypes.create_string_buffer(max(1, n))
    rc = load_library().msm377_g1_batch_mul_var_host(
        bytes(points), pf, bytes(scalars), _form(_SCALAR_FORMS, scalar_form, "scalar"), n, _var_scalar_stride(scalars, n), f, ctypes.addressof(out), ctypes.addressof(inf)
    )
    if rc:
        raise MsmError(rc, "msm377_g1_batch_mul_var_host")
    return out.raw[: stride * n], inf.raw[:n]


def batch_lincomb2_host(p: bytes, q: bytes, a: bytes, b: bytes, out_form="wire", point_form="wire", scalar_form="wire") -> Tuple[bytes, bytes]:
    """out[i] = [a_i]P_i + [b_i]Q_i on the calling thread (msm377_g1_batch_lincomb2_host): no context, no device.  ``p``,
    ``q``: records of ``point_form``, as many of one as of the other; ``a``, ``b``: each 32 bytes per pair, or 32 bytes for
    all of them.  Returns (records, identity flags) as batch_mul_host does."""
    pf = _form(_POINT_FORMS, point_form, "point")
    in_stride = _POINT_STRIDE.get(pf, 96)
    if len(p) % in_stride or len(q) != len(p):
        raise ValueError("p and q: the same number of %d-byte records" % in_stride)
    n = len(p) // in_stride
    f = _batch_mul_out_form(out_form)
    stride = _POINT_STRIDE.get(f, 96)
    out = ctypes.create_string_buffer(max(1, stride * n))
    inf = ctypes.create_string_buffer(max(1, n))
    rc = load_library().msm377_g1_batch_lincomb2_host(
        bytes(p), bytes(q), pf, bytes(a), bytes(b), _form(_SCALAR_FORMS, scalar_form, "scalar"), n, _var_scalar_stride(a, n), _var_scalar_stride(b, n), f,
        ctypes.addressof(out), ctypes.addressof(inf)
    )
    if rc:
        raise MsmError(rc, "msm377_g1_batch_lincomb2_host")
    return out.raw[: stride * n], inf.raw[:n]


def short_windows(scalar_bits: int, bucket_log: int) -> int:
    """Window slots of a short-scalar call: floor(scalar_bits / (bucket_log + 1)) + 1 (msm377_short_windows)."""
    return int(load_library().msm377_short_windows(int(scalar_bits), int(bucket_log)))


def combine_partials_bytes(partials: bytes, num_windows: int = NUM_WINDOWS) -> bytes:
    """Host-only Horner + inversion over the windows' partial records (16 plain, 8 behind the GLV front
    end; msm377_g1_combine_window_partials; replaces submission.ts:290-321)."""
    if len(partials) != num_windows * WINDOW_PARTIAL_BYTES:
        raise ValueError("expected %d bytes of partials" % (num_windows * WINDOW_PARTIAL_BYTES))
    lib = load_library()
    src = (ctypes.c_uint32 * (len(partials) // 4)).from_buffer_copy(partials)
    out = ctypes.create_string_buffer(96)
    rc = lib.msm377_g1_combine_window_partials(ctypes.addressof(src), int(num_windows), ctypes.addressof(out))
    if rc:
        raise MsmError(rc, "msm377_g1_combine_window_partials")
    return out.raw


def add_points_bytes(points: bytes) -> bytes:
    """Sum of affine wire points (96 bytes each; the identity as x = 0, y = 1): the last step of a points-partitioned
    multi-GPU MSM (msm377_g1_add_points, host-only)."""
    if len(points) % 96:
        raise ValueError("points buffer length must be a multiple of 96")
    lib = load_library()
    out = ctypes.create_string_buffer(96)
    rc = lib.msm377_g1_add_points(bytes(points), len(points) // 96, ctypes.addressof(out))
    if rc:
        raise MsmError(rc, "msm377_g1_add_points")
    return out.raw


def combine_partials_split_bytes(partials: bytes, pieces: int) -> bytes:
    """The combine of 16 Edwards-form window records computed as the threaded host tail computes it -- ``pieces``
    balanced pieces of the Horner chain, added up -- on the calling thread (msm377_g1_combine_partials_split)."""
    if len(partials) != NUM_WINDOWS * WINDOW_PARTIAL_BYTES:
        raise ValueError("expected %d bytes of partials" % (NUM_WINDOWS * WINDOW_PARTIAL_BYTES))
    lib = load_library()
    src = (ctypes.c_uint32 * (len(partials) // 4)).from_buffer_copy(partials)
    out = ctypes.create_string_buffer(96)
    rc = lib.msm377_g1_combine_partials_split(ctypes.addressof(src), int(pieces), ctypes.addressof(out))
    if rc:
        raise MsmError(rc, "msm377_g1_combine_partials_split")
    return out.raw


def fold_partials_bytes(partials: bytes) -> bytes:
    """A rank's share of the host tail before the exchange (msm377_g1_fold_window_partials): the records of its
    consecutive windows are replaced by records of the same size and total, all identity but one point."""
    if len(partials) % WINDOW_PARTIAL_BYTES:
        raise ValueError("partials must be whole window records")
    count = len(partials) // WINDOW_PARTIAL_BYTES
    if count == 0:
        return partials
    lib = load_library()
    buf = (ctypes.c_uint32 * (len(partials) // 4)).from_buffer_copy(partials)
    rc = lib.msm377_g1_fold_window_partials(ctypes.addressof(buf), count)
    if rc:
        raise MsmError(rc, "msm377_g1_fold_window_partials")
    return bytes(buf)


def xyzz_to_affine(words: Sequence[int]) -> bytes:
    """One device-format XYZZ point (52 u32) -> 96-byte affine wire format."""
    lib = load_library()
    src = (ctypes.c_uint32 * POINT_WORDS)(*[int(w) for w in words])
    out = ctypes.create_string_buffer(96)
    rc = lib.msm377_g1_xyzz_to_affine(ctypes.addressof(src), ctypes.addressof(out))
    if rc:
        raise MsmError(rc, "msm377_g1_xyzz_to_affine")
    return out.raw


class MsmEngine:
    """One HIP device context: workspace for up to ``max_points`` inputs, reusable across
    calls (the reference re-acquires and destroys the device every call,
    submission.ts:113,288)."""

    def __init__(self, max_points: int, device: int = 0):
        self._lib = load_library()
        self._ctx = ctypes.c_void_p()
        rc = self._lib.msm377_ctx_create(int(device), int(max_points), ctypes.byref(self._ctx))
        if rc:
            self._ctx = ctypes.c_void_p()
            raise MsmError(rc, "msm377_ctx_create", "device %d, max_points %d (is a HIP device visible?)" % (device, max_points))
        self.max_points = int(max_points)
        self.device = int(device)
        self._point_bytes = 96  # bytes per point of the active input form (set_input_format)

    # -- lifetime --
    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._lib.msm377_ctx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc:
            raise MsmError(rc, what, self._lib.msm377_last_error(self._ctx).decode())

    # -- native input forms (include/msm377.h) --
    def set_input_format(self, points="wire", scalars="wire"):
        """Form of the points ("wire", "mont", "mont_flag") and scalars ("wire", "mont") every G1 call of this engine
        reads from now on (msm377_ctx_set_input_format).  Results stay in the wire format.  An unknown value raises
        MsmError(EINVAL) and leaves the forms as they were."""
        pf, sf = _form(_POINT_FORMS, points, "point"), _form(_SCALAR_FORMS, scalars, "scalar")
        self._check(self._lib.msm377_ctx_set_input_format(self._ctx, pf, sf), "msm377_ctx_set_input_format")
        self._point_bytes = _POINT_STRIDE[pf]

    def get_input_format(self) -> Tuple[str, str]:
        pf, sf = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._lib.msm377_ctx_get_input_format(self._ctx, ctypes.byref(pf), ctypes.byref(sf)), "msm377_ctx_get_input_format")
        return {v: k for k, v in _POINT_FORMS.items()}[pf.value], {v: k for k, v in _SCALAR_FORMS.items()}[sf.value]

    def _count_points(self, points: bytes) -> int:
        if len(points) % self._point_bytes:
            raise ValueError("points buffer length must be a multiple of %d" % self._point_bytes)
        return len(points) // self._point_bytes

    # -- G1 MSM --
    def msm(self, points: bytes, scalars: bytes) -> bytes:
        """compute_msm on host buffers (in the active input form); returns x||y (96 bytes)."""
        n = _check_lengths(points, scalars, self._point_bytes)
        out = ctypes.create_string_buffer(96)
        self._check(self._lib.msm377_g1_msm(self._ctx, bytes(points), bytes(scalars), n, ctypes.addressof(out)), "msm377_g1_msm")
        return out.raw

    def msm_device(self, d_points: int, d_scalars: int, n: int) -> bytes:
        """Inputs already in HBM (raw device pointers, wire format)."""
        out = ctypes.create_string_buffer(96)
        self._check(self._lib.msm377_g1_msm_device(self._ctx, d_points, d_scalars, int(n), ctypes.addressof(out)), "msm377_g1_msm_device")
        return out.raw

    # -- short scalars (include/msm377.h): n x scalar_bytes little-endian bytes, every scalar below 2^scalar_bits --
    def msm_short(self, points: bytes, scalars: bytes, scalar_bytes: int, scalar_bits: int) -> bytes:
        """compute_msm on host buffers with compact scalars of a declared width: floor(bits / (L + 1)) + 1 windows
        instead of 16 or 22.  MsmError(ESCALAR) if a scalar is 2^scalar_bits or more."""
        pb = self._point_bytes
        n = len(scalars) // scalar_bytes if scalar_bytes in (4, 8, 16, 32) and len(scalars) % scalar_bytes == 0 else len(points) // pb
        if scalar_bytes in (4, 8, 16, 32) and len(points) != pb * n:
            raise ValueError("points buffer must hold %d bytes (%d per scalar), got %d" % (pb * n, pb, len(points)))
        out = ctypes.create_string_buffer(96)
        self._check(self._lib.msm377_g1_msm_short(self._ctx, bytes(points), bytes(scalars), n, int(scalar_bytes), int(scalar_bits), ctypes.addressof(out)), "msm377_g1_msm_short")
        return out.raw

    def msm_short_device(self, d_points: int, d_scalars: int, n: int, scalar_bytes: int, scalar_bits: int, out=None) -> bytes:
        """The same with inputs in HBM.  ``out``: an optional 96-byte ctypes buffer of the caller's (left untouched on error)."""
        out = ctypes.create_string_buffer(96) if out is None else out
        self._check(
            self._lib.msm377_g1_msm_short_device(self._ctx, d_points, d_scalars, int(n), int(scalar_bytes), int(scalar_bits), ctypes.addressof(out)),
            "msm377_g1_msm_short_device",
        )
        return out.raw

    def msm_fixed_base_short_device(self, d_scalars: int, n: int, scalar_bytes: int, scalar_bits: int) -> bytes:
        """Short scalars against the resident bases of the last set_bases* call (any of them)."""
        out = ctypes.create_string_buffer(96)
        self._check(
            self._lib.msm377_g1_msm_fixed_base_short_device(self._ctx, d_scalars, int(n), int(scalar_bytes), int(scalar_bits), ctypes.addressof(out)),
            "msm377_g1_msm_fixed_base_short_device",
        )
        return out.raw

    def scalars_width_device(self, d_scalars: int, n: int, scalar_bytes: int = 32) -> int:
        """Largest bit length among n scalars in HBM (msm377_scalars_width_device), 0 if all are zero."""
        bits = ctypes.c_uint32()
        self._check(self._lib.msm377_scalars_width_device(self._ctx, d_scalars, int(n), int(scalar_bytes), ctypes.byref(bits)), "msm377_scalars_width_device")
        return int(bits.value)

    def last_geometry(self) -> Tuple[int, int]:
        """(window slots, bucket_log) of the last G1 MSM call's last pass (msm377_ctx_get_last_geometry)."""
        w, log = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._lib.msm377_ctx_get_last_geometry(self._ctx, ctypes.byref(w), ctypes.byref(log)), "msm377_ctx_get_last_geometry")
        return int(w.value), int(log.value)

    def last_sort_elem_bytes(self) -> int:
        """Bytes per element of the sort's intermediate buffer in the last call's last pass: 4 packed, 8, or 0 where the
        two-level sort did not run (msm377_ctx_get_last_sort_elem_bytes)."""
        return int(self._lib.msm377_ctx_get_last_sort_elem_bytes(self._ctx))

    def set_bases(self, points: bytes):
        self._check(self._lib.msm377_g1_set_bases(self._ctx, bytes(points), self._count_points(points)), "msm377_g1_set_bases")

    def set_bases_device(self, d_points: int, n: int):
        self._check(self._lib.msm377_g1_set_bases_device(self._ctx, d_points, int(n)), "msm377_g1_set_bases_device")

    def set_bases_precomputed(self, points: bytes):
        """Resident bases WITH precomputed window multiples [2^(16 w)] P_i (msm377_g1_set_bases_precomputed): one bucket
        reduction and a 16-step tail per fixed-base MSM."""
        self._check(self._lib.msm377_g1_set_bases_precomputed(self._ctx, bytes(points), self._count_points(points)), "msm377_g1_set_bases_precomputed")

    def reserve_host_staging(self):
        """Allocate the pinned staging of the host-buffer entry points now instead of inside the first call
        (msm377_ctx_reserve_host_staging)."""
        self._check(self._lib.msm377_ctx_reserve_host_staging(self._ctx), "msm377_ctx_reserve_host_staging")

    def set_precompute_window(self, window_bits: int):
        """Window width of the next precomputed table: 16 (16 windows) or 20 (13 windows over one set of 2^19 buckets,
        msm377_ctx_set_precompute_window)."""
        self._check(self._lib.msm377_ctx_set_precompute_window(self._ctx, int(window_bits)), "msm377_ctx_set_precompute_window")

    def set_bases_precomputed_device(self, d_points: int, n: int):
        self._check(self._lib.msm377_g1_set_bases_precomputed_device(self._ctx, d_points, int(n)), "msm377_g1_set_bases_precomputed_device")

    def msm_fixed_base(self, scalars: bytes) -> bytes:
        if len(scalars) % 32:
            raise ValueError("scalars buffer length must be a multiple of 32")
        out = ctypes.create_string_buffer(96)
        self._check(self._lib.msm377_g1_msm_fixed_base(self._ctx, bytes(scalars), len(scalars) // 32, ctypes.addressof(out)), "msm377_g1_msm_fixed_base")
        return out.raw

    def msm_fixed_base_device(self, d_scalars: int, n: int) -> bytes:
        out = ctypes.create_string_buffer(96)
        self._check(self._lib.msm377_g1_msm_fixed_base_device(self._ctx, d_scalars, int(n), ctypes.addressof(out)), "msm377_g1_msm_fixed_base_device")
        return out.raw

    def msm_fixed_base_batch_device(self, d_scalars: int, n: int, batch: int) -> List[bytes]:
        """`batch` MSMs of n scalars each (contiguous in HBM) against the resident bases; the host tail
        of one MSM overlaps the GPU work of the next."""
        out = ctypes.create_string_buffer(96 * max(1, batch))
        self._check(
            self._lib.msm377_g1_msm_fixed_base_batch_device(self._ctx, d_scalars, int(n), int(batch), ctypes.addressof(out)),
            "msm377_g1_msm_fixed_base_batch_device",
        )
        return [out.raw[96 * b : 96 * b + 96] for b in range(batch)]

    def window_partials_device(self, d_points: int, d_scalars: int, n: int, win_begin: int, win_count: int) -> bytes:
        """Partial records of windows [win_begin, win_begin + win_count) (multi-GPU sharding)."""
        out = ctypes.create_string_buffer(max(1, win_count) * WINDOW_PARTIAL_BYTES)
        self._check(
            self._lib.msm377_g1_window_partials_device(self._ctx, d_points, d_scalars, int(n), int(win_begin), int(win_count), ctypes.addressof(out)),
            "msm377_g1_window_partials_device",
        )
        return out.raw[: win_count * WINDOW_PARTIAL_BYTES]

    def window_partials_resident(self, d_points: int, d_scalars: int, n: int, win_begin: int, win_count: int, d_partials_out: int):
        """The same records left in DEVICE memory at d_partials_out (win_count x WINDOW_PARTIAL_BYTES): the multi-GPU
        exchange reads them there (msm377_g1_window_partials_resident)."""
        self._check(
            self._lib.msm377_g1_window_partials_resident(self._ctx, d_points, d_scalars, int(n), int(win_begin), int(win_count), d_partials_out),
            "msm377_g1_window_partials_resident",
        )

    def combine_partials(self, partials) -> bytes:
        """Host tail over all 16 windows' records on the context's tail threads (msm377_g1_combine_partials_ctx);
        ``partials`` is bytes or anything with a buffer address of 16 x WINDOW_PARTIAL_BYTES bytes.  Raises
        MsmError(EEXCEPTIONAL) when Edwards records add up to an exceptional case (recompute in form 0)."""
        if isinstance(partials, (bytes, bytearray)):
            if len(partials) != NUM_WINDOWS * WINDOW_PARTIAL_BYTES:
                raise ValueError("expected %d bytes of partials" % (NUM_WINDOWS * WINDOW_PARTIAL_BYTES))
            src = (ctypes.c_uint32 * (len(partials) // 4)).from_buffer_copy(partials)
            addr = ctypes.addressof(src)
        else:
            addr = int(partials)
        out = ctypes.create_string_buffer(96)
        self._check(self._lib.msm377_g1_combine_partials_ctx(self._ctx, addr, ctypes.addressof(out)), "msm377_g1_combine_partials_ctx")
        return out.raw

    def fallback_info(self) -> Tuple[int, int]:
        """(count, last_mask): reruns on the Weierstrass path after an exceptional case of the Edwards law, and the
        FB_* bits of the last one."""
        count, mask = ctypes.c_uint64(), ctypes.c_uint32()
        self._check(self._lib.msm377_ctx_get_fallback_info(self._ctx, ctypes.byref(count), ctypes.byref(mask)), "msm377_ctx_get_fallback_info")
        return int(count.value), int(mask.value)

    def glv_window_partials_device(self, d_points: int, d_scalars: int, n: int, win_begin: int, win_count: int) -> bytes:
        """Same behind the GLV front end (8 windows); raises MsmError(EGLVRANGE) for out-of-range scalars."""
        out = ctypes.create_string_buffer(max(1, win_count) * WINDOW_PARTIAL_BYTES)
        self._check(
            self._lib.msm377_g1_glv_window_partials_device(self._ctx, d_points, d_scalars, int(n), int(win_begin), int(win_count), ctypes.addressof(out)),
            "msm377_g1_glv_window_partials_device",
        )
        return out.raw[: win_count * WINDOW_PARTIAL_BYTES]

    def generate_bases_device(self, seed: int, n: int, d_points_out: int):
        self._check(self._lib.msm377_g1_generate_bases_device(self._ctx, int(seed) & (2**64 - 1), int(n), d_points_out), "msm377_g1_generate_bases_device")

    def _batch_host_call(self, fn: str, n: int, out_form, *args) -> Tuple[bytes, bytes]:
        """One G1 batch call on host buffers: ``fn(ctx, *args, out form, records, flags)`` for n outputs; returns
        (records, identity flags), one flag byte per output."""
        f = _batch_mul_out_form(out_form)
        stride = _POINT_STRIDE.get(f, 96)
        out = ctypes.create_string_buffer(max(1, stride * n))
        inf = ctypes.create_string_buffer(max(1, n))
        self._check(getattr(self._lib, fn)(self._ctx, *args, f, ctypes.addressof(out), ctypes.addressof(inf)), fn)
        return out.raw[: stride * n], inf.raw[:n]

    # -- fixed-base batch multiplication (include/msm377.h): out[i] = [s_i]B, every output its own point --
    def batch_mul_device(self, base: bytes, d_scalars: int, n: int, d_out: int, d_inf: int = 0, out_form="wire"):
        """n scalars in HBM (in the engine's scalar form) times the base ``base`` (96 wire bytes, a host buffer): n
        records at ``d_out`` -- 96-byte wire or 104-byte "mont_flag" -- and, if ``d_inf`` is given, n identity flag bytes
        there (msm377_g1_batch_mul_device).  Any n; every curve point is a legal base."""
        if len(base) != 96:
            raise ValueError("a base is 96 bytes")
        rc = self._lib.msm377_g1_batch_mul_device(self._ctx, bytes(base), d_scalars, int(n), _batch_mul_out_form(out_form), d_out, d_inf or None)
        self._check(rc, "msm377_g1_batch_mul_device")

    def batch_mul(self, base: bytes, scalars: bytes, out_form="wire") -> Tuple[bytes, bytes]:
        """The same on host buffers: returns (records, identity flags), one flag byte per output (msm377_g1_batch_mul)."""
        if len(base) != 96:
            raise ValueError("a base is 96 bytes")
        if len(scalars) % 32:
            raise ValueError("scalars buffer length must be a multiple of 32")
        n = len(scalars) // 32
        return self._batch_host_call("msm377_g1_batch_mul", n, out_form, bytes(base), bytes(scalars), n)

    # -- multi-base batch multiplication (include/msm377.h): out[i] = sum_j [s_ij]B_j over k fixed bases --
    def batch_mul_multi_device(self, bases: bytes, d_scalars: int, n: int, d_out: int, d_inf: int = 0, out_form="wire", out_stride=None, base_stride: int = 32):
        """n rows of k scalars in HBM (in the engine's scalar form) over the k bases ``bases`` (96 wire bytes each, a host
        buffer): n records at ``d_out`` and, if ``d_inf`` is given, n identity flag bytes there
        (msm377_g1_batch_mul_multi_device).  s_ij is at ``d_scalars + i * out_stride + j * base_stride``; the default is
        row-major (``out_stride`` = 32 k).  Any n; every curve point is a legal base, in every relation to the others."""
        if len(bases) % 96:
            raise ValueError("a base is 96 bytes")
        k = len(bases) // 96
        if out_stride is None:
            out_stride = 32 * k
        rc = self._lib.msm377_g1_batch_mul_multi_device(
            self._ctx, bytes(bases), k, d_scalars or None, int(n), int(out_stride), int(base_stride), _batch_mul_out_form(out_form), d_out or None, d_inf or None
        )
        self._check(rc, "msm377_g1_batch_mul_multi_device")

    def batch_mul_multi(self, bases: bytes, scalars: bytes, out_form="wire", layout="rows") -> Tuple[bytes, bytes]:
        """The same on host buffers, ``scalars`` the dense k x n matrix in ``layout`` ("rows" or "columns"): returns
        (records, identity flags) (msm377_g1_batch_mul_multi)."""
        k, n, out_stride, base_stride = _multi_shape(bases, scalars, layout)
        return self._batch_host_call("msm377_g1_batch_mul_multi", n, out_form, bytes(bases), k, bytes(scalars), n, out_stride, base_stride)

    def mul_multi_table_builds(self) -> int:
        """Table slots batch_mul_multi* built on this engine so far (msm377_ctx_get_mul_multi_table_builds)."""
        return int(self._lib.msm377_ctx_get_mul_multi_table_builds(self._ctx))

    # -- row commitments (include/msm377.h): out[i] = sum_j [s_ij]G_j over a resident generator set --
    def set_generators(self, gens, window_bits: int = 0):
        """Build and keep the window tables of the generators ``gens`` (96 wire bytes each, a host buffer, up to 4 096; up
        to 64 with ``window_bits`` 16).  ``None`` or an empty buffer drops the set and frees its memory.  The old set is
        dropped first; a call that fails leaves none (msm377_g1_set_generators)."""
        gens = bytes(gens) if gens else b""
        if len(gens) % 96:
            raise ValueError("a generator is 96 bytes")
        rc = self._lib.msm377_g1_set_generators(self._ctx, gens or None, len(gens) // 96, int(window_bits))
        self._check(rc, "msm377_g1_set_generators")

    def generators(self) -> Tuple[int, int]:
        """(k, window width) of the resident generator set, (0, 0) without one (msm377_ctx_get_generators)."""
        k, c = ctypes.c_uint32(), ctypes.c_int()
        self._check(self._lib.msm377_ctx_get_generators(self._ctx, ctypes.addressof(k), ctypes.addressof(c)), "msm377_ctx_get_generators")
        return k.value, c.value

    def commit_rows_device(self, d_scalars: int, n: int, k: int, d_out: int, d_inf: int = 0, out_form="wire", out_stride=None, base_stride: int = 32):
        """n rows of k scalars in HBM (in the engine's scalar form) over the first k generators of the resident set: n
        records at ``d_out`` and, if ``d_inf`` is given, n identity flag bytes there (msm377_g1_commit_rows_device).  s_ij
        is at ``d_scalars + i * out_stride + j * base_stride``; the default is row-major (``out_stride`` = 32 k)."""
        if out_stride is None:
            out_stride = 32 * k
        rc = self._lib.msm377_g1_commit_rows_device(
            self._ctx, d_scalars or None, int(n), int(k), int(out_stride), int(base_stride), _batch_mul_out_form(out_form), d_out or None, d_inf or None
        )
        self._check(rc, "msm377_g1_commit_rows_device")

    def commit_rows(self, scalars: bytes, k: int, out_form="wire", layout="rows") -> Tuple[bytes, bytes]:
        """The same on host buffers, ``scalars`` the dense k x n matrix in ``layout`` ("rows" or "columns"): returns
        (records, identity flags) (msm377_g1_commit_rows)."""
        n, out_stride, base_stride = _rows_shape(k, scalars, layout)
        return self._batch_host_call("msm377_g1_commit_rows", n, out_form, bytes(scalars), n, int(k), out_stride, base_stride)

    # -- variable-base batch multiplication (include/msm377.h): out[i] = [s_i]P_i --
    def batch_mul_var_device(self, d_points: int, d_scalars: int, n: int, d_out: int, d_inf: int = 0, out_form="wire", scalar_stride: int = 32):
        """n points and n scalars in HBM (in the engine's point and scalar forms; ``scalar_stride`` 0: one scalar for all
        points): n records at ``d_out`` and, if ``d_inf`` is given, n identity flag bytes there
        (msm377_g1_batch_mul_var_device).  Any n; every curve point is a legal input; ``d_out`` may be ``d_points`` when
        the records have the same size."""
        rc = self._lib.msm377_g1_batch_mul_var_device(self._ctx, d_points or None, d_scalars or None, int(n), int(scalar_stride), _batch_mul_out_form(out_form), d_out or None, d_inf or None)
        self._check(rc, "msm377_g1_batch_mul_var_device")

    def batch_mul_var(self, points: bytes, scalars: bytes, out_form="wire") -> Tuple[bytes, bytes]:
        """The same on host buffers: returns (records, identity flags).  A 32-byte ``scalars`` with more than one point
        is the one scalar of all points (msm377_g1_batch_mul_var)."""
        n = self._count_points(points)
        return self._batch_host_call("msm377_g1_batch_mul_var", n, out_form, bytes(points), bytes(scalars), n, _var_scalar_stride(scalars, n))

    # -- pairwise linear combination (include/msm377.h): out[i] = [a_i]P_i + [b_i]Q_i --
    def batch_lincomb2_device(self, d_p: int, d_q: int, d_a: int, d_b: int, n: int, d_out: int, d_inf: int = 0, out_form="wire", a_stride: int = 32, b_stride: int = 32):
        """n pairs of points and of scalars in HBM (in the engine's point and scalar forms; ``a_stride`` / ``b_stride`` 0:
        one scalar for all pairs): n records at ``d_out`` and, if ``d_inf`` is given, n identity flag bytes there
        (msm377_g1_batch_lincomb2_device).  Any n; every curve point is a legal input and every relation between the two
        arrays; ``d_out`` may be ``d_p`` or ``d_q`` when the records have the same size."""
        rc = self._lib.msm377_g1_batch_lincomb2_device(
            self._ctx, d_p or None, d_q or None, d_a or None, d_b or None, int(n), int(a_stride), int(b_stride), _batch_mul_out_form(out_form), d_out or None, d_inf or None
        )
        self._check(rc, "msm377_g1_batch_lincomb2_device")

    def batch_lincomb2(self, p: bytes, q: bytes, a: bytes, b: bytes, out_form="wire") -> Tuple[bytes, bytes]:
        """The same on host buffers: returns (records, identity flags).  A 32-byte ``a`` or ``b`` with more than one pair
        is the one scalar of all pairs (msm377_g1_batch_lincomb2)."""
        n = self._count_points(p)
        if len(q) != len(p):
            raise ValueError("p and q: the same number of records")
        return self._batch_host_call("msm377_g1_batch_lincomb2", n, out_form, bytes(p), bytes(q), bytes(a), bytes(b), n, _var_scalar_stride(a, n), _var_scalar_stride(b, n))

    def set_mul_window(self, bits: int = 0):
        """Window width of the batch_mul calls' table: 8 or 16, 0 = by the number of outputs (the default;
        msm377_ctx_set_mul_window)."""
        self._check(self._lib.msm377_ctx_set_mul_window(self._ctx, int(bits)), "msm377_ctx_set_mul_window")

    def last_mul_window(self) -> int:
        """Width the last batch_mul call ran, 0 before the first (msm377_ctx_get_last_mul_window)."""
        return int(self._lib.msm377_ctx_get_last_mul_window(self._ctx))

    def mul_table_builds(self) -> int:
        """Window tables this engine has built so far: a repeated (base, width) builds none
        (msm377_ctx_get_mul_table_builds)."""
        return int(self._lib.msm377_ctx_get_mul_table_builds(self._ctx))

    # -- input validation (include/msm377.h): the verdict is the report, a finding is not an error --
    def _check_points(self, fn: str, points, n: int, flags: int) -> CheckReport:
        rep = _CheckReportStruct()
        self._check(getattr(self._lib, fn)(self._ctx, points, int(n), int(flags), ctypes.addressof(rep)), fn)
        return _report(rep)

    def check_points(self, points: bytes, flags: int = CHECK_ALL) -> CheckReport:
        """Report on G1 points (in the active point form) in a host buffer, computed on the GPU; the resident bases
        survive the call."""
        return self._check_points("msm377_g1_check_points", bytes(points), self._count_points(points), flags)

    def check_points_device(self, d_points: int, n: int, flags: int = CHECK_ALL) -> CheckReport:
        return self._check_points("msm377_g1_check_points_device", d_points, n, flags)

    def ed_check_points(self, points: bytes, flags: int = CHECK_ALL) -> CheckReport:
        if len(points) % 64:
            raise ValueError("Edwards points buffer length must be a multiple of 64")
        return self._check_points("msm377_ed_check_points", bytes(points), len(points) // 64, flags)

    def ed_check_points_device(self, d_points: int, n: int, flags: int = CHECK_ALL) -> CheckReport:
        return self._check_points("msm377_ed_check_points_device", d_points, n, flags)

    def set_base_checks(self, flags: int = CHECK_ALL):
        """Opt-in: the set_bases* calls check a base set with these flags before they convert it and raise
        MsmError(EPOINT) on a finding, leaving no resident bases (msm377_ctx_set_base_checks; 0 = off, the default)."""
        self._check(self._lib.msm377_ctx_set_base_checks(self._ctx, int(flags)), "msm377_ctx_set_base_checks")

    def last_check(self) -> CheckReport:
        """The report of the last check a set_bases* call ran (msm377_ctx_get_last_check)."""
        rep = _CheckReportStruct()
        self._check(self._lib.msm377_ctx_get_last_check(self._ctx, ctypes.addressof(rep)), "msm377_ctx_get_last_check")
        return _report(rep)

    # -- Twisted-Edwards BLS12 (BASELINE.json config 3): 64-byte points, 64-byte result --
    def ed_msm(self, points: bytes, scalars: bytes) -> bytes:
        if len(scalars) % 32 or len(points) != 2 * len(scalars):
            raise ValueError("Edwards points buffer must hold 64 bytes and scalars 32 bytes per input")
        out = ctypes.create_string_buffer(64)
        self._check(self._lib.msm377_ed_msm(self._ctx, bytes(points), bytes(scalars), len(scalars) // 32, ctypes.addressof(out)), "msm377_ed_msm")
        return out.raw

    def ed_msm_device(self, d_points: int, d_scalars: int, n: int) -> bytes:
        out = ctypes.create_string_buffer(64)
        self._check(self._lib.msm377_ed_msm_device(self._ctx, d_points, d_scalars, int(n), ctypes.addressof(out)), "msm377_ed_msm_device")
        return out.raw

    def ed_generate_bases_device(self, seed: int, n: int, d_points_out: int):
        self._check(self._lib.msm377_ed_generate_bases_device(self._ctx, int(seed) & (2**64 - 1), int(n), d_points_out), "msm377_ed_generate_bases_device")

    # -- Edwards-BLS12 batch multiplication (include/msm377.h): out[i] = sum_j [s_ij]B_j, 64-byte wire outputs --
    def ed_batch_mul_multi_device(self, bases: bytes, d_scalars: int, n: int, d_out: int, out_stride=None, base_stride: int = 32):
        """n rows of k scalars in HBM over the k Edwards-BLS12 bases ``bases`` (64 wire bytes each, a host buffer): n
        64-byte wire records at ``d_out`` (msm377_ed_batch_mul_multi_device).  s_ij is at ``d_scalars + i * out_stride + j *
        base_stride``; the default is row-major.  Any n; every curve point is a legal base, in every relation to the others."""
        if len(bases) % 64:
            raise ValueError("an Edwards base is 64 bytes")
        k = len(bases) // 64
        if out_stride is None:
            out_stride = 32 * k
        rc = self._lib.msm377_ed_batch_mul_multi_device(self._ctx, bytes(bases), k, d_scalars or None, int(n), int(out_stride), int(base_stride), d_out or None)
        self._check(rc, "msm377_ed_batch_mul_multi_device")

    def ed_batch_mul_multi(self, bases: bytes, scalars: bytes, layout="rows") -> bytes:
        """The same on host buffers, ``scalars`` the dense k x n matrix in ``layout`` ("rows" or "columns"): returns the n
        records (msm377_ed_batch_mul_multi)."""
        k, n, out_stride, base_stride = _ed_multi_shape(bases, scalars, layout)
        out = ctypes.create_string_buffer(max(1, 64 * n))
        rc = self._lib.msm377_ed_batch_mul_multi(self._ctx, bytes(bases), k, bytes(scalars), n, out_stride, base_stride, ctypes.addressof(out))
        self._check(rc, "msm377_ed_batch_mul_multi")
        return out.raw[: 64 * n]

    def ed_batch_mul_var_device(self, d_points: int, d_scalars: int, n: int, d_out: int, scalar_stride: int = 32):
        """out[i] = [s_i]P_i on Edwards-BLS12 for n 64-byte wire points at ``d_points`` and their scalars at ``d_scalars``
        (``scalar_stride`` 0: ONE 32-byte scalar for all), as 64-byte wire records at ``d_out``
        (msm377_ed_batch_mul_var_device).  Any n; every curve point is a legal input; ``d_out`` may be ``d_points``.  A
        point that is not on the curve raises MsmError(EPOINT) with its ``index``, the outputs untouched."""
        rc = self._lib.msm377_ed_batch_mul_var_device(self._ctx, d_points or None, d_scalars or None, int(n), int(scalar_stride), d_out or None)
        self._check(rc, "msm377_ed_batch_mul_var_device")

    def ed_batch_mul_var(self, points: bytes, scalars: bytes) -> bytes:
        """Host-buffer form: returns n 64-byte wire records.  A 32-byte ``scalars`` with n > 1 points is the one scalar of
        all points (msm377_ed_batch_mul_var)."""
        n, stride = _ed_var_shape(points, scalars)
        out = ctypes.create_string_buffer(max(1, 64 * n))
        rc = self._lib.msm377_ed_batch_mul_var(self._ctx, bytes(points), bytes(scalars), n, stride, ctypes.addressof(out))
        self._check(rc, "msm377_ed_batch_mul_var")
        return out.raw[: 64 * n]

    def ed_batch_lincomb2_device(self, d_p: int, d_q: int, d_a: int, d_b: int, n: int, d_out: int, p_stride: int = 64, q_stride: int = 64, a_stride: int = 32, b_stride: int = 32):
        """out[i] = [a_i]P_i + [b_i]Q_i on Edwards-BLS12 for n pairs of 64-byte wire points at ``d_p`` / ``d_q`` and their
        scalars at ``d_a`` / ``d_b``, as 64-byte wire records at ``d_out`` (msm377_ed_batch_lincomb2_device).  A stride of 0
        is ONE point or ONE scalar for all pairs (``p_stride`` 0: the Schnorr shape [s_i]G + [c_i]PK_i).  Every curve point
        is a legal input; ``d_out`` may be ``d_p`` or ``d_q`` where that array's stride is 64.  A point that is not on the
        curve raises MsmError(EPOINT) with its ``array`` and ``index``, the outputs untouched."""
        rc = self._lib.msm377_ed_batch_lincomb2_device(
            self._ctx, d_p or None, d_q or None, d_a or None, d_b or None, int(n), int(p_stride), int(q_stride), int(a_stride), int(b_stride), d_out or None
        )
        self._check(rc, "msm377_ed_batch_lincomb2_device")

    def ed_batch_lincomb2(self, p: bytes, q: bytes, a: bytes, b: bytes) -> bytes:
        """Host-buffer form: returns n 64-byte wire records, n the largest element count of the four arguments.  An
        argument of exactly one element with n > 1 is the one point or scalar of all pairs (msm377_ed_batch_lincomb2)."""
        n, ps, qs, sa, sb = _ed_lincomb2_shape(p, q, a, b)
        out = ctypes.create_string_buffer(max(1, 64 * n))
        rc = self._lib.msm377_ed_batch_lincomb2(self._ctx, bytes(p), bytes(q), bytes(a), bytes(b), n, ps, qs, sa, sb, ctypes.addressof(out))
        self._check(rc, "msm377_ed_batch_lincomb2")
        return out.raw[: 64 * n]

    def ed_batch_lincomb_device(self, terms, n: int, d_out: int):
        """out[i] = sum_j [s_ij]P_ij on Edwards-BLS12 for n outputs, as 64-byte wire records at ``d_out``
        (msm377_ed_batch_lincomb_device).  ``terms``: 1 to 8 tuples ``(d_points, d_scalars, point_stride, scalar_stride)`` of
        device pointers, ``point_stride`` 64 or 0 (ONE point for all outputs), ``scalar_stride`` 32 or 0 (ONE scalar).  Every
        curve point is a legal input in every term; ``d_out`` may be the points of any term of stride 64.  A point that is
        not on the curve raises MsmError(EPOINT) with its ``term`` and ``index``, the outputs untouched."""
        rc = self._lib.msm377_ed_batch_lincomb_device(self._ctx, _lincomb_terms(terms), len(terms), int(n), d_out or None)
        self._check(rc, "msm377_ed_batch_lincomb_device")

    def ed_batch_lincomb(self, points_list, scalars_list) -> bytes:
        """Host-buffer form: returns n 64-byte wire records, n the largest element count of all buffers.  A buffer of
        exactly one element with n > 1 is the one point or scalar of all outputs (msm377_ed_batch_lincomb)."""
        n, strides = _ed_lincomb_shape(points_list, scalars_list)
        terms, keep = _lincomb_host_terms(points_list, scalars_list, strides)
        out = ctypes.create_string_buffer(max(1, 64 * n))
        rc = self._lib.msm377_ed_batch_lincomb(self._ctx, terms, len(points_list), n, ctypes.addressof(out))
        del keep
        self._check(rc, "msm377_ed_batch_lincomb")
        return out.raw[: 64 * n]

    # -- Edwards-BLS12 row commitments (include/msm377.h): out[i] = sum_j [s_ij]G_j over that curve's resident set --
    def ed_set_generators(self, gens, window_bits: int = 0):
        """Build and keep the window tables of the Edwards-BLS12 generators ``gens`` (64 wire bytes each, a host buffer, up
        to 4 096; up to 64 with ``window_bits`` 16).  ``None`` or an empty buffer drops the set and frees its memory.  The
        old set is dropped first; a call that fails leaves none.  A generator that is not on the curve raises
        MsmError(EPOINT) with its ``index`` (msm377_ed_set_generators).  Independent of the G1 set."""
        gens = bytes(gens) if gens else b""
        if len(gens) % 64:
            raise ValueError("an Edwards-BLS12 generator is 64 bytes")
        rc = self._lib.msm377_ed_set_generators(self._ctx, gens or None, len(gens) // 64, int(window_bits))
        self._check(rc, "msm377_ed_set_generators")

    def ed_generators(self) -> Tuple[int, int]:
        """(k, window width) of the resident Edwards-BLS12 generator set, (0, 0) without one (msm377_ed_ctx_get_generators)."""
        k, c = ctypes.c_uint32(), ctypes.c_int()
        self._check(self._lib.msm377_ed_ctx_get_generators(self._ctx, ctypes.addressof(k), ctypes.addressof(c)), "msm377_ed_ctx_get_generators")
        return k.value, c.value

    def ed_commit_rows_device(self, d_scalars: int, n: int, k: int, d_out: int, out_stride=None, base_stride: int = 32):
        """n rows of k scalars in HBM over the first k generators of the resident Edwards-BLS12 set: n 64-byte wire records
        at ``d_out`` (msm377_ed_commit_rows_device).  s_ij is at ``d_scalars + i * out_stride + j * base_stride``; the
        default is row-major (``out_stride`` = 32 k)."""
        if out_stride is None:
            out_stride = 32 * k
        rc = self._lib.msm377_ed_commit_rows_device(self._ctx, d_scalars or None, int(n), int(k), int(out_stride), int(base_stride), d_out or None)
        self._check(rc, "msm377_ed_commit_rows_device")

    def ed_commit_rows(self, scalars: bytes, k: int, layout="rows") -> bytes:
        """The same on host buffers, ``scalars`` the dense k x n matrix in ``layout`` ("rows" or "columns"): returns the n
        records (msm377_ed_commit_rows)."""
        n, out_stride, base_stride = _rows_shape(k, scalars, layout)
        out = ctypes.create_string_buffer(max(1, 64 * n))
        rc = self._lib.msm377_ed_commit_rows(self._ctx, bytes(scalars), n, int(k), out_stride, base_stride, ctypes.addressof(out))
        self._check(rc, "msm377_ed_commit_rows")
        return out.raw[: 64 * n]

    def ed_read_generator_table(self, index: int = 0, first: int = 0, count=None, info_only: bool = False):
        """(MulTableInfo, records) of generator ``index`` of the resident Edwards-BLS12 set (msm377_ed_read_generator_table):
        records as ed_read_mul_table's, the key zero.  MsmError(ESTATE) without a set or for an index beyond it."""
        import numpy as np

        fn = self._lib.msm377_ed_read_generator_table
        raw = _MulTableInfoStruct()
        self._check(fn(self._ctx, int(index), ctypes.addressof(raw), 0, 0, None), "msm377_ed_read_generator_table")
        info = MulTableInfo(int(raw.width), int(raw.rows), int(raw.records), bytes(raw.key))
        if info_only:
            return info, None
        count = info.records - int(first) if count is None else int(count)
        words = np.empty((count, MUL_TABLE_RECORD_WORDS), dtype=np.uint32)
        self._check(fn(self._ctx, int(index), None, int(first), count, words.ctypes.data if count else None), "msm377_ed_read_generator_table")
        return info, words

    def ed_batch_mul(self, base: bytes, scalars: bytes) -> bytes:
        """out[i] = [s_i]B for one Edwards-BLS12 base: ed_batch_mul_multi with k = 1."""
        return self.ed_batch_mul_multi(base, scalars)

    def ed_mul_table_builds(self) -> int:
        """Table slots the Edwards-BLS12 batch calls built on this engine so far (msm377_ed_ctx_get_mul_table_builds)."""
        return int(self._lib.msm377_ed_ctx_get_mul_table_builds(self._ctx))

    def ed_read_mul_table(self, index: int = 0, first: int = 0, count=None, info_only: bool = False):
        """(MulTableInfo, records) of slot ``index`` of the Edwards-BLS12 batch calls (msm377_ed_read_mul_table): records
        are 32 u32 each -- (y - x)[9], (y + x)[9], (2dxy)[9], 5 pad; the key is the 64 base bytes, then zeros.
        MsmError(ESTATE) when the slot is not valid."""
        import numpy as np

        raw = _MulTableInfoStruct()
        self._check(self._lib.msm377_ed_read_mul_table(self._ctx, int(index), ctypes.addressof(raw), 0, 0, None), "msm377_ed_read_mul_table")
        info = MulTableInfo(int(raw.width), int(raw.rows), int(raw.records), bytes(raw.key))
        if info_only:
            return info, None
        count = info.records - int(first) if count is None else int(count)
        words = np.empty((count, MUL_TABLE_RECORD_WORDS), dtype=np.uint32)
        self._check(self._lib.msm377_ed_read_mul_table(self._ctx, int(index), None, int(first), count, words.ctypes.data if count else None), "msm377_ed_read_mul_table")
        return info, words

    # -- stage access (the reference's debug=true read-backs) --
    def set_stage_capture(self, mode=True):
        """Stage capture mode (msm377_ctx_set_stage_capture): False / 0 off, True / 1 the sixteen-equal-windows route that
        read_stage describes, 2 as run -- the call keeps its own route and read_stage_ex describes its last pass."""
        self._check(self._lib.msm377_ctx_set_stage_capture(self._ctx, int(mode)), "msm377_ctx_set_stage_capture")

    def read_stage_ex(self, slot: int, want=("digits", "row_ptr", "val_idx", "buckets")):
        """(StageInfo, dict of numpy arrays) for window slot ``slot`` of the last call's last pass, at the sizes the
        library reports (msm377_g1_read_stage_ex): a G1 call, or under mode 2 an Edwards-BLS12 call (form STAGE_FORM_ED,
        buckets of 36 words: X, Y, T, Z of 9 limbs).  MsmError(ESTATE) when nothing describable was captured."""
        import numpy as np

        raw = _StageInfoStruct()
        self._check(self._lib.msm377_g1_read_stage_ex(self._ctx, int(slot), ctypes.addressof(raw), None, None, None, None), "msm377_g1_read_stage_ex")
        w = int(raw.slots)
        info = StageInfo(w, int(raw.bucket_log), int(raw.columns), int(raw.digit_bytes), int(raw.row_ptr_len), int(raw.bucket_records), int(raw.form),
                         int(raw.table_stride), int(raw.geometry_reruns), tuple(raw.bias[:w]), tuple(raw.key_unsigned[:w]), tuple(raw.key_max[:w]))
        bufs = {
            "digits": np.empty(info.columns, dtype=np.uint32 if info.digit_bytes == 4 else np.uint16),
            "row_ptr": np.empty(info.row_ptr_len, dtype=np.uint32),
            "val_idx": np.empty(info.columns, dtype=np.uint32),
            "buckets": np.empty((info.bucket_records, ED_POINT_WORDS if info.form == STAGE_FORM_ED else POINT_WORDS), dtype=np.uint32),
        }
        res = {k: v for k, v in bufs.items() if k in want}
        if res:
            ptr = [res[k].ctypes.data if k in res else None for k in ("digits", "row_ptr", "val_idx", "buckets")]
            self._check(self._lib.msm377_g1_read_stage_ex(self._ctx, int(slot), None, *ptr), "msm377_g1_read_stage_ex")
        return info, res

    def read_partials(self, info_only: bool = False):
        """(PartialsInfo, records) of the window records the last call's last pass handed to the host tail
        (msm377_g1_read_partials): a numpy array of shape (records, points, 4, coord_words) u32, or None with
        ``info_only``.  Points beyond ``planes`` are unspecified.  MsmError(ESTATE) wherever read_stage_ex refuses."""
        import numpy as np

        raw = _PartialsInfoStruct()
        self._check(self._lib.msm377_g1_read_partials(self._ctx, ctypes.addressof(raw), None), "msm377_g1_read_partials")
        info = PartialsInfo(*(int(getattr(raw, f)) for f in PartialsInfo._fields))
        if info_only:
            return info, None
        words = np.empty((info.records, info.points, 4, info.coord_words), dtype=np.uint32)
        self._check(self._lib.msm377_g1_read_partials(self._ctx, None, words.ctypes.data), "msm377_g1_read_partials")
        return info, words

    def read_work_list(self, want=("items", "split_rows", "row_ovf_base"), ovf_first: int = 0, ovf_count: int = 0):
        """(WorkListInfo, dict of numpy arrays) of the accumulation work list the last call's last pass left
        (msm377_g1_read_work_list): ``items`` (info.items, 2) u32 (row, seg) in list order, ``split_rows``
        (info.split_rows,), ``row_ovf_base`` (info.rows,) with WORK_ROW_FOLDED on folded rows, and -- with ``ovf_count``
        -- ``ovf``: overflow records [ovf_first, ovf_first + ovf_count) of info.record_words words in the layout of a
        bucket of read_stage_ex.  MsmError(ESTATE) wherever read_stage_ex refuses, and after a check call."""
        import numpy as np

        raw = _WorkListInfoStruct()
        self._check(self._lib.msm377_g1_read_work_list(self._ctx, ctypes.addressof(raw), None, None, None, 0, 0, None), "msm377_g1_read_work_list")
        info = WorkListInfo(*(int(getattr(raw, f)) for f in WorkListInfo._fields[:-1]), tuple(raw.hist))
        bufs = {
            "items": np.empty((info.items, 2), dtype=np.uint32),
            "split_rows": np.empty(info.split_rows, dtype=np.uint32),
            "row_ovf_base": np.empty(info.rows, dtype=np.uint32),
        }
        res = {k: v for k, v in bufs.items() if k in want}
        ovf = np.empty((int(ovf_count), info.record_words), dtype=np.uint32) if ovf_count else None
        if res or ovf is not None:
            ptr = [res[k].ctypes.data if k in res and res[k].size else None for k in ("items", "split_rows", "row_ovf_base")]
            self._check(self._lib.msm377_g1_read_work_list(self._ctx, None, *ptr, int(ovf_first), int(ovf_count), ovf.ctypes.data if ovf is not None else None),
                        "msm377_g1_read_work_list")
        if ovf is not None:
            res["ovf"] = ovf
        return info, res

    def read_stage(self, slot: int, n: int, want=("digits", "row_ptr", "val_idx", "buckets")):
        """Returns a dict of numpy arrays for window slot ``slot`` of the last call."""
        import numpy as np

        res = {}
        digits = np.empty(n, dtype=np.uint16) if "digits" in want else None
        row_ptr = np.empty(NUM_BUCKETS + 2, dtype=np.uint32) if "row_ptr" in want else None
        val_idx = np.empty(n, dtype=np.uint32) if "val_idx" in want else None
        buckets = np.empty((NUM_BUCKETS, POINT_WORDS), dtype=np.uint32) if "buckets" in want else None

        def ptr(a):
            return a.ctypes.data if a is not None else None

        self._check(self._lib.msm377_g1_read_stage(self._ctx, int(slot), ptr(digits), ptr(row_ptr), ptr(val_idx), ptr(buckets)), "msm377_g1_read_stage")
        for k, v in (("digits", digits), ("row_ptr", row_ptr), ("val_idx", val_idx), ("buckets", buckets)):
            if v is not None:
                res[k] = v
        return res

    def read_bases(self, first: int = 0, count=None, info_only: bool = False):
        """(BasesInfo, records) of the base records the last conversion of this engine left (msm377_g1_read_bases): a
        numpy array of ``count`` x record_words u32 starting at record ``first`` (default: all of them), or None with
        ``info_only``.  Records of a precomputed table are window-major, w * window_stride + i.  MsmError(ESTATE) before
        the first conversion and after one that failed."""
        import numpy as np

        raw = _BasesInfoStruct()
        self._check(self._lib.msm377_g1_read_bases(self._ctx, ctypes.addressof(raw), 0, 0, None), "msm377_g1_read_bases")
        bits = tuple(raw.window_bits[: raw.windows]) if raw.windows > 1 else ()
        info = BasesInfo(int(raw.form), int(raw.record_words), int(raw.limbs), int(raw.coords), int(raw.n), int(raw.windows), int(raw.glv), int(raw.window_stride),
                         int(raw.records), int(raw.flagged), bits)
        if info_only:
            return info, None
        count = info.records - int(first) if count is None else int(count)
        words = np.empty((count, info.record_words), dtype=np.uint32)
        self._check(self._lib.msm377_g1_read_bases(self._ctx, None, int(first), count, words.ctypes.data if count else None), "msm377_g1_read_bases")
        return info, words

    def read_mul_table(self, which="single", index: int = 0, first: int = 0, count=None, info_only: bool = False):
        """(MulTableInfo, records) of a window table of the batch operations (msm377_g1_read_mul_table): ``which`` is
        "single" (batch_mul*), "multi" (slot ``index`` of batch_mul_multi*) or "generator" (generator ``index`` of the
        resident set); records are 32 u32 each -- x[13], y[13], identity flag, 5 pad.  MsmError(ESTATE) when that table is
        not valid."""
        import numpy as np

        w = _MUL_TABLES.get(which, which)
        raw = _MulTableInfoStruct()
        self._check(self._lib.msm377_g1_read_mul_table(self._ctx, int(w), int(index), ctypes.addressof(raw), 0, 0, None), "msm377_g1_read_mul_table")
        info = MulTableInfo(int(raw.width), int(raw.rows), int(raw.records), bytes(raw.key))
        if info_only:
            return info, None
        count = info.records - int(first) if count is None else int(count)
        words = np.empty((count, MUL_TABLE_RECORD_WORDS), dtype=np.uint32)
        self._check(self._lib.msm377_g1_read_mul_table(self._ctx, int(w), int(index), None, int(first), count, words.ctypes.data if count else None), "msm377_g1_read_mul_table")
        return info, words

    def read_walk_stash(self, segment: int = 0, first: int = 0, count=None, products: bool = True, info_only: bool = False):
        """(WalkStashInfo, points, running products) of what the last pass of the last batch call left in the stash
        (msm377_read_walk_stash): ``points`` is count x point_words u32 (X, Y, ZZ, ZZZ of 13 limbs, or X, Y, T, Z of 9),
        ``products`` count x (product_words + product_pad) u32 (the limbs, then the zero pad words of the last piece), or
        None without ``products`` and for a segment above 0 of a row commitment.  Default: all m points of the pass.  MsmError(ESTATE) when no completed pass is described."""
        import numpy as np

        raw = _WalkStashInfoStruct()
        self._check(self._lib.msm377_read_walk_stash(self._ctx, ctypes.addressof(raw), 0, 0, 0, None, None), "msm377_read_walk_stash")
        info = WalkStashInfo(*(int(getattr(raw, f)) for f in WalkStashInfo._fields))
        if info_only:
            return info, None, None
        count = info.m - int(first) if count is None else int(count)
        pts = np.empty((count, info.point_words), dtype=np.uint32)
        prod = np.empty((count, info.product_words + info.product_pad), dtype=np.uint32) if products and int(segment) == 0 else None
        rc = self._lib.msm377_read_walk_stash(self._ctx, None, int(segment), int(first), count, pts.ctypes.data if count else None,
                                              prod.ctypes.data if prod is not None and count else None)
        self._check(rc, "msm377_read_walk_stash")
        return info, pts, prod

    def read_walk_tables(self, table: int = 0, first: int = 0, count=None, info_only: bool = False):
        """(WalkTablesInfo, records) of the per-point tables [1..8]P_i the last pass of a variable-base or pairwise call
        walked (msm377_g1_read_walk_tables): ``records`` has shape (entries, count, 32) u32, entry e of point first + j at
        [e - 1, j].  MsmError(ESTATE) unless the last batch call was one of the two and completed."""
        import numpy as np

        raw = _WalkTablesInfoStruct()
        self._check(self._lib.msm377_g1_read_walk_tables(self._ctx, ctypes.addressof(raw), 0, 0, 0, None), "msm377_g1_read_walk_tables")
        info = WalkTablesInfo(int(raw.m), int(raw.tables), int(raw.entries))
        if info_only:
            return info, None
        count = info.m - int(first) if count is None else int(count)
        words = np.empty((info.entries, count, MUL_TABLE_RECORD_WORDS), dtype=np.uint32)
        self._check(self._lib.msm377_g1_read_walk_tables(self._ctx, None, int(table), int(first), count, words.ctypes.data if count else None), "msm377_g1_read_walk_tables")
        return info, words

    def ed_read_walk_tables(self, first: int = 0, count=None, info_only: bool = False):
        """(WalkTablesInfo, records) of the per-point tables [1..8]P_i the last pass of ed_batch_mul_var* walked
        (msm377_ed_read_walk_tables): ``records`` has shape (entries, count, 32) u32 in the MSM377_BASES_ED layout, entry e
        of point first + j at [e - 1, j].  MsmError(ESTATE) unless the last batch call was that one and completed."""
        import numpy as np

        raw = _WalkTablesInfoStruct()
        self._check(self._lib.msm377_ed_read_walk_tables(self._ctx, ctypes.addressof(raw), 0, 0, None), "msm377_ed_read_walk_tables")
        info = WalkTablesInfo(int(raw.m), int(raw.tables), int(raw.entries))
        if info_only:
            return info, None
        count = info.m - int(first) if count is None else int(count)
        words = np.empty((info.entries, count, MUL_TABLE_RECORD_WORDS), dtype=np.uint32)
        self._check(self._lib.msm377_ed_read_walk_tables(self._ctx, None, int(first), count, words.ctypes.data if count else None), "msm377_ed_read_walk_tables")
        return info, words

    def ed_read_walk_table(self, table: int = 0, first: int = 0, count=None, info_only: bool = False):
        """(WalkTablesInfo, records) of table ``table`` of the last pass of ed_batch_lincomb2* (0: [1..8]P_i, 1: [1..8]Q_i;
        info.tables = 2), of ed_batch_lincomb* (table t of term t; info.tables = k) or of ed_batch_mul_var* (table 0 only),
        records as ed_read_walk_tables returns them (msm377_ed_read_walk_table).  MsmError(ESTATE) unless the last batch
        call was one of the three and completed."""
        import numpy as np

        raw = _WalkTablesInfoStruct()
        self._check(self._lib.msm377_ed_read_walk_table(self._ctx, ctypes.addressof(raw), 0, 0, 0, None), "msm377_ed_read_walk_table")
        info = WalkTablesInfo(int(raw.m), int(raw.tables), int(raw.entries))
        if info_only:
            return info, None
        count = info.m - int(first) if count is None else int(count)
        words = np.empty((info.entries, count, MUL_TABLE_RECORD_WORDS), dtype=np.uint32)
        self._check(self._lib.msm377_ed_read_walk_table(self._ctx, None, int(table), int(first), count, words.ctypes.data if count else None), "msm377_ed_read_walk_table")
        return info, words

    def stage_form(self) -> int:
        """Coordinate system of the captured buckets: 0 = Weierstrass XYZZ, 1 = twisted Edwards (X, Y, T, Z), -1 = none."""
        return int(self._lib.msm377_ctx_get_stage_form(self._ctx))

    def set_narrow_max(self, max_points: int = 1 << 16):
        """Inputs of at most this many points run with narrow windows of 2^11 buckets (msm377_ctx_set_narrow_max; 0 = never)."""
        self._check(self._lib.msm377_ctx_set_narrow_max(self._ctx, int(max_points)), "msm377_ctx_set_narrow_max")

    def set_g1_form(self, form="edwards"):
        """Internal coordinates of the G1 full-MSM entry points: "edwards" / 1 (default, csrc/te377.hpp) or
        "weierstrass" / 0 (XYZZ behind the GLV front end)."""
        f = {"edwards": 1, "weierstrass": 0}.get(form, form)
        self._check(self._lib.msm377_ctx_set_g1_form(self._ctx, int(f)), "msm377_ctx_set_g1_form")

    def set_glv(self, mode="auto"):
        """GLV front end of the Weierstrass form: True/1 = on (the caller vouches that every point lies in the
        prime-order subgroup), False/0 or "auto"/2 = off (the default)."""
        m = 2 if mode == "auto" else int(mode)
        self._check(self._lib.msm377_ctx_set_glv(self._ctx, m), "msm377_ctx_set_glv")

    # -- measurement --
    def set_timing(self, enabled=True):
        """True / 1: HIP events around every stage; 2: around the accumulation kernel only (the other stages read 0);
        False / 0: off.  The events cost GPU idle time between the launches (~50 us per MSM with every stage on)."""
        self._check(self._lib.msm377_ctx_set_timing(self._ctx, 2 if enabled == 2 else int(bool(enabled))), "msm377_ctx_set_timing")

    def stage_ms(self) -> dict:
        arr = (ctypes.c_double * len(STAGE_NAMES))()
        self._check(self._lib.msm377_ctx_get_stage_ms(self._ctx, ctypes.addressof(arr)), "msm377_ctx_get_stage_ms")
        return dict(zip(STAGE_NAMES, list(arr)))


    def accumulate_products(self) -> int:
        """Field products per bucket addition of the last accumulation launch (10 / 8 / 7)."""
        return int(self._lib.msm377_ctx_get_products_per_addition(self._ctx))


def _check_lengths(points: bytes, scalars: bytes, point_bytes: int = 96) -> int:
    """input_size = scalars.length / 32 (submission.ts:91)."""
    if len(scalars) % 32:
        raise ValueError("scalars buffer length must be a multiple of 32")
    n = len(scalars) // 32
    if len(points) != point_bytes * n:
        raise ValueError("points buffer must hold %d bytes (%d per scalar), got %d" % (point_bytes * n, point_bytes, len(points)))
    return n
