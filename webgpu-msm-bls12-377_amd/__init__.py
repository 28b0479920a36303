"""MI355X-native BLS12-377 MSM engine: Python host side.

The directory name carries hyphens (it is fixed by the project layout), so import it through
the repo-root shim ``webgpu_msm_bls12_377_amd`` or via importlib.  Everything here is a thin
mirror of the reference's operator interface over the C ABI in include/msm377.h; the
arithmetic lives in csrc/ (hand-written HIP for gfx950).  There is no CPU fallback: loading
fails loudly when csrc/libmsm377.so is missing, and every MSM call fails when no HIP device
is usable.
"""
from .host.codecs import (  # noqa: F401
    bigIntBufferLE,
    bigIntsToBufferLE,
    bigIntsToU32Array,
    bigIntToU32Array,
    decode_points_native,
    decode_scalars_native,
    encode_points_native,
    encode_scalars,
    encode_scalars_native,
    readBigIntsFromBufferLE,
    u32ArrayToBigInts,
)
from .host.engine import (  # noqa: F401
    CHECK_ALL,
    CHECK_CANONICAL,
    CHECK_CURVE,
    CHECK_SUBGROUP,
    CheckReport,
    StageInfo,
    MsmEngine,
    MsmError,
    batch_lincomb2_host,
    batch_mul_host,
    batch_mul_multi_host,
    batch_mul_var_host,
    check_points_host,
    commit_rows_host,
    commit_rows_plan,
    ed_check_points_host,
    import_points_host,
    import_scalars_host,
    library_path,
    load_library,
    result_to_native,
    scalars_width_host,
    short_windows,
)
from .host.submission import compute_msm, points_to_buffer, scalars_to_buffer  # noqa: F401
from .host.sharding import combine_partials, windows_for_rank  # noqa: F401

__all__ = [
    "compute_msm",
    "MsmEngine",
    "MsmError",
    "CheckReport",
    "StageInfo",
    "batch_lincomb2_host",
    "batch_mul_host",
    "batch_mul_multi_host",
    "batch_mul_var_host",
    "check_points_host",
    "commit_rows_host",
    "commit_rows_plan",
    "ed_check_points_host",
    "CHECK_CANONICAL",
    "CHECK_CURVE",
    "CHECK_SUBGROUP",
    "CHECK_ALL",
    "load_library",
    "scalars_width_host",
    "short_windows",
    "encode_scalars",
    "encode_points_native",
    "decode_points_native",
    "encode_scalars_native",
    "decode_scalars_native",
    "import_points_host",
    "import_scalars_host",
    "result_to_native",
    "library_path",
    "windows_for_rank",
    "combine_partials",
    "points_to_buffer",
    "scalars_to_buffer",
    "bigIntBufferLE",
    "bigIntsToBufferLE",
    "readBigIntsFromBufferLE",
    "bigIntToU32Array",
    "bigIntsToU32Array",
    "u32ArrayToBigInts",
]
