/*
 * msm377 -- C ABI of the MI355X (gfx950) multi-scalar-multiplication engine.
 *
 * This is the drop-in boundary for the reference's hot path
 *     compute_msm(baseAffinePoints: Buffer, scalars: Buffer) -> {x, y}
 *     (/root/reference: src/submission/submission.ts:85-90, called from src/ui/Benchmark.tsx:32
 *      and src/submission/miscellaneous/full_benchmarks.ts:62,99).
 * An N-API shim (webgpu-msm-bls12-377_amd/node/) and a ctypes mirror
 * (webgpu-msm-bls12-377_amd/host/) bind exactly these entry points; see INTEGRATION.md.
 *
 * Wire format (unchanged from the reference harness, src/ui/AllBenchmarks.tsx:57-68 and
 * src/reference/webgpu/utils.ts:63-72):
 *   points   n x 96 bytes : x as 48-byte little-endian || y as 48-byte little-endian,
 *                           canonical residues < p, affine, never the point at infinity
 *   scalars  n x 32 bytes : little-endian integers < 2^255 - 2^239 (the reference requires
 *                           "no final carry" in the signed recode, cuzk/utils.ts:95-98)
 *   result   96 bytes     : affine x || y, 48-byte little-endian each; the identity (and the
 *                           empty input) is x = 0, y = 1 (submission.ts:93-95)
 *
 * All functions return 0 on success or a negative MSM377_E* code; none of them throws or
 * aborts.  A context is not thread-safe: one call in flight per context (the reference has one
 * caller thread).  There is NO CPU fallback: without a usable HIP
 * device every entry point that needs one fails with MSM377_EHIP.
 */
#ifndef MSM377_H
#define MSM377_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSM377_OK 0
#define MSM377_EINVAL (-1)    /* bad argument (null pointer, n over capacity, window range) */
#define MSM377_EHIP (-2)      /* a HIP runtime call failed; see msm377_last_error() */
#define MSM377_ESCALAR (-3)   /* a scalar overflowed the signed 16-bit recode (final carry), or the scalar_bits a short-scalar call declared */
#define MSM377_ENOMEM (-4)    /* device or host allocation failed */
#define MSM377_ESTATE (-5)    /* call sequence error (e.g. fixed-base MSM before set_bases) */
#define MSM377_EGLVRANGE (-6) /* GLV window sharding only: a scalar >~ 2^254; repeat with the plain window path */
#define MSM377_EEXCEPTIONAL (-7) /* combine of window records only: the twisted-Edwards records add up to an exceptional
                                    case of their (incomplete) addition law -- possible only with input points outside the
                                    prime-order subgroup; recompute the windows in form 0 (msm377_ctx_set_g1_form) and combine
                                    again.  The full-MSM entry points handle this themselves and never return it. */
#define MSM377_EPOINT (-8)    /* an input point failed a check the caller asked for (msm377_ctx_set_base_checks), or the canonical /
                                    on-curve check msm377_ed_batch_mul_var* always run; msm377_last_error names index and reason */

#define MSM377_NUM_WINDOWS 16          /* ceil(256 / 16): submission.ts:108-109 */
#define MSM377_WINDOW_BITS 16          /* chunk_size for n >= 2^16: submission.ts:97 */
/* One window's partial result: 16 points (plain bucket sum + 15 bit-plane sums), each four
 * coordinates (X, Y, ZZ, ZZZ) of 12 little-endian u32 words in Montgomery form, radix 2^384. */
#define MSM377_G1_PARTIAL_POINTS 16
#define MSM377_G1_POINT_WORDS 48
#define MSM377_G1_WINDOW_PARTIAL_BYTES (MSM377_G1_PARTIAL_POINTS * MSM377_G1_POINT_WORDS * 4)

typedef struct msm377_ctx msm377_ctx;

/* Library / build identification, e.g. "msm377 0.1 gfx950". */
const char* msm377_version(void);
/* Text for a MSM377_E* code. */
const char* msm377_strerror(int code);

/* Create a context on HIP device `device` with workspace for up to `max_points` inputs
 * (replaces get_device + the per-call buffer creation, cuzk/gpu.ts:2-52; unlike the reference
 * the device state persists across calls until msm377_ctx_destroy). */
int msm377_ctx_create(int device, uint64_t max_points, msm377_ctx** out);
void msm377_ctx_destroy(msm377_ctx* ctx);
/* Last HIP / argument error text for this context ("" if none). */
const char* msm377_last_error(const msm377_ctx* ctx);

/* ---- BLS12-377 G1 (short Weierstrass y^2 = x^3 + 1) ------------------------------------ */

/* compute_msm with host buffers: uploads, runs the pipeline, returns the affine result.
 * Replaces submission.ts:85-327 end to end.  Inputs of 2^18 points and more are uploaded in chunks
 * of points that accumulate into the same buckets, so the transfer overlaps the computation
 * (4.3-4.5 ms for 2^20 points from pageable memory, 2.45-2.55 ms with the inputs already on the device).
 * A context is used by one thread at a time. */
int msm377_g1_msm(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint8_t out_xy[96]);

/* Optional, right after msm377_ctx_create: allocate the pinned staging buffer (128 bytes per point of capacity) and the
 * copy streams the host-buffer entry points upload through.  They are otherwise allocated by the first such call, which
 * then takes ~35 ms instead of ~4.5 (the reference's harness times the first call like any other, src/ui/Benchmark.tsx:31-34). */
int msm377_ctx_reserve_host_staging(msm377_ctx* ctx);

/* Same with inputs already in device memory (same wire format).  This is the variant timed
 * by bench.py ("inputs resident in HBM"). */
int msm377_g1_msm_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint8_t out_xy[96]);

/* Fixed-base batches (BASELINE.json config 5): convert and keep a base set in HBM once ...
 * The resident bases are valid only after a msm377_g1_set_bases* call has returned MSM377_OK, and only until a call
 * that writes the context's base records, its raw point copy or its table -- any other G1 or Edwards-BLS12 MSM, the
 * window-partials calls, the next set-bases call.  Every set-bases call drops the resident bases first, before it
 * checks its arguments, and installs the new ones as its last step: after one that fails for whatever reason the
 * fixed-base calls return MSM377_ESTATE. */
int msm377_g1_set_bases(msm377_ctx* ctx, const uint8_t* points, uint64_t n);
int msm377_g1_set_bases_device(msm377_ctx* ctx, const void* d_points, uint64_t n);
/* The same with precomputed window multiples (BASELINE.json config 5, "precomputed-point reuse"; the reference lists
 * precomputation among its own future improvements, /root/reference README.md:558-563): additionally keeps
 * [2^(16 w)] P_i for all 16 windows (16 n affine records: 2.7 GB at n = 2^20, allocated on demand, ~38 ms once).  Every
 * window then gathers points that already carry its weight, so the sixteen bucket sets are simply added together on the
 * GPU: ONE bucket reduction, one partial record and a 16-step host tail per MSM instead of 16 and 256.  Results are
 * identical.  In the Weierstrass form (msm377_ctx_set_g1_form 0) this is msm377_g1_set_bases. */
/* Window width of the tables the next msm377_g1_set_bases_precomputed* call builds: MSM377_WINDOW_BITS (16, default: the
 * layout above) or MSM377_WIDE_WINDOW_BITS (20): 13 windows -- six of 20 bits, then seven of 19, 253 bits in all -- with
 * [2^(offset of window w)] P_i in the table (13 n affine records, 2.2 GB at n = 2^20).
 * Because every window's points already carry its weight, all windows share ONE bucket set, so the window can widen
 * without multiplying buckets: 13 n bucket additions per MSM instead of 16 n over 2^19 buckets -- as many as the
 * 16 x 2^15 of the plain path -- one 19-level reduction, a 20-step host tail.  (21-bit windows are still 13 for a
 * 253-bit scalar; 22-bit ones quadruple the buckets.)  A scalar of 2^253 and more (none below the group order) reruns
 * on the 16-window path over the table's first window.  Results are identical. */
#define MSM377_WIDE_WINDOW_BITS 20
int msm377_ctx_set_precompute_window(msm377_ctx* ctx, int window_bits);
int msm377_g1_set_bases_precomputed(msm377_ctx* ctx, const uint8_t* points, uint64_t n);
int msm377_g1_set_bases_precomputed_device(msm377_ctx* ctx, const void* d_points, uint64_t n);
/* ... then run any number of MSMs of n scalars (host or device pointer) against it. */
int msm377_g1_msm_fixed_base(msm377_ctx* ctx, const uint8_t* scalars, uint64_t n, uint8_t out_xy[96]);
int msm377_g1_msm_fixed_base_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint8_t out_xy[96]);
/* `batch` MSMs over the resident bases in one call: d_scalars holds batch x n x 32 bytes, out_xy
 * receives batch x 96 bytes.  The host tail of MSM b overlaps the GPU work of MSM b+1.  From batch = 4 on the call runs
 * as two halves side by side on two sets of streams and work buffers (a "twin" of the context's buffers, created with
 * the first such call: the context's device memory without the tables, ~0.7 GB at 2^20 points, a second time; if that
 * allocation fails, or with MSM377_TWIN_BATCH=0, the batch runs on one set) -- the low-occupancy ends of one MSM fill
 * with the other half's kernels: 2.16 -> 2.05 ms per MSM at 2^20, 2.00 -> 1.89 on the 20-bit-window table. */
int msm377_g1_msm_fixed_base_batch_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t batch, uint8_t* out_xy);

/* Window sharding for multi-GPU runs (the reference already treats the
 * 16 window subtasks as independent, submission.ts:199-224).  Computes windows
 * [win_begin, win_begin + win_count) only and writes win_count partial records of
 * MSM377_G1_WINDOW_PARTIAL_BYTES each to the HOST buffer partials_out.  The records are opaque: they carry
 * their own coordinate-system tag (twisted Edwards by default; windows that hit an exceptional case of
 * that form, and contexts in form 0, produce Weierstrass records), and the combine functions accept any
 * mixture, so ranks never have to agree on a form. */
int msm377_g1_window_partials_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n,
                                     uint32_t win_begin, uint32_t win_count, uint8_t* partials_out);
/* The same, but the records are left in DEVICE memory (d_partials_out: win_count records, 16-byte aligned): the
 * exchange of a multi-GPU run (one RCCL all-gather over xGMI) reads them where they are, no host round trip.
 * Returns with the context's stream idle, so any other stream may consume the buffer. */
int msm377_g1_window_partials_resident(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n,
                                       uint32_t win_begin, uint32_t win_count, void* d_partials_out);
/* Optional, before the exchange: a rank folds the records of its own win_count CONSECUTIVE windows (in place,
 * same size, same total: one short Horner chain over them; every point but one becomes the identity), which
 * leaves the final combine on every rank with its doublings and one addition per rank instead of 16 per
 * window -- the host tail is a fixed cost that does not shrink with the number of GPUs.  Host-only. */
int msm377_g1_fold_window_partials(uint8_t* partials, uint32_t win_count);
/* Combine the partial records of all MSM377_NUM_WINDOWS windows (window-major, gathered from
 * the ranks) into the final affine result: Horner over the windows, one field inversion.
 * Host-only; needs no context and no device (replaces the CPU tail, submission.ts:290-321). */
int msm377_g1_combine_partials(const uint8_t* partials, uint8_t out_xy[96]);
/* The same result for records in twisted Edwards form, computed the way a context's tail threads compute it -- the
 * Horner chain cut into `pieces` (1..64) balanced pieces, each doubled up to its position, then added -- but on the
 * calling thread: the decomposition of msm377_g1_combine_partials_ctx / the full-MSM entry points, checkable without a
 * GPU (tests/test_host_tail.py).  MSM377_EINVAL for records in Weierstrass form. */
int msm377_g1_combine_partials_split(const uint8_t* partials, uint32_t pieces, uint8_t out_xy[96]);
/* The same on the context's tail threads (the Horner chain cut into up to eight balanced pieces, as inside msm377_g1_msm:
 * MSM377_TAIL_THREADS, default 6): 0.08 instead of 0.14 ms.  MSM377_EHIP if a helper thread does not answer in time. */
int msm377_g1_combine_partials_ctx(msm377_ctx* ctx, const uint8_t* partials, uint8_t out_xy[96]);

/* Point sharding, the other partitioning of a multi-GPU run (SURVEY.md section 8e names it as the fallback): rank g runs a
 * COMPLETE MSM -- msm377_g1_msm_device, all 16 windows, its own host tail -- over its slice [g n / G, (g + 1) n / G) of the
 * points and scalars, the ranks all-gather their 96-byte results and every rank adds them up with this function: the
 * sum of `count` affine wire points (the identity as the wire format writes it, x = 0 and y = 1, is accepted).  Nothing
 * is replicated (conversion, decomposition, sort, reduction and tail all shrink with n / G), so it scales further than
 * window sharding, which replicates the base conversion and whose per-window fixed costs stay.  Host-only, no context.
 * MSM377_EINVAL for a coordinate that is not below p. */
int msm377_g1_add_points(const uint8_t* points_xy, uint32_t count, uint8_t out_xy[96]);

/* The same sharding behind the GLV front end (opt-in, prime-order subgroup points only -- see
 * msm377_ctx_set_glv; Weierstrass form): MSM377_GLV_WINDOWS = 8 windows over {P_i, phi(P_i)};
 * win_begin / win_count index those 8.  Returns MSM377_EGLVRANGE when a scalar does not split into
 * two 127-bit halves (every rank sees the same scalars, so every rank gets the same verdict and the
 * job repeats on the plain 16-window path).  Halving the windows halves the per-rank fixed costs
 * (bucket reduction, host tail), which dominate once the additions are spread over several GPUs. */
#define MSM377_GLV_WINDOWS 8
int msm377_g1_glv_window_partials_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n,
                                         uint32_t win_begin, uint32_t win_count, uint8_t* partials_out);
/* Combine `num_windows` gathered partial records (16 plain, 8 GLV).  Host-only. */
int msm377_g1_combine_window_partials(const uint8_t* partials, uint32_t num_windows, uint8_t out_xy[96]);

/* ---- short scalars -------------------------------------------------------------------------
 * Most callers of an MSM engine do not multiply by uniform 253-bit scalars: batch verification uses 128-bit challenges,
 * witness and range-check columns hold 64-bit values, bytes or bits, lookup multiplicities are 32-bit counts.  These
 * entry points take the scalars compact -- n x scalar_bytes little-endian bytes, scalar_bytes in {4, 8, 16, 32}, device
 * pointers 16-byte aligned as elsewhere -- together with scalar_bits, 1 .. min(8 scalar_bytes, 253): the caller's PROMISE
 * that every scalar is below 2^scalar_bits (msm377_scalars_width_* measure it).  Any other stride or width is
 * MSM377_EINVAL; n == 0 gives the identity.
 *
 * Geometry.  The path is chosen by n as for the full-width calls: 2^L buckets per window with L = 11 up to the
 * msm377_ctx_set_narrow_max size (Edwards form, plain resident bases or none) and L = 15 above it, for every
 * precomputed table and in form 0.  The call runs
 *     W = msm377_short_windows(scalar_bits, L) = floor(scalar_bits / (L + 1)) + 1
 * window slots: the first W - 1 are signed digits of L + 1 bits with a carry into the next window, the top one is the
 * unsigned rest -- scalar_bits mod (L + 1) bits plus the carry, at most 2^L -- so it never carries out and no scalar
 * below 2^scalar_bits needs a second pass.  At 253 bits W is 16 (L = 15) and 22 (L = 11), the window counts of the
 * full-width calls; 64-bit scalars run 5 windows and 128-bit ones 9 at L = 15.  Sort, bucket reduction, partial records
 * and host tail cover those W windows only.  The top window may hold a few bits or carries only; its sort ranges are
 * narrowed by its largest key like the top window of the 16-window recode.
 *
 * A scalar of 2^scalar_bits or more breaks the promise: the call fails with MSM377_ESCALAR, msm377_last_error names
 * the declared width and out_xy is left untouched.  There is no rerun at full width -- a wrong width is a caller bug.
 *
 * Form: twisted Edwards, with the automatic Weierstrass rerun on an exceptional case as for the full-width calls
 * (msm377_ctx_get_fallback_info counts it); with msm377_ctx_set_g1_form(0) W windows of XYZZ at L = 15.  Never the GLV
 * front end.  Affine records per call from MSM377_AFFINE_MIN points on, as for msm377_g1_msm_device.
 * Not covered: Edwards-BLS12, the window-partials and batch calls, a chunked upload (msm377_g1_msm_short uploads the
 * n x scalar_bytes scalars, then the points behind decomposition and sort, in one piece each). */
int msm377_g1_msm_short_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t scalar_bytes,
                               uint32_t scalar_bits, uint8_t out_xy[96]);
int msm377_g1_msm_short(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint32_t scalar_bytes,
                        uint32_t scalar_bits, uint8_t out_xy[96]);
/* Over whatever the last msm377_g1_set_bases* call left resident (MSM377_ESTATE without): plain records and the 16-bit
 * table serve window slots 0 .. W - 1 (the table's bucket sets are still added before the one reduction); the 20-bit
 * table serves through its first window's records, the points themselves, on the L = 15 path -- the wide table buys
 * nothing for short scalars.  The resident bases are left as they were. */
int msm377_g1_msm_fixed_base_short_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t scalar_bytes,
                                          uint32_t scalar_bits, uint8_t out_xy[96]);
/* The largest bit length among n scalars of scalar_bytes bytes each (0 for all-zero scalars and for n == 0): what a
 * caller passes as scalar_bits.  The device variant uses the context's stream and touches neither the resident bases
 * nor a result; n is not bounded by the context's capacity.  The host variant needs no context and no device. */
int msm377_scalars_width_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t scalar_bytes, uint32_t* bits_out);
int msm377_scalars_width_host(const uint8_t* scalars, uint64_t n, uint32_t scalar_bytes, uint32_t* bits_out);
/* W of the rule above: floor(scalar_bits / (bucket_log + 1)) + 1.  Host-only and pure; 0 for scalar_bits outside
 * 1 .. 253 or bucket_log outside 1 .. 15. */
uint32_t msm377_short_windows(uint32_t scalar_bits, uint32_t bucket_log);
/* Window slots and bucket_log (L) of the last G1 MSM call's last pass on this context, e.g. (16, 15), (22, 11),
 * (1, 19) on the 20-bit table, (5, 15) for a 64-bit short call; (0, 0) before the first call. */
int msm377_ctx_get_last_geometry(const msm377_ctx* ctx, uint32_t* windows, uint32_t* bucket_log);
/* Bytes per element of the sort's intermediate buffer in the last call's last pass: 8; 4 (packed) with MSM377_SORT_ELEM=4
 * in the environment when the context was created, for calls of at most 2^23 columns on the two-level sort of the
 * 2^15-bucket path; 0 where no such sort ran (narrow windows, before the first call).  Results do not depend on it. */
uint32_t msm377_ctx_get_last_sort_elem_bytes(const msm377_ctx* ctx);

/* ---- native input forms ---------------------------------------------------------------------
 * A prover built on arkworks or snarkVM keeps nothing in the wire format above: field elements live in Montgomery form
 * (a G1 coordinate as x * 2^384 mod p in six little-endian u64 limbs, a scalar as s * 2^256 mod r in four), and an affine
 * point carries an infinity flag (x, y and one flag byte, padded to 104 bytes).  A context can be told to read those
 * forms directly: an import pass on the GPU (csrc/kernels/import.hpp) writes wire-format data into the context's staging
 * and the pipeline runs unchanged behind it.  The default is (WIRE, WIRE): nothing is launched or allocated that was
 * not before.  Results stay in the wire format (msm377_g1_result_to_native converts one).
 *
 *   MSM377_POINTS_MONT       a coordinate value v means v * 2^-384 mod p.  Values of p or more are trusted not to occur,
 *                            as in the wire format: such a point is handed on as its bytes are, the MSM calls compute a
 *                            meaningless result from it and only the check calls classify it (non-canonical).
 *   MSM377_POINTS_MONT_FLAG  the same with a flag byte behind the coordinates.  A point whose flag byte is non-zero is
 *                            the identity: its 96 coordinate bytes are never interpreted and may hold anything, and it
 *                            contributes nothing to any sum.  Device pointers stay 16-byte aligned; single records are
 *                            8-byte aligned.
 *   MSM377_SCALARS_MONT      every 32-byte value v is accepted and means v * 2^-256 mod r, fully reduced, so a call with
 *                            this form never returns MSM377_ESCALAR.
 *
 * Honoured by (all G1): msm377_g1_msm(_device), the four msm377_g1_set_bases* calls, msm377_g1_msm_fixed_base(_device),
 * msm377_g1_msm_fixed_base_batch_device, msm377_g1_window_partials_device / _resident, msm377_g1_glv_window_partials_device;
 * with the point form only: msm377_g1_check_points(_device) and the short-scalar calls.  The identity points of a
 * resident base set are remembered with it (every fixed-base call, whatever its scalar form, leaves them out) and dropped
 * with it by the next set-bases call.  Check calls: the canonical test compares the Montgomery value the caller wrote
 * with p, the curve and subgroup tests see the imported point, flagged points are counted in no class and are never
 * first_bad, `checked` stays n; msm377_ctx_set_base_checks accepts flagged points likewise.
 * Host-buffer calls in a native form upload each array in one piece into a device buffer allocated with the first such
 * call (104 + 32 bytes per point of capacity), import from there and continue on the device-pointer path: no chunked
 * overlap of upload and computation, as for msm377_g1_msm_short.
 * Not covered: a short-scalar call while MSM377_SCALARS_MONT is set is MSM377_EINVAL (a compact Montgomery scalar does
 * not exist); the Edwards-BLS12 calls (msm377_ed_*) return MSM377_EINVAL while any non-wire form is set;
 * msm377_g1_generate_bases_device keeps writing the wire format. */
#define MSM377_POINTS_WIRE      0  /* 96 B: x || y canonical (the wire format above, the default) */
#define MSM377_POINTS_MONT      1  /* 96 B: x*2^384 mod p || y*2^384 mod p, little-endian */
#define MSM377_POINTS_MONT_FLAG 2  /* 104 B: as MONT, then one byte (0 = finite, non-zero = identity), 7 bytes ignored */
#define MSM377_SCALARS_WIRE     0  /* 32 B canonical little-endian (the wire format above, the default) */
#define MSM377_SCALARS_MONT     1  /* 32 B: s*2^256 mod r, little-endian */
/* An unknown value: MSM377_EINVAL, and the forms stay as they were. */
int msm377_ctx_set_input_format(msm377_ctx* ctx, uint32_t point_form, uint32_t scalar_form);
int msm377_ctx_get_input_format(const msm377_ctx* ctx, uint32_t* point_form, uint32_t* scalar_form);
/* The same conversions on the calling thread: no context, no device.  For callers that want wire data, and as the
 * yardstick of the GPU pass: a second implementation that shares no field code with it.  out_wire: n x 96 (n x 32) bytes;
 * out_inf_mask (may be NULL): ceil(n / 32) words, bit i % 32 of word i / 32 set for a flagged point, whose record is the
 * generator's.  in and out_wire may be the same buffer for the 96-byte forms.  A form outside the list: MSM377_EINVAL. */
int msm377_g1_import_points_host(const uint8_t* in, uint64_t n, uint32_t point_form, uint8_t* out_wire, uint32_t* out_inf_mask);
int msm377_import_scalars_host(const uint8_t* in, uint64_t n, uint32_t scalar_form, uint8_t* out_wire);
/* A wire result as a MSM377_POINTS_MONT_FLAG record: Montgomery x, y, the flag, seven zero bytes; the wire identity
 * (0, 1) sets the flag.  MSM377_EINVAL for a coordinate that is not below p. */
int msm377_g1_result_to_native(const uint8_t xy[96], uint8_t out[104]);

/* Synthetic inputs: P_i = [a_i]G, a_i the i-th SplitMix64(seed)
 * output, written in wire format to device memory d_points_out (n x 96 bytes). */
int msm377_g1_generate_bases_device(msm377_ctx* ctx, uint64_t seed, uint64_t n, void* d_points_out);

/* ---- Twisted-Edwards BLS12 ("Edwards-BLS12": a = -1, d = 3021 over the BLS12-377 scalar field;
 *      BASELINE.json config 3; the reference's orphaned Edwards shaders,
 *      src/submission/miscellaneous/wgsl/add_points_any_a.template.wgsl:24-71,
 *      src/reference/params/AleoConstants.ts:2-5) --------------------------------------------
 * Wire format (README.md:299-301): points n x 64 bytes = x || y, 32-byte little-endian each;
 * scalars as above; result 64 bytes x || y; the neutral element (and the empty input) is
 * x = 0, y = 1.  Same pipeline and workspace as G1 (extended coordinates, add-2008-hwcd-3). */
int msm377_ed_msm(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint8_t out_xy[64]);
int msm377_ed_msm_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint8_t out_xy[64]);
/* Synthetic Edwards inputs: P_i = [a_i]G_ed (src/reference/utils/FieldMath.ts:108-109), 64 bytes each. */
int msm377_ed_generate_bases_device(msm377_ctx* ctx, uint64_t seed, uint64_t n, void* d_points_out);

/* ---- input validation -------------------------------------------------------------------
 * The MSM entry points trust their input: a coordinate of p or more, a pair (x, y) that is not on the curve or a point
 * outside the prime-order subgroup goes through the pipeline like any other 96 (64) bytes and comes back as a
 * well-formed, meaningless result with MSM377_OK.  (The reference's shaders make the same assumption; it has no
 * counterpart of these calls.)  Points that come from a file or from a peer are checked with the calls below, before
 * the MSM or once per resident base set.
 *
 * The checks are a cascade, and a point is counted once, in the first class it fails: non-canonical, then off the curve,
 * then outside the subgroup.  A subgroup verdict means nothing for a point that is not on the curve (and the addition
 * laws are only guaranteed there), and the curve equation is evaluated on canonical residues, so MSM377_CHECK_SUBGROUP
 * implies the other two bits and MSM377_CHECK_CURVE implies MSM377_CHECK_CANONICAL: `flags` normalises to 1, 3 or 7.
 * flags == 0, a bit outside MSM377_CHECK_ALL or a null report pointer: MSM377_EINVAL. */
#define MSM377_CHECK_CANONICAL 1u /* every coordinate < p (Edwards-BLS12: < q, the BLS12-377 scalar field) */
#define MSM377_CHECK_CURVE     2u /* G1: y^2 = x^3 + 1;  Edwards-BLS12: -x^2 + y^2 = 1 + 3021 x^2 y^2 */
#define MSM377_CHECK_SUBGROUP  4u /* [r]P = O, r the prime group order (G1: the BLS12-377 scalar field modulus; Edwards-BLS12:
                                     2111115437357092606062206234695386632838870926408408195193685246394721360383, a
                                     quarter of the group: the Edwards cofactor is 4) */
#define MSM377_CHECK_ALL       7u

typedef struct {
  uint64_t checked;          /* n */
  uint64_t noncanonical;     /* points with a coordinate >= modulus */
  uint64_t off_curve;        /* canonical, but not on the curve */
  uint64_t outside_subgroup; /* on the curve, but [r]P != O */
  uint64_t first_bad;        /* lowest index of a point counted above; UINT64_MAX if none */
  uint32_t first_bad_reason; /* the MSM377_CHECK_* bit that point failed; 0 if none */
  uint32_t reserved;         /* 0 */
} msm377_check_report;

/* A check call that ran returns MSM377_OK whatever it found: the verdict is the report.  The report is deterministic
 * (first_bad is the LOWEST failing index, whatever order the GPU visits the points in) and correct for every input,
 * like the MSM itself: the wire format cannot encode the identity, but [r]P passes through it for the points of order
 * 2, 3, 4 and 6 and for P + T with T one of them; all of those are reported outside the subgroup.  (The subgroup
 * test of G1 therefore runs in Weierstrass XYZZ coordinates, whatever msm377_ctx_set_g1_form says.)
 * n == 0: MSM377_OK, all counters zero, first_bad == UINT64_MAX.  n over the context's capacity, a null or misaligned
 * (16 bytes) device pointer: MSM377_EINVAL, as for the MSM calls.
 * The calls use the context's stream and work buffers while they run and touch neither the resident bases nor their
 * table: "check the set, then run the batch" and "run, then audit" both work, and d_points may be memory of the caller's
 * that it passed to msm377_g1_set_bases*_device before.  msm377_ctx_get_fallback_info is left alone.  The host-buffer
 * variants upload the points first.  0.08 ms (canonical + curve) and 44 ms (with the subgroup test) per 2^20 G1 points. */
int msm377_g1_check_points_device(msm377_ctx* ctx, const void* d_points, uint64_t n, uint32_t flags, msm377_check_report* out);
int msm377_g1_check_points(msm377_ctx* ctx, const uint8_t* points, uint64_t n, uint32_t flags, msm377_check_report* out);
int msm377_ed_check_points_device(msm377_ctx* ctx, const void* d_points, uint64_t n, uint32_t flags, msm377_check_report* out);
int msm377_ed_check_points(msm377_ctx* ctx, const uint8_t* points, uint64_t n, uint32_t flags, msm377_check_report* out);
/* The same reports computed on the calling thread: no context, no device.  For small sets (a subgroup test is ~0.1 ms
 * per G1 point here) and as the yardstick of the GPU path: a second implementation that shares no field or chain code
 * with it. */
int msm377_g1_check_points_host(const uint8_t* points, uint64_t n, uint32_t flags, msm377_check_report* out);
int msm377_ed_check_points_host(const uint8_t* points, uint64_t n, uint32_t flags, msm377_check_report* out);

/* Opt-in, default 0 = no check (also MSM377_BASE_CHECKS in the environment at msm377_ctx_create): the four
 * msm377_g1_set_bases* calls check the base set with these flags after they have dropped the resident bases and before
 * they convert it.  A set with a finding leaves NO resident bases (the fixed-base calls answer MSM377_ESTATE, as after
 * any failed set-bases call), the call returns MSM377_EPOINT and msm377_last_error names index and reason.  flags is 0
 * or a valid check mask, else MSM377_EINVAL. */
int msm377_ctx_set_base_checks(msm377_ctx* ctx, uint32_t flags);
/* The report of the last check a msm377_g1_set_bases* call ran on this context (checked == 0, first_bad == UINT64_MAX
 * before the first one). */
int msm377_ctx_get_last_check(const msm377_ctx* ctx, msm377_check_report* out);

/* ---- stage access for parity tests (the reference's debug=true read-backs,
 *      submission.ts:466-520, 613-641, 724-798) ------------------------------------------- */

/* After any g1 MSM call: copy stage outputs of window slot `slot` (0-based within the windows
 * computed by the last call) to host buffers; any pointer may be NULL.
 *   digits   n u16          biased signed digits, d + 2^15
 *   row_ptr  32770 u32      CSR offsets over keys |d| = 0..32768 (key 0 = digit 0)
 *   val_idx  n u32          point index | (sign << 31), grouped by key
 *   buckets  32768 x 52 u32 bucket t = 1..32768 at row t-1: X, Y, ZZ, ZZZ (13 Montgomery words
 *                           each) as left by bucket accumulation
 * Only valid when the context was created with stage capture enabled.
 *
 * The bucket words describe the coordinate system the call ended in (msm377_ctx_get_stage_form): XYZZ as above for
 * form 0 and for calls that fell back to it, (X, Y, T, Z) extended twisted Edwards coordinates (csrc/te377.hpp: lazy
 * residues below p + 2^354, the identity stored as (0, c, 0, c)) for the default form. */
#define MSM377_STAGE_FORM_XYZZ 0
#define MSM377_STAGE_FORM_TE 1
/* Edwards-BLS12 calls (msm377_ed_msm*), msm377_stage_info.form only: (X, Y, T, Z) extended twisted Edwards coordinates over
 * the 9-limb field Fq, 9 Montgomery words each (radix 2^261, lazy residues below q + e, the identity stored as (0, c, 0, c)):
 * 36 words per record.  Read as run only (capture mode 2, msm377_g1_read_stage_ex). */
#define MSM377_STAGE_FORM_ED 2
int msm377_ctx_get_stage_form(const msm377_ctx* ctx); /* -1: nothing captured, or the last call was an Edwards-BLS12 one */
int msm377_ctx_set_stage_capture(msm377_ctx* ctx, int enabled);
int msm377_g1_read_stage(msm377_ctx* ctx, uint32_t slot, uint16_t* digits, uint32_t* row_ptr, uint32_t* val_idx, uint32_t* buckets);

/* Capture modes of msm377_ctx_set_stage_capture (any other value: MSM377_EINVAL, the mode stays as it was; before mode 2
 * existed every non-zero value meant mode 1).  msm377_g1_read_stage answers under mode 1 only, msm377_g1_read_stage_ex
 * under modes 1 and 2; each returns MSM377_ESTATE otherwise.  Mode 1 and msm377_g1_read_stage describe G1 calls only:
 * after an Edwards-BLS12 call both read-backs return MSM377_ESTATE under mode 1.
 *   0  off.
 *   1  the route the read-backs above describe: sixteen equal 16-bit windows of 2^15 buckets, whatever the input size --
 *      the narrow-window path, the even geometry, the chunked upload and twin batches are switched off while it is set.
 *   2  AS RUN: the call takes the route it would take without capture (narrow windows, the even geometry, short
 *      scalars, the wide table, the GLV front end, reruns) and msm377_g1_read_stage_ex describes whatever its LAST pass
 *      launched.  Out of scope, and therefore still switched off by mode 2 as by mode 1: the chunked upload of the
 *      host-buffer calls (msm377_g1_msm and msm377_ed_msm alike) and twin batches, whose rows are laid out per chunk / per
 *      half.  Edwards-BLS12 calls are described like G1 calls: the even geometry, or sixteen equal windows after a rerun
 *      or under MSM377_EVEN_WINDOWS=0, with records of form MSM377_STAGE_FORM_ED.  Not described (MSM377_ESTATE):
 *      window-partials calls that do not start at window 0.
 *
 * msm377_stage_info is filled from the arguments the last pass's kernels were launched with:
 *   slots           window slots (16; 22 narrow; floor(bits / (L + 1)) + 1 short; 1 wide table; 8 GLV)
 *   bucket_log      L: 2^L buckets per slot, keys 0 .. 2^L
 *   columns         entries per slot: n, 2 n behind the GLV front end (column n + i = phi(P_i)), 13 n on the wide table
 *                   (window-major: digit column w n + i; val_idx entries name table record w * table_stride + i)
 *   digit_bytes     2 or 4: element size of `digits`
 *   row_ptr_len     2^L + 2
 *   bucket_records  2^L records per slot, bucket t = key t + 1 at record t: 52 words each (four coordinates of 13 limbs), 36
 *                   (four of 9) for MSM377_STAGE_FORM_ED
 *   form            MSM377_STAGE_FORM_* of the records
 *   table_stride    records per window of a precomputed table (0: every slot gathers from the same base records)
 *   geometry_reruns passes this context has discarded so far because a scalar did not fit their window geometry (2^253 and
 *                   more, a carry out of the top window, or a GLV half of 2^127 and more) and run again on another one; counted up to and including the
 *                   call described, so a test can tell a silent rerun from none
 *   bias[s]         stored digit = digit + bias[s]
 *   key_unsigned[s] 1: the sort reads the slot's stored digits as unsigned keys (the top slot of a short call on 2^15 buckets)
 *   key_max[s]      the slot's key_max word as the sort read it (bit 31 = tracked, bit 30 = unsigned, low bits = largest
 *                   key; 0 = not tracked, and always 0 where the sort takes no such word: narrow windows, the wide table) */
#define MSM377_STAGE_MAX_SLOTS 22
typedef struct msm377_stage_info {
  uint32_t slots, bucket_log;
  uint64_t columns;
  uint32_t digit_bytes, row_ptr_len, bucket_records;
  int32_t form;
  uint64_t table_stride;
  uint64_t geometry_reruns;
  uint32_t bias[MSM377_STAGE_MAX_SLOTS];
  uint32_t key_unsigned[MSM377_STAGE_MAX_SLOTS];
  uint32_t key_max[MSM377_STAGE_MAX_SLOTS];
} msm377_stage_info;
/* Stage outputs of window slot `slot` of the last G1 or Edwards-BLS12 MSM call, at the sizes `info` reports (any pointer
 * may be NULL; call once with buffers NULL to size them): digits columns x digit_bytes, row_ptr row_ptr_len u32, val_idx
 * columns u32, buckets bucket_records x 52 u32 (x 36 for MSM377_STAGE_FORM_ED).  MSM377_ESTATE (and nothing written) unless capture is on and the last call's last
 * pass ran to the end under it on a route the mode describes. */
int msm377_g1_read_stage_ex(msm377_ctx* ctx, uint32_t slot, msm377_stage_info* info, void* digits, uint32_t* row_ptr, uint32_t* val_idx, uint32_t* buckets);

/* ---- window records (what the bucket reduction hands to the host tail) ----
 *
 * msm377_g1_read_partials describes and copies the window records of the LAST PASS of the last call: what
 * k_gather_partials (csrc/kernels/reduce.hpp) wrote after the bucket reduction, before the host tail combined them.  It
 * answers exactly where msm377_g1_read_stage_ex answers (capture mode 1 or 2, a whole G1 or -- mode 2 -- Edwards-BLS12
 * call from window 0; after a rerun the pass that produced the result) and returns MSM377_ESTATE, writing nothing,
 * everywhere else.  It waits for the context's stream first: a call returns to its caller while the gather kernel is
 * still finishing.  `info` is written down on the host beside the launches it describes; with capture off a call launches
 * and allocates exactly what it did without the read-back.  `words` = NULL only fills `info` (sizes the buffer:
 * records * points * 4 * coord_words u32).
 *
 *   records        window records (wc_out): one per window slot; ONE behind a precomputed table (the wide table's single
 *                  slot, or the sixteen slots of the 16-bit table folded into slot 0 by k_fold_windows)
 *   points         points per record (pp): 16, or 20 in the one record of the wide table
 *   planes         L, the bucket_log of the pass: point 0 is the sum of all 2^L buckets, point 1 + b (b < L) the sum of the
 *                  buckets whose index has bit b set (bucket index t holds key t + 1).  Points beyond index `planes` are
 *                  UNSPECIFIED: the gather kernel does not write them and the host tail does not read them
 *   coord_words    u32 words per coordinate: 12, or 8 for MSM377_STAGE_FORM_ED; a point is four coordinates
 *   form           MSM377_STAGE_FORM_* of the records
 *   folded_slots   window slots added into each record before the reduction (16 behind the 16-bit table, else 1)
 *   tail_kind      the host tail the records went to: 0 twisted Edwards, 1 Weierstrass (XYZZ), 2 Edwards-BLS12
 *   tail_windows, tail_cbits, tail_planes, tail_short_from
 *                  the geometry that tail was called with: window count, bits between two windows, bit planes per window,
 *                  and the first window that is one bit narrower (0: none)
 *   coop_from, tail_from, columns, tail_lds
 *                  the reduction schedule of the pass.  Levels [0, tail_from) ran as column launches of up to four levels
 *                  (k_tree_columns; columns = 1) or one launch per level (columns = 0: k_tree_step below coop_from,
 *                  k_tree_step_quad from there on); levels [tail_from, planes) in one launch, k_reduce_tail_lds (tail_lds
 *                  = 1) or k_reduce_tail.  Below coop_from an empty bucket is skipped, from there on it is added
 *
 * The record contract (pack_partial in csrc/kernels/reduce.hpp; readers in csrc/fp64_host.hpp):
 *   - point p of record w starts at word ((w * points + p) * 4) * coord_words; its coordinates are X, Y, T, Z (twisted
 *     Edwards forms) or X, Y, ZZ, ZZZ (Weierstrass), coord_words little-endian u32 each;
 *   - EVERY coordinate of every point up to `planes` is CANONICAL: the Montgomery residue v * 2^(32 coord_words) mod p
 *     (mod q for Edwards-BLS12), below the modulus -- whatever lazy form the bucket held;
 *   - the tag: bit 31 of the last word of coordinate 0 of POINT 0 of every record of form MSM377_STAGE_FORM_TE is set
 *     (values are below 2^377, the bit is free) and must be cleared before the coordinate is used.  It is set in no other
 *     word: not in another coordinate, not in another point, and in no word of a Weierstrass or Edwards-BLS12 record;
 *   - the identity is (0 : c : 0 : c), c != 0, in both Edwards forms -- any c: from level coop_from on empty buckets are
 *     added like any other, and a sum that cancels leaves whatever Z it came to -- and ZZ = ZZZ = 0 in the Weierstrass form;
 *   - every point satisfies its form's invariant: T Z = X Y and the curve equation; ZZ^3 = ZZZ^2. */
typedef struct msm377_partials_info {
  uint32_t records, points, planes, coord_words;
  int32_t form;
  uint32_t folded_slots;
  uint32_t tail_kind, tail_windows, tail_cbits, tail_planes, tail_short_from;
  uint32_t coop_from, tail_from, columns, tail_lds;
  uint32_t reserved;
} msm377_partials_info;
int msm377_g1_read_partials(msm377_ctx* ctx, msm377_partials_info* info, uint32_t* words);

/* ---- the accumulation work list (what the dominant kernel is handed, and the overflow partials of split rows) ----
 *
 * The accumulation stage cuts every bucket row into work items of at most `seg` entries (csrc/row_split.hpp), sorts
 * them by length, longest first, across all window slots (k_work_hist / k_work_scatter), runs one thread or lane quad
 * per item (k_accumulate / k_accumulate_quad: item 0 of a row writes the bucket, item s >= 1 the overflow record
 * row_ovf_base[row] + s - 1) and adds the overflow records back (k_fold_long_rows for the long rows of the top slot of
 * a short-scalar call, then k_merge_split_rows_quad).  msm377_g1_read_work_list describes and copies what the LAST PASS
 * of the last call left of all that.  It answers exactly where msm377_g1_read_stage_ex answers (capture mode 1 or 2, a
 * whole G1 or -- mode 2 -- Edwards-BLS12 call from window 0; after a rerun the pass that produced the result) and
 * returns MSM377_ESTATE, writing nothing, everywhere else.  It STOPS ANSWERING (MSM377_ESTATE) once a later call has
 * used the front of the work-list block as scratch -- msm377_g1_check_points*, msm377_ed_check_points*,
 * msm377_scalars_width_device -- until the next describable MSM call: the counters are read where the kernels left
 * them and are not copied aside under capture.  It waits for the context's stream first.  With capture off a call
 * launches and allocates exactly what it did without the read-back.
 *
 * Written on the host beside the launches, from the values they were given:
 *   seg             entries per work item (SEG) of the pass
 *   rows            window slots x 2^L: row = slot 2^L + t is bucket t (key t + 1) of the slot
 *   max_items       the bound the accumulation grid was sized for: rows + entries / seg
 *   quad            1: k_accumulate_quad ran (a lane quad per item), 0: k_accumulate
 *   fold_slot       the window slot k_fold_long_rows was launched on (the top one), -1: not launched
 *   record_words    u32 words per overflow record as copied out: 52, or 36 for MSM377_STAGE_FORM_ED -- the layout of a
 *                   bucket record of msm377_g1_read_stage_ex
 *   form            MSM377_STAGE_FORM_* of the records
 *   bucket_log      L
 * Read from the device once the stream is idle:
 *   items           work items in the list (what the accumulation kernel read as its count)
 *   split_rows      rows of more than one item
 *   overflow_slots  overflow records reserved: the sum of nseg - 1 over the split rows
 *   hist[b]         work items of b entries, b = 0 .. 128 (rows without entries are items of length 0)
 *
 * Buffers, any of which may be NULL (call once with `info` alone to size them):
 *   items_out         items x 2 u32: (row, seg) in list order, longest first
 *   split_rows_out    split_rows u32: the rows of the split-row list, in the order the merge walks them
 *   row_ovf_base_out  rows u32: the first overflow slot of a split row; bit 31 (the fold mark) set on the rows
 *                     k_fold_long_rows added up into their first record.  Words of rows that are not split are
 *                     UNSPECIFIED (nothing writes them)
 *   ovf_out           ovf_count x record_words u32: overflow records [ovf_first, ovf_first + ovf_count), which must lie
 *                     inside [0, overflow_slots) (MSM377_EINVAL otherwise).  The records of a row with the fold mark
 *                     hold the fold's intermediate sums; its first record is the sum of all its partials */
#define MSM377_WORK_HIST_BINS 129
#define MSM377_WORK_ROW_FOLDED 0x80000000u
typedef struct msm377_work_list_info {
  uint32_t seg, rows;
  uint64_t max_items;
  uint32_t quad;
  int32_t fold_slot;
  uint32_t record_words;
  int32_t form;
  uint32_t bucket_log;
  uint32_t items, split_rows, overflow_slots;
  uint32_t hist[MSM377_WORK_HIST_BINS];
  uint32_t reserved;
} msm377_work_list_info;
int msm377_g1_read_work_list(msm377_ctx* ctx, msm377_work_list_info* info, uint32_t* items_out, uint32_t* split_rows_out, uint32_t* row_ovf_base_out, uint64_t ovf_first,
                             uint64_t ovf_count, uint32_t* ovf_out);

/* ---- base records and window tables (what the hot kernels gather from) ----
 *
 * msm377_g1_read_bases describes and copies the base records the LAST CONVERSION of this context left: any G1 or
 * Edwards-BLS12 MSM entry point (a chunked host-buffer call: all its chunks), any msm377_g1_set_bases* call, a
 * window-partials call, and the Weierstrass rerun of any of them (the records then are the rerun's).  The layout is
 * written down on the host where the conversion is queued, so it holds whatever the capture mode is; a call that does not
 * use the read-back launches and allocates exactly what it did without it.  MSM377_ESTATE, and nothing written, before
 * the first conversion and after a converting call that returned an error (its conversion failed, or the records may be
 * half written: nothing is described until the next conversion succeeds).  `words` = NULL only fills `info`.
 *
 *   form           MSM377_BASES_*:
 *                    TE_PROJECTIVE  64 words: Y - X, Y + X, 2d T, 2 Z of csrc/te377.hpp (13 limbs each, canonical), 12 pad
 *                    TE_AFFINE      40 words: y - x, y + x (canonical), 2d x y (a lazy product below p + 2^354), 1 pad
 *                    WEIERSTRASS    32 words: x, y (13 limbs each, canonical), 6 pad
 *                    ED             32 words: y - x, y + x, 2d x y of Edwards-BLS12 (9 limbs each, canonical), 5 pad
 *                  every coordinate a Montgomery residue in 29-bit limbs (radix 2^406; 2^261 for ED); pad words are zero
 *   record_words   words per record
 *   limbs          limbs per coordinate (13, or 9)
 *   coords         coordinates per record (4, 3, 2, 3)
 *   n              points of the conversion
 *   windows        1, or the windows of a precomputed table (16, or 13 at 20-bit windows)
 *   window_stride  records per window: record w * window_stride + i is [2^offset_w] P_i, offset_w the sum of window_bits[0 .. w)
 *   window_bits[w] width of window w (0 beyond `windows`, and where windows == 1)
 *   glv            1: records n .. 2n - 1 are phi(P_i) = (BETA x_i, y_i)
 *   records        records the read-back addresses: windows * window_stride, 2 n behind the GLV front end, else n
 *   flagged        input points that came in with an infinity flag (MSM377_POINTS_MONT_FLAG): their records hold the generator
 * Records [first, first + count) go to `words`, record_words each; first + count <= records, else MSM377_EINVAL. */
#define MSM377_BASES_TE_PROJECTIVE 0
#define MSM377_BASES_TE_AFFINE 1
#define MSM377_BASES_WEIERSTRASS 2
#define MSM377_BASES_ED 3
typedef struct msm377_bases_info {
  uint32_t form, record_words, limbs, coords;
  uint64_t n;
  uint32_t windows, glv;
  uint64_t window_stride;
  uint64_t records;
  uint32_t flagged, reserved;
  uint32_t window_bits[16];
} msm377_bases_info;
int msm377_g1_read_bases(msm377_ctx* ctx, msm377_bases_info* info, uint64_t first, uint64_t count, uint32_t* words);

/* The window table of a batch operation: records of 32 words -- x[13], y[13] (canonical Montgomery limbs), an identity flag
 * (then x = y = 0) and 5 pad words.  Record w * 2^(c-1) + (d - 1) is [d 2^(c w)]B for w < W = ceil(256 / c), d = 1 .. 2^(c-1);
 * the last record, W 2^(c-1), is [2^(c W)]B, the carry's entry.
 *   which  MSM377_MUL_TABLE_SINGLE (msm377_g1_batch_mul*; index 0), _MULTI (slot `index` of msm377_g1_batch_mul_multi*),
 *          _GENERATOR (generator `index` of the resident set of msm377_g1_set_generators)
 *   info   width c, rows W + 1, records W 2^(c-1) + 1, and the table's key: the 96 wire bytes of its base (zero for a
 *          generator table: the set is not keyed)
 * Records [first, first + count) go to `words`; call with count = 0 and `words` = NULL to fill `info` alone.
 * MSM377_ESTATE, and nothing written, when that table is not valid (never built, a build that failed, a dropped set, an
 * index beyond the set).  The per-pass [1..8]P tables of the variable-base and pairwise calls are not window tables and are
 * not read from here: msm377_g1_read_walk_tables (below) copies the tables of the last pass. */
#define MSM377_MUL_TABLE_SINGLE 0
#define MSM377_MUL_TABLE_MULTI 1
#define MSM377_MUL_TABLE_GENERATOR 2
typedef struct msm377_mul_table_info {
  uint32_t width, rows;
  uint64_t records;
  uint8_t key[96];
} msm377_mul_table_info;
int msm377_g1_read_mul_table(msm377_ctx* ctx, uint32_t which, uint32_t index, msm377_mul_table_info* info, uint64_t first, uint64_t count, uint32_t* words);

/* ---- the stash of a batch call (what the walk kernels hand to the normalisation) ----
 *
 * msm377_read_walk_stash describes and copies what the LAST PASS of the last batch DEVICE call left in the stash: the
 * projective point of every output as its walk kernel stored it (k_bm_accumulate, k_bmm_accumulate, k_cr_accumulate and
 * k_cr_fold, k_bmv_accumulate, k_bl2_accumulate, k_edbm_accumulate, k_edbmv_accumulate, k_edbl2_accumulate, k_edbl_accumulate,
 * k_edcr_accumulate and k_edcr_fold) and the exclusive running products the up-sweep of the
 * normalisation (k_bm_up, k_edbm_up) put beside them.  It covers msm377_g1_batch_mul*, _batch_mul_multi*, _commit_rows*,
 * _batch_mul_var*, _batch_lincomb2* and msm377_ed_batch_mul_multi*, _batch_mul_var*, _batch_lincomb2*, _batch_lincomb*, _commit_rows*; a host-buffer call is one device call per piece of at
 * most 2^20 scalars, and the description is that of its last piece.  `info` is written down on the host beside the
 * launches it describes; a call that does not use the read-back launches and allocates exactly what it did without it.
 *
 *   kind           MSM377_WALK_*: the call
 *   form           MSM377_WALK_FORM_XYZZ: 52 point words X, Y, ZZ, ZZZ (13 limbs each) and 13 running-product words
 *                  MSM377_WALK_FORM_ED:   36 point words X, Y, T, Z (9 limbs each) and 9 running-product words
 *   point_words, product_words   52 and 13, or 36 and 9
 *   product_pad    3: the words the last 16-byte piece of a running product holds behind its limbs; they are zero
 *   n              outputs of the device call
 *   pass_offset, m the last pass: outputs pass_offset .. pass_offset + m - 1 of the call; stash point i is output pass_offset + i
 *   width          window width the pass walked: 8 or 16; 4 for the variable-base and the pairwise call
 *   k              bases, generators or terms per output: 1 (batch_mul, batch_mul_var), 2 (batch_lincomb2), else the call's k
 *   segments, stride   row commitments: the plan's segments and the stride the launches were given -- the partial sum of
 *                  segment g of row i is stash point g * stride + i.  Segment 0 holds the fold (k_cr_fold's sum over all
 *                  segments; the walk's own sum where segments == 1), segments 1 and up the partial sums the fold read and
 *                  left.  Edwards-BLS12 row commitments (k_edcr_fold, in groups of 16): segment 0 holds the row's sum;
 *                  when segments > 16, a segment g > 0 with g % 16 == 0 holds the sum of segments g .. min(segments, g + 16) - 1;
 *                  every other segment holds its own partial sum.  Running products exist for segment 0 only.
 *                  Every other call: segments 1, stride 0
 *
 * The stash contract (csrc/kernels/batch_mul.hpp, ed_batch_mul.hpp; tools/check_lazy_bounds.py NORMALISATION_OPERANDS):
 *   - XYZZ: limbs 0..11 of every coordinate below 2^29; X below 5p + 2^354, Y, ZZ, ZZZ below p + 2^354; ZZ^3 = ZZZ^2; a live
 *     point has ZZ and ZZZ non-zero mod p; the identity is X = 0, Y = the Montgomery 1, ZZ = ZZZ = 0, word for word;
 *   - ED: every coordinate canonical (below q), Z non-zero, T Z = X Y; the identity is any (0 : c : 0 : c);
 *   - running products: for thread tid of workgroup blk, whose outputs are blk * 1024 + j * 256 + tid, j < 4, the words of
 *     output j = 0 are the Montgomery 1, those of output j + 1 the lazy (XYZZ) or canonical (ED) Montgomery product of the
 *     words of output j with its ZZZ (Z), an identity counting as 1.
 *
 * Points [first, first + count) of segment `segment` go to `point_words` (count x point_words u32) and, where
 * `product_words` is not NULL, their running products to `product_words` (count x (product_words + product_pad) u32: the
 * limbs, then the pad words; segment 0 only: the up-sweep runs over the m outputs).  first + count <= m and segment < segments, else MSM377_EINVAL.  count = 0 with
 * NULL buffers fills `info` alone.
 *
 * MSM377_ESTATE, and nothing written: before the first batch call; after a batch call that returned an error or had
 * n = 0 (it ran no pass); after msm377_g1_set_generators or msm377_ed_set_generators (a table build goes through the stash).  A batch call forgets
 * the description when it starts and writes a new one when its last pass is through.  MSM, check and set-bases calls do
 * not touch the stash and leave the description valid.
 *
 * msm377_g1_read_walk_tables copies the per-point tables [1..8]P_i the last pass of a variable-base call (tables = 1) or of
 * a pairwise call (tables = 2: table 0 of the P_i, table 1 of the Q_i) walked: window-table records of 32 words (above;
 * a flagged input or an entry that is the identity: x = y = 0, flag 1).  In the engine entry e of point i of table t is
 * record ((t * 8) + e - 1) * m + i; the read-back writes entry e of point first + j at record (e - 1) * count + j of
 * `words` (entries * count * 32 u32).  MSM377_ESTATE as above, and after any batch call of another kind. */
#define MSM377_WALK_BATCH_MUL 1
#define MSM377_WALK_BATCH_MUL_MULTI 2
#define MSM377_WALK_COMMIT_ROWS 3
#define MSM377_WALK_BATCH_MUL_VAR 4
#define MSM377_WALK_BATCH_LINCOMB2 5
#define MSM377_WALK_ED_BATCH_MUL_MULTI 6
#define MSM377_WALK_ED_BATCH_MUL_VAR 7 /* k_edbmv_accumulate; its tables: msm377_ed_read_walk_tables */
#define MSM377_WALK_ED_BATCH_LINCOMB2 8 /* k_edbl2_accumulate: form ED, width 4, k 2; its two tables: msm377_ed_read_walk_table */
#define MSM377_WALK_ED_COMMIT_ROWS 9 /* k_edcr_accumulate and k_edcr_fold: form ED, the set's width, the call's k, the plan's segments */
#define MSM377_WALK_ED_BATCH_LINCOMB 10 /* k_edbl_accumulate: form ED, width 4, the call's k; its k tables: msm377_ed_read_walk_table */
#define MSM377_WALK_FORM_XYZZ 0
#define MSM377_WALK_FORM_ED 1
typedef struct msm377_walk_stash_info {
  uint32_t kind, form, point_words, product_words;
  uint64_t n, pass_offset, m;
  uint32_t width, k;
  uint32_t segments, product_pad;
  uint64_t stride;
} msm377_walk_stash_info;
int msm377_read_walk_stash(msm377_ctx* ctx, msm377_walk_stash_info* info, uint32_t segment, uint64_t first, uint64_t count, uint32_t* point_words, uint32_t* product_words);
typedef struct msm377_walk_tables_info {
  uint64_t m;
  uint32_t tables, entries;
} msm377_walk_tables_info;
int msm377_g1_read_walk_tables(msm377_ctx* ctx, msm377_walk_tables_info* info, uint32_t table, uint64_t first, uint64_t count, uint32_t* words);

/* Convert one Montgomery XYZZ point (52 words) to the affine wire format (host-only). */
int msm377_g1_xyzz_to_affine(const uint32_t xyzz[52], uint8_t out_xy[96]);

/* GLV front end of the Weierstrass form (msm377_ctx_set_g1_form 0) of the G1 full-MSM entry points:
 * k = k1 + k2 LAMBDA, 8 windows over the 2n points {P_i, phi(P_i)}.  OPT-IN:
 * phi(P) = [LAMBDA] P holds only in the prime-order subgroup, so mode 1 is a promise by the caller that every
 * input point lies in it (true for every protocol use; the reference makes no such assumption, hence the
 * default 0; 2 = the library's choice = 0).  Scalars outside the GLV range (>~ 2^254) rerun on the plain
 * 16-window path automatically.  1.24 vs 1.39 ms at 2^18, 3.51 vs 3.56 ms at 2^20, 12.4 vs 12.6 ms at 2^22. */
int msm377_ctx_set_glv(msm377_ctx* ctx, int mode);
/* The promise of mode 1 can be verified for resident base sets: with MSM377_CHECK_SUBGROUP among the flags of
 * msm377_ctx_set_base_checks, the msm377_g1_set_bases* calls refuse a set with a point outside the subgroup (MSM377_EPOINT). */

/* Internal coordinate system of the G1 full-MSM entry points (msm, msm_device, set_bases + fixed_base*); results
 * are identical.  form 1 (default): the twisted Edwards form of BLS12-377 G1 (csrc/te377.hpp) -- 7 field products per
 * bucket addition on affine base records (inputs of 2^20 points and more, resident tables), 8 on projective ones,
 * instead of the 10 of form 0, no case distinctions; inputs that hit an exceptional case of its addition law (only
 * possible with points outside the prime-order subgroup) rerun in form 0 automatically.  form 0: short Weierstrass
 * XYZZ coordinates behind the GLV front end selected by msm377_ctx_set_glv.  The window-partials entry points follow
 * the same setting and tag their records with the form they are in (form 1: twisted Edwards records; a shard that hit
 * an exceptional case, or form 0: Weierstrass records); the stage read-backs report theirs (msm377_ctx_get_stage_form). */
int msm377_ctx_set_g1_form(msm377_ctx* ctx, int form);

/* Small inputs: G1 full-MSM calls of at most `max_points` points (default and at most 2^16; 0 = never) run with
 * narrow windows -- 22 windows of 2 048 buckets (eleven signed 12-bit and eleven unsigned 11-bit digits per scalar)
 * instead of 16 of 32 768: 0.22-0.53 instead of 0.52-0.60 ms -- the
 * counterpart of the reference's switch to narrower windows for small inputs (src/submission/submission.ts:97: 4-bit
 * below 65 536 points).  Same results, and the error condition of the 16-bit recode for every input size (the reference's own
 * 4-bit branch rejects more NON-canonical scalars, k > 0x777...7; every k < r passes both); scalars of 2^253 and more rerun
 * on the 16-bit path. */
int msm377_ctx_set_narrow_max(msm377_ctx* ctx, uint64_t max_points);

/* How often this context had to rerun (part of) a call on the Weierstrass path because the twisted Edwards form hit
 * an exceptional case of its addition law, and where the last one surfaced (MSM377_FB_* bits).  Zero for inputs in
 * the prime-order subgroup; the parity tests use it to prove that each check fires. */
#define MSM377_FB_ACCUMULATE 4  /* a bucket addition in k_accumulate */
#define MSM377_FB_MERGE 8       /* the merge of a split row's partial sums */
#define MSM377_FB_TREE 16       /* a bucket-reduction level */
#define MSM377_FB_TAIL 32       /* the host tail (Horner over the partial records) */
#define MSM377_FB_CONVERT 64    /* an input point the Edwards model cannot represent (order 2 or 4) */
int msm377_ctx_get_fallback_info(const msm377_ctx* ctx, uint64_t* count, uint32_t* last_mask);

/* ---- fixed-base batch multiplication ------------------------------------------------------ */

/* out[i] = [s_i]B: n scalar multiples of ONE base point, each returned as its own affine point (arkworks' batch_mul /
 * FixedBase::msm: an SRS [tau^i]G, the G1 query vectors of a proving key, any base set for msm377_g1_set_bases*).  The
 * reference has no counterpart: it computes sums only.
 *
 * Meaning.  s_i is the integer its 32 bytes encode; every value in [0, 2^256) is accepted -- no MSM377_ESCALAR, no rerun
 * -- and it is NOT reduced mod r in the wire scalar form, because the answer is right for EVERY curve point B, not only
 * for the prime-order subgroup: bases of order 2, 3, 4, 6, of 2-power order, P + T.  Every exceptional case of the
 * addition formulas is followed through (csrc/kernels/batch_mul.hpp).
 *
 * Base and scalars.  base_xy is a HOST pointer, always the 96-byte wire format (the context's point form does not apply
 * to it), trusted like any MSM input except that a coordinate of p or more is MSM377_EINVAL.  The scalars follow the
 * context's SCALAR form (msm377_ctx_set_input_format): MSM377_SCALARS_WIRE, or MSM377_SCALARS_MONT (v 2^-256 mod r, fully
 * reduced, the product of the import pass).  msm377_g1_batch_mul_host takes wire scalars.
 *
 * Output.  out_form is MSM377_POINTS_WIRE or MSM377_POINTS_MONT_FLAG; plain MSM377_POINTS_MONT cannot say "identity" and
 * is MSM377_EINVAL.
 *   MSM377_POINTS_WIRE       96-byte records; an identity result is x = 0, y = 1 as compute_msm writes it.  (0, 1) is ALSO a
 *                            real point of order 3, so out_inf is the only unambiguous record.
 *   MSM377_POINTS_MONT_FLAG  104-byte records, byte for byte what msm377_g1_result_to_native makes of the wire record, but
 *                            with the flag set ONLY for a true identity; they can be handed straight to
 *                            msm377_g1_set_bases* on a context set to that point form.
 *   out_inf (may be NULL)    n bytes: 1 for the identity, 0 otherwise, in either form.
 *
 * Arguments.  Any n: 0 is MSM377_OK without a launch, and n may exceed the context's max_points (the scratch has a fixed
 * size, ~330 MB of device memory allocated by the first call, and the call walks n in chunks of 2^20).  Device pointers:
 * scalars and wire records 16-byte aligned, mont_flag records 8-byte aligned.  A null pointer with n > 0 or an unknown
 * form is MSM377_EINVAL with the outputs untouched.  The calls are synchronous: on return the outputs are complete.
 *
 * Table.  The call keeps a window table of the base on the context -- rows w = 0 .. ceil(256 / c) - 1 of [d 2^(c w)]B,
 * d = 1 .. 2^(c-1), signed digits pick the negative, plus [2^(c ceil(256 / c))]B for the carry out of the top window --
 * keyed by the 96 base bytes and the width c.  It is rebuilt only when either changes (msm377_ctx_get_mul_table_builds
 * counts the builds), is freed by msm377_ctx_destroy, and a failed build leaves none behind.  The resident MSM bases and
 * a check call's state are untouched by these calls, and the other way round.
 * Widths: c = 8 (33 additions per output, a 0.5 MB table) and c = 16 (17 additions, 64 MB).  msm377_ctx_set_mul_window:
 * 0 = the rule by n (default: 16 from 2^19 outputs on, else 8), 8 or 16 forces the width, anything else is
 * MSM377_EINVAL.  msm377_ctx_get_last_mul_window: the width the last batch_mul call ran, 0 before the first. */
int msm377_g1_batch_mul_device(msm377_ctx* ctx, const uint8_t base_xy[96], const void* d_scalars, uint64_t n, uint32_t out_form, void* d_out_points, uint8_t* d_out_inf);
int msm377_g1_batch_mul(msm377_ctx* ctx, const uint8_t base_xy[96], const uint8_t* scalars, uint64_t n, uint32_t out_form, uint8_t* out_points, uint8_t* out_inf);
/* The same on ONE CPU thread: no device, no context (csrc/batch_mul_host.hpp) -- small batches, and the yardstick of the
 * device call. */
int msm377_g1_batch_mul_host(const uint8_t base_xy[96], const uint8_t* scalars, uint64_t n, uint32_t out_form, uint8_t* out_points, uint8_t* out_inf);
int msm377_ctx_set_mul_window(msm377_ctx* ctx, int window_bits);
int msm377_ctx_get_last_mul_window(const msm377_ctx* ctx);
uint64_t msm377_ctx_get_mul_table_builds(const msm377_ctx* ctx);

/* ---- multi-base batch multiplication ------------------------------------------------------ */

/* out[i] = sum_{j<k} [s_ij]B_j: n outputs over a handful of fixed bases, each returned as its own affine point (Pedersen
 * commitments [m_i]G + [r_i]H, the second half of an ElGamal ciphertext [m_i]G + [r_i]PK, a hiding SRS
 * [tau^i]G + [rho_i]H, commitments to n short vectors over k generators).  Wherever the two overlap the contract is that
 * of msm377_g1_batch_mul* above -- the meaning of a scalar (every 32-byte value, a wire scalar NOT reduced mod r, no
 * MSM377_ESCALAR), the context's scalar form (the host twin takes wire scalars), bases as 96 wire bytes in HOST memory
 * with a coordinate of p or more MSM377_EINVAL, every curve point a legal base, the two output forms and out_inf, any n
 * in passes of 2^20 outputs over the same scratch, the alignment of device pointers, synchronous calls, MSM377_EINVAL
 * with the outputs untouched -- and this section states only what differs (csrc/kernels/batch_mul_multi.hpp).
 *
 * Bases and scalars.  bases_xy holds k records of 96 bytes, k = 1 .. MSM377_MUL_MAX_BASES.  s_ij is the 32 bytes at
 * scalars + i * out_stride + j * base_stride; both strides are byte counts and non-zero multiples of 32:
 *   row-major       out_stride = 32 k, base_stride = 32
 *   column-major    out_stride = 32,   base_stride = 32 n
 *   padded rows     out_stride > 32 k, base_stride = 32
 * Scalars are only read, so rows may overlap as the caller likes.  Any other k or stride is MSM377_EINVAL.  k = 1
 * returns byte for byte what msm377_g1_batch_mul* returns.
 *
 * Relations.  Every relation between the bases is legal and followed through: B_1 = B_0, B_1 = -B_0, B_1 = [m]B_0, bases
 * of order 2, 3, 4 and 6, an output of O with no term O.
 *
 * Width.  msm377_ctx_set_mul_window applies (0 = the rule, 8, 16) and msm377_ctx_get_last_mul_window reports the width
 * the call ran.  The rule of THIS call (csrc/batch_mul_recode.hpp batch_mul_multi_rule) depends on n and k.
 *
 * State.  MSM377_MUL_MAX_BASES table slots on the context, beside the single-base table: slot j holds the window table
 * of (the 96 bytes of the base at position j, the width).  A call reuses slot j < k if it is valid and both keys match
 * and rebuilds every other slot among j < k in ONE build (msm377_ctx_get_mul_multi_table_builds counts the slots
 * built); slots at k and above are left as they are; a failed build leaves the slots it touched invalid.  A slot's
 * memory (0.5 MB at c = 8, 64 MB at c = 16) is allocated when it is first built and freed by msm377_ctx_destroy.  The
 * resident MSM bases, the single-base table (msm377_ctx_get_mul_table_builds does not move), the variable-base table
 * memory and a check call's state are untouched by these calls, and the other way round.  msm377_g1_batch_mul_multi
 * accepts the same layouts in host memory, repacks them row-major and stages them through device memory in pieces of at
 * most 2^20 scalars. */
#define MSM377_MUL_MAX_BASES 16
int msm377_g1_batch_mul_multi_device(msm377_ctx* ctx, const uint8_t* bases_xy /* k x 96, HOST */, uint32_t k, const void* d_scalars, uint64_t n, uint64_t out_stride,
                                     uint64_t base_stride, uint32_t out_form, void* d_out_points, uint8_t* d_out_inf);
int msm377_g1_batch_mul_multi(msm377_ctx* ctx, const uint8_t* bases_xy, uint32_t k, const uint8_t* scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride,
                              uint32_t out_form, uint8_t* out_points, uint8_t* out_inf);
/* The same on ONE CPU thread: no device, no context (csrc/batch_mul_multi_host.hpp): the terms of each base by the
 * single-base twin, then general additions; the yardstick of the device call. */
int msm377_g1_batch_mul_multi_host(const uint8_t* bases_xy, uint32_t k, const uint8_t* scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, uint32_t out_form,
                                   uint8_t* out_points, uint8_t* out_inf);
uint64_t msm377_ctx_get_mul_multi_table_builds(const msm377_ctx* ctx);

/* ---- Edwards-BLS12 batch multiplication --------------------------------------------------- */

/* out[i] = sum_{j<k} [s_ij]B_j on Edwards-BLS12 (a = -1, d = 3021 over Fq, cofactor 4), k = 1 .. MSM377_MUL_MAX_BASES, every
 * output its own 64-byte wire point x || y: account addresses and view keys [sk_i]G, Pedersen-style record and value
 * commitments [m_i]G + [r_i]H, ElGamal halves, Schnorr nonces, batches of public keys.  k = 1 is the single-base call.
 * Wherever the two overlap the contract is that of msm377_g1_batch_mul_multi* above -- s_ij at
 * scalars + i * out_stride + j * base_stride with both strides non-zero multiples of 32, rows that may overlap, any n in
 * passes of 2^20 over the same scratch, 16-byte aligned device pointers, synchronous calls, MSM377_EINVAL with the outputs
 * untouched, n = 0 MSM377_OK without a launch, msm377_ctx_set_mul_window / msm377_ctx_get_last_mul_window -- and this
 * section states only what differs (csrc/kernels/ed_batch_mul.hpp).
 *
 * Scalars.  Every 32-byte value is a legal scalar, read as an integer and NOT reduced: no MSM377_ESCALAR, no rerun.  The
 * context's scalar form MSM377_SCALARS_MONT is defined for Fr, not for this curve: while any non-wire input form is set the
 * calls return MSM377_EINVAL, like every msm377_ed_* call.
 *
 * Bases.  bases_xy holds k records of 64 wire bytes in HOST memory.  Every curve point is a legal base and every relation
 * between bases is followed through: the identity (0, 1), the point of order 2, both points of order 4, P + T,
 * B_1 = +-B_0, B_1 = [m]B_0.  The addition law is complete ON THE CURVE, and the batched inversion relies on it, so the
 * bases are verified on the host before anything is launched: a coordinate of q or more, or a point off the curve, is
 * MSM377_EINVAL.
 *
 * Output.  64-byte wire records; the identity is (0, 1), an ordinary record.  There is no out_form and no flag bytes.
 *
 * State.  MSM377_MUL_MAX_BASES table slots of their own on the context, beside the G1 tables and independent of them: slot
 * j is keyed by (the 64 bytes of the base at position j, the width).  A call rebuilds, in ONE build, only the slots among
 * j < k whose key changed (msm377_ed_ctx_get_mul_table_builds counts the slots built); slots at k and above are left as
 * they are; a failed build leaves the slots it touched invalid; a slot's memory (0.5 MB at c = 8, 64 MB at c = 16) is
 * allocated at its first build and freed by msm377_ctx_destroy.  The resident MSM bases, every G1 table and build counter,
 * the generator set and a check call's state are untouched by these calls, and the other way round.  The width rule is
 * the G1 call's (csrc/batch_mul_recode.hpp batch_mul_multi_rule): inherited, not measured for this curve.
 *
 * msm377_ed_read_mul_table: slot `index` as msm377_g1_read_mul_table reads a G1 table, with records in the
 * MSM377_BASES_ED layout -- (y - x)[9], (y + x)[9], (2d x y)[9] canonical limbs in the Montgomery radix 2^261, then 5 zero
 * words; the identity is the ordinary record (1, 1, 0).  Record w * 2^(c-1) + (d - 1) is [d 2^(c w)]B, the last record
 * [2^(c W)]B.  info->key holds the 64 base bytes, then zeros.  MSM377_ESTATE when the slot is not valid, MSM377_EINVAL for
 * an index of MSM377_MUL_MAX_BASES or more. */
int msm377_ed_batch_mul_multi_device(msm377_ctx* ctx, const uint8_t* bases_xy /* k x 64, HOST */, uint32_t k, const void* d_scalars, uint64_t n, uint64_t out_stride,
                                     uint64_t base_stride, void* d_out_points);
int msm377_ed_batch_mul_multi(msm377_ctx* ctx, const uint8_t* bases_xy, uint32_t k, const uint8_t* scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride,
                              uint8_t* out_points);
/* The same on ONE CPU thread: no device, no context (csrc/ed_batch_mul_host.hpp): plain double-and-add per term, general
 * additions, one inversion per output; the yardstick of the device call. */
int msm377_ed_batch_mul_multi_host(const uint8_t* bases_xy, uint32_t k, const uint8_t* scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, uint8_t* out_points);
uint64_t msm377_ed_ctx_get_mul_table_builds(const msm377_ctx* ctx);
int msm377_ed_read_mul_table(msm377_ctx* ctx, uint32_t index, msm377_mul_table_info* info, uint64_t first, uint64_t count, uint32_t* words);

/* ---- Edwards-BLS12 variable-base batch multiplication -------------------------------------- */

/* out[i] = [s_i]P_i on Edwards-BLS12: n scalar multiples of n points, every output its own 64-byte wire point, with n
 * scalars or ONE scalar for all points (record scanning [view_key] nonce_i; the ElGamal / ECDH halves [r_i]PK_i).  Wherever
 * they overlap the contract is word for word that of msm377_ed_batch_mul_multi* above and of msm377_g1_batch_mul_var*
 * below -- 64-byte wire records x || y in and out, the identity the ordinary record (0, 1), no out_form and no flag bytes;
 * every 32-byte value a legal scalar, read as an integer and NOT reduced, no MSM377_ESCALAR, no rerun; scalar_stride 32, or
 * 0 for ONE 32-byte scalar for all points; any n, in passes of 2^17 over a fixed scratch, n = 0 MSM377_OK without a
 * launch; 16-byte aligned device pointers; synchronous calls; MSM377_EINVAL while a non-wire input form is set, for a
 * misaligned pointer, a null pointer with n > 0 or another stride, with the outputs untouched -- and this section states
 * only what differs (csrc/kernels/ed_batch_mul_var.hpp).
 *
 * Points.  Every curve point is a legal input, mixed freely within one array: the identity, the point of order 2, both
 * points of order 4, P + T for a subgroup point P and each torsion point T, P_i = +-P_j.  No subgroup test is run.  A point
 * that is NOT on the curve is refused: the addition law is complete on the curve only, and the one batched inversion of a
 * pass needs every Z non-zero, so a single bad point would corrupt every output of its pass.  Before anything is written
 * the device call runs the canonical + on-curve check over all n points (the kernel of msm377_ed_check_points*, into
 * counters of the call's own: the state of a check call is not touched); a finding is MSM377_EPOINT with the outputs
 * untouched, and msm377_last_error names the lowest failing index and the reason (a coordinate that is not below q / not
 * on the curve).  The host-buffer call works in pieces of 2^20 points: a call of several pieces runs the same check over
 * all of them first (its points go up twice), so that no piece has come down when a later one is refused.
 *
 * In place.  d_out_points == d_points is allowed: a pass reads its points before it writes its outputs, and passes cover
 * disjoint index ranges.  Any other overlap is the caller's bug.
 *
 * State.  The per-point tables [1..8]P_i of a pass live in the table memory of msm377_g1_batch_mul_var* (128 MB, allocated
 * by the first call of either, never valid between calls).  The resident MSM bases, every G1 table, slot and build counter,
 * the 16 Edwards-BLS12 table slots and msm377_ed_ctx_get_mul_table_builds, the generator set and a check call's state are
 * untouched, and the other way round.
 *
 * msm377_ed_read_walk_tables copies the per-point tables of the last pass as msm377_g1_read_walk_tables does for G1
 * (there is one table): entry e of point first + j at record (e - 1) * count + j of `words`, 32 words each in the
 * MSM377_BASES_ED layout of msm377_ed_read_mul_table.  MSM377_ESTATE after any batch call of another kind. */
int msm377_ed_batch_mul_var_device(msm377_ctx* ctx, const void* d_points /* n x 64 */, const void* d_scalars, uint64_t n, uint32_t scalar_stride /* 32 or 0 */,
                                   void* d_out_points /* n x 64 */);
int msm377_ed_batch_mul_var(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint32_t scalar_stride, uint8_t* out_points);
/* The same on ONE CPU thread: no device, no context (csrc/ed_batch_mul_var_host.hpp): the same checks and codes, plain
 * double-and-add on the canonical formulas, one inversion per output; the yardstick of the device call.  There is no
 * context to carry the text of a refusal: msm377_ed_check_points_host names the index and the reason. */
int msm377_ed_batch_mul_var_host(const uint8_t* points, const uint8_t* scalars, uint64_t n, uint32_t scalar_stride, uint8_t* out_points);
int msm377_ed_read_walk_tables(msm377_ctx* ctx, msm377_walk_tables_info* info, uint64_t first, uint64_t count, uint32_t* words);

/* ---- Edwards-BLS12 pairwise linear combination --------------------------------------------- */

/* out[i] = [a_i]P_i + [b_i]Q_i on Edwards-BLS12: n pairs of points, two scalars each, every output its own 64-byte wire
 * point (Schnorr verification R_i = [s_i]G + [c_i]PK_i; ElGamal decryption C2_i - [sk]C1_i and re-randomisation
 * [r_i]G + [r_i']PK_i; plain P_i + Q_i with a = b = 1).  Wherever they overlap the contract is word for word that of
 * msm377_ed_batch_mul_var* above and of msm377_g1_batch_lincomb2* below -- 64-byte wire records in and out, the identity
 * the record (0, 1), no out_form and no flag bytes; every 32-byte value a legal scalar, not reduced, no MSM377_ESCALAR, no
 * rerun; any n, n = 0 MSM377_OK without a launch; 16-byte aligned device pointers; synchronous calls; MSM377_EINVAL while
 * a non-wire input form is set, for a misaligned pointer, a null pointer with n > 0 or a stride outside its set, with the
 * outputs untouched -- and this section states only what differs (csrc/kernels/ed_batch_lincomb2.hpp).
 *
 * Strides.  a_stride and b_stride are each 32 or 0, p_stride and q_stride each 64 or 0; 0 means ONE scalar or ONE point
 * for all n pairs, and only its 32 or 64 bytes are read.  The four are independent: p_stride = 0 with q_stride = 64 is the
 * Schnorr shape.  (The G1 call has no point strides: the one deliberate difference in shape.)
 *
 * Points and relations.  Every curve point is a legal input in either array, mixed freely, and every relation between the
 * two is followed through by the complete law itself: Q_i = P_i, Q_i = -P_i, Q_i = [m]P_i, a sum of O from two terms that
 * are not O, both terms O.  No subgroup test is run.
 *
 * Refusal.  Before anything is written the device call runs the canonical + on-curve check over BOTH arrays (a stride-0
 * array is ONE point), into counters of the call's own; a finding is MSM377_EPOINT with the outputs untouched, and
 * msm377_last_error reads "point <i> of p ..." or "point <i> of q ...": the array, the lowest failing index in it, and the
 * reason.  Of a finding in each array the one with the lower index is reported; p where they are equal.  The host-buffer
 * call works in pieces of 2^20 pairs; a call of several pieces checks every piece of both arrays first, on the device.
 *
 * Overlap.  d_p and d_q are only read and may overlap or be the same pointer.  d_out_points may equal d_p or d_q where
 * that array's stride is 64, and the fold in place works (d_q = d_p + h records, d_out_points = d_p, n = h): a pass reads
 * all of its inputs before it writes its outputs, and passes cover disjoint index ranges.  d_out_points equal to the
 * pointer of a stride-0 array is MSM377_EINVAL.  Any other overlap is the caller's bug.
 *
 * State.  Passes are 2^16 pairs: both per-point tables [1..8]P_i and [1..8]Q_i of a pass, 16 x 2^16 records, are exactly
 * the table memory of msm377_g1_batch_mul_var* (128 MB, never valid between calls) and one normalisation chunk.  The
 * resident MSM bases, every G1 table, slot and build counter, the 16 Edwards-BLS12 table slots and
 * msm377_ed_ctx_get_mul_table_builds, the generator set and a check call's state are untouched, and the other way round.
 *
 * msm377_ed_read_walk_table copies table `table` of the last pass (0: of the P_i, 1: of the Q_i; info.tables = 2), records
 * as msm377_ed_read_walk_tables above, which is table 0 of it and stays valid after a variable-base call (tables = 1).  A
 * stride-0 array's table holds the same eight records for every i.  msm377_g1_read_walk_tables is MSM377_ESTATE after
 * this call.  After msm377_ed_batch_lincomb* it answers with info.tables = k, the call's terms (below). */
int msm377_ed_batch_lincomb2_device(msm377_ctx* ctx, const void* d_p, const void* d_q, const void* d_a, const void* d_b, uint64_t n, uint32_t p_stride /* 64 or 0 */,
                                    uint32_t q_stride /* 64 or 0 */, uint32_t a_stride /* 32 or 0 */, uint32_t b_stride /* 32 or 0 */, void* d_out_points /* n x 64 */);
int msm377_ed_batch_lincomb2(msm377_ctx* ctx, const uint8_t* p, const uint8_t* q, const uint8_t* a, const uint8_t* b, uint64_t n, uint32_t p_stride, uint32_t q_stride, uint32_t a_stride,
                             uint32_t b_stride, uint8_t* out_points);
/* The same on ONE CPU thread: no device, no context (csrc/ed_batch_lincomb2_host.hpp): the same checks and codes, each term
 * by plain double-and-add on the canonical formulas, then one addition and one inversion per output; the yardstick of the
 * device call.  There is no context to carry the text of a refusal: msm377_ed_check_points_host names index and reason. */
int msm377_ed_batch_lincomb2_host(const uint8_t* p, const uint8_t* q, const uint8_t* a, const uint8_t* b, uint64_t n, uint32_t p_stride, uint32_t q_stride, uint32_t a_stride,
                                  uint32_t b_stride, uint8_t* out_points);
int msm377_ed_read_walk_table(msm377_ctx* ctx, msm377_walk_tables_info* info, uint32_t table, uint64_t first, uint64_t count, uint32_t* words);

/* ---- Edwards-BLS12 k-term linear combination ----------------------------------------------- */

/* out[i] = sum_{j<k} [s_ij]P_ij on Edwards-BLS12, 1 <= k <= MSM377_LINCOMB_MAX_TERMS: n outputs, every one its own 64-byte
 * wire point, every term its own array of points and of scalars (a Schnorr check as one sum [s_i]G - [c_i]PK_i - R_i
 * compared with O; both halves of a Chaum-Pedersen / DLEQ proof; address derivation pk_sig_i + pr_sig_i + [sk_prf_i]G;
 * ElGamal re-encryption [r_i]G + [r_i']PK_i + C_i; a random linear combination of a few key vectors).  Per term the
 * contract is word for word that of msm377_ed_batch_lincomb2* above -- 64-byte wire records in and out, the identity the
 * record (0, 1); every 32-byte value a legal scalar, not reduced; any n, n = 0 MSM377_OK without a launch once the shape
 * has been checked; 16-byte aligned device pointers; synchronous calls; MSM377_EINVAL while a non-wire input form is set,
 * for a misaligned pointer, a null pointer with n > 0 or a stride outside its set, with the outputs untouched -- and this
 * section states only what differs (csrc/kernels/ed_batch_lincomb.hpp).
 *
 * Terms.  `terms` points to k descriptors in HOST memory; the pointers inside are device pointers (_device) or host
 * pointers (the other two).  point_stride is 64 or 0, scalar_stride 32 or 0; 0 means ONE point or ONE scalar for all n
 * outputs, and only its 64 or 32 bytes are read.  All strides are independent: term 0 a stride-0 point and term 2 a
 * stride-0 scalar is the Schnorr check as one sum.  k = 0, k above MSM377_LINCOMB_MAX_TERMS and a null `terms` are
 * MSM377_EINVAL, whatever n.
 *
 * Points and relations.  Every curve point is a legal input in every term, mixed freely, and every relation among the k
 * points of one output is followed through by the complete law itself: P_ij = +-P_ij', one term a multiple of another, a
 * sum of O from terms none of which is O, every term O.  No subgroup test is run.
 *
 * Refusal.  Before anything is written the device call runs the canonical + on-curve check over the points of every term
 * (a stride-0 term is ONE point), into k sets of counters of the call's own; a finding is MSM377_EPOINT with the outputs
 * untouched, and msm377_last_error reads "point <i> of term <j> ...": the lowest failing index, the term, and the reason.
 * Of several findings the one with the lowest index is reported; among equal indices the lowest term.  The host-buffer
 * call works in pieces of 2^20 outputs; a call of several pieces checks every piece of every term first, on the device.
 *
 * Overlap.  Point arrays are only read and may overlap or be the same pointer.  d_out_points may equal any term's points
 * where that term's point_stride is 64, and the fold in place works: a pass reads all of its inputs before it writes its
 * outputs, and passes cover disjoint index ranges.  d_out_points equal to the pointer of a stride-0 point is
 * MSM377_EINVAL.  Any other overlap is the caller's bug.
 *
 * State.  A pass is 2^16 outputs whatever k.  The per-point tables [1..8]P_ij of a pass, k x 2^19 records of 128 bytes
 * (k x 64 MB), are ONE allocation of this call's own: it grows when a call brings a larger k, never shrinks, is released
 * by msm377_ctx_destroy and is never valid between calls.  The table memory of msm377_g1_batch_mul_var*, the resident MSM
 * bases, every G1 table, slot and build counter, the 16 Edwards-BLS12 table slots and msm377_ed_ctx_get_mul_table_builds,
 * both generator sets and a check call's state are untouched, and the other way round.
 *
 * k = 1 and k = 2 run this call's own kernels; their outputs are byte for byte those of msm377_ed_batch_mul_var_device and
 * msm377_ed_batch_lincomb2_device, which remain the calls to use for one and two terms.
 *
 * msm377_read_walk_stash answers with kind MSM377_WALK_ED_BATCH_LINCOMB (form ED, width 4, k the call's k): stash point i
 * is the sum of output pass_offset + i.  msm377_ed_read_walk_table answers with info.tables = k and copies table t < k,
 * records as after the pairwise call: entry e of term t of output i is record ((t * 8) + e - 1) * m + i of the engine's
 * tables, m the outputs of the pass.  msm377_ed_read_walk_tables is table 0 of it; msm377_g1_read_walk_tables is
 * MSM377_ESTATE after this call. */
#define MSM377_LINCOMB_MAX_TERMS 8
typedef struct msm377_lincomb_term {
  const void* points;      /* n x 64-byte wire records, or ONE record (point_stride 0) */
  const void* scalars;     /* n x 32 bytes, or ONE scalar (scalar_stride 0)           */
  uint32_t point_stride;   /* 64 or 0 */
  uint32_t scalar_stride;  /* 32 or 0 */
} msm377_lincomb_term;
/* out[i] = sum_{j<k} [s_ij]P_ij.  terms: k descriptors in HOST memory; the pointers inside are device pointers */
int msm377_ed_batch_lincomb_device(msm377_ctx* ctx, const msm377_lincomb_term* terms, uint32_t k, uint64_t n, void* d_out_points);
int msm377_ed_batch_lincomb(msm377_ctx* ctx, const msm377_lincomb_term* terms /* host pointers */, uint32_t k, uint64_t n, uint8_t* out_points);
/* The same on ONE CPU thread: no device, no context (csrc/ed_batch_lincomb_host.hpp): the same checks and codes, each term
 * by plain double-and-add on the canonical formulas, the terms added in order, one inversion per output; the yardstick of
 * the device call.  There is no context to carry the text of a refusal: msm377_ed_check_points_host names index and reason. */
int msm377_ed_batch_lincomb_host(const msm377_lincomb_term* terms, uint32_t k, uint64_t n, uint8_t* out_points);

/* ---- variable-base batch multiplication --------------------------------------------------- */

/* out[i] = [s_i]P_i: n scalar multiples of n points, each returned as its own affine point (an SRS or powers-of-tau
 * update [tau^i]P_i, key specialisation [delta^-1]L_i, each half of an inner-product basis fold).  Wherever the two
 * overlap the contract is that of msm377_g1_batch_mul* above -- the meaning of a scalar (every 32-byte value, a wire scalar
 * NOT reduced mod r, no MSM377_ESCALAR, no rerun), the context's scalar form, the two output forms and out_inf, any n in
 * passes over a fixed scratch, synchronous calls, MSM377_EINVAL with the outputs untouched -- and this section states only
 * what differs (csrc/kernels/batch_mul_var.hpp).
 *
 * Points.  They follow the context's POINT form (msm377_ctx_set_input_format): MSM377_POINTS_WIRE, MSM377_POINTS_MONT or
 * MSM377_POINTS_MONT_FLAG.  A flagged record is the identity: its coordinate bytes are never interpreted, its output is
 * the identity with out_inf = 1.  Every curve point is a legal input, mixed freely within one array: orders 2, 3, 4 and
 * 6, points outside the prime-order subgroup, P + T.  Coordinates of p or more are trusted not to occur, as in the MSM
 * calls.
 *
 * Scalars.  scalar_stride is 32 (one scalar per point) or 0 (ONE scalar for all n points: 32 bytes are read); any other
 * value is MSM377_EINVAL.
 *
 * Arguments.  Device pointers: scalars and 96-byte records 16-byte aligned, 104-byte records 8-byte aligned, inputs
 * and outputs alike; a misaligned pointer is MSM377_EINVAL.  d_out_points == d_points is allowed when input and
 * output records have the same size (wire to wire, mont_flag to mont_flag); ANY other overlap of an output with an input
 * or with the other output is the caller's bug and the result is undefined.
 *
 * State.  The call walks n in passes of 2^17 points; per pass it builds the table [1..8]P_i of every point (128 MB of
 * device memory beside the batch_mul scratch, allocated by the first call, freed by msm377_ctx_destroy, never valid
 * between calls).  The resident MSM bases, the batch_mul window table (msm377_ctx_get_mul_table_builds does not move)
 * and a check call's state are untouched by these calls, and the other way round.  msm377_g1_batch_mul_var stages host
 * buffers through device memory in pieces of 2^20 points. */
int msm377_g1_batch_mul_var_device(msm377_ctx* ctx, const void* d_points, const void* d_scalars, uint64_t n, uint32_t scalar_stride, uint32_t out_form, void* d_out_points,
                                   uint8_t* d_out_inf);
int msm377_g1_batch_mul_var(msm377_ctx* ctx, const uint8_t* points, const uint8_t* scalars, uint64_t n, uint32_t scalar_stride, uint32_t out_form, uint8_t* out_points,
                            uint8_t* out_inf);
/* The same on ONE CPU thread: no device, no context (csrc/batch_mul_var_host.hpp): plain double-and-add, the yardstick of
 * the device call.  The forms are arguments here. */
int msm377_g1_batch_mul_var_host(const uint8_t* points, uint32_t point_form, const uint8_t* scalars, uint32_t scalar_form, uint64_t n, uint32_t scalar_stride,
                                 uint32_t out_form, uint8_t* out_points, uint8_t* out_inf);

/* ---- pairwise linear combination ---------------------------------------------------------- */

/* out[i] = [a_i]P_i + [b_i]Q_i: n combinations of n pairs of points, each returned as its own affine point (a basis fold
 * G'_i = [x^-1]G_i + [x]G_{i+n/2} of an inner-product argument, an SRS update with a blinding term, a random linear
 * combination of two key vectors; with a = b = 1, plain P_i + Q_i).  Wherever the two overlap the contract is that of
 * msm377_g1_batch_mul_var* above -- the meaning of a scalar (every 32-byte value, a wire scalar NOT reduced mod r, no
 * MSM377_ESCALAR), the context's scalar form for BOTH scalars and its point form for BOTH point arrays (a flagged record
 * is the identity, its coordinate bytes are never interpreted), every curve point a legal input in either array, the two
 * output forms and out_inf, any n, the alignment of device pointers (all four inputs and the output), synchronous calls,
 * MSM377_EINVAL with the outputs untouched -- and this section states only what differs (csrc/kernels/batch_lincomb2.hpp).
 *
 * Scalars.  a_stride and b_stride are each, independently, 32 (one scalar per pair) or 0 (ONE scalar for all n pairs: 32
 * bytes are read); any other value is MSM377_EINVAL.
 *
 * Relations.  Every relation between the two arrays is legal and followed through: Q_i = P_i, Q_i = -P_i, Q_i a multiple
 * of P_i, a result of O with P_i != +-Q_i.
 *
 * Overlap.  d_p and d_q are only read: they may overlap or be the same pointer.  d_out_points may equal d_p OR equal d_q
 * when input and output records have the same size.  A pass reads all of its inputs before it writes, and passes cover
 * disjoint index ranges, so a fold in place works: d_p = G, d_q = G + h records, d_out_points = G, n = h.  ANY other
 * overlap of an output with an input or with the other output is the caller's bug and the result is undefined.
 *
 * State.  The call walks n in passes of 2^16 pairs; per pass it builds the tables [1..8]P_i and [1..8]Q_i in the table
 * memory of msm377_g1_batch_mul_var* (allocated by the first call of either, never valid between calls): one joint walk
 * of 3 584 field products per output instead of two walks of 2 944 and an addition.  The resident MSM bases, the
 * batch_mul window table (msm377_ctx_get_mul_table_builds does not move) and a check call's state are untouched by these
 * calls, and the other way round.  msm377_g1_batch_lincomb2 stages host buffers through device memory in pieces of 2^20
 * pairs; a stride-0 scalar is uploaded once. */
int msm377_g1_batch_lincomb2_device(msm377_ctx* ctx, const void* d_p, const void* d_q, const void* d_a, const void* d_b, uint64_t n, uint32_t a_stride, uint32_t b_stride,
                                    uint32_t out_form, void* d_out_points, uint8_t* d_out_inf);
int msm377_g1_batch_lincomb2(msm377_ctx* ctx, const uint8_t* p, const uint8_t* q, const uint8_t* a, const uint8_t* b, uint64_t n, uint32_t a_stride, uint32_t b_stride,
                             uint32_t out_form, uint8_t* out_points, uint8_t* out_inf);
/* The same on ONE CPU thread: no device, no context (csrc/batch_lincomb2_host.hpp): each term by plain double-and-add,
 * then one general addition; the yardstick of the device call.  The forms are arguments here. */
int msm377_g1_batch_lincomb2_host(const uint8_t* p, const uint8_t* q, uint32_t point_form, const uint8_t* a, const uint8_t* b, uint32_t scalar_form, uint64_t n, uint32_t a_stride,
                                  uint32_t b_stride, uint32_t out_form, uint8_t* out_points, uint8_t* out_inf);

/* ---- row commitments ---------------------------------------------------------------------- */

/* out[i] = sum_{j<k} [s_ij]G_j: n row commitments over a RESIDENT set of up to MSM377_GEN_MAX generators, each returned as
 * its own affine point (Pedersen vector commitments: the rows of a Hyrax / Spartan-style polynomial commitment, the
 * per-row commitments of a witness matrix, n ElGamal-style vectors over 32 or 64 generators).  It fills the gap between
 * msm377_g1_batch_mul_multi* (k <= 16) and one MSM pipeline pass per row.  Wherever the two overlap the contract is that
 * of msm377_g1_batch_mul_multi* above, word for word -- the meaning of a scalar (every 32-byte value, a wire scalar NOT
 * reduced mod r, no MSM377_ESCALAR), the context's scalar form (the host twin takes it as an argument), s_ij at
 * scalars + i * out_stride + j * base_stride with both strides non-zero multiples of 32 (rows may overlap), every curve
 * point a legal generator and every relation between generators followed through, the two output forms and out_inf, the
 * alignment of device pointers, any n, synchronous calls, MSM377_EINVAL with the outputs untouched -- and this section
 * states only what differs (csrc/kernels/commit_rows.hpp, csrc/commit_rows_plan.hpp).
 *
 * The set.  msm377_g1_set_generators builds and keeps the window tables of k generators (96 wire bytes each, HOST
 * memory; a coordinate of p or more is MSM377_EINVAL).  window_bits: 8, 16 (k <= MSM377_GEN_WIDE_MAX only) or 0 = 8; the
 * width belongs to the set and msm377_ctx_set_mul_window does not apply.  The call follows the rule of the resident base
 * table: it drops the old set FIRST, whatever its arguments, and installs the new one as its last step; a call that
 * fails for any reason leaves no set.  gens_xy == NULL or k == 0 drops the set and frees its memory (MSM377_OK).  The
 * set is ONE allocation of k tables: 0.5 MB per generator at width 8 (2 GB at 4 096), 64 MB per generator at width 16;
 * msm377_ctx_destroy frees it.  It is independent of the resident MSM bases, the single-base table, the 16 multi-base
 * slots and both build counters, the variable-base table memory and a check call's state, in both directions.
 * msm377_ctx_get_generators reports (k, width) of the set, (0, 0) without one.
 *
 * The calls.  msm377_g1_commit_rows* run over the FIRST k generators of the set, 1 <= k <= the resident k.  Without a set,
 * or with k above the resident k (and within MSM377_GEN_MAX), they return MSM377_ESTATE; argument errors are reported
 * first, and n == 0 is MSM377_OK with or without a set.  With a resident k of 1 the outputs are byte for byte those of
 * msm377_g1_batch_mul_device at the set's width.  A row's walk is split across ceil(k / 16) threads whose partial sums
 * are folded by general additions (msm377_commit_rows_plan: segments, generators per segment, rows per pass of the 2^20
 * partial sums the scratch of the batch calls holds).  msm377_g1_commit_rows accepts the same layouts in host memory,
 * repacks them row-major and stages them in pieces of at most 2^20 scalars.
 *
 * Against one MSM per row (msm377_g1_set_bases once, then msm377_g1_msm_fixed_base_batch_device with n = k and batch =
 * rows), measured on one MI355X at width 8 (profiles/commit_rows/sweep.txt): the call takes 9.9 / 5.8 / 6.1 / 6.5 / 8.8 ms
 * for 2^16 x 32 / 2^14 x 64 / 2^12 x 256 / 2^10 x 1 024 / 2^8 x 4 096 full-width scalars where one MSM per row takes
 * 0.16 to 0.29 ms per ROW (10.5 s .. 72 ms).  The crossover: at k = 4 096 a call costs 8 to 10 ms however few the rows
 * (one thread walks 16 tables, one thread folds 256 partial sums), so below about 32 rows one MSM per row is the faster
 * way (16 rows: 4.9 against 9.8 ms; 64 rows: 18.5 against 8.2 ms). */
#define MSM377_GEN_MAX      4096   /* generators of a resident set */
#define MSM377_GEN_WIDE_MAX   64   /* ... of a set with 16-bit tables (64 MB each) */
int msm377_g1_set_generators(msm377_ctx* ctx, const uint8_t* gens_xy /* k x 96, HOST */, uint32_t k, int window_bits);
int msm377_ctx_get_generators(const msm377_ctx* ctx, uint32_t* k, int* window_bits);
int msm377_g1_commit_rows_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t k, uint64_t out_stride, uint64_t base_stride, uint32_t out_form, void* d_out_points,
                                 uint8_t* d_out_inf);
int msm377_g1_commit_rows(msm377_ctx* ctx, const uint8_t* scalars, uint64_t n, uint32_t k, uint64_t out_stride, uint64_t base_stride, uint32_t out_form, uint8_t* out_points,
                          uint8_t* out_inf);
/* The same on ONE CPU thread: no device, no context, the generators an argument (csrc/commit_rows_host.hpp): the terms of
 * each generator by the single-base twin, then general additions; the yardstick of the device call.  The forms are
 * arguments as in msm377_g1_batch_mul_var_host. */
int msm377_g1_commit_rows_host(const uint8_t* gens_xy, uint32_t k, const uint8_t* scalars, uint32_t scalar_form, uint64_t n, uint64_t out_stride, uint64_t base_stride,
                               uint32_t out_form, uint8_t* out_points, uint8_t* out_inf);
/* Pure, host-only: how a call over k generators is cut.  0 segments (and zeros) for k outside 1 .. MSM377_GEN_MAX.  Any of
 * the three pointers may be null. */
void msm377_commit_rows_plan(uint32_t k, uint32_t* segments, uint32_t* bases_per_segment, uint64_t* rows_per_pass);

/* ---- Edwards-BLS12 row commitments -------------------------------------------------------- */

/* out[i] = sum_{j<k} [s_ij]G_j over the FIRST k generators of a resident Edwards-BLS12 set of up to MSM377_GEN_MAX
 * generators, every output its own 64-byte wire record x || y (Pedersen and BHP-style hashes, vector commitments: sums
 * over hundreds to thousands of fixed generators, one per record, Merkle node or witness row).  The contract is that of
 * msm377_g1_commit_rows* above wherever that applies to this curve, and that of msm377_ed_batch_mul_multi* for everything
 * about the curve; this section states the two lists and what differs (csrc/kernels/ed_commit_rows.hpp).
 *
 * From msm377_g1_commit_rows*.  The set is resident: msm377_ed_set_generators drops the old set FIRST and installs the new
 * one as its last step, behind the wait for the build; a call that fails leaves none; gens_xy == NULL or k == 0 drops the
 * set and frees it (MSM377_OK).  window_bits is 8, 16 (k <= MSM377_GEN_WIDE_MAX only) or 0 = 8; another width, or a k
 * above the limits, is MSM377_EINVAL.  The set is ONE allocation, table j at record j * (records of a table), 128-byte
 * records in the MSM377_BASES_ED layout msm377_ed_read_mul_table documents.  The calls return MSM377_ESTATE without a
 * set or with k above the resident k; the shape (k, both strides: non-zero multiples of 32) is checked first, also for
 * n = 0, and n = 0 is MSM377_OK with nothing launched.  s_ij is the 32 bytes at scalars + i * out_stride + j *
 * base_stride: rows, columns, padded and sliding layouts all work.  A pass is msm377_commit_rows_plan(k)'s rows_per_pass
 * rows long -- the one plan of both curves -- and the host-buffer call works in pieces of 2^20 / k rows, repacked
 * row-major.  The width belongs to the set: msm377_ctx_set_mul_window does not apply and
 * msm377_ctx_get_last_mul_window is unchanged by these calls.  With a resident k of 1 the outputs are byte for byte those
 * of msm377_ed_batch_mul_multi_device with k = 1 at the set's width.
 *
 * From msm377_ed_batch_mul_multi*.  Every 32-byte value is a legal scalar, read as an integer and NOT reduced: no
 * MSM377_ESCALAR, no rerun.  No out_form, no flag bytes: the identity is the record (0, 1).  Device pointers are 16-byte
 * aligned.  msm377_ed_set_generators, msm377_ed_commit_rows_device and msm377_ed_commit_rows return MSM377_EINVAL while
 * a non-wire input form is set, and change nothing.  Every curve point is a legal generator -- the identity, the point of
 * order 2, both points of order 4, P + T, G_j = +-G_i, G_j = [m]G_i -- and every relation is followed through by the
 * complete addition law: a row sum of O from partial sums that are not O, relations across the threads that share a row.
 *
 * Generators that are not on the curve.  msm377_ed_set_generators uploads the k generators and runs the canonical +
 * on-curve check over them on the DEVICE (no subgroup test).  A finding is MSM377_EPOINT with no set afterwards;
 * msm377_last_error names the lowest failing index ("point <i> of the generators ...") and the reason.  This differs on
 * purpose from msm377_ed_batch_mul_multi*, which checks its at most 16 bases on the host and returns MSM377_EINVAL: the
 * host check takes 11 us per point, about 45 ms at 4 096 generators.  The host twin checks on the host and returns
 * MSM377_EPOINT too.
 *
 * State.  The set is a second one on the context, independent of G1's: both may be resident at once, and setting,
 * dropping or failing one leaves the other alone.  The set, the resident MSM bases, every G1 table, slot and counter, the
 * 16 Edwards-BLS12 slots with msm377_ed_ctx_get_mul_table_builds, and a check call's state are mutually untouched.
 * msm377_ed_ctx_get_generators reports (k, width), (0, 0) without a set.  msm377_ed_read_generator_table reads generator
 * `index`'s table as msm377_ed_read_mul_table reads a slot, with a zero key; MSM377_ESTATE without a set or for an index
 * beyond it.
 *
 * The fold.  A row's walk is split across S = ceil(k / 16) threads as on G1; their partial sums are folded in groups of 16:
 * one launch adds segments 16 h .. 16 h + 15 into segment 16 h, and for S > 16 a second one adds segments 0, 16, 32, ..
 * into segment 0 (30 dependent additions at k = 4 096 where G1's chain has 255).  Addition is associative and the outputs
 * are normalised, so the order does not show in the bytes.  What msm377_read_walk_stash finds after a pass: above.
 *
 * The same on ONE CPU thread (csrc/ed_commit_rows_host.hpp): every term by plain double-and-add on the canonical
 * formulas, added in the order j = 0 .. k - 1, one inversion per output; k = 1 .. MSM377_GEN_MAX; refusals leave the
 * outputs untouched. */
int msm377_ed_set_generators(msm377_ctx* ctx, const uint8_t* gens_xy /* k x 64, HOST */, uint32_t k, int window_bits);
int msm377_ed_ctx_get_generators(const msm377_ctx* ctx, uint32_t* k, int* window_bits);
int msm377_ed_commit_rows_device(msm377_ctx* ctx, const void* d_scalars, uint64_t n, uint32_t k, uint64_t out_stride, uint64_t base_stride, void* d_out_points);
int msm377_ed_commit_rows(msm377_ctx* ctx, const uint8_t* scalars, uint64_t n, uint32_t k, uint64_t out_stride, uint64_t base_stride, uint8_t* out_points);
int msm377_ed_commit_rows_host(const uint8_t* gens_xy, uint32_t k, const uint8_t* scalars, uint64_t n, uint64_t out_stride, uint64_t base_stride, uint8_t* out_points);
int msm377_ed_read_generator_table(msm377_ctx* ctx, uint32_t index, msm377_mul_table_info* info, uint64_t first, uint64_t count, uint32_t* words);

/* ---- measurement ------------------------------------------------------------------------ */

#define MSM377_STAGE_CONVERT 0     /* points -> Montgomery records */
#define MSM377_STAGE_DECOMPOSE 1   /* scalars -> signed 16-bit digits */
#define MSM377_STAGE_SORT 2        /* histogram + scan + scatter (CSR build) */
#define MSM377_STAGE_ACCUMULATE 3  /* bucket accumulation (SMVP) -- the dominant kernel */
#define MSM377_STAGE_REDUCE 4      /* bucket reduction tree */
#define MSM377_STAGE_TAIL 5        /* D2H of the partial records + host Horner/inversion */
#define MSM377_STAGE_ACC_KERNEL 6  /* the k_accumulate launch alone (inside STAGE_ACCUMULATE, which also
                                      covers the work-list kernels and the split-row merge) */
#define MSM377_NUM_STAGES 7
/* HIP-event timing on the context's streams (off by default).  enabled = 1: every stage; 2: the accumulation
 * kernel alone (MSM377_STAGE_ACC_KERNEL; the other entries read 0).  Every event pair costs a few microseconds of
 * GPU idle time between the launches it separates -- ~50 us per MSM with all stages on -- so a timed loop that only
 * needs the kernel's duration uses 2.  A msm377_*_check_points* call with enabled = 1 reports its curve kernel as
 * MSM377_STAGE_CONVERT and its subgroup kernel as MSM377_STAGE_ACC_KERNEL (the other entries read 0). */
int msm377_ctx_set_timing(msm377_ctx* ctx, int enabled);
/* Durations in milliseconds of the last call's stages (MSM377_NUM_STAGES entries; the TAIL
 * entry is host wall time). */
int msm377_ctx_get_stage_ms(msm377_ctx* ctx, double* ms_out);
/* Field products per bucket addition of the last accumulation launch (10 Weierstrass XYZZ, 8 twisted Edwards with
 * projective base records, 7 with affine ones): bench.py prices the int32 multiply-add roof with it. */
int msm377_ctx_get_products_per_addition(const msm377_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* MSM377_H */
