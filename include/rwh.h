/*
 * rwh.h -- C ABI of librwh_hip.so: MI355X (gfx950) kernels for the
 * RANSAC-homography + backward-warp hot path of choice17/ransac_with_homography.
 *
 * The reference is pure Python/numpy and has no FFI of its own; the boundary a
 * maintainer would bind (ctypes) is the set of numpy calls on its hot path.
 * Each entry point below names the reference lines it replaces.  All pointers
 * named `d_*` are DEVICE pointers; everything else is host memory read before
 * the function returns.  `stream` is a hipStream_t (NULL = default stream).
 * Functions enqueue work and return without synchronising, except where an entry
 * point says otherwise (rwh_ransac_run, rwh_sequence_seams*); they allocate
 * nothing and keep no state, so they may be captured into a hipGraph.
 *
 * Return value: 0 on success, a negative RWH_E_* code otherwise (never throws).
 */
#ifndef RWH_H
#define RWH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RWH_ABI_VERSION 5   /* 5: rwh_settle_decide and its two callback types (additive);
                               4: rwh_stitch_panorama_ex and the element types after RWH_F64 (additive);
                               3 (round 4): rwh_ransac_run takes hyp_base and returns packed keys, RWH_HYP_DEGENERATE, rwh_score_interval;
                               2: blend modes of rwh_stitch_panorama, RWH_BATCH_EARLY_STOP (d_counts may hold -1), rwh_lab_clock_probe, RWH_HYP_ILLCOND */
#define RWH_API __attribute__((visibility("default")))

enum {
    RWH_OK = 0,
    RWH_E_INVALID = -1,      /* bad argument (NULL pointer, size <= 0, unknown enum) */
    RWH_E_UNSUPPORTED = -2,  /* valid but not implemented combination (dtype / channels) */
    RWH_E_LAUNCH = -3        /* HIP reported a launch / memset failure */
};

/* element types of image planes (the codes after RWH_F64 are taken by rwh_stitch_panorama_ex and by the exact warps,
   rwh_warp_backward with RWH_WARP_EXACT and rwh_sample_points; a bool plane is RWH_U8) */
enum { RWH_U8 = 0, RWH_F32 = 1, RWH_F64 = 2, RWH_I8 = 3, RWH_U16 = 4, RWH_I16 = 5, RWH_I32 = 6, RWH_I64 = 7, RWH_U32 = 8,
       RWH_U64 = 9, RWH_F16 = 10 };
/* interpolators: reference homography.py:140 `convertfunc` keys */
enum { RWH_NEAREST = 0, RWH_BILINEAR = 1 };
/* RANSAC loss: reference ransac.py:84-98 `computeLoss` method */
enum { RWH_LOSS_FWD = 0, RWH_LOSS_BACKWARD = 1, RWH_LOSS_REPROJ = 2 };

/* flags for rwh_warp_backward */
#define RWH_WARP_ZERO_ORIGIN 1u /* write zeros into texel (0,0) of every source image first, exactly
                                   like homography.py:112-116 / 126-130 do to the caller's array */

#define RWH_WARP_EXACT 2u       /* reproduce the reference's float64 arithmetic operation by operation (dgemm
                                   k-order, IEEE divides, separately rounded float64 lerps): results bit-identical to
                                   numpy's; dst_dtype F64 (bilinear), U8 (bilinear, truncated) or the source dtype
                                   (nearest).  Several times slower than the default kernels. */

/* channel limit of the any-dtype exact warp (rwh_warp_backward with RWH_WARP_EXACT, rwh_sample_points) */
#define RWH_WARP_MAX_CHANNELS 64

RWH_API int rwh_abi_version(void);
RWH_API const char* rwh_strerror(int code);

/*
 * Lab / TEST-ONLY hook, not part of the data path and not thread-safe (plain process-wide globals): pins a launch heuristic
 * (value 0 = back to the library's own choice).  RWH_TUNE_WARP_SHAPE: log2 of the fast bilinear kernel's patch width (5, 6, 7; 13, 14 = 32 x 16 / 64 x 8 patches staged by halves, the minification form of the uint8 RGB kernel); RWH_TUNE_SCORE_HPW:
 * hypotheses per wavefront of the scorer (1..64); RWH_TUNE_SCORE_EXACT: 1 = the scorer skips its reciprocal-based
 * filter and runs the two IEEE divisions for every pair (the filter only ever decides pairs that clear the threshold
 * by a proven error band, so counts and masks are the same either way); RWH_TUNE_WARP_FRAMES (round 4): frames per block of
 * the multi-frame form of the uint8 RGB bilinear kernel (one homography, batch >= 2: warp_rgb8_fast8m, a lab kernel that shares
 * a patch's coordinate / weight arithmetic between the frames of a batch) -- 0 = the library's choice (the one-frame kernel, or
 * its batch form for 24 or more frames of at most 4K), 1 = one frame per block, forced, 2..64 = that many; 102..164 = 100 + that
 * many with one staging window per block (warp_rgb8_fast8mb).  Results never depend on any of them (tests/test_gpu_parity.py,
 * tests/test_warp_batch_walk_gpu.py).
 */
enum { RWH_TUNE_WARP_SHAPE = 0, RWH_TUNE_SCORE_HPW = 1, RWH_TUNE_SCORE_EXACT = 2, RWH_TUNE_WARP_FRAMES = 3 };
RWH_API int rwh_lab_tune(int knob, int value);

/*
 * Lab / measurement hook, not part of the data path: ONE wavefront that stays resident for `milliseconds` (<= 2000) of
 * the 100 MHz constant clock and then writes d_out[0] = shader-clock cycles elapsed (s_memtime), d_out[1] = 100 MHz ticks
 * elapsed (s_memrealtime).  Launched on a side stream beside the kernels being timed, d_out[0] / d_out[1] * 100 MHz is the
 * shader clock the chip held under that load (bench.py: roofline.sclk_mhz).  d_out: 2 x uint64 on the device.
 */
RWH_API int rwh_lab_clock_probe(uint64_t* d_out, double milliseconds, void* stream);

/*
 * Backward perspective warp.  Replaces, per call, the body of
 *   wrapPerspective      homography.py:166-179  (grid -> inv(H) -> divide -> interpolate)
 *   wrapPerspectiveScan  homography.py:197-208
 *   nearestNeighbor      homography.py:108-121
 *   bilinear             homography.py:123-138
 * and, with dst_dtype == RWH_U8 on a bilinear warp, the `astype(np.uint8)`
 * truncation of transformImage / transformImageH (homography.py:225, 240-241).
 *
 * Source: `batch` images of src_h x src_w x channels, element type src_dtype,
 * rows contiguous, image b at d_src + b*src_image_stride (bytes).
 * Output pixel (r, c) of the full out_h x out_w grid sits at output coordinate
 *   x = (c == out_w-1 ? x_last : x0 + c*step_x),  y likewise
 * (numpy.linspace semantics, homography.py:166-167 / 197-198); its source
 * coordinate is inv_h (row-major 3x3, float64, = numpy.linalg.inv(H) computed by
 * the caller as in homography.py:172) applied to (x, y, 1) and dehomogenised in
 * float64.  Coordinates outside [0, bound_w-1] x [0, bound_h-1] give 0
 * (homography.py:117-118 / 131-132; scan mode passes the OUTPUT resolution here,
 * homography.py:208).  bound_w/bound_h are clipped to the source size.
 * Bilinear weights come from the float64 fraction; the blend itself runs in
 * float32 (tolerance vs the float64 reference: 1e-4 relative, typ. 3e-7).
 * Mask edge, fast kernels (no RWH_WARP_EXACT): source coordinates are rounded once onto a 2^-32 px grid before the bounds
 * test, so a coordinate inside (-2^-33, 0) or (bound-1, bound-1 + 2^-33) counts as ON the edge texel where the reference
 * (which tests the unrounded float64, homography.py:131) returns 0.  On a generic map that is one pixel in ~10^9; an
 * axis-aligned map whose inv(H) carries 1e-16 round-off (a rotation by numpy's pi) can put a whole border row or column
 * there.  RWH_WARP_EXACT reproduces the reference's decision bit for bit (tests: test_warp_image_edge_band_vs_oracle).
 * Non-finite inv_h entries: a pixel whose denominator is +-Inf maps to (0, 0) in IEEE arithmetic (finite / Inf = 0) and shows
 * source texel (0,0) in the reference and in the exact kernels; the fast bilinear kernels mask it (0).  The reference blanks
 * texel (0,0) before it samples (RWH_WARP_ZERO_ORIGIN), so the two differ only for a caller that skips the blanking.
 * A NaN coordinate (0 / 0, Inf / Inf) escapes the reference's comparisons and makes it raise IndexError (it indexes with
 * INT_MIN, homography.py:133-135); every kernel here returns 0 for such a pixel.
 *
 * Only rows [row_begin, row_end) are produced; d_dst points at row `row_begin`
 * of image 0 and image b at d_dst + b*dst_image_stride (bytes).  This is the
 * unit of multi-GPU sharding (output-row tiles or images; no collective).
 *
 * Supported: channels 3 or 4; src_dtype U8 or F32; dst_dtype == src_dtype for
 * RWH_NEAREST; dst_dtype U8 (truncating) or F32 for RWH_BILINEAR (F64 or U8 with RWH_WARP_EXACT).
 * With RWH_WARP_EXACT also every other source: src_dtype any code RWH_U8 .. RWH_F16, channels 1 .. RWH_WARP_MAX_CHANNELS
 * (the any-dtype kernel takes every configuration but U8 / F32 with 3 or 4 channels, which keep their kernels).  Nearest
 * copies texels bit for bit (dst_dtype == src_dtype); bilinear converts each tap to float64 as numpy does (int64 / uint64
 * round to nearest) and gives F64, or U8 as numpy's astype(np.uint8) of that float64 (low byte of the truncation, 0 where it
 * does not fit int32).  On this kernel a coordinate outside the bounds reads texel (0,0) (nearest) or is interpolated at
 * (0, 0) (bilinear), as the reference does, instead of giving 0; RWH_WARP_ZERO_ORIGIN blanks channels 0..2 of texel (0,0),
 * and channel 3 only when channels == 4 (homography.py:112-116).  Without RWH_WARP_EXACT these sources return
 * RWH_E_UNSUPPORTED; rwh_warp_plan tells whether a configuration is served.
 * n_h is 1 (one homography for the whole batch) or `batch` (inv_h holds batch
 * 3x3 matrices, image b uses the b-th; any batch size -- the library launches
 * groups of images that share a kernel configuration).
 */
RWH_API int rwh_warp_backward(const void* d_src, int src_h, int src_w, int channels, int src_dtype,
                      int64_t src_image_stride, int batch,
                      const double* inv_h, int n_h,
                      double x0, double step_x, double x_last,
                      double y0, double step_y, double y_last,
                      int out_h, int out_w, int bound_h, int bound_w, int interp,
                      void* d_dst, int dst_dtype, int64_t dst_image_stride,
                      int row_begin, int row_end, unsigned flags, void* stream);

/*
 * The interpolators on coordinates the caller computed: replaces convertfunc[convert](z_t, img, h, w, mh, mw), i.e.
 *   nearestNeighbor  homography.py:108-121   (z + 0.5 truncated to int32, mask on the integers, gather)
 *   bilinear         homography.py:123-138   (mask on the float64 coordinates, truncation, float64 lerps)
 * d_x / d_y: the n source coordinates (rows 0 and 1 of the reference's dehomogenised 3 x N z_t), float64, on the device;
 * d_out: n x channels, element type = the image's for RWH_NEAREST (dst_dtype == src_dtype), float64 for RWH_BILINEAR
 * (dst_dtype RWH_F64) -- the reference's float64 arithmetic operation by operation, bit-identical to numpy's;
 * (bound_h, bound_w): the `h, w` arguments of the reference's call (clipped to the image); flags: RWH_WARP_ZERO_ORIGIN
 * blanks texel (0,0) of the image first, as both interpolators do to the caller's array.  Sources: as rwh_warp_backward with
 * RWH_WARP_EXACT (any code RWH_U8 .. RWH_F16, channels 1 .. RWH_WARP_MAX_CHANNELS, the same kernel split).  The +1 taps are clamped to the
 * image where the reference raises IndexError (their weight is 0 there).
 */
RWH_API int rwh_sample_points(const void* d_img, int src_h, int src_w, int channels, int src_dtype,
                      const double* d_x, const double* d_y, int64_t n, int bound_h, int bound_w, int interp,
                      void* d_out, int dst_dtype, unsigned flags, void* stream);

/*
 * Would the REFERENCE raise IndexError on this warp?  Its interpolators index the image with every coordinate its mask lets
 * through (homography.py:117-121, 131-135): bilinear reads texel x + 1, so a coordinate exactly ON the last column / row
 * (the identity homography) indexes one past the image; a scan-mode `res` larger than the image lets coordinates beyond it
 * through; a NaN coordinate passes the float mask and indexes with INT_MIN.  The kernels of this library clamp / mask such
 * pixels; a drop-in host layer that wants the reference's error behaviour asks here first.  Coordinates by the exact
 * kernels' arithmetic; no image access.  bound_h / bound_w: the reference's mask (NOT clipped to the source).
 * *d_flag (device int32) = OR of: 1 an index past the last column (axis 1), 2 past the last row (axis 0), 4 a NaN coordinate.
 */
RWH_API int rwh_warp_index_check(int src_h, int src_w, const double* inv_h, double x0, double step_x, double x_last,
                         double y0, double step_y, double y_last, int out_h, int out_w, int bound_h, int bound_w,
                         int interp, int* d_flag, void* stream);

/*
 * Which kernel rwh_warp_backward would launch for these arguments (same dispatch code, nothing is launched, no device
 * pointer is needed): writes the kernel's name as rocprofv3 prints it, e.g. "rwh::warp_rgb8_fast8<unsigned char, 6>"
 * (with one homography per image: the first group's kernel).  For reports (bench.py's roofline.kernel) and tests.
 */
RWH_API int rwh_warp_plan(int src_h, int src_w, int channels, int src_dtype, int batch, const double* inv_h, int n_h,
                  double x0, double step_x, double x_last, double y0, double step_y, double y_last,
                  int out_h, int out_w, int bound_h, int bound_w, int interp, int dst_dtype,
                  int row_begin, int row_end, unsigned flags, char* kernel_name, int name_len);

/*
 * Batched 4-point DLT hypothesis generator.  Replaces K calls of
 *   HomoModel.fit(X[:,idx], Y[:,idx])   ransac.py:178-180 -> 52
 *   calcHomography / calc_corresp        homography.py:71-88 / 4-14
 * d_pts_a, d_pts_b: M x 2 float32 (the `matchespoints` layout, points in rows);
 * d_idx: K x 4 int32 sample indices in [0, M) -- a PRECONDITION: device tables are not range-checked (the host entry points
 *   rwh_ransac_run / rwh_host_dlt4_svd and the Python mirror check theirs) -- (drawn by the caller from numpy's
 * legacy generator for parity, ransac.py:177);
 * d_h: K x 9 float32, row-major 3x3 with h[8] == 1;
 * d_flags: K bytes, bit 0 = repeated index in the sample, bit 1 = non-finite
 * result (singular system), bit 2 = ill-conditioned sample (RWH_HYP_ILLCOND below).  The 8x9 system is built from float32-rounded
 * products like the reference, solved in float64, scaled to unit norm, rounded
 * to float32 and divided by its 9th element in float32.
 */
#define RWH_HYP_REPEATED 1u
#define RWH_HYP_SINGULAR 2u
#define RWH_HYP_ILLCOND 4u   /* bit 2: ill-conditioned sample -- a pivot of the elimination below 1e-3 of its column's scale
                                (three collinear source points, equal coordinates at different indices, ...) or a unit null
                                vector whose 9th element is below 1e-7: H is finite but K1's elimination and LAPACK's SVD
                                (the reference's solver) may round to different float32 H.  RANSAC.run re-derives flagged
                                samples on the host with the reference's own solver; ~2 % of the samples on natural matches.
                                In searches that invert the hypotheses (rwh_ransac_search / _batched with 'backward' or 'reproj')
                                the bit is also set for a nearly singular H (|det| below 1e-6 of the sum of the six products'
                                magnitudes): its inverse must be numpy.linalg.inv's own (rwh_score_count_inv). */
#define RWH_HYP_DEGENERATE 8u /* bit 3 (round 4; implies bit 2): the ill-conditioned samples whose H says nothing about the
                                reference's -- a pivot below 1e-7 of its column's scale, |n[8]| < 1e-7, a nearly singular H in a
                                search that inverts.  Always host-solved.  The other RWH_HYP_ILLCOND samples are accurate
                                here and, under 'fwd', are bounded by rwh_score_interval instead. */
RWH_API int rwh_dlt4_batched(const float* d_pts_a, const float* d_pts_b, int m,
                     const int32_t* d_idx, int k,
                     float* d_h, uint8_t* d_flags, void* stream);

/*
 * Hypothesis x correspondence reprojection-error inlier scorer.  Replaces, per
 * hypothesis,
 *   computeLoss(X, Y, method)           ransac.py:182 -> 84-98 (fwd 55-64, reproj 66-76, dist 78-82)
 *   inliers_pos = err < th ; np.sum     ransac.py:183-184
 * and the accept rules of ransac.py:186-202 in order-independent form.
 * One wavefront scores a run of consecutive hypotheses: lanes stride over the M
 * correspondences (kept in registers; M > 256: one wavefront per chunk of 256, counts
 * accumulated with integer atomic adds after a fill kernel), `err < th` is ballotted and
 * popcounted.  A pair whose distance clears `th` by a proven error band is decided from a
 * reciprocal; a hypothesis with any pair inside the band (or a NaN) is redone with the
 * reference's two IEEE float32 divisions: counts and masks are bit-identical to the
 * reference's arithmetic either way.
 * d_counts: K int32.  d_masks: optional (may be NULL) K x ceil(M/64) uint64
 * inlier bitmasks (bit j of word w = correspondence 64*w + j).
 * d_best: 2 x uint64, accumulated with atomic max, so several calls (hypothesis
 * shards, `hyp_base` = global index of row 0) may share it after ONE memset:
 *   word 0 = (count << 32) | (0xFFFFFFFF - global_index)  -> max count, lowest index on ties
 *   word 1 = 0xFFFFFFFF - (lowest global_index with count >= need), 0 if none
 * which is also the payload of the one RCCL all-reduce(max) in the sharded run.
 * `th` is compared as (double)err < th.
 * d_err: optional (may be NULL) K x M float32, the per-correspondence loss itself
 * (what HomoModel.computeLoss returns, ransac.py:84-98).
 */
RWH_API int rwh_score_count(const float* d_h, const float* d_pts_a, const float* d_pts_b, int m, int k,
                    double th, int loss, int need, int64_t hyp_base,
                    int32_t* d_counts, uint64_t* d_masks, uint64_t* d_best, float* d_err, void* stream);

/*
 * The same with the INVERSE of every hypothesis supplied by the caller (d_hinv: K x 9 float32, row-major; NULL = as above).
 * 'backward' and 'reproj' project through numpy.linalg.inv(val) (ransac.py:74: float64 LAPACK dgesv on the identity, cast
 * to float32).  The kernels' own float64 elimination gives the same float32 matrix for every homography a sane sample
 * produces, but NOT for a nearly singular one (a sample drawn from two or three clusters): there the two round apart, and so
 * do the losses.  The settle step of RANSAC.run therefore inverts the hypotheses it re-scores with numpy's own routine
 * (rwh_host_inv3) and scores them through this entry point.
 */
RWH_API int rwh_score_count_inv(const float* d_h, const float* d_hinv, const float* d_pts_a, const float* d_pts_b, int m, int k,
                        double th, int loss, int need, int64_t hyp_base, int32_t* d_counts, uint64_t* d_masks,
                        uint64_t* d_best, float* d_err, void* stream);

/*
 * Project M points through one homography.  Replaces HomoModel.fwd (ransac.py:55-64,
 * inverse == 0) and HomoModel.reproj (ransac.py:66-76, inverse != 0: through the
 * float64 inverse rounded to float32).  d_h: 9 float32; d_pts: M x 2 float32;
 * d_out: 3 x M float32 = (val @ [x;y;1]) / (row2 + 1e-10), same rounding recipe as
 * rwh_score_count.
 */
RWH_API int rwh_project_points(const float* d_h, const float* d_pts, int m, int inverse,
                       float* d_out, void* stream);

/*
 * General form of the same two methods: d_h 9 elements, d_pts3 3 x M (rows x, y, w: the caller's third row, which a 3 x M
 * input keeps, ransac.py:58-62), d_out 3 x M, all float32 (dtype RWH_F32) or all float64 (RWH_F64: what numpy computes when
 * model.val -- the float64 refit after RANSAC.run -- or the points are float64).  For reproj the caller passes inv(val)
 * (numpy.linalg.inv on the host, as ransac.py:74 does).  Same k-order: rounded multiply, FMA, FMA; IEEE divides.
 */
RWH_API int rwh_project_points_ex(const void* d_h, const void* d_pts3, int m, int dtype, void* d_out, void* stream);

/*
 * The RANSAC search of ransac.py:176-202 as ONE call: (optional) reset of the two packed keys, then
 * rwh_dlt4_batched + rwh_score_count on the same stream with caller-provided workspaces (d_h K x 9,
 * d_flags K, d_counts K, d_masks K x ceil(M/64) or NULL).  Saves two host round trips per run; arguments
 * as in the two functions above.
 */
RWH_API int rwh_ransac_search(const float* d_pts_a, const float* d_pts_b, int m, const int32_t* d_idx, int k,
                      double th, int loss, int need, int64_t hyp_base,
                      float* d_h, uint8_t* d_flags, int32_t* d_counts, uint64_t* d_masks, uint64_t* d_best,
                      int reset_best, void* stream);

/* flag for rwh_ransac_batched */
#define RWH_BATCH_DEVICE_SAMPLING 1u /* fill d_idx on the device (Philox4x32-10) instead of reading the caller's table */
#define RWH_BATCH_EARLY_STOP 2u      /* the `break` of ransac.py:186-190 as saved work: once a hypothesis of a problem has reached
                                        its `need`, scorer waves of LATER hypotheses of that problem skip (their d_counts entry is
                                        -1, their mask words 0).  The winner is unchanged -- the lowest index that reaches `need`
                                        -- because a skipped hypothesis always has a lower-index exit on record. */

/*
 * Many independent RANSAC searches in one submission (no counterpart in the reference,
 * whose RANSAC.run handles one image pair per call, ransac.py:159-213): the loop of ransac.py:176-202 for P problems
 * x K hypotheses each, as three launches (sampling, 4-point DLT, scorer) regardless of P.
 *   d_pts_a, d_pts_b: the problems' correspondences concatenated, total x 2 float32;
 *   d_offsets: P+1 int32, problem p owns rows d_offsets[p] .. d_offsets[p+1]-1; m_max >= the largest problem;
 *   d_idx: P x K x 4 int32, indices LOCAL to each problem.  Without RWH_BATCH_DEVICE_SAMPLING the caller provides it
 *     (e.g. numpy's stream, then every problem's result equals rwh_ransac_search on that table bit for bit); with the
 *     flag the library fills it: Philox4x32-10, counter (hypothesis, problem_base + problem, 0, 0) -- `problem_base` is
 *     the global index of this call's first problem, so that a problem list sharded over several calls / GPUs draws
 *     the tables of the unsharded run --, key = seed, four DISTINCT indices
 *     per hypothesis by multiply-shift range reduction -- NOT the reference's sampler (ransac.py:177 draws with
 *     replacement from numpy's legacy generator), a documented non-parity mode; problems with fewer than 4
 *     correspondences get (0,0,0,0) and are flagged RWH_HYP_REPEATED;
 *   d_need: P int32, per-problem early-exit count (ceil(M*d/100 + n), ransac.py:169);
 *   d_h P*K x 9, d_flags P*K, d_counts P*K, d_masks P*K x ceil(m_max/64) (or NULL; words past a problem's own
 *     ceil(M/64) are written as 0);
 *   d_best: P x 2 uint64, reset here; per problem the two packed keys of rwh_score_count with the hypothesis index
 *     counted inside the problem.
 * Scoring arithmetic, tie-break and early-exit rules are those of rwh_score_count.
 */
RWH_API int rwh_ransac_batched(const float* d_pts_a, const float* d_pts_b, const int32_t* d_offsets, int n_problems,
                       int m_max, int k, int32_t* d_idx, uint64_t seed, int64_t problem_base, double th, int loss,
                       const int32_t* d_need, float* d_h, uint8_t* d_flags, int32_t* d_counts,
                       uint64_t* d_masks, uint64_t* d_best, unsigned flags, void* stream);

/*
 * The final N-point refit of the winners of rwh_ransac_batched, on the device.  Replaces, per problem,
 *   finalModel = model.fit(X[:, inliers], Y[:, inliers], collective=True)   ransac.py:206-211
 *   calc_correspLinearCollective + inv(A.T @ A) @ (A.T @ b)                 homography.py:48-69 / 90-105
 * as ONE launch for P problems (one workgroup each), results left on the device.  A documented NON-PARITY mode: the reference
 * forms and solves the normal equations in float32 through BLAS / LAPACK (an undefined summation order, and a poor solve:
 * cond(A^T A) is 1e13 .. 1e15 on pixel coordinates); this entry point solves the SAME least-squares problem in float64 and is
 * not the reference's float32 bits -- it is closer to the exact least-squares solution than the reference is.
 *   Problem p's inliers are the bits set in row p of d_masks (P x mask_words uint64): bit i of word i / 64 = correspondence
 *   d_offsets[p] + i, the layout rwh_ransac_batched writes; bits at or past the problem's size are ignored.  d_pts_a, d_pts_b,
 *   d_offsets (P + 1 int32) as rwh_ransac_batched.  The problems' sizes live on the device, so the CALLER guarantees mask_words >=
 *   ceil(M_p / 64) for every problem; a shorter row is never read past its end (correspondences beyond it count as outliers).
 *   Each inlier (x, y) -> (x', y') gives the rows [x, y, 1, 0, 0, 0, -x x', -y x' | x'] and [0, 0, 0, x, y, 1, -x y', -y y' | y']
 *   (float32 inputs converted to float64, products exact); d_h (P x 9 float64, row-major 3 x 3) = the least-squares h with
 *   h[8] = 1, from the float64 normal equations: moments summed in a fixed order (no atomics: a rerun is bit-identical),
 *   symmetric diagonal equilibration, Cholesky.
 *   d_status (P int32): RWH_REFIT_OK; RWH_REFIT_FEW, fewer than 4 inliers (the reference's refit asserts, ransac.py:38);
 *   RWH_REFIT_SINGULAR, a diagonal entry or pivot that is not a positive finite number, or a non-finite solution (the inliers do
 *   not determine a homography).  Anything but OK: all nine entries NaN.  Problems do not affect one another.
 * RWH_E_INVALID: NULL pointer, n_problems <= 0, mask_words <= 0.
 *
 * rwh_host_refit: the same operations in the same order on the HOST for one problem (no device, no stream; works without a GPU):
 * pts_a, pts_b m x 2 float32, mask_words ceil(m / 64) uint64, out_h9 9 float64, out_status one int32.  m == 0 gives
 * RWH_REFIT_FEW; RWH_E_INVALID: NULL pointer, m < 0.
 */
enum { RWH_REFIT_OK = 0, RWH_REFIT_FEW = 1, RWH_REFIT_SINGULAR = 2 };
RWH_API int rwh_refit_batched(const float* d_pts_a, const float* d_pts_b, const int32_t* d_offsets, int n_problems,
                      const uint64_t* d_masks, int mask_words, double* d_h, int32_t* d_status, void* stream);
RWH_API int rwh_host_refit(const float* pts_a, const float* pts_b, int m, const uint64_t* mask_words,
                   double* out_h9, int32_t* out_status);

/*
 * Brute-force Hamming matcher with cross-check for P image pairs in one submission: the stage in front of rwh_ransac_batched.
 * Replaces, per pair,
 *   bf = cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=True); bf.match(featuresA, featuresB)     ransac.py:258-259
 * and leaves the order of ransac.py:260-261 (sorted by distance) to the caller, who gets one record per query row.
 * THE RULE.  A: na x nbytes uint8 binary descriptors (OpenCV's "query" side), B: nb x nbytes (the "train" side),
 * D[i][j] = popcount(A[i] xor B[j]) over all 8 * nbytes bits.
 *   1. For every train row j: q[j] = the query i with the smallest D[i][j], the lowest i on ties; dT[j] = D[q[j]][j].
 *   2. For every query row i: among the j with q[j] == i, the one with the smallest dT[j], the lowest j on ties, is i's match;
 *      if no j chose i, query i has no match.
 *   3. The match list of the reference is the surviving (i, j, distance) ordered by (distance, i): its stable sort by distance
 *      of a list that arrives in query order.
 * PROVENANCE AND CAVEAT.  This is how the crossCheck=True path of OpenCV 4's BFMatcher::match reads (a 1-nearest search from
 * the train side, turned round and reduced per query row).  It is NOT the textbook mutual nearest neighbour: a query can be
 * matched to a train row that is not its own nearest, and only the train -> query direction needs the full distance matrix.
 * OpenCV is not a dependency of this project and was not available where this was written: parity with OpenCV is NOT VERIFIED.
 * The code is held to the rule above (tests/match_cases.py restates it in numpy); every quantity is an integer, so results are
 * exact and a rerun is bit-identical.
 *   d_desc_a / d_desc_b: the problems' descriptors concatenated, total_a x nbytes / total_b x nbytes uint8, rows contiguous, any
 *   alignment; d_offsets_a / d_offsets_b: P + 1 int32 each, problem p owns rows d_offsets[p] .. d_offsets[p+1]-1 of its side (the
 *   layout of rwh_ransac_batched; a problem whose range is not inside [0, total] is treated as empty);
 *   nbytes: 1 .. RWH_MATCH_MAX_BYTES (ORB / BRIEF / LATCH 32, BRISK / FREAK 64, AKAZE 61), else RWH_E_UNSUPPORTED;
 *   d_train_idx, d_distance: total_a int32 each, per query row of the concatenated A its match's train row (LOCAL to the problem)
 *   and distance, -1 / -1 for no match.  A problem with na == 0 or nb == 0 is legal and has no matches;
 *   d_workspace: workspace_bytes >= rwh_match_workspace_bytes(P, total_a, total_b) = 8 * (total_a + total_b + P + 1) bytes of
 *   device memory, 8-byte aligned, contents irrelevant before and after.
 * Work is split into blocks of RWH_MATCH_TILE_TRAIN train rows x RWH_MATCH_SEG_QUERY query rows (query rows staged
 * RWH_MATCH_CHUNK_QUERY at a time) whose partial minima are combined with 64-bit integer atomic minima: the result does not
 * depend on the split.  Four launches, whatever P.
 * RWH_E_INVALID (before any device is touched): a NULL offsets table or workspace, a NULL descriptor / output array of a side
 * that has rows, n_problems <= 0, a negative total, a workspace that is too small or misaligned.
 *
 * rwh_host_match_hamming: the same rule in plain C++ on the HOST for one pair (no device, no stream; works without a GPU):
 * desc_a na x nbytes, desc_b nb x nbytes, train_idx / distance na int32.  RWH_E_INVALID: na < 0, nb < 0, a NULL array of a side
 * that has rows; RWH_E_UNSUPPORTED: nbytes outside 1 .. RWH_MATCH_MAX_BYTES.
 */
#define RWH_MATCH_MAX_BYTES 64
#define RWH_MATCH_TILE_TRAIN 256
#define RWH_MATCH_CHUNK_QUERY 64
#define RWH_MATCH_SEG_QUERY 256
/* the most blocks the main kernel is launched with (256 CUs x 8 blocks of 4 waves); a longer block list is walked with that stride */
#define RWH_MATCH_GRID_MAX 2048
RWH_API int64_t rwh_match_workspace_bytes(int n_problems, int total_a, int total_b);
RWH_API int rwh_match_hamming_batched(const uint8_t* d_desc_a, const uint8_t* d_desc_b, int nbytes, const int32_t* d_offsets_a,
                              const int32_t* d_offsets_b, int n_problems, int total_a, int total_b, int32_t* d_train_idx,
                              int32_t* d_distance, void* d_workspace, int64_t workspace_bytes, void* stream);
RWH_API int rwh_host_match_hamming(const uint8_t* desc_a, int na, const uint8_t* desc_b, int nb, int nbytes, int32_t* train_idx,
                           int32_t* distance);

/*
 * Hamming matcher with the 2-nearest RATIO TEST over a PAIR GRAPH: the matcher in front of a pair graph (rwh_bundle_*), where
 * most proposed pairs do not overlap.  The cross-check rule above gives nearly every train row a partner whether the images overlap
 * or not (two unrelated sets of 300 random 32-byte rows: 192 "matches" in tests/test_match_ratio_cpu.py), and an acceptance rule of the form
 * inliers > 8 + 0.3 matches (Brown & Lowe 2007, eq. 13) pays for that ballast.  Images 0 .. N-1 each own a block of rows of ONE
 * descriptor array, and a pair (s, d) names its query and its train image: no descriptor is copied per pair.
 * THE RATIO RULE.  Pair p = (s, d): A = the na rows of image s (query side), B = the nb rows of image d (train side),
 * D[i][j] = popcount(A[i] xor B[j]); parameters: integers 0 < num <= den <= RWH_MATCH2_RATIO_MAX.
 *   1. For every query i: d1[i] = min_j D[i][j], j1[i] a row that attains it, d2[i] = the smallest D[i][j] over j != j1[i] (so
 *      d2 == d1 when two rows tie).  With nb < 2 there is no d2 and no query of the pair is a candidate.
 *   2. Query i is a CANDIDATE iff den d1[i] < num d2[i] -- on integers, strict.  A tie for the nearest row is therefore never a
 *      candidate, whatever the ratio, and which of the tied rows is called j1 cannot show.
 *   3. One query per train row: among the candidates with the same j1 the one with the smallest d1 survives, the lowest i on ties;
 *      the others have no match.
 *   4. The pair's match list is the survivors (i, j1, d1) ordered by (d1, i) -- left to the caller, who gets one record per query
 *      row; the correspondences are keypoint i of image s, keypoint j1 of image d, in that order (H maps s into d).
 * PROVENANCE.  Rules 1 and 2 are Lowe's ratio test (Lowe 2004, section 7.1), the usual matcher in front of a pair graph (OpenCV's
 * stitcher is remembered to use d1 < (1 - match_conf) d2 with match_conf 0.3 for ORB: a convention quoted from memory, parity is
 * NOT claimed); rule 3 is added so that the search sees one-to-one correspondences.  The code is held to the statement above
 * (tests/match_ratio_cases.py restates it in numpy), not to OpenCV; every quantity is an integer, so results are exact, do not
 * depend on how the work is split, and a rerun is bit-identical.
 *   d_desc: total_rows x nbytes uint8, rows contiguous, any alignment; d_image_offsets: n_images + 1 int32, image k owns rows
 *   d_image_offsets[k] .. d_image_offsets[k+1]-1 (an image whose range is not inside [0, total_rows] has no rows);
 *   d_pairs: n_pairs x 2 int32 (s, d).  s == d, a pair listed twice, both (s, d) and (d, s) and an image without rows are legal; a
 *   pair that names an image outside 0 .. n_images-1 reads nothing and has no matches;
 *   total_query = sum_p na(s_p), total_train = sum_p nb(d_p) (the caller knows the row counts; no download is needed);
 *   d_train_idx, d_distance, d_second: total_query int32 each; the row of (pair p, query i) is sum_{q<p} na(s_q) + i and holds
 *   (j1 LOCAL to image d, d1, d2) for a survivor and -1 / -1 / -1 otherwise.  Rows at or beyond total_query are never written;
 *   a pair whose rows would pass total_query or total_train (totals smaller than the tables say) has no matches;
 *   nbytes: 1 .. RWH_MATCH_MAX_BYTES, else RWH_E_UNSUPPORTED;
 *   d_workspace: workspace_bytes >= rwh_match_ratio_workspace_bytes(P, total_query, total_train, max_train_rows) bytes of device
 *   memory, 8-byte aligned, contents irrelevant before and after; max_train_rows = the largest nb.  The size is
 *   8 * (total_train + 4 (P + 1) + total_query * ceil(max(max_train_rows, 1) / RWH_MATCH2_SEG_TRAIN)).  The call itself cannot know
 *   max_train_rows without a download: it refuses a workspace below the size for max_train_rows = 1, and a pair whose partial
 *   results would not fit into the workspace given has no matches -- never a write outside it.  The three bounds (total_query,
 *   total_train, the workspace) are held against sums that run over the pairs in order, so behind the first pair that has no
 *   matches for one of these reasons none has any either: its rows inside total_query hold -1 / -1 / -1.
 * Work is split into blocks of RWH_MATCH2_TILE_QUERY query rows x RWH_MATCH2_SEG_TRAIN train rows (train rows staged
 * RWH_MATCH2_CHUNK_TRAIN at a time); a block leaves its two nearest per query row, a second kernel merges them (the (distance, row)
 * keys of one query are distinct, so the merge is commutative and associative), applies rule 2 and claims the train row of rule 3
 * with a 64-bit integer atomic minimum.  Four launches, whatever P.
 * RWH_E_INVALID (before any device is touched): a NULL table or workspace, a NULL descriptor array with total_rows > 0, a NULL output
 * array with total_query > 0, n_images <= 0, n_pairs <= 0, a negative total, num / den outside the bounds above, a workspace that is
 * too small or misaligned.
 *
 * rwh_host_match_ratio: the same rule in plain C++ on the HOST for one pair (no device, no stream; works without a GPU): desc_a
 * na x nbytes, desc_b nb x nbytes, train_idx / distance / second na int32.  RWH_E_INVALID: na < 0, nb < 0, a NULL array of a side
 * that has rows, num / den outside the bounds; RWH_E_UNSUPPORTED: nbytes outside 1 .. RWH_MATCH_MAX_BYTES.
 */
#define RWH_MATCH2_TILE_QUERY 256   /* query rows per block, one per lane            */
#define RWH_MATCH2_CHUNK_TRAIN 64   /* train rows staged in LDS at a time            */
#define RWH_MATCH2_SEG_TRAIN  256   /* train rows per block                          */
#define RWH_MATCH2_RATIO_MAX 1024   /* the largest denominator of the ratio          */
/* the most blocks the main kernel is launched with (256 CUs x 8 blocks of 4 waves); a longer block list is walked with that stride */
#define RWH_MATCH2_GRID_MAX 2048
RWH_API int64_t rwh_match_ratio_workspace_bytes(int n_pairs, int total_query, int total_train, int max_train_rows);
RWH_API int rwh_match_ratio_graph(const uint8_t* d_desc, int nbytes, const int32_t* d_image_offsets, int n_images, int total_rows,
                          const int32_t* d_pairs, int n_pairs, int total_query, int total_train, int ratio_num, int ratio_den,
                          int32_t* d_train_idx, int32_t* d_distance, int32_t* d_second, void* d_workspace, int64_t workspace_bytes,
                          void* stream);
RWH_API int rwh_host_match_ratio(const uint8_t* desc_a, int na, const uint8_t* desc_b, int nb, int nbytes, int ratio_num, int ratio_den,
                         int32_t* train_idx, int32_t* distance, int32_t* second);

/*
 * Feature extractor for a batch of images: FAST-9 corners with non-maximum suppression, intensity-centroid orientation in 12-degree
 * bins and a steered BRIEF descriptor -- the stage in front of rwh_match_hamming_batched.  Stands where the reference calls
 *   cv2.cvtColor(img, cv2.COLOR_RGB2GRAY); cv2.ORB_create().detectAndCompute(gray, None)      ransac.py:252-257
 * PROVENANCE AND CAVEAT.  The rule below is taken from the ORB paper (Rublee, Rabaud, Konolige, Bradski 2011: FAST-9, intensity
 * centroid, BRIEF steered in 12-degree steps, 5 x 5 box tests), on ONE scale (rules 1 - 5) or on the levels of a scale pyramid
 * (rules 6 - 8, below the entry points of the one-scale rule).  It is NOT OpenCV's ORB: not its pyramid's resampling, no Harris
 * ranking, no learned test pattern as a default, no sub-pixel refinement.  OpenCV is not a dependency of this project and was not
 * available where this was written: parity with OpenCV's ORB is NEITHER CLAIMED NOR VERIFIED.  The code is held to the rule as
 * stated (tests/orb_cases.py restates it in numpy); every quantity is an integer, so results are exact, do not depend on the order
 * in which the device finds keypoints, and a rerun is bit-identical.  Any binary descriptor serves the matcher.
 * THE RULE, for one image of h rows x w columns.
 *   1. Gray.  Pixels are uint8.  c == 1: the plane is gray already.  c == 3 (R, G, B) or c == 4 (R, G, B, alpha; alpha ignored):
 *        g = (4899 R + 9617 G + 1868 B + 8192) >> 14        (the 8-bit fixed-point form of COLOR_RGB2GRAY)
 *   2. Score.  The 16 circle pixels p_0 .. p_15 of pixel (x, y) sit at the offsets (dx, dy), y downwards,
 *        (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3)
 *      and d_i = p_i - g(x, y).  An arc is 9 circle pixels with consecutive indices modulo 16 (16 arcs).
 *        S(x, y) = max( max over the arcs of min over the arc of d_i,  max over the arcs of min over the arc of -d_i,  0 )
 *      for 3 <= x < w - 3 and 3 <= y < h - 3; S = 0 elsewhere (in particular outside the image).
 *   3. Keypoints.  (x, y) is a keypoint when S(x, y) > threshold, S(x, y) > S at each of its eight neighbours, and
 *      RWH_ORB_BORDER <= x <= w - 1 - RWH_ORB_BORDER, RWH_ORB_BORDER <= y <= h - 1 - RWH_ORB_BORDER (the patch of radius 15 plus one
 *      pixel).  An image with a side below 2 RWH_ORB_BORDER + 1 has none.  Keypoints are ordered by (S descending, y ascending, x
 *      ascending) -- a total order -- and the first n_features are kept.
 *   4. Orientation.  Over the offsets with dx^2 + dy^2 <= 15^2:  m10 = sum dx g(x + dx, y + dy),  m01 = sum dy g(x + dx, y + dy).
 *      The caller passes the bin table: RWH_ORB_BINS boundary directions b_k = (bx_k, by_k) = round(2^15 (cos, sin)((k - 1/2) 12
 *      degrees)), int32, k = 0 .. 29, and b_30 = b_0.  With cross(b, m) = bx m01 - by m10 in 64-bit integers, the bin is the k with
 *      cross(b_k, m) >= 0 and cross(b_(k+1), m) < 0 (exactly one k for m != 0: the 12-degree sector centred on k 12 degrees that
 *      holds m, its lower boundary included); m == (0, 0) gives bin 0.  No atan2 anywhere.
 *   5. Descriptor.  The caller passes the rotated patterns: int8 [RWH_ORB_BINS][nbits][4], nbits = 8 nbytes, row (k, t) = the test
 *      (x1, y1, x2, y2) of bit t rotated by k 12 degrees and rounded to integers, every coordinate in [-RWH_ORB_TEST_RADIUS,
 *      RWH_ORB_TEST_RADIUS] (a PRECONDITION of the device entry point, whose table lives on the device: coordinates outside are
 *      clamped there to keep the reads inside the patch; the host twin refuses such a table).  box(u, v) = the sum of g over the 5 x 5
 *      window centred on (u, v).  Bit t of a keypoint (x, y) with bin k is  box(x + x1, y + y1) < box(x + x2, y + y2),  stored in byte
 *      t >> 3 at bit t & 7.
 * rwh_orb_detect_batched: rules 1 - 3 without the order, for n_images images in one submission.
 *   d_images: the images' bytes concatenated (images_bytes in all); d_table: n_images x 5 int64 on the device, row i = (byte offset
 *   of image i in d_images, byte offset of its gray plane in d_gray, h, w, c), pixels interleaved, rows contiguous.  A row that does
 *   not describe an image inside the two buffers (negative offset, h or w outside 1 .. 65536, c not 1, 3 or 4, an end past
 *   images_bytes / gray_bytes) is treated as an image without pixels;
 *   d_gray (gray_bytes): receives every image's gray plane (rule 1), h x w uint8, for rwh_orb_describe_batched;
 *   d_keys: n_images x capacity uint64, d_counts: n_images int32.  Every keypoint of image i (threshold 0 .. 254) is appended to row i
 *   of d_keys, in no particular order, as the key (255 - S) << 32 | y << 16 | x: ascending keys are the order of rule 3.  d_counts[i]
 *   = the number of keypoints FOUND.  OVERFLOW: d_counts[i] > capacity says that only `capacity` of them, an arbitrary subset, were
 *   stored -- nothing is written past the row; the caller repeats the call with a larger capacity (ceil((w - 32) / 2) x ceil((h -
 *   32) / 2) always holds every keypoint, since no two keypoints are neighbours).  Unused entries of a row are RWH_ORB_KEY_NONE, above every key as signed and as unsigned words;
 *   d_workspace: workspace_bytes >= rwh_orb_workspace_bytes(n_images) = 8 (n_images + 1) bytes of device memory, 8-byte aligned.
 * Work: one block of 256 lanes per tile of RWH_ORB_TILE_W x RWH_ORB_TILE_H pixels, staged with a halo of 4 as gray bytes in LDS; one
 * atomic per wave that found a keypoint.  Two launches and two fill kernels, whatever n_images.
 * RWH_E_INVALID (before any device is touched): NULL pointer, n_images <= 0, capacity <= 0, negative sizes, threshold outside 0 ..
 * 254, a workspace that is too small or misaligned.
 * rwh_orb_describe_batched: rules 4 and 5 for the first min(d_counts[i], n_features, key_stride) keys of row i of d_keys (n_images
 *   rows of key_stride uint64: the rows of rwh_orb_detect_batched after the caller sorted each), one wavefront per keypoint.  Slot j
 *   of image i writes row i n_features + j of d_kps (float32 x, y), d_desc (nbytes uint8), d_score (int32 S) and d_bin (int32);
 *   other rows are not written.  A key whose (x, y) is not inside the border of its image writes nothing.
 *   d_bin_table: RWH_ORB_BINS x 2 int32; d_pattern: RWH_ORB_BINS x 8 nbytes x 4 int8 (rules 4 and 5), both on the device.
 *   nbytes: 1 .. RWH_MATCH_MAX_BYTES, else RWH_E_UNSUPPORTED.  RWH_E_INVALID: NULL pointer, n_images <= 0, n_features <= 0,
 *   key_stride <= 0, gray_bytes < 0.  One launch.
 * rwh_host_orb_extract: the whole rule in plain C++ on the HOST for one image (no device, no stream; works without a GPU).
 *   img: h x w x c uint8; bin_table and pattern as above, on the host; kps n_features x 2 float32, desc n_features x nbytes, score and
 *   bin n_features int32; *out_count = the number of keypoints written (<= n_features), *out_found (may be NULL) = the number found
 *   before the cut.  RWH_E_INVALID: NULL pointer, h or w outside 1 .. 65536, n_features < 0, threshold outside 0 .. 254, a pattern
 *   coordinate outside +-RWH_ORB_TEST_RADIUS; RWH_E_UNSUPPORTED: c not 1, 3 or 4, nbytes outside 1 .. RWH_MATCH_MAX_BYTES.
 *
 * THE SCALE PYRAMID (ORB paper, section 6.1: the rule above on every level of a pyramid), rules 6 - 8.  With n_levels == 1 they
 * reduce to rules 1 - 5: the result is that of the one-scale entry points bit for bit.  Still not OpenCV's ORB; no parity claimed.
 *   6. Levels.  The caller passes scales: int32 [n_levels] in Q8, scales[0] == RWH_ORB_SCALE_ONE, strictly increasing, every entry
 *      <= RWH_ORB_SCALE_MAX, 1 <= n_levels <= RWH_ORB_LEVELS_MAX.  With s = scales[l], level l of an h x w image has
 *        w_l = (256 w + s / 2) / s  columns and  h_l = (256 h + s / 2) / s  rows      (floor divisions);
 *      a level with w_l == 0 or h_l == 0 has no pixels.  Level 0 is the gray plane of rule 1.  For l >= 1, pixel (X, Y) of level l is
 *      the exact area average of level 0 over [X s, (X + 1) s) x [Y s, (Y + 1) s), source pixel j covering [256 j, 256 (j + 1)):
 *      wx_j = the length of the overlap on x, an integer in 0 .. 256, wy_i likewise on y; a source index beyond the last column or row
 *      reads the last one (the overshoot is at most half a footprint);
 *        g_l(X, Y) = (sum_i sum_j wy_i wx_j g(j, i) + s^2 / 2) / s^2                   (floor division).
 *      Every sum is below 2^31 (s^2 255 <= 1024^2 255).  No intermediate is rounded, so a SEPARABLE evaluation -- the row sums
 *      sum_j wx_j g(j, i) first, then their column sum with wy_i, one rounding at the end -- gives the same bits; the device kernel
 *      uses that, the host twin evaluates the double sum as written.  Every level is made from level 0, never from the level above:
 *      the levels have no order between them and one launch makes all of them for the whole batch.
 *   7. Per level.  Rules 2 - 5 apply to each level as if it were an image of h_l x w_l (the border of RWH_ORB_BORDER holds in level
 *      pixels: a level with a side below 33 has no keypoints).  The caller passes quotas: int32 [n_levels], each >= 0; the first
 *      quotas[l] keypoints of level l in rule 3's order are kept.  A shortfall on one level is not handed to another level.
 *   8. Merge.  An image's keypoints are its levels' keypoints in level order, rule 3's order inside a level.  A keypoint (x, y) of
 *      level l is reported at level-0 coordinates, the centre of its footprint: the float32 nearest to ((2 x + 1) s - 256) / 512, and
 *      likewise for y (on level 0 that is x itself; the numerator is an integer below 2^27, its conversion to float32 rounds to
 *      nearest and the division by 512 is exact).  Alongside go level (int32) and size = 31 s / 256 (float32, exact).
 * rwh_orb_pyramid_bytes: the bytes of the planes of levels 1 .. n_levels - 1 of one h x w image, sum of h_l w_l (0 for n_levels ==
 *   1); RWH_E_INVALID for a bad scales table (HOST pointer) or h, w outside 1 .. 65536.
 * rwh_orb_pyramid_batched: rule 6 for n_images images in one submission.  d_images (images_bytes in all) holds the images in its
 *   head, [0, planes_offset), and receives the level planes in its tail, [planes_offset, images_bytes): input and output are
 *   disjoint regions of one buffer, so that ONE rwh_orb_detect_batched call (with a d_gray of its own) takes all of them as rows of
 *   its table.  d_table: n_images x n_levels rows of 5 int64 on the device in the layout of rwh_orb_detect_batched, row i n_levels +
 *   l = level l of image i: row i n_levels is the image itself (offset, gray offset, h, w, c), row i n_levels + l, l >= 1, is (offset
 *   of the plane, gray offset, h_l, w_l, 1).  The gray offsets are not read here.  A level-0 row that does not describe an image
 *   inside [0, planes_offset) (as for rwh_orb_detect_batched) leaves every level of that image unwritten; a level row whose (h, w,
 *   c) is not (h_l, w_l, 1) of its image, or whose plane does not lie inside [planes_offset, images_bytes), is not written (a level
 *   without pixels is any row that fails this, e.g. all zeros).  Nothing else of d_images is written.  Rule 1 is applied on read,
 *   so level 0 needs no gray pass first.  scales: HOST pointer (the 16 ints travel as a kernel argument).
 *   d_workspace: workspace_bytes >= rwh_orb_workspace_bytes(n_images n_levels), 8-byte aligned.
 *   Work: one block of 256 lanes per tile of RWH_ORB_PYR_TILE_W x RWH_ORB_PYR_TILE_H output pixels over (image, level), the list
 *   built on the device as for the detector; the source window (at most 258 x 66 at s = 1024) is staged as gray bytes in LDS, the
 *   row sums go to a second LDS plane, a lane sums four adjacent columns and stores them as one word where the address is aligned.
 *   Two launches (none for n_levels == 1), whatever n_images; the whole pyramid extractor is then: pyramid (2 launches), detect (2
 *   launches, 2 fill kernels), the caller's sort, describe (1 launch).
 *   RWH_E_INVALID (before any device is touched): NULL pointer, n_images <= 0, a bad scales table, planes_offset outside 0 ..
 *   images_bytes, n_images n_levels >= 2^31, a workspace that is too small or misaligned.
 * rwh_host_orb_pyramid: rule 6 on the HOST for one image: planes (planes_bytes >= rwh_orb_pyramid_bytes) receives levels 1 ..
 *   n_levels - 1, concatenated in level order.  RWH_E_INVALID / RWH_E_UNSUPPORTED as rwh_host_orb_extract, and for a bad table.
 * rwh_host_orb_extract_pyramid: rules 1 - 8 on the HOST for one image.  kps (x, y at level-0 coordinates), desc, score, bin, level
 *   and size have room for sum(quotas) keypoints; *out_count = the number written; out_found (may be NULL): int32 [n_levels], the
 *   keypoints found on each level before its quota.  RWH_E_INVALID also for a negative quota or sum(quotas) >= 2^31.
 */
#define RWH_ORB_BORDER 16
#define RWH_ORB_BINS 30
#define RWH_ORB_PATCH_RADIUS 15
#define RWH_ORB_TEST_RADIUS 13
#define RWH_ORB_TILE_W 64
#define RWH_ORB_TILE_H 16
#define RWH_ORB_KEY_NONE 0x7F7F7F7F7F7F7F7Full
#define RWH_ORB_SCALE_ONE 256
#define RWH_ORB_SCALE_MAX 1024
#define RWH_ORB_LEVELS_MAX 16
#define RWH_ORB_PYR_TILE_W 64
#define RWH_ORB_PYR_TILE_H 16
RWH_API int64_t rwh_orb_workspace_bytes(int n_images);
RWH_API int rwh_orb_detect_batched(const uint8_t* d_images, int64_t images_bytes, const int64_t* d_table, int n_images, int threshold,
                           uint8_t* d_gray, int64_t gray_bytes, uint64_t* d_keys, int capacity, int32_t* d_counts,
                           void* d_workspace, int64_t workspace_bytes, void* stream);
RWH_API int rwh_orb_describe_batched(const uint8_t* d_gray, int64_t gray_bytes, const int64_t* d_table, int n_images,
                             const uint64_t* d_keys, int key_stride, const int32_t* d_counts, int n_features,
                             const int32_t* d_bin_table, const int8_t* d_pattern, int nbytes, float* d_kps, uint8_t* d_desc,
                             int32_t* d_score, int32_t* d_bin, void* stream);
RWH_API int rwh_host_orb_extract(const uint8_t* img, int h, int w, int c, int threshold, int n_features, const int32_t* bin_table,
                         const int8_t* pattern, int nbytes, float* kps, uint8_t* desc, int32_t* score, int32_t* bin,
                         int32_t* out_count, int32_t* out_found);
RWH_API int64_t rwh_orb_pyramid_bytes(int h, int w, const int32_t* scales, int n_levels);
RWH_API int rwh_orb_pyramid_batched(uint8_t* d_images, int64_t images_bytes, int64_t planes_offset, const int64_t* d_table, int n_images,
                            const int32_t* scales, int n_levels, void* d_workspace, int64_t workspace_bytes, void* stream);
RWH_API int rwh_host_orb_pyramid(const uint8_t* img, int h, int w, int c, const int32_t* scales, int n_levels, uint8_t* planes,
                         int64_t planes_bytes);
RWH_API int rwh_host_orb_extract_pyramid(const uint8_t* img, int h, int w, int c, int threshold, const int32_t* scales,
                                 const int32_t* quotas, int n_levels, const int32_t* bin_table, const int8_t* pattern, int nbytes,
                                 float* kps, uint8_t* desc, int32_t* score, int32_t* bin, int32_t* level, float* size,
                                 int32_t* out_count, int32_t* out_found);

/*
 * HOST helper of the settle step (no device work, no stream): the reference's own 4-point solve for n samples,
 *   calc_corresp (homography.py:4-14: 8 x 9 float32 DLT matrix, float32 products) -> numpy.linalg.svd (LAPACK dgesdd,
 *   float64 inside) -> last row of V^T cast to float32 -> / its 9th element in float32   (homography.py:71-88),
 * on `threads` host threads.  pts_a / pts_b: m x 2 float32 HOST arrays; idx_rows: n x 4 int32 (HOST); out_h: n x 9 float32.
 * dgesdd_ilp64: address of the Fortran symbol dgesdd (64-bit integers) of the LAPACK the caller's numpy uses
 * (numpy >= 2: `scipy_dgesdd_64_` in numpy.libs/libscipy_openblas64_*.so): called with numpy's own arguments, so every H is
 * numpy.linalg.svd's bit for bit -- this entry point only moves the loop off the Python interpreter and onto several
 * cores.  The accept rules of RANSAC.run need this solver (LAPACK's null vector of a rank-deficient sample is arbitrary
 * but is what the reference uses, ransac.py:177-180) for samples K1 flags and for hypotheses near the decision.
 * Returns RWH_E_LAUNCH if LAPACK reported info != 0 for a sample (numpy would raise LinAlgError).
 */
RWH_API int rwh_host_dlt4_svd(const float* pts_a, const float* pts_b, int m, const int32_t* idx_rows, int n,
                      void* dgesdd_ilp64, int threads, float* out_h);

/*
 * HOST helper: n x numpy.linalg.inv of a float32 3 x 3 (ransac.py:74) -- float64 dgesv on the identity, the routine numpy
 * calls, by address (`scipy_dgesv_64_`), cast back to float32.  h, out: n x 9 float32 HOST arrays, row-major.  A singular
 * matrix (numpy raises LinAlgError) gives NaNs.
 */
RWH_API int rwh_host_inv3(const float* h, int n, void* dgesv_ilp64, float* out);

/*
 * The inlier count of listed hypotheses as an interval ('fwd' loss, ransac.py:55-64 + 78-82 + 183): for row d_rows[i] of d_h
 * (d_rows NULL: rows 0 .. n_rows-1), d_lo[i] = the pairs that are inliers for EVERY H within the perturbation budget of d_h's row,
 * d_hi[i] = the pairs that are inliers for SOME such H.  Budget: every entry may move by delta x its natural scale (rows 0 / 1:
 * s, s, s C; row 2: s / C, s / C, s with C = coord_scale >= 1, the magnitude of the coordinates, and s the largest scale-free
 * entry), delta = delta1 for rows whose d_flags byte has RWH_HYP_ILLCOND set, delta0 otherwise (d_flags may be NULL).  The settle
 * step of RANSAC.run uses it to decide which hypotheses need the reference's own solver: LAPACK's float32 H lies within a few
 * ulps (natural scale) of K1's, so d_lo == d_hi means the reference's count IS rwh_score_count's, and a d_hi below the best
 * d_lo cannot win.  th as in rwh_score_count.
 */
RWH_API int rwh_score_interval(const float* d_h, const int32_t* d_rows, int n_rows, const uint8_t* d_flags, const float* d_pts_a,
                       const float* d_pts_b, int m, double th, double coord_scale, double delta0, double delta1,
                       int32_t* d_lo, int32_t* d_hi, void* stream);

/*
 * Host code: `count` draws of numpy's LEGACY np.random.randint(0, m, ...) (ransac.py:177 samples with it) from the MT19937 state
 * the caller took with RandomState.get_state() -- key[624], pos, updated in place for set_state() --: the identical stream
 * (one 32-bit output per draw, masked, rejected above m - 1; m == 1 draws nothing), without the interpreter and the generator's
 * lock around every draw.  out32 (int32, the index table the kernels take) and / or out64 (what numpy returns) may be NULL.
 * 1 <= m < 2^31.  tests/test_settle_cpu.py holds it to numpy's own output.
 */
RWH_API int rwh_host_legacy_randint(uint32_t* key, int32_t* pos, int64_t m, int64_t count, int32_t* out32, int64_t* out64);

/*
 * The host driver of RANSAC.run (ransac.py:159-213 up to, not including, the final refit) as ONE native call: upload,
 * rwh_ransac_search, the settle step, and the accept rules: the first hypothesis with count >= need wins and ends the search,
 * else the first maximum.  Winner, count and inlier mask equal the reference loop's on the same index table (tests: every
 * RANSAC fixture the reference produced).
 * The settle step gives the reference's own H (rwh_host_dlt4_svd, re-scored by rwh_score_count) to every hypothesis whose K1 H
 * may not stand for it in the decision; the repeated-index samples are solved on host threads while the GPU searches.
 *   'fwd' (round 4): repeated-index / non-finite / RWH_HYP_DEGENERATE samples always; of the others -- every RWH_HYP_ILLCOND
 *   sample and every hypothesis within 32 counts of the best or of `need` get a count INTERVAL (rwh_score_interval, budgets of 16 /
 *   64 float32 ulps of natural scale) -- those whose interval is not a point AND reaches the best lower bound or `need`.
 *   'backward' / 'reproj': every flagged sample and every hypothesis within min(margin_cap, 3 + count / 16) of a decision.
 *   The 'fwd' rule is exact under this MODEL, and assumes nothing more: (a) a sample without an always-bit (REPEATED / SINGULAR /
 *   DEGENERATE) has the reference's count inside its interval, and K2's count too; (b) an UNFLAGGED sample has the reference's count
 *   within 16 of K2's (the 32-count window is placed by the best count of an unflagged sample); (c) an RWH_HYP_ILLCOND sample's
 *   count is bounded only by its interval; (d) always-bit samples carry no information.  The winner is then settled or has a point
 *   interval.  (A NaN or Inf coordinate in pts_a: the margin rule.)
 * What remains EMPIRICAL in both: that LAPACK's float32 H lies within the budget (resp. that an unflagged K1 count is within the
 * margin) of K1's -- measured on 13 problem families and ~30 000 soak cases (profiles/r04_lab_notes.txt), not proven.
 *   pts_a, pts_b: m x 2 float32, idx: k x 4 int32 -- HOST arrays (the reference's inputs are host arrays; idx = the first
 *   four columns of numpy's draws, ransac.py:177);
 *   d_ws / h_ws: device workspace and PAGE-LOCKED host workspace of the sizes rwh_ransac_run_layout reports (offsets[11] and
 *   offsets[19]); after the call d_ws holds K1's H (k x 9 float32 at offsets[3]), K2's counts (int32, offsets[4]), K1's flags
 *   (offsets[5]) and the masks (offsets[6]); h_ws holds K2's raw counts (offsets[13]), the flags (offsets[14]) and the counts
 *   after the settle step (offsets[15]);
 *   hyp_base (round 4): global index of hypothesis 0 -- a rank of a sharded search passes its slice of the table and its offset;
 *   out: 8 x int32 = winner index inside this table (-1: nothing ever scored > 0), early exit (0 / 1), winner's count, hypotheses
 *   solved on the host, settle rounds, samples flagged by K1, hypotheses given an interval, 0;
 *   out_keys (may be NULL): 2 x uint64, this table's packed keys as rwh_score_count packs them -- (count << 32) | (0xFFFFFFFF -
 *   (hyp_base + winner)) and 0xFFFFFFFF - (hyp_base + first hypothesis with count >= need), or 0 --: the payload of the ONE
 *   all-reduce(MAX) of a sharded search;  out_mask: ceil(m / 64) x uint64, the winner's inlier bitmask.
 *   dgesv_ilp64: address of LAPACK dgesv in the same library (numpy.linalg.inv's routine), or NULL: with it the hypotheses
 *   the settle step re-scores under 'backward' / 'reproj' are inverted by rwh_host_inv3 (see rwh_score_count_inv).
 * Synchronises `stream` (its results are host values).  rwh_ransac_run_layout: fills offsets[0 .. 27), returns 27.
 */
RWH_API int rwh_ransac_run_layout(int m, int k, long long* offsets, int n_offsets);
RWH_API int rwh_ransac_run(const float* pts_a, const float* pts_b, int m, const int32_t* idx, int k, double th, int loss,
                   int need, int margin_cap, void* dgesdd_ilp64, void* dgesv_ilp64, int threads, void* d_ws, void* h_ws,
                   int64_t hyp_base, int32_t* out, uint64_t* out_keys, uint64_t* out_mask, void* stream);

/*
 * HOST only (no device memory, no stream; works without a GPU): the settle step's DECISION as rwh_ransac_run takes it, with the
 * GPU and LAPACK work handed to the caller's callbacks -- what the step-by-step drivers of the Python package run.
 *   k hypotheses; flags [k]: K1's flags; counts [k]: K2's raw counts in (a row already settled holds its settled count), the
 *   settled counts out; slot [k]: -1 or the settle order 0 .. nset-1 of rows the caller settled beforehand in, the settle order of
 *   every settled row out; pts_a: m x 2 float32 (HOST), read for the coordinate scale only (largest |entry|, at least 1);
 *   allow_iv: 'fwd' with K1's H at hand -- the interval rule runs if the coordinate scale is finite (below 1e30), else the margin
 *   rule with margin_cap, as in rwh_ransac_run;
 *   interval(rows, n, coord_scale, lo, hi, user): [lo, hi] of every listed row (rwh_score_interval), written at lo[row], hi[row];
 *   solve(rows, n, counts, user): the reference's count of every listed row (host solver, then K2), written at counts[row];
 *     the rows take the next n slots.  A callback returns 0, or a nonzero status that ends the call;
 *   out: 5 x int32 = winner (-1: none), early exit (0 / 1), winner's count, settle rounds, hypotheses given an interval.
 * Returns 0, RWH_E_INVALID (NULL pointer, k < 0, m < 0, margin_cap < 0, slots that are not exactly 0 .. nset-1), or the first
 * nonzero status a callback returned -- counts, slot and out then hold the state as far as the rule got.
 */
typedef int (*rwh_settle_interval_fn)(const int32_t* rows, int n, double coord_scale, int32_t* lo, int32_t* hi, void* user);
typedef int (*rwh_settle_solve_fn)(const int32_t* rows, int n, int32_t* counts, void* user);
RWH_API int rwh_settle_decide(int k, const uint8_t* flags, int32_t* counts, int32_t* slot, const float* pts_a, int m, int need,
                              int allow_iv, int margin_cap, rwh_settle_interval_fn interval, rwh_settle_solve_fn solve, void* user,
                              int32_t* out);

/*
 * Fused panorama compositor.  Replaces the body of stitchPanorama (homography.py:288-338) after its canvas
 * geometry (host, homography.py:303-321): addAlpha('Rate') + transformImageH + paste / alpha blend, in one pass
 * over the canvas, float64 arithmetic in the reference's order -> uint8 canvas bit-identical to the reference's.
 * d_img_t: imgT (t_h x t_w x 3 uint8, the image warped by H); d_img_q: imgQ (q_h x q_w x 3 uint8).
 * inv_h: inv(H); (grid_x0, grid_y0, warp_w, warp_h): wrapPerspective's output grid (min_x, min_y, max_w, max_h);
 * (tsx, tsy) / (qsx, qsy): where the warped imgT / imgQ sit on the canvas_h x canvas_w canvas.
 * blend == 0: paste imgQ over the warped imgT; 1: the 'Rate' alpha blend with blendrate `rate`; 2: the 'Gradient' blend
 * (alpha of imgT = the (x + y) / (w + h) / 2 ramp of homography.py:260-265, alpha of imgQ = 1; always the exact kernel);
 * 3 (round 4): any OTHER truthy `blending` of the reference -- addAlpha then leaves imgT's alpha plane at 0 (homography.py:250-266),
 * the alpha-weighted mean keeps imgQ / 0 everywhere and the warp only decides where the reference would raise (exact kernel).
 * Any other value: RWH_E_INVALID.
 * flags: RWH_WARP_ZERO_ORIGIN blanks texel (0,0) of imgT first, as bilinear() does to the caller's array;
 * RWH_STITCH_FAST: the staged float32-blend warp kernel with the compositor as its epilogue (rwh::warp_rgb8_comp) instead of
 * the exact float64 kernel (four pixels per lane; 0.24 ms paste / 0.57 ms blend for a 13 181 x 6 313 canvas): 1.5-2.6x faster, canvas
 * within 1 LSB of the reference's (the alpha plane's own
 * bilinear lerp is taken as constant: the one output pixel whose taps include the blanked texel (0,0) can differ more).
 */
#define RWH_STITCH_FAST 4u
RWH_API int rwh_stitch_panorama(const void* d_img_t, int t_h, int t_w, const void* d_img_q, int q_h, int q_w,
                        const double* inv_h, int grid_x0, int grid_y0, int warp_w, int warp_h,
                        int tsx, int tsy, int qsx, int qsy, int canvas_h, int canvas_w,
                        int blend, double rate, void* d_canvas, unsigned flags, void* stream);

/*
 * The same, canvas rows [row_begin, row_end) only (d_canvas still points at row 0; always the exact kernel): lets a host layer
 * that gets its images as host arrays compose a row tile as soon as the image rows it reads have arrived, and send it
 * back while later rows are still on their way up (full-duplex PCIe).  RWH_WARP_ZERO_ORIGIN: pass it with the FIRST tile
 * only (it writes texel (0,0) of imgT).
 */
RWH_API int rwh_stitch_panorama_rows(const void* d_img_t, int t_h, int t_w, const void* d_img_q, int q_h, int q_w,
                             const double* inv_h, int grid_x0, int grid_y0, int warp_w, int warp_h,
                             int tsx, int tsy, int qsx, int qsy, int canvas_h, int canvas_w,
                             int blend, double rate, void* d_canvas, int row_begin, int row_end, unsigned flags, void* stream);

/*
 * The exact compositor on images of any numeric element type: stitchPanorama (homography.py:288-338) where imgT / imgQ are not
 * uint8 RGB.  d_img_t: t_h x t_w x t_c elements of t_dtype (t_c 3 or 4); d_img_q: q_h x q_w x q_c elements of q_dtype (q_c 1, 3
 * or 4); dtypes: any RWH_U8 .. RWH_F16 code, both read in their own type.  Geometry, blend and rate as rwh_stitch_panorama;
 * canvas rows [row_begin, row_end) of a canvas_h x canvas_w x canvas_c uint8 canvas (d_canvas points at row 0).
 * The reference's numpy conversions, operation by operation, canvas bit-identical to the reference's:
 *   paste (blend 0): canvas_c == t_c; the texels are lerped in float64 (every integer promoted to float64), the warp is cast to
 *     uint8 (truncation toward zero, low byte of the int32; 0 where that does not fit int32: NaN, +-inf, |v| >= 2^31); imgQ is
 *     assigned over it, integers by their low byte, floats by the same cast; q_c == t_c, or 1 (broadcast);
 *   blend (1..3): canvas_c == 3; addAlpha's float32 copy of imgT (integers rounded to nearest, int64 directly) is warped in
 *     float64, imgQ's channels 0..2 enter as float32 (q_c 1 broadcasts), the float32 canvas is cast to uint8.  t_c == 3: the
 *     alpha plane of rwh_stitch_panorama; t_c == 4: the warped channel 3 of imgT is imgT's weight (what the reference's 5-channel
 *     warp hands its blend), and blend 1 differs from 2 and 3 only in imgQ's alpha.
 * flags: RWH_WARP_ZERO_ORIGIN only (anything else is RWH_E_INVALID).  Paste: blanks texel (0,0) of imgT in memory, every channel,
 * as bilinear() does to the caller's array (pass it with the first row tile only); blend: imgT is never written, texel (0,0) is
 * read with channels 0..2 (t_c 3: and its alpha) at 0 -- the copy addAlpha made is what bilinear() blanks (pass it with every tile).
 * RWH_E_INVALID: NULL pointer, unknown dtype code, blend outside 0..3, size <= 0, bad row range, another flag;
 * RWH_E_UNSUPPORTED: t_c, q_c or canvas_c outside the sets above (the reference raises IndexError / ValueError there, or
 * composites more channels than this entry point takes).  Where the reference's warp indexes past imgT it raises IndexError:
 * rwh_warp_index_check tells, the canvas is then meaningless (the +1 taps are clamped).
 */
RWH_API int rwh_stitch_panorama_ex(const void* d_img_t, int t_h, int t_w, int t_c, int t_dtype,
                                   const void* d_img_q, int q_h, int q_w, int q_c, int q_dtype,
                                   const double* inv_h, int grid_x0, int grid_y0, int warp_w, int warp_h,
                                   int tsx, int tsy, int qsx, int qsy, int canvas_h, int canvas_w, int canvas_c,
                                   int blend, double rate, void* d_canvas, int row_begin, int row_end, unsigned flags, void* stream);

/*
 * The sequence compositor: N images into ONE panorama, every image warped once into a common frame and every canvas pixel
 * written once.  The reference has no counterpart (stitchPanorama takes two images, homography.py:288-338); this is its paste
 * compositor generalised, held to THE SEQUENCE RULE below.  At N = 2 with blend RWH_SEQ_PASTE the canvas is, byte for byte,
 * stitchPanorama(images[0], images[1], H) with G_1 = H.
 *
 * The sequence rule.
 *   Inputs.  images[0 .. N-1]: uint8 [h_i, w_i, 3], sizes may differ, h_i, w_i >= 2.  G_i: float64 3 x 3, maps image i's pixel
 *     coordinates into the anchor's frame.  1 <= N <= RWH_SEQ_MAX_IMAGES.
 *   The anchor.  Exactly one image, a, is the anchor; it enters unwarped, as imgQ does in the reference.
 *   Rectangle of a warped image.  The four corners (0,0), (w-1,0), (w-1,h-1), (0,h-1) through G_i, dehomogenised; min / max
 *     truncated toward zero (homography.py:143-163): (mx_i, my_i, wt_i, ht_i) = (min_x, min_y, max_x - min_x + 1, max_y - min_y + 1).
 *     The anchor's rectangle is (0, 0, w_a, h_a).
 *   Canvas.  The union of the rectangles: origin (ox, oy) = (min mx_i, min my_i), fw = max(mx_i + wt_i) - ox, fh likewise.
 *     Canvas pixel (cx, cy) is frame point (x, y) = (ox + cx, oy + cy).
 *   Sample of a warped image at a frame point.  inv = numpy.linalg.inv(G_i) on the host; X = fma(inv1, y, inv0 * x) + inv2, Y
 *     and W likewise with rows 1 and 2; sx = X / W, sy = Y / W; valid = sx >= 0 & sx <= w-1 & sy >= 0 & sy <= h-1 (a NaN is not
 *     valid); ix, iy = sx, sy truncated; taps at ix, min(ix + 1, w-1), iy, min(iy + 1, h-1); texel (0,0) reads as 0 in all
 *     channels; fx = sx - ix, fy = sy - iy; top = p00 * (1 - fx) + p01 * fx, bot likewise, v = top * (1 - fy) + bot * fy, all in
 *     float64 and no operation contracted.
 *   Coverage.  Image i covers a canvas pixel when the pixel lies in its rectangle and the sample is valid.  The anchor covers
 *     its rectangle.
 *   RWH_SEQ_PASTE.  `order` is a permutation of 0 .. N-1.  The pixel takes the first image in `order` that covers it: the
 *     anchor's bytes as they are (its texel (0,0) is NOT blanked), (uint8)(int)v per channel for a warped image; 0 where nothing covers.
 *   RWH_SEQ_FEATHER.  Every covering image contributes with weight g = min(min(sx, (w-1) - sx), min(sy, (h-1) - sy)) + 1.0; for
 *     the anchor sx, sy are its integer pixel coordinates and v its bytes as float64.  Per channel num += g * v, den += g, both
 *     accumulated from 0.0 in image-index order; the pixel is (uint8)(int)(num / den), 0 where nothing covers.  `order` is
 *     validated and otherwise ignored.
 *   The images are never written.
 *
 * rwh_stitch_sequence: d_images: N device pointers (a HOST array of them); hw: N x (h, w); inv_g: N x 9, inv(G_i) (the anchor's
 * is not read); rects: N x (mx, my, wt, ht); canvas rows [row_begin, row_end) of the canvas_h x canvas_w x 3 uint8 canvas whose
 * pixel (0, 0) is frame point (origin_x, origin_y) (d_canvas points at row 0).  d_workspace: rwh_stitch_sequence_workspace_bytes(n)
 * bytes on the device, 8-byte aligned: the call lays the descriptor table down there (it travels in kernel arguments: nothing on
 * the host has to outlive the call).  One pass over the canvas: a block tests its 256 x 4 tile once against the N rectangles,
 * its pixels visit only those candidates.
 * RWH_E_INVALID, before anything is launched: a NULL pointer (an image's among them), N outside 1 .. RWH_SEQ_MAX_IMAGES, anchor
 * outside 0 .. N-1, an unknown blend, `order` that is not a permutation, h or w < 2, wt or ht <= 0, a rectangle that does not lie
 * on the canvas, an anchor rectangle other than (0, 0, w_a, h_a), a non-finite inv(G_i), a canvas side outside 1 .. 65535 or a
 * canvas above 2^31 - 1 bytes, a bad row range, a workspace too small or misaligned.
 * rwh_host_stitch_sequence: the same arithmetic on host memory (every pointer a host pointer), no GPU involved.
 */
#define RWH_SEQ_MAX_IMAGES 64
enum { RWH_SEQ_PASTE = 0, RWH_SEQ_FEATHER = 1 };
RWH_API int64_t rwh_stitch_sequence_workspace_bytes(int n);
RWH_API int rwh_stitch_sequence(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                int anchor, const int32_t* order, int blend, void* d_canvas, int canvas_h, int canvas_w,
                                int origin_x, int origin_y, int row_begin, int row_end, void* d_workspace, int64_t workspace_bytes,
                                void* stream);
RWH_API int rwh_host_stitch_sequence(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                     int anchor, const int32_t* order, int blend, void* canvas, int canvas_h, int canvas_w,
                                     int origin_x, int origin_y, int row_begin, int row_end);

/*
 * Exposure gain compensation for the sequence compositor (Brown & Lowe 2007, section 6; what OpenCV's GainCompensator does): one
 * gain per image, solved from pairwise overlap statistics, applied while compositing.  The reference has no counterpart; this is
 * held to THE GAIN RULE below.  Everything not restated is the sequence rule's: rectangles, canvas, sampling recipe, coverage, and
 * texel (0,0) of a warped image reading as 0.
 *
 * The gain rule.
 *   Overlap statistics.  Inputs: those of the sequence rule plus `stride`, 1 <= stride <= 255.  The sample set is the canvas pixels
 *     with cx % stride == 0 and cy % stride == 0.  At a sample, C is the set of images that cover it (the sequence rule's Coverage).
 *     The bytes of image i at the sample are the bytes paste would write: the anchor's own bytes for the anchor, (uint8)(int)v_k per
 *     channel for a warped image.  L_i is the sum of the three bytes, 0 <= L_i <= 765.  For every ordered pair (i, j) with i in C and
 *     j in C, i = j included: count[i][j] += 1 and sum[i][j] += L_i.  Both tables are uint64 [n][n], row-major; a call writes them
 *     whole (the caller need not zero them), pairs that never meet are 0.  count is symmetric, sum is not.  The statistics are
 *     integers: they do not depend on the order in which they are added.  They are always taken on the uncompensated bytes.
 *   Gains.  Inputs: count, sum, sigma_n (default 10.0) and sigma_g (default 0.1), both finite and > 0.  alpha = 1 / sigma_n^2,
 *     beta = 1 / sigma_g^2.  N_ij = (double)count[i][j]; I_ij = (double)sum[i][j] / (3.0 * N_ij) where count > 0, else 0.0: the
 *     mean intensity of i where it meets j, on the 0 .. 255 scale.  A (n x n) and b (n) are built from zero in this order: for each
 *     i with count[i][i] == 0, A_ii = 1 and b_i = 1, the rest of row i stays 0; for each other i, j = 0 .. n-1 in turn:
 *     A_ii += beta * N_ij and b_i += beta * N_ij, and if j != i: A_ii += 2 * alpha * I_ij * I_ij * N_ij and
 *     A_ij -= 2 * alpha * I_ij * I_ji * N_ij (products left to right).  This is the normal equation of
 *     e = 1/2 sum_i sum_j N_ij [alpha (g_i I_ij - g_j I_ji)^2 + beta (1 - g_i)^2], the diagonal N_ii counted in the prior: A is
 *     symmetric positive definite, and an image that meets nobody gets gain 1 exactly.  The gains are the float64 solution of
 *     A g = b by Cholesky, in its square-root-free form A = L D L^T on the lower triangle.  A non-positive pivot or a non-finite
 *     result is refused (RWH_E_INVALID).
 *   Applying gains.  gains: N float64 values, each finite and > 0 (otherwise RWH_E_INVALID before any launch).  Wherever the
 *     sequence rule uses a sample value v_k of image i -- the anchor's bytes as float64 included -- it uses min(v_k * g_i, 255.0)
 *     instead, in paste and in feather; the product is rounded on its own, not contracted.  The anchor under paste is therefore
 *     (uint8)(int)min((double)b * g_a, 255.0), no longer its bytes as they are.  Feather weights and coverage do not change.  With
 *     every g_i = 1.0 the canvas is byte for byte the one without gains.
 *
 * rwh_sequence_overlap_stats: images, hw, inv_g, rects, n, anchor, canvas and origin as rwh_stitch_sequence's; d_count, d_sum: device,
 * uint64 [n][n], 8-byte aligned, written whole by every call; d_workspace: rwh_sequence_overlap_stats_workspace_bytes(n,
 * canvas_h, canvas_w, stride) bytes on the device, 8-byte aligned (the descriptor table and 64 copies of the two tables, zeroed on
 * the stream by every call).  One pass over the SAMPLE grid: a block takes 256 x 4 samples, tests their footprint once against the
 * N rectangles, reduces its pairs in LDS and adds each non-zero pair once with a 64-bit integer atomic into one of the copies; a
 * second kernel sums the copies into d_count and d_sum.  RWH_E_INVALID, before anything is launched: what rwh_stitch_sequence refuses (no order, canvas buffer or row
 * range here), a stride outside 1 .. 255, a NULL or misaligned table.
 * rwh_host_sequence_overlap_stats: the same per-sample arithmetic on host memory, no GPU involved.
 * rwh_host_sequence_gains: the Gains step (host only, plain C++; no LAPACK).  RWH_E_INVALID: a NULL pointer, n outside
 * 1 .. RWH_SEQ_MAX_IMAGES, a sigma that is not finite and > 0, a non-positive pivot, a non-finite gain.
 * rwh_stitch_sequence_ex / rwh_host_stitch_sequence_ex: rwh_stitch_sequence / rwh_host_stitch_sequence with `gains` (a HOST array of
 * N; they travel in the kernel arguments).  gains == NULL is the call without _ex; the gain-free kernels are the code they were.
 */
RWH_API int64_t rwh_sequence_overlap_stats_workspace_bytes(int n, int canvas_h, int canvas_w, int stride);
RWH_API int rwh_sequence_overlap_stats(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                       int anchor, int canvas_h, int canvas_w, int origin_x, int origin_y, int stride,
                                       uint64_t* d_count, uint64_t* d_sum, void* d_workspace, int64_t workspace_bytes, void* stream);
RWH_API int rwh_host_sequence_overlap_stats(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                            int anchor, int canvas_h, int canvas_w, int origin_x, int origin_y, int stride,
                                            uint64_t* count, uint64_t* sum);
RWH_API int rwh_host_sequence_gains(const uint64_t* count, const uint64_t* sum, int n, double sigma_n, double sigma_g, double* gains);
RWH_API int rwh_stitch_sequence_ex(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                   int anchor, const int32_t* order, int blend, void* d_canvas, int canvas_h, int canvas_w,
                                   int origin_x, int origin_y, int row_begin, int row_end, void* d_workspace, int64_t workspace_bytes,
                                   void* stream, const double* gains);
RWH_API int rwh_host_stitch_sequence_ex(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                        int anchor, const int32_t* order, int blend, void* canvas, int canvas_h, int canvas_w,
                                        int origin_x, int origin_y, int row_begin, int row_end, const double* gains);

/*
 * Block exposure gains for the sequence compositor (what OpenCV's BlocksGainCompensator does, and its stitcher's default): one gain
 * MAP per image instead of one gain, so that what varies inside an image -- vignetting, a sky brighter on one side -- is
 * compensated too.  The reference has no counterpart; this is held to THE BLOCK GAIN RULE below.  Everything not restated is the
 * sequence, gain and projection rule's.  There is no ring form.
 *
 * The block gain rule.
 *   Cells.  `block` is B = 2^s, one of 16, 32, 64, 128 (s = `shift`, 4 .. 7); 32 is OpenCV's block size, a convention and not a
 *     measured optimum.  The canvas is cut into gh x gw cells of B x B pixels, gw = ceil(fw / B), gh = ceil(fh / B); cell (gx, gy)
 *     holds the canvas pixels [gx B, min(gx B + B, fw)) x [gy B, min(gy B + B, fh)): edge cells are partial.  The candidates of a cell
 *     are the images whose rectangles meet those pixels, in index order; the rank of a candidate is its place among them.  K
 *     (`slots`) is the largest candidate count over all cells; the host computes it from the rectangles (rwh_sequence_cell_slots).
 *   Cell statistics.  The sample set is the gain rule's (cx % stride == 0 and cy % stride == 0, 1 <= stride <= 255; the Python
 *     default 1 is a convention).  For every cell, count and sum of the gain rule over the samples that lie in the cell, indexed by
 *     candidate rank: tables is uint32 [gh][gw][2][K][K], count then sum (a 128 x 128 cell gives at most 16384 * 765 < 2^32).  A call
 *     writes the table whole; ranks at or above the cell's candidate count are 0, as are pairs that never meet.  The values are
 *     integers: they do not depend on the order of the adds.  Consequence: scattered back to image indices and summed over the
 *     cells, the tables are the gain rule's count and sum at the same stride, exactly.
 *   Cell gains.  Inputs: tables, `base` (N gains, each finite and > 0; NULL: all 1.0), sigma_n and sigma_g as the gain rule's.  Per
 *     cell, the gain rule's Gains step on the candidates' K' x K' sub-tables with one change: I_ij = (double)sum / (3.0 * N_ij) *
 *     base_i, the product rounded on its own.  The solution is r_{i,c}, the correction of image i in cell c on top of its base
 *     gain.  r = 1.0 exactly for an image that is no candidate of the cell or that meets nobody in it.  A non-positive pivot or a
 *     non-finite value anywhere refuses the call.
 *   Smoothing.  `smooth` iterations, an integer of 0 .. 8 (the Python default 2 is OpenCV's convention).  Each applies
 *     out = ((a + 2.0 * b) + c) * 0.25 to every plane r_i (float64 [gh][gw]), first along x (a, b, c = the left neighbour, the cell, the
 *     right neighbour), then along y on the result, with edge replication, in that order of operations.
 *   Maps.  M_i[c] = base_i * r_i[c]: float64 [N][gh][gw].  An entry that is not finite and > 0 refuses the call.
 *   Applying maps.  At canvas pixel (cx, cy): u = ((double)cx + 0.5) / B - 0.5 (exact).  If u <= 0: x0 = x1 = 0 and t = 0; if
 *     u >= gw - 1: x0 = x1 = gw - 1 and t = 0; otherwise x0 = floor(u), x1 = x0 + 1, t = u - x0.  The same for y with fraction q.
 *     top = M[y0][x0] * (1 - t) + M[y0][x1] * t, bot likewise on row y1, g = top * (1 - q) + bot * q; nothing is contracted.
 *     Wherever the gain rule uses g_i this uses g: the sample value is min(v_k * g, 255.0).  With every entry 1.0 the canvas is the
 *     canvas without gains.  With every entry of M_i equal to g_i the canvas is the gain rule's for those g_i, byte for byte,
 *     WHENEVER g_i has at most 53 - (s + 1) significant bits (any float32 value has): t and q are multiples of 2^-(s+1), so the two
 *     products are then exact and their sum is g_i.  For another g_i the lerp of a constant may round to a neighbour of g_i (1.3 does,
 *     at t = 3/16), and a byte whose product lies on an integer may then differ by one.
 *   The seam finder's survey (the seam rule) keeps scalar gains: with maps in use it is given `base`.
 *
 * rwh_sequence_cell_slots: K from the rectangles (rects, origin and canvas as rwh_stitch_sequence's; (0, 0) on a projected canvas).
 * RWH_E_INVALID (negative): a shift outside 4 .. 7, n outside 1 .. RWH_SEQ_MAX_IMAGES, a rectangle off the canvas.
 * rwh_sequence_cell_stats / _proj: images .. origin (or ray tables) as rwh_sequence_overlap_stats / _proj; slots must be
 * rwh_sequence_cell_slots's value; d_tables: device, uint32, rwh_sequence_cell_stats_table_bytes(canvas_h, canvas_w, shift, slots)
 * bytes, 4-byte aligned, written whole by every call; d_workspace: rwh_sequence_cell_stats_workspace_bytes(n) bytes, 8-byte aligned
 * (the descriptor table).  One workgroup owns one cell: it tests the clipped cell once against the N rectangles, walks the cell's
 * samples, reduces per-pair wave sums into 2 x K x K uint32 accumulators in LDS and stores its slot -- no global atomics, no second
 * kernel.  RWH_E_INVALID, before anything is launched: what rwh_sequence_overlap_stats refuses, a shift outside 4 .. 7, another
 * `slots`, a NULL or misaligned table.  rwh_host_sequence_cell_stats / _proj: the same per-sample arithmetic on host memory.
 * rwh_host_sequence_block_gains: Cell gains, Smoothing and Maps (host only, plain C++; the cell solves are the gain rule's solver).
 * maps: float64 [n][gh][gw], written whole.  RWH_E_INVALID: a NULL pointer, what rwh_sequence_cell_slots refuses, another `slots`, a
 * sigma or base gain that is not finite and > 0, smooth outside 0 .. 8, a non-positive pivot, a map entry not finite and > 0.
 * rwh_stitch_sequence_maps / _proj: rwh_stitch_sequence_ex / _proj with the gains read from maps: d_maps, device, float64
 * [n][gh][gw] for `shift`, 8-byte aligned (a pointer and the block travel in the kernel arguments where the N gains travel).  The
 * kernels of the calls without maps are the code they were.  RWH_E_INVALID: what rwh_stitch_sequence refuses, NULL or misaligned
 * maps, a shift outside 4 .. 7.  The device entries cannot read the maps' values; rwh_host_stitch_sequence_maps / _proj (the host
 * twins, maps in host memory) refuse an entry that is not finite and > 0.
 * rwh_stitch_multiband_maps / _proj and rwh_stitch_sequence_labels_maps / _proj, with their host twins: rwh_stitch_multiband(_labels)
 * and rwh_stitch_sequence_labels with `d_maps, shift` where those take `gains`.  The multi-band calls take a label plane that may be
 * NULL: NULL is the multi-band rule's Winner, a plane the seam rule's.  Refusals as the calls they extend, plus the maps' and shift's.
 */
RWH_API int rwh_sequence_cell_slots(const int32_t* rects, int n, int canvas_h, int canvas_w, int origin_x, int origin_y, int shift);
RWH_API int64_t rwh_sequence_cell_stats_workspace_bytes(int n);
RWH_API int64_t rwh_sequence_cell_stats_table_bytes(int canvas_h, int canvas_w, int shift, int slots);
RWH_API int rwh_sequence_cell_stats(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                    int anchor, int canvas_h, int canvas_w, int origin_x, int origin_y, int shift, int stride, int slots,
                                    uint32_t* d_tables, void* d_workspace, int64_t workspace_bytes, void* stream);
RWH_API int rwh_sequence_cell_stats_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                         const double* d_col, const double* d_row, int canvas_h, int canvas_w, int shift, int stride,
                                         int slots, uint32_t* d_tables, void* d_workspace, int64_t workspace_bytes, void* stream);
RWH_API int rwh_host_sequence_cell_stats(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                         int anchor, int canvas_h, int canvas_w, int origin_x, int origin_y, int shift, int stride,
                                         int slots, uint32_t* tables);
RWH_API int rwh_host_sequence_cell_stats_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                              const double* col, const double* row, int canvas_h, int canvas_w, int shift, int stride,
                                              int slots, uint32_t* tables);
RWH_API int rwh_host_sequence_block_gains(const uint32_t* tables, const int32_t* rects, int n, int canvas_h, int canvas_w, int origin_x,
                                          int origin_y, int shift, int slots, const double* base, double sigma_n, double sigma_g,
                                          int smooth, double* maps);
RWH_API int rwh_stitch_sequence_maps(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                     int anchor, const int32_t* order, int blend, void* d_canvas, int canvas_h, int canvas_w,
                                     int origin_x, int origin_y, int row_begin, int row_end, void* d_workspace, int64_t workspace_bytes,
                                     void* stream, const double* d_maps, int shift);
RWH_API int rwh_stitch_sequence_maps_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                          const int32_t* order, int blend, const double* d_col, const double* d_row, void* d_canvas,
                                          int canvas_h, int canvas_w, int row_begin, int row_end, void* d_workspace,
                                          int64_t workspace_bytes, void* stream, const double* d_maps, int shift);
RWH_API int rwh_host_stitch_sequence_maps(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                          int anchor, const int32_t* order, int blend, void* canvas, int canvas_h, int canvas_w,
                                          int origin_x, int origin_y, int row_begin, int row_end, const double* maps, int shift);
RWH_API int rwh_host_stitch_sequence_maps_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                               const int32_t* order, int blend, const double* col, const double* row, void* canvas,
                                               int canvas_h, int canvas_w, int row_begin, int row_end, const double* maps, int shift);
RWH_API int rwh_stitch_multiband_maps(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                      int anchor, int bands, const double* d_maps, int shift, const unsigned char* d_labels,
                                      void* d_canvas, int canvas_h, int canvas_w, int origin_x, int origin_y, void* d_workspace,
                                      int64_t workspace_bytes, void* stream);
RWH_API int rwh_stitch_multiband_maps_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                           int bands, const double* d_maps, int shift, const unsigned char* d_labels,
                                           const double* d_col, const double* d_row, void* d_canvas, int canvas_h, int canvas_w,
                                           void* d_workspace, int64_t workspace_bytes, void* stream);
RWH_API int rwh_host_stitch_multiband_maps(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                           int anchor, int bands, const double* maps, int shift, const unsigned char* labels,
                                           void* canvas, int canvas_h, int canvas_w, int origin_x, int origin_y);
RWH_API int rwh_host_stitch_multiband_maps_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                                int bands, const double* maps, int shift, const unsigned char* labels,
                                                const double* col, const double* row, void* canvas, int canvas_h, int canvas_w);
RWH_API int rwh_stitch_sequence_labels_maps(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                            int anchor, const double* d_maps, int shift, const unsigned char* d_labels, void* d_canvas,
                                            int canvas_h, int canvas_w, int origin_x, int origin_y, void* d_workspace,
                                            int64_t workspace_bytes, void* stream);
RWH_API int rwh_stitch_sequence_labels_maps_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                                 const double* d_maps, int shift, const unsigned char* d_labels, const double* d_col,
                                                 const double* d_row, void* d_canvas, int canvas_h, int canvas_w, void* d_workspace,
                                                 int64_t workspace_bytes, void* stream);
RWH_API int rwh_host_stitch_sequence_labels_maps(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects,
                                                 int n, int anchor, const double* maps, int shift, const unsigned char* labels,
                                                 void* canvas, int canvas_h, int canvas_w, int origin_x, int origin_y);
RWH_API int rwh_host_stitch_sequence_labels_maps_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects,
                                                      int n, const double* maps, int shift, const unsigned char* labels,
                                                      const double* col, const double* row, void* canvas, int canvas_h, int canvas_w);

/*
 * Multi-band blending for the sequence compositor (Burt & Adelson 1983, as Brown & Lowe 2007, section 7, and OpenCV's stitcher use
 * it): low frequencies are blended over a wide region, so no exposure step remains, and high frequencies come from one image, so
 * a misregistration of a pixel or two does not ghost.  The reference has no counterpart; this is held to THE MULTI-BAND RULE below.
 * Everything not restated is the sequence rule's: rectangles, canvas, the sampling recipe, Coverage, the feather weight g, and texel
 * (0,0) of a warped image reading as 0.  From the planes onward everything is integer arithmetic, so the result does not depend on
 * the order of the additions: device, host twin and a restatement agree exactly.
 *
 * The multi-band rule.
 *   Inputs.  Those of the sequence rule, without `order` and without a row range; bands = K, 1 <= K <= RWH_SEQ_MAX_BANDS; optional
 *     gains, as in the gain rule.
 *   Padded canvas.  PW = fw rounded up to a multiple of 2^K, PH likewise.  Level l (0 .. K) is a (PH >> l) x (PW >> l) plane;
 *     everything beyond a plane's edge reads as 0.
 *   Bytes of image i at a canvas pixel it covers: what paste would write -- the anchor's own bytes for the anchor, (uint8)(int)v_k
 *     for a warped image; with gains (uint8)(int)min(v_k * g_i, 255.0) for both.
 *   Winner.  At a canvas pixel covered by at least one image, the covering image with the greatest feather weight g (float64, as
 *     the sequence rule computes it); on equal weights the lowest index.  P is the winner's bytes there, 0 where nothing covers and
 *     0 in the padding.
 *   Planes of image i, over the whole padded canvas.  I_i: image i's bytes where i covers, P elsewhere (an image has no black
 *     surround).  W_i: 16384 where i is the winner, 0 elsewhere.
 *   Reduce (values and weights alike, all non-negative).  down(S)[y][x] = (sum_{ky,kx = -2..2} w[ky] w[kx] S[2y+ky][2x+kx] + 128) >> 8,
 *     w = 1 4 6 4 1.  G_i^0 = I_i, G_i^{l+1} = down(G_i^l) per channel; W_i^{l+1} = down(W_i^l).
 *   Expand.  up(S)[y][x] = floor((sum w[ky] w[kx] S[(y+ky)/2][(x+kx)/2] + 32) / 64), the sum over the ky, kx in -2..2 for which
 *     y+ky and x+kx are both even; floor division also for negative sums (an arithmetic shift); the output has twice the size each way.
 *   Bands.  L_i^l = G_i^l - up(G_i^{l+1}) for l < K, L_i^K = G_i^K.  |L| <= 255.
 *   Accumulate, per level and channel.  num^l = sum_i L_i^l W_i^l, den^l = sum_i W_i^l; both fit int32.
 *   Normalise.  B^l = 0 where den^l == 0, elsewhere sign(num) ((|num| + den / 2) / den), `/` truncating: a single contributor
 *     gives L back exactly.
 *   Collapse.  R^K = B^K, R^l = B^l + up(R^{l+1}).  |R| <= 255 (K + 1): int16.
 *   Canvas.  clamp(R^0, 0, 255) per channel where at least one image covers the pixel, 0 elsewhere.  The images are never written.
 *   Consequences.  With N = 1 the canvas is paste's.  Where all covering images agree in their bytes the canvas is paste's.  With
 *     every g_i = 1.0 the canvas is the one without gains.
 *   Working in windows.  Image i contributes only where W_i^l > 0, so an implementation may hold, per image and level, a window of
 *     the plane instead of the plane.  Per axis, with [a, b) the rectangle's canvas coordinates: D_0 = [a, b) and
 *     D_{l+1} = [floor((a_l - 1) / 2), floor((b_l + 1) / 2)] hold every non-zero W^l (the reduce taps 2x - 2 .. 2x + 2 that meet D_l);
 *     the bands read G^l on E_l = D_l united, for l >= 1, with the expand taps of D_{l-1}, [floor(a_{l-1} / 2) - 1,
 *     floor((b_{l-1} - 1) / 2) + 1]; G^l has to be the rule's on N_K = E_K and N_l = E_l united with the reduce taps of N_{l+1},
 *     [2 lo - 2, 2 hi + 2].  The window of level l is N_l clipped to the plane.  By induction from level 0, which is exact everywhere,
 *     every value stored in a window is the rule's, and what lies outside a window is either never read with a non-zero weight or
 *     beyond the plane and 0.  D_l and E_l stay within 4 pixels of the rectangle scaled by 2^-l, so the margin obeys
 *     m_l = 2 m_{l+1} + 2, m_K <= 4: the level-0 window reaches less than 6 * 2^K + 2 pixels beyond the rectangle.
 *
 * rwh_stitch_multiband_workspace_bytes: the bytes rwh_stitch_multiband needs for these rectangles, canvas and bands (the two tables,
 * the P / winner plane, the R planes of levels 1 .. K and every image's windows, four int16 per pixel); <= 0 for arguments the
 * main call would refuse.
 * rwh_stitch_multiband: images, hw, inv_g, rects, n, anchor, canvas and origin as rwh_stitch_sequence's; gains: a HOST array of N,
 * or NULL; d_workspace: that many bytes on the device, 8-byte aligned -- the call writes everything it reads there, it does not
 * depend on what the workspace held.  Writes the whole canvas.  Launches: the winner pass over the padded canvas, level 0 of all
 * images (one launch), K reduce launches (all images each; the 5 x 5 stencil from LDS tiles), K + 1 blend-and-collapse passes over
 * the canvas planes from level K down.  num and den are summed in registers by the pixel that owns them: no atomics.
 * RWH_E_INVALID, before anything is launched: everything rwh_stitch_sequence_ex refuses (no order or row range here), bands outside
 * 1 .. RWH_SEQ_MAX_BANDS, a workspace too small or misaligned.
 * rwh_host_stitch_multiband: the same arithmetic on host memory, no workspace (it allocates its own), no GPU involved.
 */
#define RWH_SEQ_MAX_BANDS 8
RWH_API int64_t rwh_stitch_multiband_workspace_bytes(const int32_t* rects, int n, int canvas_h, int canvas_w, int origin_x, int origin_y,
                                                     int bands);
RWH_API int rwh_stitch_multiband(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                 int anchor, int bands, const double* gains, void* d_canvas, int canvas_h, int canvas_w,
                                 int origin_x, int origin_y, void* d_workspace, int64_t workspace_bytes, void* stream);
RWH_API int rwh_host_stitch_multiband(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                      int anchor, int bands, const double* gains, void* canvas, int canvas_h, int canvas_w,
                                      int origin_x, int origin_y);

/*
 * Cylindrical and spherical canvases for the sequence compositor.  The sequence rule projects every image onto the anchor's image
 * plane, which suits a narrow sweep only: the plane grows with tan of the angle and ends at 90 degrees, beyond which an image lands
 * mirrored.  Panorama stitchers therefore composite onto a cylinder or a sphere about the camera (Szeliski & Shum 1997).  The
 * reference's cylindericlMap is a stub and has no compositor behind it; this is held to THE PROJECTION RULE below.  Everything not
 * restated is the sequence rule's.
 *
 * The projection rule.
 *   Inputs.  Those of the sequence rule; focal = f, finite and > 0, in pixels; the kind of surface, cylinder or sphere.
 *     K = [[f, 0, (w_a - 1) / 2], [0, f, (h_a - 1) / 2], [0, 0, 1]] from the anchor's shape.  Every G_i is multiplied by
 *     sign(det G_i); a zero or non-finite determinant is refused.
 *   Surface and canvas.  A ray r = (r0, r1, r2) in the anchor's camera has theta = atan2(r0, r2) and t = r1 / hypot(r0, r2) on the
 *     cylinder, t = atan2(r1, hypot(r0, r2)) on the sphere; its surface point is (u, s) = (f theta, f t).  Canvas pixel (cx, cy) is
 *     surface point (ox + cx, oy + cy), ox and oy integers.
 *   Ray tables.  The compositor knows nothing of sin or cos: it takes two float64 tables made on the host with numpy,
 *     col[cx] = (sin(u / f), cos(u / f)), and row[cy] = (s / f, 1.0) on the cylinder, (sin(s / f), cos(s / f)) on the sphere.  The ray
 *     of a pixel is r0 = col[cx][0] * row[cy][1], r1 = row[cy][0], r2 = col[cx][1] * row[cy][1].  Device, host twin and a numpy
 *     restatement read the same numbers and agree exactly; none of them calls a transcendental function.
 *   Sample.  M_i = numpy.linalg.inv(G_i) @ K in float64 on the host; the anchor's M is K exactly.  X = fma(m2, r2, fma(m1, r1,
 *     m0 * r0)), Y and W likewise with rows 1 and 2 of M_i; no other contraction.  valid = W > 0 and the sequence rule's bounds test on
 *     sx = X / W, sy = Y / W.  W <= 0 is a ray behind image i's camera: what the plane would show mirrored.  From sx, sy on, the
 *     taps, texel (0,0) reading as 0, the lerps, the feather weight g and the gain are the sequence rule's recipe for a warped
 *     image.  EVERY image is sampled this way, the anchor included: on a curved canvas no image enters unwarped.
 *   Rectangles, in surface pixels.  The surface points of all perimeter pixels of image i, whose rays are inv(K) G_i (x, y, 1),
 *     not dehomogenised; the rectangle runs from floor(min) - 1 to ceil(max) + 1 on each axis.  Refused: a non-finite point; two
 *     consecutive perimeter points whose theta differ by pi or more (the image straddles the seam behind the anchor); a perimeter
 *     whose wrapped theta differences do not sum to 0 (the image contains a pole).  The canvas is the union of the rectangles,
 *     under the sequence rule's size limits.  The library takes the rectangles in CANVAS coordinates (origin subtracted).
 *   Coverage.  Inside the rectangle and valid.  The rectangle only has to contain every valid pixel.
 *   Paste order, feather, the gain rule, the overlap statistics and the multi-band rule are unchanged on this Sample and Coverage.
 *
 * rwh_stitch_sequence_proj, rwh_sequence_overlap_stats_proj, rwh_stitch_multiband_proj: arguments as rwh_stitch_sequence_ex's,
 * rwh_sequence_overlap_stats's and rwh_stitch_multiband's, except: m (N x 9, the M_i) stands in place of inv_g; d_col and d_row are
 * the two tables on the device, exactly canvas_w x 2 and canvas_h x 2 doubles, 16-byte aligned, read only at indices inside the
 * canvas (a lane's pair is one 16-byte load, a wave's row entry a scalar load); rects are in canvas coordinates; there is no anchor
 * and no origin; gains may be NULL.  Workspaces: the sizes of rwh_stitch_sequence_workspace_bytes,
 * rwh_sequence_overlap_stats_workspace_bytes and rwh_stitch_multiband_workspace_bytes (with origin (0, 0)).  The reduce and collapse
 * passes of the multi-band call work on canvas planes and are the planar call's.  RWH_E_INVALID, before anything is launched:
 * everything the planar siblings refuse, a NULL or misaligned table, a non-finite M (no image is exempt).
 * rwh_host_*_proj: the same arithmetic on host memory (the tables 8-byte aligned), no GPU involved.
 */
RWH_API int rwh_stitch_sequence_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                     const int32_t* order, int blend, const double* d_col, const double* d_row, void* d_canvas,
                                     int canvas_h, int canvas_w, int row_begin, int row_end, void* d_workspace, int64_t workspace_bytes,
                                     void* stream, const double* gains);
RWH_API int rwh_host_stitch_sequence_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                          const int32_t* order, int blend, const double* col, const double* row, void* canvas,
                                          int canvas_h, int canvas_w, int row_begin, int row_end, const double* gains);
RWH_API int rwh_sequence_overlap_stats_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                            const double* d_col, const double* d_row, int canvas_h, int canvas_w, int stride,
                                            uint64_t* d_count, uint64_t* d_sum, void* d_workspace, int64_t workspace_bytes, void* stream);
RWH_API int rwh_host_sequence_overlap_stats_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                                 const double* col, const double* row, int canvas_h, int canvas_w, int stride,
                                                 uint64_t* count, uint64_t* sum);
RWH_API int rwh_stitch_multiband_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                      int bands, const double* gains, const double* d_col, const double* d_row, void* d_canvas,
                                      int canvas_h, int canvas_w, void* d_workspace, int64_t workspace_bytes, void* stream);
RWH_API int rwh_host_stitch_multiband_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                           int bands, const double* gains, const double* col, const double* row, void* canvas,
                                           int canvas_h, int canvas_w);

/*
 * Full-circle panoramas.  The projection rule refuses an image across the seam behind the anchor, and with it every sweep that
 * closes the circle.  The compositor knows nothing of sin or cos -- it reads two ray tables -- so a canvas that wraps around is a
 * matter of index arithmetic only: which columns a rectangle covers, which candidates a tile has, where a multi-band window sits,
 * where a pyramid tap lands.  That arithmetic is THE RING RULE below.  Everything not restated is the projection rule's.
 *
 * The ring rule.
 *   Inputs.  Those of the projection rule, and a period P: a positive multiple of 256, P <= 65280.  The default is
 *     P = 256 * max(1, rint(2 pi f / 256)) with numpy's rint; the caller may give another multiple of 256.  The radius is
 *     rho = P / (2.0 * pi) in float64.
 *   The camera keeps f.  K is the projection rule's K with the focal f, M_i = inv(G_i) @ K, the anchor's M is K exactly.  f is not
 *     snapped to the period: the camera model would be wrong and the loop would not close.
 *   The surface takes rho.  (u, s) = (rho theta, rho t).  The ray tables are the projection rule's with rho for f:
 *     col[cx] = (sin, cos)((ox + cx) / rho), row[cy] from (oy + cy) / rho.
 *   Canvas.  fw = P exactly, ox = -P / 2: the seam lies at +-pi, behind the anchor.  oy and fh come from the union of the
 *     rectangles' rows; the size limits are the sequence rule's.  A multiple of 256 makes every level of a pyramid of up to
 *     RWH_SEQ_MAX_BANDS bands periodic with the integer period P >> l, and keeps the kernels' 256 x 4 tiles from straddling the seam
 *     or hanging over the canvas's edge.
 *   Rectangles.  The perimeter rays and theta are the projection rule's.  The column extent is taken on the UNWRAPPED angle:
 *     theta_u[0] = theta[0], theta_u[k+1] = theta_u[k] + wrapped(theta[k+1] - theta[k]), wrapped(x) = (x + pi) mod 2 pi - pi;
 *     lo = floor(min rho theta_u) - 1, hi = ceil(max rho theta_u) + 1, wt = min(hi - lo + 1, P).  In canvas coordinates
 *     mx = (lo - ox) mod P, and mx = 0 when wt == P.  The rows are the projection rule's, with rho.  Still refused: a non-finite
 *     perimeter point; a perimeter whose wrapped differences do not sum to 0 (a pole inside the image).  No longer refused: an
 *     image across the seam.
 *   Coverage.  ((cx - mx) mod P) < wt, the modulo non-negative, and my <= cy < my + ht, and the projection rule's valid, W > 0
 *     included.
 *   Paste, feather, gains and the overlap statistics are unchanged on this Coverage.
 *   Multi-band.  The multi-band rule with PW = P, and every plane of level l periodic in x with period P >> l: the reduce and
 *     expand taps read column x mod (P >> l).  Above and below the plane they read 0, as before.
 *   Working in windows.  A window is an interval [x0, x0 + w) of the unwrapped column axis with w <= P >> l; x0 may be negative,
 *     or x0 + w may pass the period.  Plane column x belongs to the window iff ((x - x0) mod (P >> l)) < w.  An interval that
 *     would reach the period is the whole ring: x0 = 0, w = P >> l.  The recursion D_l, E_l, N_l of the multi-band rule is
 *     unchanged apart from dropping the clip in x.
 *   Consequences.  (a) With f == P / (2 pi) as a float64 and no image across the seam, paste and feather give, on the columns and
 *     rows of the projection rule's canvas, that canvas byte for byte: the table entries are the same numbers.  (b) Rolling the
 *     column table by s columns and every mx to (mx + s) mod P rolls the canvas by s, exactly: for every s under paste and feather,
 *     for s a multiple of stride in the statistics, for s a multiple of 2^bands under multi-band.
 *
 * rwh_stitch_sequence_ring, rwh_sequence_overlap_stats_ring, rwh_stitch_multiband_ring: arguments as the _proj siblings', with
 * canvas_w the period.  Rectangles are in canvas coordinates with 0 <= mx < canvas_w and 1 <= wt <= canvas_w; mx + wt may pass the
 * edge.  Workspaces: rwh_stitch_sequence_workspace_bytes, rwh_sequence_overlap_stats_workspace_bytes and
 * rwh_stitch_multiband_ring_workspace_bytes (the ring's windows are not the plane's).  RWH_E_INVALID, before anything is launched:
 * everything the _proj calls refuse, a canvas_w that is not a multiple of 256, mx outside [0, canvas_w), wt > canvas_w.  The _proj and
 * planar entry points go on refusing a rectangle that leaves the canvas.
 * rwh_host_*_ring: the same arithmetic on host memory (the tables 8-byte aligned), no GPU involved.
 */
RWH_API int rwh_stitch_sequence_ring(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                     const int32_t* order, int blend, const double* d_col, const double* d_row, void* d_canvas,
                                     int canvas_h, int canvas_w, int row_begin, int row_end, void* d_workspace, int64_t workspace_bytes,
                                     void* stream, const double* gains);
RWH_API int rwh_host_stitch_sequence_ring(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                          const int32_t* order, int blend, const double* col, const double* row, void* canvas,
                                          int canvas_h, int canvas_w, int row_begin, int row_end, const double* gains);
RWH_API int rwh_sequence_overlap_stats_ring(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                            const double* d_col, const double* d_row, int canvas_h, int canvas_w, int stride,
                                            uint64_t* d_count, uint64_t* d_sum, void* d_workspace, int64_t workspace_bytes, void* stream);
RWH_API int rwh_host_sequence_overlap_stats_ring(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                                 const double* col, const double* row, int canvas_h, int canvas_w, int stride,
                                                 uint64_t* count, uint64_t* sum);
RWH_API int64_t rwh_stitch_multiband_ring_workspace_bytes(const int32_t* rects, int n, int canvas_h, int canvas_w, int bands);
RWH_API int rwh_stitch_multiband_ring(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                      int bands, const double* gains, const double* d_col, const double* d_row, void* d_canvas,
                                      int canvas_h, int canvas_w, void* d_workspace, int64_t workspace_bytes, void* stream);
RWH_API int rwh_host_stitch_multiband_ring(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                           int bands, const double* gains, const double* col, const double* row, void* canvas,
                                           int canvas_h, int canvas_w);

/*
 * Seam finding for the sequence compositor: which image owns a canvas pixel, decided by what the images show instead of by geometry
 * alone.  Paste takes the first image in `order` and multi-band the image with the greatest feather weight, so their seams lie
 * where the rectangles put them, and an object that moved between two shots, or parallax on a near one, is cut along the overlap's
 * midline.  Stitchers place a seam finder between exposure compensation and blending (OpenCV's pipeline does); the usual graph cut
 * has no order-independent answer, so this is a geodesic, watershed-style seam (distance-transform watersheds, Meyer 1994; OpenCV's
 * seam finders are the same idea with other costs), whose result is the unique fixed point of an integer shortest-path problem:
 * any relaxation order on the device, Dijkstra in the host twin and Jacobi sweeps in a restatement give the same integers.  The
 * reference has no counterpart; this is held to THE SEAM RULE below.  Everything not restated is the sequence rule's, and on a
 * curved canvas the projection rule's: rectangles, canvas, Sample, Coverage, the feather weight g, gains.
 *
 * The seam rule.
 *   Inputs.  Those of the sequence rule without `order` and the row range; optional gains; margin, float64, >= 0, may be +inf
 *     (default 8.0); tau, an integer of 1 .. 766 (default 64).  Both defaults are conventions, not measured optima.
 *   Bytes, C, feather winner.  As the multi-band rule defines them: C(p) is the set of images that cover canvas pixel p, b_i(p) the
 *     bytes paste would write of image i there (with gains where given), w(p) the covering image of greatest g, the lowest index
 *     on equal weights.
 *   Disagreement and cost.  d(p) = sum over the three channels of (max_{i in C} b_i - min_{i in C} b_i), 0 .. 765, 0 where one
 *     image covers.  c(p) = max(1, tau - d(p)): where the images disagree by tau or more a step costs 1, where they agree it costs tau.
 *   Seeds.  p is a seed of w(p) when every other covering image j has g_j(p) <= margin, compared in float64; a pixel with a single
 *     covering image is always a seed; no other image has a seed at p.  An image owns beyond dispute what lies within `margin` of
 *     every other image's border (or outside them).
 *   Distance.  For image i, dist_i(p) is defined on the pixels i covers.  It is 0 at i's seeds; elsewhere it is the minimum, over
 *     all 4-connected paths from a seed of i to p that stay inside i's coverage, of the sum of c(q) over the pixels q of the path
 *     that are not seeds of i (the start is one; p itself is not); unreached if there is no such path.  Distances are uint32: a call
 *     is refused when wt_i * ht_i * tau > 2^32 - 3 for some i, so that no sum can wrap.
 *   Label.  label(p) = the i in C(p) with the smallest (dist_i(p), i) among the reached; w(p) if p is covered and no covering image
 *     reaches it; 0xff where nothing covers.  Labels are a uint8 plane of fh x fw.
 *   Consequences.  margin = +inf gives label = w everywhere.  tau = 1 gives every c = 1: the label is the nearest seed by city-block
 *     path length inside coverage.  With N = 1 every covered pixel has label 0.  An image without seeds labels nothing.  label(p)
 *     always covers p.
 *   Termination.  A relaxation stores only lengths of real paths -- upper bounds that only decrease, on integers -- so "repeat
 *     until nothing changes" ends, and its fixed point is the definition above whatever the order and whatever races occur between
 *     monotone 32-bit stores.
 *   Using labels.  Winner of the multi-band rule becomes: label(p), if label(p) < N and that image covers p; otherwise the
 *     multi-band rule's own Winner.  A caller's plane therefore cannot index out of range, and an all-0xff plane gives the canvas
 *     without labels byte for byte.  Label paste: the canvas is the Winner's bytes under that same definition (the P plane of the
 *     multi-band rule), 0 where nothing covers.  Feather has no single owner and takes no labels.
 *   Out.  The wrap-around canvas (no ring form), 8-connected paths, gradient terms in the cost, graph cuts, seams on a downscaled
 *     canvas, images that are not uint8.
 *
 * rwh_sequence_seams_workspace_bytes: the bytes rwh_sequence_seams needs for these rectangles and canvas (the two tables, a
 * coverage set and a survey dword per canvas pixel, a uint32 distance per pixel of every rectangle, two dirty bytes per tile); <= 0
 * for arguments the main call would refuse.
 * rwh_sequence_seams: images, hw, inv_g, rects, n, anchor, canvas size and origin as rwh_stitch_sequence's; gains: a HOST array of
 * N, or NULL; d_labels: device, canvas_h x canvas_w uint8, written whole; d_workspace: that many bytes on the device, 8-byte
 * aligned -- the call writes everything it reads there.  passes: NULL, or receives the number of relaxation passes that changed a
 * distance.  Launches: the survey pass over the canvas (cost, feather winner, seed flag and coverage set, every candidate sampled
 * once), the first distances of all images (one launch), relaxation passes over all images' RWH_SEAM_TILE_W x RWH_SEAM_TILE_H
 * tiles (a block relaxes its tile in LDS and stores what changed; a tile that did not change and whose four neighbours did not
 * either leaves at once), the label pass.  The host launches passes until one changes nothing and reads a 4-byte flag every fourth
 * pass to learn it: UNLIKE THE OTHER ENTRY POINTS THIS CALL SYNCHRONISES ITS STREAM, and it cannot be captured into a hipGraph.
 * There is no pass limit other than termination itself.
 * RWH_E_INVALID, before anything is launched: everything rwh_stitch_multiband refuses (no bands here), a margin that is NaN or
 * negative, tau outside 1 .. 766, a rectangle with wt * ht * tau > 2^32 - 3, a NULL label plane, a workspace too small or misaligned.
 * rwh_host_sequence_seams: the same rule on host memory by Dijkstra with a binary heap -- on purpose another algorithm than the
 * device's --, no workspace, no GPU involved.
 * rwh_stitch_multiband_labels / rwh_host_stitch_multiband_labels: rwh_stitch_multiband / rwh_host_stitch_multiband with the label
 * plane (d_labels: device, canvas_h x canvas_w uint8; NULL is refused) as the Winner; workspace of rwh_stitch_multiband_workspace_bytes.
 * rwh_stitch_sequence_labels / rwh_host_stitch_sequence_labels: label paste; workspace of rwh_stitch_sequence_workspace_bytes(n).
 * The _proj forms take m, d_col and d_row as the projection rule's calls do, rectangles in canvas coordinates, no anchor, no origin.
 */
#define RWH_SEAM_TILE_W 64
#define RWH_SEAM_TILE_H 16
RWH_API int64_t rwh_sequence_seams_workspace_bytes(const int32_t* rects, int n, int canvas_h, int canvas_w, int origin_x, int origin_y);
RWH_API int rwh_sequence_seams(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                               int anchor, const double* gains, double margin, int tau, unsigned char* d_labels, int canvas_h,
                               int canvas_w, int origin_x, int origin_y, void* d_workspace, int64_t workspace_bytes, void* stream,
                               int32_t* passes);
RWH_API int rwh_sequence_seams_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                    const double* gains, double margin, int tau, const double* d_col, const double* d_row,
                                    unsigned char* d_labels, int canvas_h, int canvas_w, void* d_workspace, int64_t workspace_bytes,
                                    void* stream, int32_t* passes);
RWH_API int rwh_host_sequence_seams(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                    int anchor, const double* gains, double margin, int tau, unsigned char* labels, int canvas_h,
                                    int canvas_w, int origin_x, int origin_y);
RWH_API int rwh_host_sequence_seams_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                         const double* gains, double margin, int tau, const double* col, const double* row,
                                         unsigned char* labels, int canvas_h, int canvas_w);
RWH_API int rwh_stitch_multiband_labels(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                        int anchor, int bands, const double* gains, const unsigned char* d_labels, void* d_canvas,
                                        int canvas_h, int canvas_w, int origin_x, int origin_y, void* d_workspace,
                                        int64_t workspace_bytes, void* stream);
RWH_API int rwh_stitch_multiband_labels_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                             int bands, const double* gains, const unsigned char* d_labels, const double* d_col,
                                             const double* d_row, void* d_canvas, int canvas_h, int canvas_w, void* d_workspace,
                                             int64_t workspace_bytes, void* stream);
RWH_API int rwh_host_stitch_multiband_labels(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                             int anchor, int bands, const double* gains, const unsigned char* labels, void* canvas,
                                             int canvas_h, int canvas_w, int origin_x, int origin_y);
RWH_API int rwh_host_stitch_multiband_labels_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                                  int bands, const double* gains, const unsigned char* labels, const double* col,
                                                  const double* row, void* canvas, int canvas_h, int canvas_w);
RWH_API int rwh_stitch_sequence_labels(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                       int anchor, const double* gains, const unsigned char* d_labels, void* d_canvas, int canvas_h,
                                       int canvas_w, int origin_x, int origin_y, void* d_workspace, int64_t workspace_bytes,
                                       void* stream);
RWH_API int rwh_stitch_sequence_labels_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                            const double* gains, const unsigned char* d_labels, const double* d_col,
                                            const double* d_row, void* d_canvas, int canvas_h, int canvas_w, void* d_workspace,
                                            int64_t workspace_bytes, void* stream);
RWH_API int rwh_host_stitch_sequence_labels(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects,
                                            int n, int anchor, const double* gains, const unsigned char* labels, void* canvas,
                                            int canvas_h, int canvas_w, int origin_x, int origin_y);
RWH_API int rwh_host_stitch_sequence_labels_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects,
                                                 int n, const double* gains, const unsigned char* labels, const double* col,
                                                 const double* row, void* canvas, int canvas_h, int canvas_w);

/*
 * Registration of a sequence over a pair graph: the maps G_i of the sequence rule refined jointly over the inliers of every verified
 * pair (bundle adjustment, Brown & Lowe 2007, section 4; Triggs et al. 1999), instead of chained from N - 1 adjacent pairs.  The
 * reference has no counterpart; this is held to THE BUNDLE RULE below.  The per-edge normal-equation blocks are summed on the
 * device, the small dense system is solved on the host, as for the gain rule.
 *
 * The bundle rule.
 *   Geometry.  G_i: float64 3 x 3, maps image i into the anchor's frame, as in the sequence rule; G_anchor is the identity exactly
 *     and is never updated.  1 <= N <= RWH_SEQ_MAX_IMAGES.  An edge e = (s, d), s != d, has M_e >= 0 correspondences, a in image s
 *     and b in image d, float32 rows (x, y); 1 <= E <= RWH_BUNDLE_MAX_EDGES (2016 = 64 * 63 / 2).  Its transfer is
 *     T_e = inv(G_d) G_s, made on the HOST in float64 (numpy.linalg.inv, then the product) and divided by its largest |entry|.  The
 *     library takes T_e as input and inverts nothing.
 *   Parameterisation.  The update is local, on the image side: G_i <- G_i (I + D(delta_i)), D(delta) the 3 x 3 matrix with
 *     delta_0 .. delta_7 in row-major order and D[2][2] = 0.  G[2][2] is not fixed to 1, so the system stays well conditioned where
 *     G[2][2] passes through zero (a sweep of 90 degrees on a cylinder or a sphere).  To first order T_e becomes
 *     (I - D(delta_d)) T_e (I + D(delta_s)).
 *   Per correspondence, all in float64, nothing contracted except the two fma written out:
 *     x, y, bx, by: the float32 inputs converted.  a~ = (x, y, 1).
 *     p_i = fma(T[i][1], y, T[i][0] * x) + T[i][2], i = 0, 1, 2  (rounded multiply, fma, then the fma with w = 1, which is an
 *       addition: the k-order of rwh_project_points_ex).
 *     q0 = p0 / p2, q1 = p1 / p2.  r0 = q0 - bx, r1 = q1 - by.
 *     Valid iff p2 is finite and > 0 and q0 and q1 are finite.  An inlier that is not valid contributes nothing and sets its
 *       edge's status to RWH_BUNDLE_BEHIND.
 *     J is 2 x 16: columns 0 .. 7 for delta_s, 8 .. 15 for delta_d.  For k = 3 rho + c, k < 8:
 *       delta_s: dp = a~[c] * T[:, rho], three rounded products (for c = 2 the entries of T themselves);
 *       delta_d: dp = -p[c] e_rho (one non-zero component, an exact negation);
 *       J[0][.] = (dp0 - q0 * dp2) / p2, J[1][.] = (dp1 - q1 * dp2) / p2: the product, the difference and the quotient each
 *       rounded.  With an exactly zero dp2 (or dp0, dp1) the operations on it may be left out: x - q * 0 = x and 0 - q * 0 = +0
 *       for finite q.
 *   Per edge.  A block of RWH_BUNDLE_BLOCK = 153 float64 -- the 136 entries of the upper triangle of S = sum J^T J (row-major:
 *     S[0][0..15], S[1][1..15], ...), the 16 entries of g = sum J^T r, and c = sum r.r -- an int32 count of the rows summed and an
 *     int32 status, RWH_BUNDLE_OK or RWH_BUNDLE_BEHIND.  The sums run over the rows whose bit is set in the edge's mask row (the
 *     layout of rwh_refit_batched: bit i of word i / 64 = correspondence d_offsets[e] + i; never read past mask_words, rows beyond
 *     it are no inliers) and that are valid.  An edge without such rows gives an all-zero block, count 0, status OK.
 *   Summation order, part of the rule.  Four partial sums P0 .. P3 per entry, Pw over the rows with index = w (mod 4) in
 *     increasing index (the index inside the edge, counting every row, masked or not), each from +0.0; one step is
 *     acc = acc + (u0 * v0 + u1 * v1), both products rounded, then their sum, then the addition: (u, v) = (J[.][a], J[.][b]) for
 *     S[a][b], (J[.][k], r) for g[k], (r, r) for c.  The entry is (P0 + P1) + (P2 + P3).  Rows that contribute nothing are skipped.
 *     No atomics: a rerun gives the same bits, and device, host twin and a numpy restatement agree exactly.
 *   The step (host).  A (8N x 8N) and g (8N) are built from zero by adding the blocks in edge order, columns 0 .. 7 of a block at
 *     parameters 8 s .. 8 s + 7 and 8 .. 15 at 8 d .. 8 d + 7; the anchor's eight rows and columns are dropped; lambda * A_ii is
 *     added to every diagonal entry (Marquardt scaling); A delta = -g is solved by Cholesky, A = L L^T.  A pivot that is not a
 *     positive finite number (an image that no edge touches) or a non-finite delta gives RWH_BUNDLE_SINGULAR and delta = 0.
 *     The anchor's delta is 0.
 *
 * rwh_bundle_blocks: one launch for all edges, one workgroup of 256 lanes per edge.  d_pts_a, d_pts_b (total x 2 float32), d_offsets
 * (E + 1 int32), d_masks (E x mask_words uint64) as rwh_refit_batched's; d_transfers: E x 9 float64; d_blocks: E x 153 float64;
 * d_count, d_status: E int32 -- all written whole.  The rows of an edge are staged 128 at a time in LDS (34 values each, a lane
 * per row); then each of the four waves owns one partial and each of its lanes up to three of the 153 accumulators, walking the
 * staged rows in the stated order.  RWH_E_INVALID, before anything is launched: a NULL pointer, n_edges outside
 * 1 .. RWH_BUNDLE_MAX_EDGES, mask_words <= 0.
 * rwh_host_bundle_blocks: the same operations in the same order on HOST memory; no device, works without a GPU.
 * rwh_host_bundle_step: the step (host only, plain C++; no LAPACK).  edges: n_edges x (s, d) int32; blocks: n_edges x 153; lambda
 * finite and >= 0; out_delta: 8 n float64, always written; *out_status: RWH_BUNDLE_OK or RWH_BUNDLE_SINGULAR.  RWH_E_INVALID: a NULL
 * pointer, n outside 1 .. RWH_SEQ_MAX_IMAGES, anchor outside 0 .. n - 1, n_edges outside 1 .. RWH_BUNDLE_MAX_EDGES, an edge with an
 * end outside 0 .. n - 1 or with s == d, a lambda that is not finite or < 0.
 */
#define RWH_BUNDLE_BLOCK 153
#define RWH_BUNDLE_MAX_EDGES 2016
enum { RWH_BUNDLE_OK = 0, RWH_BUNDLE_BEHIND = 1, RWH_BUNDLE_SINGULAR = 2 };
RWH_API int rwh_bundle_blocks(const float* d_pts_a, const float* d_pts_b, const int32_t* d_offsets, int n_edges, const uint64_t* d_masks,
                              int mask_words, const double* d_transfers, double* d_blocks, int32_t* d_count, int32_t* d_status,
                              void* stream);
RWH_API int rwh_host_bundle_blocks(const float* pts_a, const float* pts_b, const int32_t* offsets, int n_edges, const uint64_t* masks,
                                   int mask_words, const double* transfers, double* blocks, int32_t* count, int32_t* status);
RWH_API int rwh_host_bundle_step(int n, int anchor, const int32_t* edges, int n_edges, const double* blocks, double lambda,
                                 double* out_delta, int32_t* out_status);

/*
 * Registration over rotations and focal lengths: the second model beside the bundle rule.  A camera that turns about its centre
 * has three free parameters and a focal length where the bundle rule gives an image eight; here G_i = K_a R_i inv(K_i) with an
 * actual rotation R_i, and the focal length is refined over every inlier (Brown & Lowe 2007, section 4; Szeliski 2006, section
 * 5.1).  The reference has no counterpart; this is held to THE CAMERA RULE below.  The blocks are summed on the device, the small
 * dense system is solved on the host, as for the bundle rule.
 *
 * The camera rule.
 *   Geometry.  Image i has K_i = [[f_i, 0, cx_i], [0, f_i, cy_i], [0, 0, 1]] with (cx_i, cy_i) = ((w_i - 1) / 2, (h_i - 1) / 2), fixed
 *     (the convention of the projection rule), and a rotation R_i; R_anchor is the identity exactly and is never updated.
 *     G_i = K_a R_i inv(K_i) maps image i into the anchor's frame.  N, E and the edges as in the bundle rule.  An edge (s, d) carries
 *     its EDGE RECORD of RWH_CAMERA_RECORD = 15 float64, made on the HOST: R = R_d^T R_s (row-major), then f_s, cx_s, cy_s, f_d,
 *     cx_d, cy_d.  The library inverts nothing.
 *   Parameterisation.  Four per image, a local update: R_i <- R_i exp([omega_i]x), f_i <- f_i (1 + phi_i).  To first order R_i
 *     becomes R_i (I + [omega_i]x), which is all the blocks need; the exponential is the caller's.
 *   Per correspondence a = (x, y) in s, b = (bx, by) in d, all in float64, nothing contracted except the fma written out:
 *     x, y, bx, by: the float32 inputs converted.
 *     u = (x - cx_s, y - cy_s, f_s).
 *     v_i = fma(R[i][2], u2, fma(R[i][1], u1, R[i][0] * u0)), i = 0, 1, 2.
 *     m0 = v0 / v2, m1 = v1 / v2.  q0 = fma(f_d, m0, cx_d), q1 = fma(f_d, m1, cy_d).  r0 = q0 - bx, r1 = q1 - by.
 *     Valid iff v2 is finite and > 0 and q0 and q1 are finite.  An inlier that is not valid contributes nothing and sets its
 *       edge's status to RWH_BUNDLE_BEHIND (the bundle rule's enum serves both rules).
 *     J is 2 x 8: columns 0 .. 2 for omega_s, 3 for phi_s, 4 .. 6 for omega_d, 7 for phi_d.  Each column but the last has a dv:
 *       omega_s,0: dv = R (e_0 x u): dv_i = fma(R[i][2], u1, R[i][1] * -u2)
 *       omega_s,1: dv = R (e_1 x u): dv_i = fma(R[i][2], -u0, R[i][0] * u2)
 *       omega_s,2: dv = R (e_2 x u): dv_i = fma(R[i][1], u0, R[i][0] * -u1)     (negations are exact; one rounded product, one fma)
 *       phi_s:     dv = f_s R[:, 2]: dv_i = R[i][2] * u2
 *       omega_d,0: dv = v x e_0 = (0, v2, -v1);  omega_d,1: dv = v x e_1 = (-v2, 0, v0);  omega_d,2: dv = v x e_2 = (v1, -v0, 0)
 *       J[0][k] = (f_d * (dv0 - m0 * dv2)) / v2, J[1][k] = (f_d * (dv1 - m1 * dv2)) / v2: the product m dv2, the difference, the
 *       product with f_d and the quotient, each rounded, in this order.  A zero component of dv is the operand +0.0; the
 *       operations on it may as well be left out (x - m * 0 = x, 0 - t = -t), which changes at most the sign of a zero J entry,
 *       and no block entry sees that: every accumulator starts from +0.0.
 *       phi_d: J[0][7] = f_d * m0, J[1][7] = f_d * m1.
 *   Per edge.  A block of RWH_CAMERA_BLOCK = 45 float64 -- the 36 entries of the upper triangle of S = sum J^T J (row-major:
 *     S[0][0..7], S[1][1..7], ...), the 8 entries of g = sum J^T r, and c = sum r.r -- an int32 count of the rows summed and an int32
 *     status, RWH_BUNDLE_OK or RWH_BUNDLE_BEHIND.  Masks, offsets, the rows that count and the empty edge: as the bundle rule's.
 *   Summation order, part of the rule: the bundle rule's.  Four partial sums P0 .. P3 per entry, Pw over the rows with index = w
 *     (mod 4) in increasing index (the index inside the edge, counting every row, masked or not), each from +0.0; one step is
 *     acc = acc + (u0 * v0 + u1 * v1), both products rounded, then their sum, then the addition; the entry is
 *     (P0 + P1) + (P2 + P3).  Rows that contribute nothing are skipped.  No atomics: a rerun gives the same bits, and device, host
 *     twin and a numpy restatement agree exactly.
 *   The step (host).  The unknowns are omega of every image but the anchor, 3 (N - 1) in image order, then the focal unknowns:
 *     N of them, image i's at 3 (N - 1) + i (RWH_CAMERA_FOCAL_PER_IMAGE; the anchor's included), or one
 *     (RWH_CAMERA_FOCAL_SHARED), to which the phi column of every image maps; the contributions add, so the cross term S[3][7] of
 *     an edge then enters that diagonal entry twice.  A and g are built from zero by adding the blocks in edge order; the anchor's
 *     omega rows and columns are dropped; lambda * A_ii is added to every diagonal entry (Marquardt scaling); A delta = -g is
 *     solved by Cholesky, A = L L^T.  A pivot that is not a positive finite number (an image that no edge touches) or a non-finite
 *     delta gives RWH_BUNDLE_SINGULAR and delta = 0.  delta is 4 N float64, (omega_0, omega_1, omega_2, phi) per image: the anchor's
 *     omega is 0, and with one focal for all every image's phi holds the common value.
 *
 * rwh_camera_blocks: one launch for all edges, one workgroup of 256 lanes per edge.  Arguments as rwh_bundle_blocks', with
 * d_records (E x 15 float64) in place of d_transfers and d_blocks E x 45 float64 -- all outputs written whole.  The rows of an edge
 * are staged 128 at a time in LDS (18 values each, 19 doubles apart, a lane per row); then each of the four waves owns one partial
 * and 45 of its 64 lanes one accumulator each, walking the staged rows in the stated order.  RWH_E_INVALID, before anything is
 * launched: a NULL pointer, n_edges outside 1 .. RWH_BUNDLE_MAX_EDGES, mask_words <= 0.
 * rwh_host_camera_blocks: the same operations in the same order on HOST memory; no device, works without a GPU.
 * rwh_host_camera_step: the step (host only, plain C++; no LAPACK).  focals: RWH_CAMERA_FOCAL_SHARED or _PER_IMAGE; edges: n_edges x
 * (s, d) int32; blocks: n_edges x 45; lambda finite and >= 0; out_delta: 4 n float64, always written; *out_status: RWH_BUNDLE_OK or
 * RWH_BUNDLE_SINGULAR.  RWH_E_INVALID: what rwh_host_bundle_step refuses, or another value of focals.
 */
#define RWH_CAMERA_BLOCK 45
#define RWH_CAMERA_RECORD 15
enum { RWH_CAMERA_FOCAL_SHARED = 0, RWH_CAMERA_FOCAL_PER_IMAGE = 1 };
RWH_API int rwh_camera_blocks(const float* d_pts_a, const float* d_pts_b, const int32_t* d_offsets, int n_edges, const uint64_t* d_masks,
                              int mask_words, const double* d_records, double* d_blocks, int32_t* d_count, int32_t* d_status,
                              void* stream);
RWH_API int rwh_host_camera_blocks(const float* pts_a, const float* pts_b, const int32_t* offsets, int n_edges, const uint64_t* masks,
                                   int mask_words, const double* records, double* blocks, int32_t* count, int32_t* status);
RWH_API int rwh_host_camera_step(int n, int anchor, int focals, const int32_t* edges, int n_edges, const double* blocks, double lambda,
                                 double* out_delta, int32_t* out_status);

#ifdef __cplusplus
}
#endif
#endif /* RWH_H */
