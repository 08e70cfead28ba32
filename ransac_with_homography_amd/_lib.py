"""ctypes binding of librwh_hip.so (C ABI in include/rwh.h).

The product has no CPU fallback: if the library is missing or the process has
no MI355X, every hot-path call raises `RwhUnavailable` instead of silently
computing on the host.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librwh_hip.so")

ABI_VERSION = 5          # RWH_ABI_VERSION of the include/rwh.h this binding was written against
RWH_U8, RWH_F32, RWH_F64 = 0, 1, 2
RWH_I8, RWH_U16, RWH_I16, RWH_I32, RWH_I64, RWH_U32, RWH_U64, RWH_F16 = 3, 4, 5, 6, 7, 8, 9, 10    # stitch_ex and the exact warps
RWH_WARP_MAX_CHANNELS = 64
RWH_NEAREST, RWH_BILINEAR = 0, 1
RWH_LOSS = {"fwd": 0, "backward": 1, "reproj": 2}
RWH_WARP_ZERO_ORIGIN = 1
RWH_WARP_EXACT = 2
RWH_STITCH_FAST = 4
RWH_HYP_REPEATED, RWH_HYP_SINGULAR, RWH_HYP_ILLCOND, RWH_HYP_DEGENERATE = 1, 2, 4, 8
RWH_BATCH_DEVICE_SAMPLING = 1
RWH_BATCH_EARLY_STOP = 2
RWH_REFIT_OK, RWH_REFIT_FEW, RWH_REFIT_SINGULAR = 0, 1, 2
RWH_E_INVALID, RWH_E_UNSUPPORTED, RWH_E_LAUNCH = -1, -2, -3
RWH_MATCH_MAX_BYTES = 64
RWH_MATCH_TILE_TRAIN, RWH_MATCH_CHUNK_QUERY, RWH_MATCH_SEG_QUERY = 256, 64, 256   # the matcher's block shape (include/rwh.h)
# the ratio matcher over a pair graph (include/rwh.h, the ratio rule): query rows per block, train rows staged at a time, train rows
# per block; the largest denominator of the ratio
RWH_MATCH2_TILE_QUERY, RWH_MATCH2_CHUNK_TRAIN, RWH_MATCH2_SEG_TRAIN, RWH_MATCH2_RATIO_MAX = 256, 64, 256, 1024
# the most blocks either matcher's main kernel is launched with; a longer block list is walked with that stride
RWH_MATCH_GRID_MAX, RWH_MATCH2_GRID_MAX = 2048, 2048
# the extractor (include/rwh.h): border of a keypoint's centre, orientation bins, radius of the moment patch and of the test points,
# the detector's tile
RWH_ORB_BORDER, RWH_ORB_BINS, RWH_ORB_PATCH_RADIUS, RWH_ORB_TEST_RADIUS, RWH_ORB_TILE_W, RWH_ORB_TILE_H = 16, 30, 15, 13, 64, 16
# the pyramid (rules 6 - 8): scales are Q8, 256 .. 1024, at most 16 levels; the pyramid kernel's output tile
RWH_ORB_SCALE_ONE, RWH_ORB_SCALE_MAX, RWH_ORB_LEVELS_MAX, RWH_ORB_PYR_TILE_W, RWH_ORB_PYR_TILE_H = 256, 1024, 16, 64, 16
# the sequence compositor (include/rwh.h, the sequence rule): most images per call, its blend modes; the gain rule's largest stride
RWH_SEQ_MAX_IMAGES, RWH_SEQ_PASTE, RWH_SEQ_FEATHER = 64, 0, 1
RWH_SEQ_MAX_STRIDE = 255
RWH_SEQ_BLOCKS = (16, 32, 64, 128)     # the block gain rule: the cell sizes; most smoothing iterations
RWH_SEQ_MAX_SMOOTH = 8
RWH_SEQ_MAX_BANDS = 8         # the multi-band rule: most bands
RWH_SEAM_TILE_W, RWH_SEAM_TILE_H = 64, 16      # the seam rule: the relaxation kernel's tile
# the bundle rule: float64 values per edge block, most edges (64 * 63 / 2), the statuses of an edge and of a step
RWH_BUNDLE_BLOCK, RWH_BUNDLE_MAX_EDGES = 153, 2016
RWH_BUNDLE_OK, RWH_BUNDLE_BEHIND, RWH_BUNDLE_SINGULAR = 0, 1, 2
# the camera rule: float64 values per edge block and per edge record, the two focal models of its step
RWH_CAMERA_BLOCK, RWH_CAMERA_RECORD = 45, 15
RWH_CAMERA_FOCAL_SHARED, RWH_CAMERA_FOCAL_PER_IMAGE = 0, 1
RWH_TUNE_WARP_SHAPE, RWH_TUNE_SCORE_HPW, RWH_TUNE_SCORE_EXACT, RWH_TUNE_WARP_FRAMES = 0, 1, 2, 3

# every symbol include/rwh.h declares (tests check the library exports them all)
EXPORTS = ("rwh_abi_version", "rwh_strerror", "rwh_lab_tune", "rwh_lab_clock_probe", "rwh_warp_backward", "rwh_warp_plan", "rwh_sample_points", "rwh_dlt4_batched",
           "rwh_score_count", "rwh_project_points", "rwh_project_points_ex", "rwh_ransac_search", "rwh_ransac_batched", "rwh_stitch_panorama",
           "rwh_host_dlt4_svd", "rwh_ransac_run", "rwh_ransac_run_layout", "rwh_warp_index_check", "rwh_score_count_inv", "rwh_host_inv3", "rwh_stitch_panorama_rows",
           "rwh_host_legacy_randint", "rwh_score_interval", "rwh_stitch_panorama_ex", "rwh_settle_decide", "rwh_refit_batched", "rwh_host_refit",
           "rwh_match_workspace_bytes", "rwh_match_hamming_batched", "rwh_host_match_hamming",
           "rwh_match_ratio_workspace_bytes", "rwh_match_ratio_graph", "rwh_host_match_ratio",
           "rwh_orb_workspace_bytes", "rwh_orb_detect_batched", "rwh_orb_describe_batched", "rwh_host_orb_extract",
           "rwh_orb_pyramid_bytes", "rwh_orb_pyramid_batched", "rwh_host_orb_pyramid", "rwh_host_orb_extract_pyramid",
           "rwh_stitch_sequence_workspace_bytes", "rwh_stitch_sequence", "rwh_host_stitch_sequence",
           "rwh_sequence_overlap_stats_workspace_bytes", "rwh_sequence_overlap_stats", "rwh_host_sequence_overlap_stats",
           "rwh_host_sequence_gains", "rwh_stitch_sequence_ex", "rwh_host_stitch_sequence_ex",
           "rwh_stitch_multiband_workspace_bytes", "rwh_stitch_multiband", "rwh_host_stitch_multiband",
           "rwh_stitch_sequence_proj", "rwh_host_stitch_sequence_proj", "rwh_sequence_overlap_stats_proj",
           "rwh_host_sequence_overlap_stats_proj", "rwh_stitch_multiband_proj", "rwh_host_stitch_multiband_proj",
           "rwh_stitch_sequence_ring", "rwh_host_stitch_sequence_ring", "rwh_sequence_overlap_stats_ring",
           "rwh_host_sequence_overlap_stats_ring", "rwh_stitch_multiband_ring_workspace_bytes", "rwh_stitch_multiband_ring",
           "rwh_host_stitch_multiband_ring",
           "rwh_sequence_seams_workspace_bytes", "rwh_sequence_seams", "rwh_sequence_seams_proj", "rwh_host_sequence_seams",
           "rwh_host_sequence_seams_proj", "rwh_stitch_multiband_labels", "rwh_stitch_multiband_labels_proj",
           "rwh_host_stitch_multiband_labels", "rwh_host_stitch_multiband_labels_proj", "rwh_stitch_sequence_labels",
           "rwh_stitch_sequence_labels_proj", "rwh_host_stitch_sequence_labels", "rwh_host_stitch_sequence_labels_proj",
           "rwh_sequence_cell_slots", "rwh_sequence_cell_stats_workspace_bytes", "rwh_sequence_cell_stats_table_bytes",
           "rwh_sequence_cell_stats", "rwh_sequence_cell_stats_proj", "rwh_host_sequence_cell_stats", "rwh_host_sequence_cell_stats_proj",
           "rwh_host_sequence_block_gains", "rwh_stitch_sequence_maps", "rwh_stitch_sequence_maps_proj",
           "rwh_host_stitch_sequence_maps", "rwh_host_stitch_sequence_maps_proj",
           "rwh_stitch_multiband_maps", "rwh_stitch_multiband_maps_proj", "rwh_host_stitch_multiband_maps",
           "rwh_host_stitch_multiband_maps_proj", "rwh_stitch_sequence_labels_maps", "rwh_stitch_sequence_labels_maps_proj",
           "rwh_host_stitch_sequence_labels_maps", "rwh_host_stitch_sequence_labels_maps_proj",
           "rwh_bundle_blocks", "rwh_host_bundle_blocks", "rwh_host_bundle_step",
           "rwh_camera_blocks", "rwh_host_camera_blocks", "rwh_host_camera_step")

# the two callbacks of rwh_settle_decide: interval(rows, n, coord_scale, lo, hi, user) and solve(rows, n, counts, user) -> status
_I32P = ctypes.POINTER(ctypes.c_int32)
SETTLE_INTERVAL_FN = ctypes.CFUNCTYPE(ctypes.c_int, _I32P, ctypes.c_int, ctypes.c_double, _I32P, _I32P, ctypes.c_void_p)
SETTLE_SOLVE_FN = ctypes.CFUNCTYPE(ctypes.c_int, _I32P, ctypes.c_int, _I32P, ctypes.c_void_p)


class RwhUnavailable(RuntimeError):
    """librwh_hip.so (or a GPU to run it on) is not available."""


class RwhError(RuntimeError):
    """A library call returned a negative RWH_E_* status."""


_lib = None


def _bind(lib):
    c = ctypes
    vp, i32, i64, f64, u32 = c.c_void_p, c.c_int, c.c_int64, c.c_double, c.c_uint
    lib.rwh_abi_version.restype = i32
    lib.rwh_abi_version.argtypes = []
    lib.rwh_strerror.restype = c.c_char_p
    lib.rwh_strerror.argtypes = [i32]
    lib.rwh_lab_tune.restype = i32
    lib.rwh_lab_tune.argtypes = [i32, i32]
    lib.rwh_lab_clock_probe.restype = i32
    lib.rwh_lab_clock_probe.argtypes = [vp, f64, vp]
    lib.rwh_warp_backward.restype = i32
    lib.rwh_warp_backward.argtypes = [vp, i32, i32, i32, i32, i64, i32,        # src, h, w, c, dtype, stride, batch
                                      c.POINTER(f64), i32,                    # inv_h, n_h
                                      f64, f64, f64, f64, f64, f64,           # x0 step_x x_last y0 step_y y_last
                                      i32, i32, i32, i32, i32,                # out_h out_w bound_h bound_w interp
                                      vp, i32, i64, i32, i32, u32, vp]        # dst dtype stride row_begin row_end flags stream
    lib.rwh_warp_plan.restype = i32
    lib.rwh_warp_plan.argtypes = [i32, i32, i32, i32, i32, c.POINTER(f64), i32, f64, f64, f64, f64, f64, f64,
                                  i32, i32, i32, i32, i32, i32, i32, i32, u32, c.c_char_p, i32]
    lib.rwh_warp_index_check.restype = i32
    lib.rwh_warp_index_check.argtypes = [i32, i32, c.POINTER(f64), f64, f64, f64, f64, f64, f64, i32, i32, i32, i32, i32, vp, vp]
    lib.rwh_sample_points.restype = i32
    lib.rwh_sample_points.argtypes = [vp, i32, i32, i32, i32, vp, vp, i64, i32, i32, i32, vp, i32, u32, vp]
    lib.rwh_dlt4_batched.restype = i32
    lib.rwh_dlt4_batched.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp]
    lib.rwh_score_count.restype = i32
    lib.rwh_score_count.argtypes = [vp, vp, vp, i32, i32, f64, i32, i32, i64, vp, vp, vp, vp, vp]
    lib.rwh_score_count_inv.restype = i32
    lib.rwh_score_count_inv.argtypes = [vp, vp, vp, vp, i32, i32, f64, i32, i32, i64, vp, vp, vp, vp, vp]
    lib.rwh_host_inv3.restype = i32
    lib.rwh_host_inv3.argtypes = [vp, i32, vp, vp]
    lib.rwh_ransac_search.restype = i32
    lib.rwh_ransac_search.argtypes = [vp, vp, i32, vp, i32, f64, i32, i32, i64, vp, vp, vp, vp, vp, i32, vp]
    lib.rwh_ransac_batched.restype = i32
    lib.rwh_ransac_batched.argtypes = [vp, vp, vp, i32, i32, i32, vp, c.c_uint64, i64, f64, i32, vp, vp, vp, vp, vp, vp, u32, vp]
    lib.rwh_stitch_panorama.restype = i32
    lib.rwh_stitch_panorama.argtypes = [vp, i32, i32, vp, i32, i32, c.POINTER(f64), i32, i32, i32, i32,
                                        i32, i32, i32, i32, i32, i32, i32, f64, vp, u32, vp]
    lib.rwh_stitch_panorama_rows.restype = i32
    lib.rwh_stitch_panorama_rows.argtypes = [vp, i32, i32, vp, i32, i32, c.POINTER(f64), i32, i32, i32, i32,
                                             i32, i32, i32, i32, i32, i32, i32, f64, vp, i32, i32, u32, vp]
    lib.rwh_stitch_panorama_ex.restype = i32
    lib.rwh_stitch_panorama_ex.argtypes = [vp, i32, i32, i32, i32, vp, i32, i32, i32, i32,    # img_t h w c dtype, img_q h w c dtype
                                           c.POINTER(f64), i32, i32, i32, i32,               # inv_h, grid x0 y0, warp w h
                                           i32, i32, i32, i32, i32, i32, i32,                # tsx tsy qsx qsy, canvas h w c
                                           i32, f64, vp, i32, i32, u32, vp]                  # blend rate canvas row_begin row_end flags stream
    lib.rwh_project_points_ex.restype = i32
    lib.rwh_project_points_ex.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.rwh_project_points.restype = i32
    lib.rwh_project_points.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.rwh_host_dlt4_svd.restype = i32
    lib.rwh_host_dlt4_svd.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp]
    lib.rwh_score_interval.restype = i32
    lib.rwh_score_interval.argtypes = [vp, vp, i32, vp, vp, vp, i32, f64, f64, f64, f64, vp, vp, vp]
    lib.rwh_host_legacy_randint.restype = i32
    lib.rwh_host_legacy_randint.argtypes = [vp, vp, i64, i64, vp, vp]
    lib.rwh_ransac_run_layout.restype = i32
    lib.rwh_ransac_run_layout.argtypes = [i32, i32, vp, i32]
    lib.rwh_ransac_run.restype = i32
    lib.rwh_ransac_run.argtypes = [vp, vp, i32, vp, i32, f64, i32, i32, i32, vp, vp, i32, vp, vp, i64, vp, vp, vp, vp]
    lib.rwh_settle_decide.restype = i32
    lib.rwh_settle_decide.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, i32, SETTLE_INTERVAL_FN, SETTLE_SOLVE_FN, vp, vp]
    lib.rwh_refit_batched.restype = i32
    lib.rwh_refit_batched.argtypes = [vp, vp, vp, i32, vp, i32, vp, vp, vp]
    lib.rwh_host_refit.restype = i32
    lib.rwh_host_refit.argtypes = [vp, vp, i32, vp, vp, vp]
    lib.rwh_match_workspace_bytes.restype = i64
    lib.rwh_match_workspace_bytes.argtypes = [i32, i32, i32]
    lib.rwh_match_hamming_batched.restype = i32
    lib.rwh_match_hamming_batched.argtypes = [vp, vp, i32, vp, vp, i32, i32, i32, vp, vp, vp, i64, vp]
    lib.rwh_host_match_hamming.restype = i32
    lib.rwh_host_match_hamming.argtypes = [vp, i32, vp, i32, i32, vp, vp]
    lib.rwh_match_ratio_workspace_bytes.restype = i64
    lib.rwh_match_ratio_workspace_bytes.argtypes = [i32, i32, i32, i32]
    lib.rwh_match_ratio_graph.restype = i32
    lib.rwh_match_ratio_graph.argtypes = [vp, i32, vp, i32, i32, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp]
    lib.rwh_host_match_ratio.restype = i32
    lib.rwh_host_match_ratio.argtypes = [vp, i32, vp, i32, i32, i32, i32, vp, vp, vp]
    lib.rwh_orb_workspace_bytes.restype = i64
    lib.rwh_orb_workspace_bytes.argtypes = [i32]
    lib.rwh_orb_detect_batched.restype = i32
    lib.rwh_orb_detect_batched.argtypes = [vp, i64, vp, i32, i32, vp, i64, vp, i32, vp, vp, i64, vp]
    lib.rwh_orb_describe_batched.restype = i32
    lib.rwh_orb_describe_batched.argtypes = [vp, i64, vp, i32, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.rwh_host_orb_extract.restype = i32
    lib.rwh_host_orb_extract.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.rwh_orb_pyramid_bytes.restype = i64
    lib.rwh_orb_pyramid_bytes.argtypes = [i32, i32, vp, i32]
    lib.rwh_orb_pyramid_batched.restype = i32
    lib.rwh_orb_pyramid_batched.argtypes = [vp, i64, i64, vp, i32, vp, i32, vp, i64, vp]
    lib.rwh_host_orb_pyramid.restype = i32
    lib.rwh_host_orb_pyramid.argtypes = [vp, i32, i32, i32, vp, i32, vp, i64]
    lib.rwh_host_orb_extract_pyramid.restype = i32
    lib.rwh_host_orb_extract_pyramid.argtypes = [vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    # the sequence family (include/rwh.h: the sequence, gain, multi-band, projection, ring and seam rules).  Every entry point takes
    #     images hw mats rects n [anchor] | the operation's own | [col row] | [out] h w | [origin_x origin_y] | the operation's tail
    # with anchor and origin on the anchor's plane only (form ""), the ray tables on a curved ("_proj") or wrap-around ("_ring")
    # canvas only, and `workspace bytes stream` inside the tail; a host twin is the same list without those three.
    # kernels.SeqGeometry.layout lays the calls out in the same order.
    def front(form, own, canvas, tail):
        """An entry point's list up to `workspace bytes stream`."""
        if form == "":
            return [vp, vp, vp, vp, i32, i32] + own + canvas + [i32, i32] + tail
        return [vp, vp, vp, vp, i32] + own + [vp, vp] + canvas + tail

    def bind(name, types):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = i32, types

    ws, out, forms = [vp, i64, vp], [vp, i32, i32], ("", "_proj", "_ring")
    # the compositor: order blend | canvas h w | row_begin row_end, workspace bytes stream, gains.  On the plane the call with
    # gains is `_ex`, and the plain call is that list without gains
    for form in forms:
        f = front(form, [vp, i32], out, [i32, i32])
        bind("rwh_stitch_sequence" + (form or "_ex"), f + ws + [vp])
        bind("rwh_host_stitch_sequence" + (form or "_ex"), f + [vp])
    bind("rwh_stitch_sequence", lib.rwh_stitch_sequence_ex.argtypes[:-1])
    bind("rwh_host_stitch_sequence", lib.rwh_host_stitch_sequence_ex.argtypes[:-1])
    # the overlap statistics: nothing of their own | h w, no out | stride count sum, workspace bytes stream
    for form in forms:
        f = front(form, [], [i32, i32], [i32, vp, vp])
        bind("rwh_sequence_overlap_stats" + form, f + ws)
        bind("rwh_host_sequence_overlap_stats" + form, f)
    # multi-band: bands gains | canvas h w | workspace bytes stream
    for form in forms:
        f = front(form, [i32, vp], out, [])
        bind("rwh_stitch_multiband" + form, f + ws)
        bind("rwh_host_stitch_multiband" + form, f)
    for form in ("", "_proj"):                     # the seam rule has no ring form
        # multi-band with labels: bands gains labels | canvas h w | workspace bytes stream
        f = front(form, [i32, vp, vp], out, [])
        bind("rwh_stitch_multiband_labels" + form, f + ws)
        bind("rwh_host_stitch_multiband_labels" + form, f)
        # label paste: gains labels | canvas h w | workspace bytes stream
        f = front(form, [vp, vp], out, [])
        bind("rwh_stitch_sequence_labels" + form, f + ws)
        bind("rwh_host_stitch_sequence_labels" + form, f)
        # the seam finder: gains margin tau | labels h w | workspace bytes stream passes; the host twin has no passes
        f = front(form, [vp, f64, i32], out, [])
        bind("rwh_sequence_seams" + form, f + ws + [vp])
        bind("rwh_host_sequence_seams" + form, f)
    # their workspace sizes, and the gain rule's host solve
    for fn, types in ((lib.rwh_stitch_sequence_workspace_bytes, [i32]),                                       # n
                      (lib.rwh_sequence_overlap_stats_workspace_bytes, [i32, i32, i32, i32]),                 # n canvas h w stride
                      (lib.rwh_stitch_multiband_workspace_bytes, [vp, i32, i32, i32, i32, i32, i32]),         # rects n canvas h w origin_x origin_y bands
                      (lib.rwh_stitch_multiband_ring_workspace_bytes, [vp, i32, i32, i32, i32]),              # rects n canvas_h canvas_w bands
                      (lib.rwh_sequence_seams_workspace_bytes, [vp, i32, i32, i32, i32, i32])):               # rects n canvas h w origin_x origin_y
        fn.restype, fn.argtypes = i64, types
    lib.rwh_host_sequence_gains.restype = i32
    lib.rwh_host_sequence_gains.argtypes = [vp, vp, i32, f64, f64, vp]                   # count sum n sigma_n sigma_g gains
    # the block gain rule (no ring form): the cell statistics -- nothing of their own | h w, no out | shift stride slots tables,
    # workspace bytes stream -- and the compositor on gain maps: the compositor's list with `maps shift` where it has `gains`
    for form in forms[:2]:
        f = front(form, [], [i32, i32], [i32, i32, i32, vp])
        bind("rwh_sequence_cell_stats" + form, f + ws)
        bind("rwh_host_sequence_cell_stats" + form, f)
        f = front(form, [vp, i32], out, [i32, i32])
        bind("rwh_stitch_sequence_maps" + form, f + ws + [vp, i32])
        bind("rwh_host_stitch_sequence_maps" + form, f + [vp, i32])
        f = front(form, [i32, vp, i32, vp], out, [])                                     # multi-band: bands maps shift labels (or NULL)
        bind("rwh_stitch_multiband_maps" + form, f + ws)
        bind("rwh_host_stitch_multiband_maps" + form, f)
        f = front(form, [vp, i32, vp], out, [])                                          # label paste: maps shift labels
        bind("rwh_stitch_sequence_labels_maps" + form, f + ws)
        bind("rwh_host_stitch_sequence_labels_maps" + form, f)
    bind("rwh_sequence_cell_slots", [vp, i32, i32, i32, i32, i32, i32])                  # rects n canvas h w origin_x origin_y shift
    lib.rwh_sequence_cell_stats_workspace_bytes.restype, lib.rwh_sequence_cell_stats_workspace_bytes.argtypes = i64, [i32]
    lib.rwh_sequence_cell_stats_table_bytes.restype, lib.rwh_sequence_cell_stats_table_bytes.argtypes = i64, [i32, i32, i32, i32]
    # tables rects n canvas h w origin_x origin_y shift slots base sigma_n sigma_g smooth maps
    bind("rwh_host_sequence_block_gains", [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, f64, f64, i32, vp])
    # the bundle rule: the edge blocks (device and host twin) and the damped step
    lib.rwh_bundle_blocks.restype = i32
    lib.rwh_bundle_blocks.argtypes = [vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]     # pts_a pts_b offsets n_edges masks words T blocks count status stream
    lib.rwh_host_bundle_blocks.restype = i32
    lib.rwh_host_bundle_blocks.argtypes = [vp, vp, vp, i32, vp, i32, vp, vp, vp, vp]
    lib.rwh_host_bundle_step.restype = i32
    lib.rwh_host_bundle_step.argtypes = [i32, i32, vp, i32, vp, f64, vp, vp]            # n anchor edges n_edges blocks lambda delta status
    # the camera rule: the same three calls over rotations and focal lengths
    lib.rwh_camera_blocks.restype = i32
    lib.rwh_camera_blocks.argtypes = [vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]     # pts_a pts_b offsets n_edges masks words records blocks count status stream
    lib.rwh_host_camera_blocks.restype = i32
    lib.rwh_host_camera_blocks.argtypes = [vp, vp, vp, i32, vp, i32, vp, vp, vp, vp]
    lib.rwh_host_camera_step.restype = i32
    lib.rwh_host_camera_step.argtypes = [i32, i32, i32, vp, i32, vp, f64, vp, vp]       # n anchor focals edges n_edges blocks lambda delta status
    return lib


def load():
    """Load (once) and return the bound library.  torch must be imported first
    so that librwh_hip.so resolves libamdhip64.so.7 to the HIP runtime torch
    already mapped (one runtime per process: streams and pointers are shared)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RwhUnavailable(
                "%s not found: build it with `make -C ransac_with_homography_amd/csrc` "
                "(or `python -c 'import __graft_entry__ as g; g.build()'`)" % LIB_PATH)
        import torch  # noqa: F401  (maps the HIP runtime)
        try:
            _lib = _bind(ctypes.CDLL(LIB_PATH))
        except OSError as e:
            raise RwhUnavailable("cannot load %s: %s" % (LIB_PATH, e)) from e
        if _lib.rwh_abi_version() != ABI_VERSION:
            got = _lib.rwh_abi_version()
            _lib = None
            raise RwhUnavailable("librwh_hip.so reports ABI version %d, this package binds version %d: rebuild it "
                                 "(`make -C ransac_with_homography_amd/csrc`)" % (got, ABI_VERSION))
    return _lib


def require_gpu():
    """Return the torch device of the GPU the hot path runs on, or raise."""
    import torch
    if not torch.cuda.is_available():
        raise RwhUnavailable("no MI355X visible to this process: the RANSAC/warp hot path has no CPU fallback")
    load()
    return torch.device("cuda", torch.cuda.current_device())


def check(status, what):
    if status != 0:
        raise RwhError("%s failed: %s (%d)" % (what, load().rwh_strerror(status).decode(), status))


def stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
