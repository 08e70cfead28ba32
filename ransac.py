"""Drop-in module: `from ransac import stitching` (reference app.py:10) resolves to the
MI355X-backed implementation; `HomoModel`, `RANSAC`, `Model` likewise."""
from ransac_with_homography_amd.ransac import (DEBUG, LVL, HomoModel, Model, RANSAC, stitching, run_batch, DeviceProblems,  # noqa: F401
                                               match_descriptors, match_batch, extract_batch, detect_and_describe, default_pattern,
                                               rotate_pattern, orb_bin_table, orb_scales, orb_level_quotas,
                                               calcHomography, calcHomographyLinear, cylindericlMap,
                                               stitchPanorama, stitch_sequence, stitchSequence, sequence_plan, sequence_gains)
