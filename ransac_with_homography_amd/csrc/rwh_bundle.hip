// rwh_bundle.hip: the entry points of the bundle rule (include/rwh.h): the normal-equation blocks of a bundle adjustment over a
// pair graph, one workgroup per edge, their host twin, and the damped Gauss-Newton step the host solves from them.  The
// per-correspondence arithmetic is csrc/rwh_bundle.h; the kernel, the twin and the solver are csrc/rwh_edge_blocks.h.
#include "rwh_bundle.h"

extern "C" int rwh_bundle_blocks(const float* d_pts_a, const float* d_pts_b, const int32_t* d_offsets, int n_edges, const uint64_t* d_masks,
                                 int mask_words, const double* d_transfers, double* d_blocks, int32_t* d_count, int32_t* d_status,
                                 void* stream) {
    return rwh_edge::device_blocks<rwh::BundleRule>(d_pts_a, d_pts_b, d_offsets, n_edges, d_masks, mask_words, d_transfers, d_blocks, d_count,
                                                    d_status, stream);
}

extern "C" int rwh_host_bundle_blocks(const float* pts_a, const float* pts_b, const int32_t* offsets, int n_edges, const uint64_t* masks,
                                      int mask_words, const double* transfers, double* blocks, int32_t* count, int32_t* status) {
    return rwh_edge::host_blocks<rwh::BundleRule>(pts_a, pts_b, offsets, n_edges, masks, mask_words, transfers, blocks, count, status);
}

// Unknowns: the 8 parameters of every image but the anchor, in image order; the anchor's rows and columns are dropped.
extern "C" int rwh_host_bundle_step(int n, int anchor, const int32_t* edges, int n_edges, const double* blocks, double lambda,
                                    double* out_delta, int32_t* out_status) {
    if (!rwh_edge::step_args_ok(n, anchor, edges, n_edges, blocks, lambda, out_delta, out_status)) return RWH_E_INVALID;
    auto at = [&](int image, int k) { return image == anchor ? -1 : 8 * (image - (image > anchor)) + k; };
    return rwh_edge::host_step<rwh::BundleRule>(n, edges, n_edges, blocks, lambda, at, 8 * (n - 1), out_delta, out_status);
}
