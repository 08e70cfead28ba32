// rwh_camera.hip: the entry points of the camera rule (include/rwh.h): the normal-equation blocks of a bundle adjustment over
// rotations and focal lengths, one workgroup per edge, their host twin, and the damped Gauss-Newton step the host solves from them.
// The per-correspondence arithmetic is csrc/rwh_camera.h; the kernel, the twin and the solver are csrc/rwh_edge_blocks.h.
#include "rwh_camera.h"

extern "C" int rwh_camera_blocks(const float* d_pts_a, const float* d_pts_b, const int32_t* d_offsets, int n_edges, const uint64_t* d_masks,
                                 int mask_words, const double* d_records, double* d_blocks, int32_t* d_count, int32_t* d_status,
                                 void* stream) {
    return rwh_edge::device_blocks<rwh::CameraRule>(d_pts_a, d_pts_b, d_offsets, n_edges, d_masks, mask_words, d_records, d_blocks, d_count,
                                                    d_status, stream);
}

extern "C" int rwh_host_camera_blocks(const float* pts_a, const float* pts_b, const int32_t* offsets, int n_edges, const uint64_t* masks,
                                      int mask_words, const double* records, double* blocks, int32_t* count, int32_t* status) {
    return rwh_edge::host_blocks<rwh::CameraRule>(pts_a, pts_b, offsets, n_edges, masks, mask_words, records, blocks, count, status);
}

// Unknowns: omega of every image but the anchor (3 (n - 1), in image order), then the focal unknowns -- one per image, the
// anchor's included, or one for all.  With one focal for all, phi_s and phi_d of an edge meet in the same unknown and their cross
// term enters its diagonal twice.
extern "C" int rwh_host_camera_step(int n, int anchor, int focals, const int32_t* edges, int n_edges, const double* blocks, double lambda,
                                    double* out_delta, int32_t* out_status) {
    if (!rwh_edge::step_args_ok(n, anchor, edges, n_edges, blocks, lambda, out_delta, out_status) ||
        (focals != RWH_CAMERA_FOCAL_SHARED && focals != RWH_CAMERA_FOCAL_PER_IMAGE))
        return RWH_E_INVALID;
    const int n_rot = 3 * (n - 1);
    auto at = [&](int image, int k) {
        if (k == 3) return n_rot + (focals == RWH_CAMERA_FOCAL_PER_IMAGE ? image : 0);
        return image == anchor ? -1 : 3 * (image - (image > anchor)) + k;
    };
    return rwh_edge::host_step<rwh::CameraRule>(n, edges, n_edges, blocks, lambda, at, n_rot + (focals == RWH_CAMERA_FOCAL_PER_IMAGE ? n : 1),
                                                out_delta, out_status);
}
