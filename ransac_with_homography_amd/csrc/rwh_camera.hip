// rwh_camera.hip: the normal-equation blocks of a bundle adjustment over rotations and focal lengths (the camera rule of
// include/rwh.h), one workgroup per edge, with their host twin, and the damped Gauss-Newton step the host solves from them.  The
// per-correspondence arithmetic and the block layout are csrc/rwh_camera.h, shared by both sides.
#include <math.h>
#include <string.h>

#include <vector>

#include "rwh_common.h"
#include "rwh_camera.h"

namespace rwh {

using namespace rwh_camera;

// Edge e = blockIdx.x.  The edge's rows are taken CHUNK at a time.  Phase 1: lane t < CHUNK computes the 18 values of row base + t
// into LDS (STRIDE doubles apart) and a flag saying whether the row contributes.  Phase 2: wave w owns partial w -- the rows with
// index = w (mod 4), which it walks in increasing order; lane l < 45 holds the accumulator of entry l of the block, the other lanes
// of the wave hold none.  A row is skipped by the whole wave (the flag is wave-uniform), its lanes read the same staged row at
// different columns.  At the end entry e is (P0 + P1) + (P2 + P3).  No atomics: a rerun gives the same bits.
__global__ __launch_bounds__(THREADS) void camera_blocks_kernel(const float* __restrict__ pts_a, const float* __restrict__ pts_b,
                                                                const int32_t* __restrict__ offsets, const uint64_t* __restrict__ masks,
                                                                int mask_words, const double* __restrict__ records,
                                                                double* __restrict__ blocks, int32_t* __restrict__ count,
                                                                int32_t* __restrict__ status) {
    __shared__ double rows[CHUNK * STRIDE];
    __shared__ double part[PARTIALS][BLOCK];
    __shared__ int32_t flag[CHUNK];
    __shared__ int32_t tally[2][CHUNK];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & (RWH_WAVE - 1), wave = tid / RWH_WAVE;
    const long long o0 = offsets[e];
    long long m = (long long)offsets[e + 1] - o0;
    if (m > 64ll * mask_words) m = 64ll * mask_words;      // rows past the mask row are no inliers; nothing is read there
    const uint64_t* mrow = masks + (size_t)e * mask_words;
    double rec[RECORD];
#pragma unroll
    for (int i = 0; i < RECORD; ++i) rec[i] = records[(long long)RECORD * e + i];
    const Entry ent = entry_of(lane < BLOCK ? lane : 0);
    double acc = 0.0;
    int32_t n_in = 0, n_bad = 0;
    for (long long base = 0; base < m; base += CHUNK) {
        if (tid < CHUNK) {
            const long long i = base + tid;
            int32_t f = 0;
            if (i < m && ((mrow[i >> 6] >> (i & 63)) & 1ull)) {
                const float* a = pts_a + 2 * (o0 + i);
                const float* b = pts_b + 2 * (o0 + i);
                if (row_values(rec, a[0], a[1], b[0], b[1], rows + tid * STRIDE)) { f = 1; ++n_in; }
                else n_bad = 1;
            }
            flag[tid] = f;
        }
        __syncthreads();
        if (lane < BLOCK)
            for (int r = wave; r < CHUNK; r += PARTIALS) {
                if (!flag[r]) continue;
                acc = step(acc, rows + r * STRIDE, ent);
            }
        __syncthreads();
    }
    if (lane < BLOCK) part[wave][lane] = acc;
    if (tid < CHUNK) { tally[0][tid] = n_in; tally[1][tid] = n_bad; }
    __syncthreads();
    if (tid < BLOCK) blocks[(size_t)e * BLOCK + tid] = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
    if (tid == THREADS - 1) {
        int32_t n = 0, bad = 0;
        for (int t = 0; t < CHUNK; ++t) { n += tally[0][t]; bad |= tally[1][t]; }
        count[e] = n;
        status[e] = bad ? RWH_BUNDLE_BEHIND : RWH_BUNDLE_OK;
    }
}

static bool camera_args_ok(const void* a, const void* b, const void* offsets, int n_edges, const void* masks, int mask_words, const void* rec,
                           const void* blocks, const void* count, const void* status) {
    return a && b && offsets && masks && rec && blocks && count && status && n_edges >= 1 && n_edges <= RWH_BUNDLE_MAX_EDGES && mask_words >= 1;
}

}  // namespace rwh

extern "C" int rwh_camera_blocks(const float* d_pts_a, const float* d_pts_b, const int32_t* d_offsets, int n_edges, const uint64_t* d_masks,
                                 int mask_words, const double* d_records, double* d_blocks, int32_t* d_count, int32_t* d_status,
                                 void* stream) {
    using namespace rwh;
    if (!camera_args_ok(d_pts_a, d_pts_b, d_offsets, n_edges, d_masks, mask_words, d_records, d_blocks, d_count, d_status)) return RWH_E_INVALID;
    hipLaunchKernelGGL(camera_blocks_kernel, dim3((unsigned)n_edges), dim3(rwh_camera::THREADS), 0, static_cast<hipStream_t>(stream), d_pts_a,
                       d_pts_b, d_offsets, d_masks, mask_words, d_records, d_blocks, d_count, d_status);
    return check_launch();
}

extern "C" int rwh_host_camera_blocks(const float* pts_a, const float* pts_b, const int32_t* offsets, int n_edges, const uint64_t* masks,
                                      int mask_words, const double* records, double* blocks, int32_t* count, int32_t* status) {
    using namespace rwh_camera;
    if (!rwh::camera_args_ok(pts_a, pts_b, offsets, n_edges, masks, mask_words, records, blocks, count, status)) return RWH_E_INVALID;
    Entry ent[BLOCK];
    for (int t = 0; t < BLOCK; ++t) ent[t] = entry_of(t);
    for (int e = 0; e < n_edges; ++e) {
        const long long o0 = offsets[e];
        long long m = (long long)offsets[e + 1] - o0;
        if (m > 64ll * mask_words) m = 64ll * mask_words;
        const uint64_t* mrow = masks + (size_t)e * mask_words;
        double part[PARTIALS][BLOCK], row[ROW];
        memset(part, 0, sizeof(part));
        int32_t n_in = 0, bad = 0;
        for (long long i = 0; i < m; ++i) {
            if (!((mrow[i >> 6] >> (i & 63)) & 1ull)) continue;
            if (!row_values(records + (long long)RECORD * e, pts_a[2 * (o0 + i)], pts_a[2 * (o0 + i) + 1], pts_b[2 * (o0 + i)],
                            pts_b[2 * (o0 + i) + 1], row)) {
                bad = 1;
                continue;
            }
            ++n_in;
            double* p = part[i % PARTIALS];
            for (int t = 0; t < BLOCK; ++t) p[t] = step(p[t], row, ent[t]);
        }
        for (int t = 0; t < BLOCK; ++t) blocks[(size_t)e * BLOCK + t] = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
        count[e] = n_in;
        status[e] = bad ? RWH_BUNDLE_BEHIND : RWH_BUNDLE_OK;
    }
    return RWH_OK;
}

// The damped step.  Unknowns: omega of every image but the anchor (3 (n - 1), in image order), then the focal unknowns -- one per
// image, or one for all.  The edge blocks are scatter-added in edge order (with one focal for all, phi_s and phi_d of an edge meet in
// the same unknown and their cross term enters its diagonal twice), lambda * diag(A) is added (Marquardt scaling), A delta = -g is
// solved by Cholesky (A = L L^T on the lower triangle).
extern "C" int rwh_host_camera_step(int n, int anchor, int focals, const int32_t* edges, int n_edges, const double* blocks, double lambda,
                                    double* out_delta, int32_t* out_status) {
    using namespace rwh_camera;
    if (!edges || !blocks || !out_delta || !out_status || n < 1 || n > RWH_SEQ_MAX_IMAGES || anchor < 0 || anchor >= n || n_edges < 1 ||
        n_edges > RWH_BUNDLE_MAX_EDGES || !(isfinite(lambda) && lambda >= 0.0) ||
        (focals != RWH_CAMERA_FOCAL_SHARED && focals != RWH_CAMERA_FOCAL_PER_IMAGE))
        return RWH_E_INVALID;
    for (int e = 0; e < n_edges; ++e) {
        const int s = edges[2 * e], d = edges[2 * e + 1];
        if (s < 0 || s >= n || d < 0 || d >= n || s == d) return RWH_E_INVALID;
    }
    const int n_rot = 3 * (n - 1), N = n_rot + (focals == RWH_CAMERA_FOCAL_PER_IMAGE ? n : 1);
    for (int i = 0; i < 4 * n; ++i) out_delta[i] = 0.0;
    *out_status = RWH_BUNDLE_OK;
    std::vector<double> A((size_t)N * N, 0.0), g(N, 0.0);
    auto at = [&](int image, int k) {
        if (k == 3) return n_rot + (focals == RWH_CAMERA_FOCAL_PER_IMAGE ? image : 0);
        return image == anchor ? -1 : 3 * (image - (image > anchor)) + k;
    };
    for (int e = 0; e < n_edges; ++e) {
        const double* blk = blocks + (size_t)e * BLOCK;
        int where[PARAMS];
        for (int u = 0; u < PARAMS; ++u) where[u] = at(edges[2 * e + (u >= 4)], u & 3);
        int t = 0;
        for (int a = 0; a < PARAMS; ++a)
            for (int b = a; b < PARAMS; ++b, ++t) {
                if (where[a] < 0 || where[b] < 0) continue;
                A[(size_t)where[a] * N + where[b]] += blk[t];
                if (a != b) A[(size_t)where[b] * N + where[a]] += blk[t];
            }
        for (int u = 0; u < PARAMS; ++u)
            if (where[u] >= 0) g[where[u]] += blk[N_S + u];
    }
    for (int i = 0; i < N; ++i) A[(size_t)i * N + i] += lambda * A[(size_t)i * N + i];
    for (int j = 0; j < N; ++j) {
        double piv = A[(size_t)j * N + j];
        for (int k = 0; k < j; ++k) piv -= A[(size_t)j * N + k] * A[(size_t)j * N + k];
        if (!(piv > 0.0) || !isfinite(piv)) { *out_status = RWH_BUNDLE_SINGULAR; return RWH_OK; }
        const double l = sqrt(piv);
        A[(size_t)j * N + j] = l;
        for (int i = j + 1; i < N; ++i) {
            double v = A[(size_t)i * N + j];
            for (int k = 0; k < j; ++k) v -= A[(size_t)i * N + k] * A[(size_t)j * N + k];
            A[(size_t)i * N + j] = v / l;
        }
    }
    std::vector<double> z(N);
    for (int i = 0; i < N; ++i) {       // L z = -g
        double v = -g[i];
        for (int k = 0; k < i; ++k) v -= A[(size_t)i * N + k] * z[k];
        z[i] = v / A[(size_t)i * N + i];
    }
    for (int i = N - 1; i >= 0; --i) {  // L^T delta = z
        double v = z[i];
        for (int k = i + 1; k < N; ++k) v -= A[(size_t)k * N + i] * z[k];
        z[i] = v / A[(size_t)i * N + i];
    }
    for (int i = 0; i < N; ++i)
        if (!isfinite(z[i])) { *out_status = RWH_BUNDLE_SINGULAR; return RWH_OK; }
    for (int image = 0; image < n; ++image)
        for (int k = 0; k < 4; ++k) {
            const int w = at(image, k);
            if (w >= 0) out_delta[4 * image + k] = z[w];
        }
    return RWH_OK;
}
