// rwh_refit.hip: the final N-point refit of RANSAC.run (ransac.py:206-211 -> homography.py:90-105 with collective=True) for the
// winners of a batched search, on the device: one workgroup per problem accumulates the 23 float64 moments of A^T A and A^T b over
// the problem's inliers, solves the 8 x 8 system and corrects the solution once by the residual of the correspondences
// (csrc/rwh_refit.h).  Not the reference's float32 bits: the same least-squares problem, solved in float64 (include/rwh.h).
// rwh_host_refit runs the same operations in the same order on the host.
#include "rwh_common.h"
#include "rwh_refit.h"

namespace rwh {

using namespace rwh_refit;

// The block's sum of each lane's s[0 .. N): the wave's shuffle-down tree, then waves 0..3 in order by thread 0, whose s holds the
// sums on return -- a fixed order without atomics, so a rerun gives the same bits.  Every thread of the block calls it.
template <int N>
__device__ __forceinline__ void block_sum(double* s, double (*red)[N_MOMENTS]) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double v = s[j];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, RWH_WAVE);
        s[j] = v;
    }
    const int lane = threadIdx.x & (RWH_WAVE - 1), wave = threadIdx.x / RWH_WAVE;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) red[wave][j] = s[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            double v = red[0][j];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) v += red[w][j];
            s[j] = v;
        }
    }
}

// Problem p = blockIdx.x.  Lane t takes correspondences t, t + 256, ...; the word holding a correspondence's bit is uniform over
// each run of 64 lanes.  Two passes over the inliers, each summed per lane in index order and then by block_sum: the moments, which
// thread 0 solves, and -- only where the solve says it pays (CORRECT_ABOVE, csrc/rwh_refit.h) -- the residual sums of that
// solution, by which thread 0 corrects it.
__global__ __launch_bounds__(THREADS) void refit_kernel(const float* __restrict__ pts_a, const float* __restrict__ pts_b,
                                                        const int32_t* __restrict__ offsets, const uint64_t* __restrict__ masks,
                                                        int mask_words, double* __restrict__ h_out, int32_t* __restrict__ status) {
    __shared__ double red[WAVES][N_MOMENTS];
    __shared__ double h_first[N_RESIDUALS];
    __shared__ int st_first, again;
    const int p = blockIdx.x;
    const long long o0 = offsets[p];
    long long m = (long long)offsets[p + 1] - o0;
    if (m > 64ll * mask_words) m = 64ll * mask_words;      // correspondences past the mask row are no inliers; nothing is read there
    const uint64_t* row = masks + (size_t)p * mask_words;
    double s[N_MOMENTS];
#pragma unroll
    for (int j = 0; j < N_MOMENTS; ++j) s[j] = 0.0;
    for (long long i = threadIdx.x; i < m; i += THREADS) {
        if ((row[i >> 6] >> (i & 63)) & 1ull) {
            const float* a = pts_a + 2 * (o0 + i);
            const float* b = pts_b + 2 * (o0 + i);
            moment_update(s, a[0], a[1], b[0], b[1]);
        }
    }
    block_sum<N_MOMENTS>(s, red);
    Factor f;
    double h9[9];
    if (threadIdx.x == 0) {
        st_first = solve(s, f, h9);
        again = st_first == RWH_REFIT_OK && inverse_trace(f) >= CORRECT_ABOVE;
#pragma unroll
        for (int i = 0; i < N_RESIDUALS; ++i) h_first[i] = h9[i];
    }
    __syncthreads();                    // h_first, st_first and again are written; thread 0 has read red
    if (!again) {                       // the same value in every thread: the block leaves together
        if (threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) h_out[9ll * p + i] = h9[i];
            status[p] = st_first;
        }
        return;
    }
    double h[N_RESIDUALS], t[N_RESIDUALS];
#pragma unroll
    for (int j = 0; j < N_RESIDUALS; ++j) { h[j] = h_first[j]; t[j] = 0.0; }
    for (long long i = threadIdx.x; i < m; i += THREADS) {
        if ((row[i >> 6] >> (i & 63)) & 1ull) {
            const float* a = pts_a + 2 * (o0 + i);
            const float* b = pts_b + 2 * (o0 + i);
            residual_update(t, h, a[0], a[1], b[0], b[1]);
        }
    }
    block_sum<N_RESIDUALS>(t, red);
    if (threadIdx.x == 0) {
        const int st = correct(f, t, h9);
#pragma unroll
        for (int i = 0; i < 9; ++i) h_out[9ll * p + i] = h9[i];
        status[p] = st;
    }
}

}  // namespace rwh

extern "C" int rwh_refit_batched(const float* d_pts_a, const float* d_pts_b, const int32_t* d_offsets, int n_problems,
                                 const uint64_t* d_masks, int mask_words, double* d_h, int32_t* d_status, void* stream) {
    using namespace rwh;
    if (!d_pts_a || !d_pts_b || !d_offsets || !d_masks || !d_h || !d_status || n_problems <= 0 || mask_words <= 0) return RWH_E_INVALID;
    hipLaunchKernelGGL(refit_kernel, dim3((unsigned)n_problems), dim3(rwh_refit::THREADS), 0, static_cast<hipStream_t>(stream),
                       d_pts_a, d_pts_b, d_offsets, d_masks, mask_words, d_h, d_status);
    return check_launch();
}

// the kernel's block_sum over the 256 per-lane partials part[t][0 .. n): each wave's tree, then waves 0..3 in order
static void host_block_sum(const double (*part)[rwh_refit::N_MOMENTS], int n, double* s) {
    using namespace rwh_refit;
    double v[64];
    for (int j = 0; j < n; ++j) {
        for (int w = 0; w < WAVES; ++w) {
            for (int l = 0; l < 64; ++l) v[l] = part[64 * w + l][j];
            const double t = wave_tree(v);
            s[j] = w == 0 ? t : s[j] + t;
        }
    }
}

extern "C" int rwh_host_refit(const float* pts_a, const float* pts_b, int m, const uint64_t* mask_words, double* out_h9,
                              int32_t* out_status) {
    using namespace rwh_refit;
    if (!pts_a || !pts_b || !mask_words || !out_h9 || !out_status || m < 0) return RWH_E_INVALID;
    static thread_local double part[THREADS][N_MOMENTS];     // the kernel's 256 per-lane partial sums
    for (int t = 0; t < THREADS; ++t)
        for (int j = 0; j < N_MOMENTS; ++j) part[t][j] = 0.0;
    for (int i = 0; i < m; ++i)
        if ((mask_words[i >> 6] >> (i & 63)) & 1ull)
            moment_update(part[i % THREADS], pts_a[2ll * i], pts_a[2ll * i + 1], pts_b[2ll * i], pts_b[2ll * i + 1]);
    double s[N_MOMENTS];
    host_block_sum(part, N_MOMENTS, s);
    Factor f;
    *out_status = solve(s, f, out_h9);
    if (!(*out_status == RWH_REFIT_OK && inverse_trace(f) >= CORRECT_ABOVE)) return RWH_OK;
    for (int t = 0; t < THREADS; ++t)
        for (int j = 0; j < N_RESIDUALS; ++j) part[t][j] = 0.0;
    for (int i = 0; i < m; ++i)
        if ((mask_words[i >> 6] >> (i & 63)) & 1ull)
            residual_update(part[i % THREADS], out_h9, pts_a[2ll * i], pts_a[2ll * i + 1], pts_b[2ll * i], pts_b[2ll * i + 1]);
    host_block_sum(part, N_RESIDUALS, s);
    *out_status = correct(f, s, out_h9);
    return RWH_OK;
}
