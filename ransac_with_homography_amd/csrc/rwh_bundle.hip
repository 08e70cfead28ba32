// rwh_bundle.hip: the normal-equation blocks of a bundle adjustment over a pair graph (the bundle rule of include/rwh.h), one
// workgroup per edge, with their host twin, and the damped Gauss-Newton step the host solves from them.  The per-correspondence
// arithmetic and the block layout are csrc/rwh_bundle.h, shared by both sides.
#include <math.h>
#include <string.h>

#include <vector>

#include "rwh_common.h"
#include "rwh_bundle.h"

namespace rwh {

using namespace rwh_bundle;

// Edge e = blockIdx.x.  The edge's rows are taken CHUNK at a time.  Phase 1: lane t < CHUNK computes the 34 values of row base + t
// into LDS (STRIDE doubles apart) and a flag saying whether the row contributes.  Phase 2: wave w owns partial w -- the rows with
// index = w (mod 4), which it walks in increasing order; lane l holds the accumulators of entries l, l + 64 and l + 128 of the
// block.  A row is skipped by the whole wave (the flag is wave-uniform), its lanes read the same staged row at different columns.
// At the end entry e is (P0 + P1) + (P2 + P3).  No atomics: a rerun gives the same bits.
__global__ __launch_bounds__(THREADS) void bundle_blocks_kernel(const float* __restrict__ pts_a, const float* __restrict__ pts_b,
                                                                const int32_t* __restrict__ offsets, const uint64_t* __restrict__ masks,
                                                                int mask_words, const double* __restrict__ transfers,
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
    double T[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) T[i] = transfers[9ll * e + i];
    Entry ent[3];
    double acc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        ent[j] = entry_of(lane + 64 * j < BLOCK ? lane + 64 * j : 0);
        acc[j] = 0.0;
    }
    int32_t n_in = 0, n_bad = 0;
    for (long long base = 0; base < m; base += CHUNK) {
        if (tid < CHUNK) {
            const long long i = base + tid;
            int32_t f = 0;
            if (i < m && ((mrow[i >> 6] >> (i & 63)) & 1ull)) {
                const float* a = pts_a + 2 * (o0 + i);
                const float* b = pts_b + 2 * (o0 + i);
                if (row_values(T, a[0], a[1], b[0], b[1], rows + tid * STRIDE)) { f = 1; ++n_in; }
                else n_bad = 1;
            }
            flag[tid] = f;
        }
        __syncthreads();
        for (int r = wave; r < CHUNK; r += PARTIALS) {
            if (!flag[r]) continue;
            const double* row = rows + r * STRIDE;
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[j] = step(acc[j], row, ent[j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (lane + 64 * j < BLOCK) part[wave][lane + 64 * j] = acc[j];
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

static bool bundle_args_ok(const void* a, const void* b, const void* offsets, int n_edges, const void* masks, int mask_words, const void* t,
                           const void* blocks, const void* count, const void* status) {
    return a && b && offsets && masks && t && blocks && count && status && n_edges >= 1 && n_edges <= RWH_BUNDLE_MAX_EDGES && mask_words >= 1;
}

}  // namespace rwh

extern "C" int rwh_bundle_blocks(const float* d_pts_a, const float* d_pts_b, const int32_t* d_offsets, int n_edges, const uint64_t* d_masks,
                                 int mask_words, const double* d_transfers, double* d_blocks, int32_t* d_count, int32_t* d_status,
                                 void* stream) {
    using namespace rwh;
    if (!bundle_args_ok(d_pts_a, d_pts_b, d_offsets, n_edges, d_masks, mask_words, d_transfers, d_blocks, d_count, d_status)) return RWH_E_INVALID;
    hipLaunchKernelGGL(bundle_blocks_kernel, dim3((unsigned)n_edges), dim3(rwh_bundle::THREADS), 0, static_cast<hipStream_t>(stream), d_pts_a,
                       d_pts_b, d_offsets, d_masks, mask_words, d_transfers, d_blocks, d_count, d_status);
    return check_launch();
}

extern "C" int rwh_host_bundle_blocks(const float* pts_a, const float* pts_b, const int32_t* offsets, int n_edges, const uint64_t* masks,
                                      int mask_words, const double* transfers, double* blocks, int32_t* count, int32_t* status) {
    using namespace rwh_bundle;
    if (!rwh::bundle_args_ok(pts_a, pts_b, offsets, n_edges, masks, mask_words, transfers, blocks, count, status)) return RWH_E_INVALID;
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
            if (!row_values(transfers + 9ll * e, pts_a[2 * (o0 + i)], pts_a[2 * (o0 + i) + 1], pts_b[2 * (o0 + i)], pts_b[2 * (o0 + i) + 1], row)) {
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

// The damped step: the edge blocks scatter-added, in edge order, into the 8n x 8n system, the anchor's rows and columns dropped,
// lambda * diag(A) added (Marquardt scaling), A delta = -g solved by Cholesky (A = L L^T on the lower triangle).
extern "C" int rwh_host_bundle_step(int n, int anchor, const int32_t* edges, int n_edges, const double* blocks, double lambda,
                                    double* out_delta, int32_t* out_status) {
    using namespace rwh_bundle;
    if (!edges || !blocks || !out_delta || !out_status || n < 1 || n > RWH_SEQ_MAX_IMAGES || anchor < 0 || anchor >= n || n_edges < 1 ||
        n_edges > RWH_BUNDLE_MAX_EDGES || !(isfinite(lambda) && lambda >= 0.0))
        return RWH_E_INVALID;
    for (int e = 0; e < n_edges; ++e) {
        const int s = edges[2 * e], d = edges[2 * e + 1];
        if (s < 0 || s >= n || d < 0 || d >= n || s == d) return RWH_E_INVALID;
    }
    const int N = 8 * (n - 1);
    for (int i = 0; i < 8 * n; ++i) out_delta[i] = 0.0;
    *out_status = RWH_BUNDLE_OK;
    if (N == 0) return RWH_OK;
    std::vector<double> A((size_t)N * N, 0.0), g(N, 0.0);
    auto at = [&](int image, int k) { return image == anchor ? -1 : 8 * (image - (image > anchor)) + k; };
    for (int e = 0; e < n_edges; ++e) {
        const double* blk = blocks + (size_t)e * BLOCK;
        int where[PARAMS];
        for (int u = 0; u < PARAMS; ++u) where[u] = at(edges[2 * e + (u >= 8)], u & 7);
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
        for (int k = 0; k < 8; ++k)
            if (image != anchor) out_delta[8 * image + k] = z[at(image, k)];
    return RWH_OK;
}
