// rwh_edge_blocks.h: what the registration rules of include/rwh.h (the bundle rule, the camera rule) do not decide, written once for
// both: the layout of an edge's block, the kernel that sums it (one workgroup per edge), its host twin, and the damped Gauss-Newton
// step the host solves from the blocks.  A RULE is a struct with
//   PARAMS   columns of J: the parameters of image s, then those of image d (PARAMS / 2 each)
//   RECORD   float64 the host hands over per edge
//   static RWH_HD bool row_values(const double* record, float x, float y, float bx, float by, double* out)
//            the ROW values [J[0][0 .. PARAMS), J[1][0 .. PARAMS), r0, r1] of one correspondence; false, with out unspecified,
//            for a correspondence that is not valid
// (csrc/rwh_bundle.h, csrc/rwh_camera.h).  Everything is float64 and no operation is contracted.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "rwh_common.h"

#pragma clang fp contract(off)

#ifndef RWH_HD
#define RWH_HD __host__ __device__ __forceinline__
#endif

namespace rwh_edge {

static constexpr int PARTIALS = 4;                          // partial sums over rows with index = 0, 1, 2, 3 (mod 4)
static constexpr int CHUNK = 128;                           // rows the kernel stages in LDS at a time (a multiple of PARTIALS)
static constexpr int THREADS = 64 * PARTIALS;               // one wave per partial

struct Entry { int i0, j0, i1, j1; };

template <class Rule>
struct Layout {
    static constexpr int PARAMS = Rule::PARAMS;
    static constexpr int ROW = 2 * PARAMS + 2;              // J[0][0 .. PARAMS), J[1][0 .. PARAMS), r0, r1
    static constexpr int N_S = PARAMS * (PARAMS + 1) / 2;   // upper triangle of S, row-major
    static constexpr int BLOCK = N_S + PARAMS + 1;          // S, g, c
    static constexpr int STRIDE = ROW + 1;                  // doubles per staged row: odd, so that 16 lanes' 8-byte stores meet no bank twice
    static constexpr int ACCS = (BLOCK + 63) / 64;          // accumulators per lane: lane l holds entries l, l + 64, ...
    static constexpr int LANES = BLOCK < 64 ? BLOCK : 64;   // BLOCK <= 64: one lane of a wave per block entry, the others hold none

    // Entry e of a block is the sum over the edge's rows of row[i0] * row[j0] + row[i1] * row[j1]:
    //   e < N_S: S[a][b], a <= b, row-major upper triangle: J[0][a] J[0][b] + J[1][a] J[1][b]
    //   N_S <= e < N_S + PARAMS: g[k], k = e - N_S: J[0][k] r0 + J[1][k] r1
    //   e == N_S + PARAMS: c = r0 r0 + r1 r1
    static RWH_HD Entry entry_of(int e) {
        if (e >= N_S + PARAMS) return {2 * PARAMS, 2 * PARAMS, 2 * PARAMS + 1, 2 * PARAMS + 1};
        if (e >= N_S) return {e - N_S, 2 * PARAMS, PARAMS + e - N_S, 2 * PARAMS + 1};
        int a = 0, left = e;
        while (left >= PARAMS - a) { left -= PARAMS - a; ++a; }
        return {a, a + left, PARAMS + a, PARAMS + a + left};
    }
};

// one step of an accumulator: both products rounded, their sum rounded, then the addition
RWH_HD double step(double acc, const double* row, const Entry& t) {
    return acc + (row[t.i0] * row[t.j0] + row[t.i1] * row[t.j1]);
}

// Edge e = blockIdx.x.  The edge's rows are taken CHUNK at a time.  Phase 1: lane t < CHUNK computes the ROW values of row base + t
// into LDS (STRIDE doubles apart) and a flag saying whether the row contributes.  Phase 2: wave w owns partial w -- the rows with
// index = w (mod 4), which it walks in increasing order; lane l < LANES holds the accumulators of entries l, l + 64, ... of the
// block (three for the bundle rule's 153, one for the camera rule's 45).  A row is skipped by the whole wave (the flag is
// wave-uniform), its lanes read the same staged row at different columns.  At the end entry e is (P0 + P1) + (P2 + P3).  No
// atomics: a rerun gives the same bits.
template <class Rule>
__global__ __launch_bounds__(THREADS) void edge_blocks_kernel(const float* __restrict__ pts_a, const float* __restrict__ pts_b,
                                                              const int32_t* __restrict__ offsets, const uint64_t* __restrict__ masks,
                                                              int mask_words, const double* __restrict__ records,
                                                              double* __restrict__ blocks, int32_t* __restrict__ count,
                                                              int32_t* __restrict__ status) {
    constexpr int RECORD = Rule::RECORD, BLOCK = Layout<Rule>::BLOCK, STRIDE = Layout<Rule>::STRIDE, ACCS = Layout<Rule>::ACCS;
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
    Entry ent[ACCS];
    double acc[ACCS];
#pragma unroll
    for (int j = 0; j < ACCS; ++j) {
        ent[j] = Layout<Rule>::entry_of(lane + 64 * j < BLOCK ? lane + 64 * j : 0);
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
                if (Rule::row_values(rec, a[0], a[1], b[0], b[1], rows + tid * STRIDE)) { f = 1; ++n_in; }
                else n_bad = 1;
            }
            flag[tid] = f;
        }
        __syncthreads();
        if (lane < Layout<Rule>::LANES)
            for (int r = wave; r < CHUNK; r += PARTIALS) {
                if (!flag[r]) continue;
                const double* row = rows + r * STRIDE;
#pragma unroll
                for (int j = 0; j < ACCS; ++j) acc[j] = step(acc[j], row, ent[j]);
            }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < ACCS; ++j)
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

static inline bool args_ok(const void* a, const void* b, const void* offsets, int n_edges, const void* masks, int mask_words, const void* rec,
                           const void* blocks, const void* count, const void* status) {
    return a && b && offsets && masks && rec && blocks && count && status && n_edges >= 1 && n_edges <= RWH_BUNDLE_MAX_EDGES && mask_words >= 1;
}

// rwh_<rule>_blocks: the kernel on `stream`, one workgroup per edge.
template <class Rule>
int device_blocks(const float* d_pts_a, const float* d_pts_b, const int32_t* d_offsets, int n_edges, const uint64_t* d_masks, int mask_words,
                  const double* d_records, double* d_blocks, int32_t* d_count, int32_t* d_status, void* stream) {
    if (!args_ok(d_pts_a, d_pts_b, d_offsets, n_edges, d_masks, mask_words, d_records, d_blocks, d_count, d_status)) return RWH_E_INVALID;
    hipLaunchKernelGGL(edge_blocks_kernel<Rule>, dim3((unsigned)n_edges), dim3(THREADS), 0, static_cast<hipStream_t>(stream), d_pts_a, d_pts_b,
                       d_offsets, d_masks, mask_words, d_records, d_blocks, d_count, d_status);
    return rwh::check_launch();
}

// rwh_host_<rule>_blocks: the kernel's host twin, the same operations in the same order.
template <class Rule>
int host_blocks(const float* pts_a, const float* pts_b, const int32_t* offsets, int n_edges, const uint64_t* masks, int mask_words,
                const double* records, double* blocks, int32_t* count, int32_t* status) {
    constexpr int RECORD = Rule::RECORD, BLOCK = Layout<Rule>::BLOCK;
    if (!args_ok(pts_a, pts_b, offsets, n_edges, masks, mask_words, records, blocks, count, status)) return RWH_E_INVALID;
    Entry ent[BLOCK];
    for (int t = 0; t < BLOCK; ++t) ent[t] = Layout<Rule>::entry_of(t);
    for (int e = 0; e < n_edges; ++e) {
        const long long o0 = offsets[e];
        long long m = (long long)offsets[e + 1] - o0;
        if (m > 64ll * mask_words) m = 64ll * mask_words;
        const uint64_t* mrow = masks + (size_t)e * mask_words;
        double part[PARTIALS][BLOCK], row[Layout<Rule>::ROW];
        memset(part, 0, sizeof(part));
        int32_t n_in = 0, bad = 0;
        for (long long i = 0; i < m; ++i) {
            if (!((mrow[i >> 6] >> (i & 63)) & 1ull)) continue;
            if (!Rule::row_values(records + (long long)RECORD * e, pts_a[2 * (o0 + i)], pts_a[2 * (o0 + i) + 1], pts_b[2 * (o0 + i)],
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

// What both steps refuse with RWH_E_INVALID.
static inline bool step_args_ok(int n, int anchor, const int32_t* edges, int n_edges, const double* blocks, double lambda,
                                const double* out_delta, const int32_t* out_status) {
    if (!edges || !blocks || !out_delta || !out_status || n < 1 || n > RWH_SEQ_MAX_IMAGES || anchor < 0 || anchor >= n || n_edges < 1 ||
        n_edges > RWH_BUNDLE_MAX_EDGES || !(isfinite(lambda) && lambda >= 0.0))
        return false;
    for (int e = 0; e < n_edges; ++e) {
        const int s = edges[2 * e], d = edges[2 * e + 1];
        if (s < 0 || s >= n || d < 0 || d >= n || s == d) return false;
    }
    return true;
}

// The edge blocks scatter-added, in edge order, into the N x N system A (row-major, both triangles) and g.  at(image, k) is the
// unknown of parameter k (0 .. PARAMS / 2) of an image, or < 0 for a parameter that is held fixed.  Two parameters of an edge may
// share an unknown: their cross term then enters its diagonal twice.
template <class Rule, class At>
void scatter_blocks(const int32_t* edges, int n_edges, const double* blocks, At at, int N, std::vector<double>& A, std::vector<double>& g) {
    constexpr int PARAMS = Rule::PARAMS, HALF = PARAMS / 2, N_S = Layout<Rule>::N_S, BLOCK = Layout<Rule>::BLOCK;
    for (int e = 0; e < n_edges; ++e) {
        const double* blk = blocks + (size_t)e * BLOCK;
        int where[PARAMS];
        for (int u = 0; u < PARAMS; ++u) where[u] = at(edges[2 * e + (u >= HALF)], u % HALF);
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
}

// The damped step: lambda * diag(A) added (Marquardt scaling), A delta = -g solved by Cholesky (A = L L^T on the lower triangle,
// in place) -> delta in z.  false (RWH_BUNDLE_SINGULAR) on a pivot that is not > 0 and finite or a delta that is not finite.
static inline bool solve_damped(std::vector<double>& A, const std::vector<double>& g, int N, double lambda, std::vector<double>& z) {
    for (int i = 0; i < N; ++i) A[(size_t)i * N + i] += lambda * A[(size_t)i * N + i];
    for (int j = 0; j < N; ++j) {
        double piv = A[(size_t)j * N + j];
        for (int k = 0; k < j; ++k) piv -= A[(size_t)j * N + k] * A[(size_t)j * N + k];
        if (!(piv > 0.0) || !isfinite(piv)) return false;
        const double l = sqrt(piv);
        A[(size_t)j * N + j] = l;
        for (int i = j + 1; i < N; ++i) {
            double v = A[(size_t)i * N + j];
            for (int k = 0; k < j; ++k) v -= A[(size_t)i * N + k] * A[(size_t)j * N + k];
            A[(size_t)i * N + j] = v / l;
        }
    }
    z.resize(N);
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
        if (!isfinite(z[i])) return false;
    return true;
}

// rwh_host_<rule>_step after its argument checks: the system of N unknowns assembled and solved; the WIDTH = PARAMS / 2 parameters
// of every image written to out_delta (zero where at() < 0, and everywhere on RWH_BUNDLE_SINGULAR).
template <class Rule, class At>
int host_step(int n, const int32_t* edges, int n_edges, const double* blocks, double lambda, At at, int N, double* out_delta,
              int32_t* out_status) {
    constexpr int WIDTH = Rule::PARAMS / 2;
    for (int i = 0; i < WIDTH * n; ++i) out_delta[i] = 0.0;
    *out_status = RWH_BUNDLE_OK;
    if (N == 0) return RWH_OK;          // nothing but the anchor: nothing is allocated
    std::vector<double> A((size_t)N * N, 0.0), g(N, 0.0), z;
    scatter_blocks<Rule>(edges, n_edges, blocks, at, N, A, g);
    if (!solve_damped(A, g, N, lambda, z)) { *out_status = RWH_BUNDLE_SINGULAR; return RWH_OK; }
    for (int image = 0; image < n; ++image)
        for (int k = 0; k < WIDTH; ++k) {
            const int w = at(image, k);
            if (w >= 0) out_delta[WIDTH * image + k] = z[w];
        }
    return RWH_OK;
}

}  // namespace rwh_edge
