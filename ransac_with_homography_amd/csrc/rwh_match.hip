// rwh_match.hip: the brute-force Hamming matcher with cross-check in front of the batched RANSAC (the reference's
// cv2.BFMatcher(cv2.NORM_HAMMING, crossCheck=True).match + sorted(..., key=distance), ransac.py:258-261), for P image pairs in
// one submission.  The rule is stated in include/rwh.h; everything is an integer minimum, so the result is exact and does not
// depend on how the work is split.  rwh_host_match_hamming is the same rule in plain C++ for one pair.
//
// Work: one block per (problem, tile of MATCH_TILE_TRAIN train rows, segment of MATCH_SEG_QUERY query rows).  A lane keeps its
// train descriptor in NW dwords of registers; the query rows pass through LDS in chunks of MATCH_CHUNK_QUERY and are read at a
// wave-uniform address (every lane the same 16-byte slot: a broadcast, no bank conflict; 2 x ds_read_b128 per 32-byte row = 8 LDS
// cycles against 18 VALU instructions = 72 cycles, so the loop sits on the VALU).  Per pair and dword: one v_xor and one
// v_bcnt (popcount with accumulate); per pair one shift-or and one unsigned minimum on the packed key distance << 16 | row in
// segment, which implements "lowest query index on ties".  The segment's minimum goes into best_b[train row] with a 64-bit vector
// atomic minimum on distance << 32 | query index: partial minima of different segments combine to the same value in any order.
// The block list is built on the device (the problems' sizes live there): a prefix sum of blocks per problem, which a fixed
// grid walks with a stride.
#include "rwh_match.h"            // desc_dword, match_range, MATCH_NONE: shared with rwh_match_ratio.hip

namespace rwh {

static_assert(RWH_MATCH_SEG_QUERY % RWH_MATCH_CHUNK_QUERY == 0 && RWH_MATCH_SEG_QUERY <= 65536, "the row in its segment takes 16 bits");
// resets the two key arrays and (block 0) writes prefix[p] = blocks of the problems before p, prefix[P] = all
__global__ __launch_bounds__(256) void match_setup_kernel(const int32_t* __restrict__ offsets_a, const int32_t* __restrict__ offsets_b,
                                                          int n_problems, int total_a, int total_b,
                                                          unsigned long long* __restrict__ prefix, unsigned long long* __restrict__ best_a,
                                                          unsigned long long* __restrict__ best_b) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total_a; i += stride) best_a[i] = MATCH_NONE;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total_b; i += stride) best_b[i] = MATCH_NONE;
    if (blockIdx.x != 0) return;
    __shared__ unsigned long long part[256];
    const int per = (n_problems + 255) / 256;                       // a run of consecutive problems per thread
    const int p0 = min(n_problems, (int)threadIdx.x * per), p1 = min(n_problems, p0 + per);
    unsigned long long sum = 0;
    for (int p = p0; p < p1; ++p) {
        long long base; int na, nb;
        match_range(offsets_a, p, total_a, base, na);
        match_range(offsets_b, p, total_b, base, nb);
        sum += (unsigned long long)((na + RWH_MATCH_SEG_QUERY - 1) / RWH_MATCH_SEG_QUERY) *
               (unsigned long long)((nb + RWH_MATCH_TILE_TRAIN - 1) / RWH_MATCH_TILE_TRAIN);
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {                                         // 256 additions: exclusive scan of the runs
        unsigned long long run = 0;
        for (int t = 0; t < 256; ++t) { const unsigned long long v = part[t]; part[t] = run; run += v; }
        prefix[n_problems] = run;
    }
    __syncthreads();
    sum = part[threadIdx.x];
    for (int p = p0; p < p1; ++p) {
        long long base; int na, nb;
        match_range(offsets_a, p, total_a, base, na);
        match_range(offsets_b, p, total_b, base, nb);
        prefix[p] = sum;
        sum += (unsigned long long)((na + RWH_MATCH_SEG_QUERY - 1) / RWH_MATCH_SEG_QUERY) *
               (unsigned long long)((nb + RWH_MATCH_TILE_TRAIN - 1) / RWH_MATCH_TILE_TRAIN);
    }
}

// rule 1 (rwh.h): best_b[train row] = min over the query rows of distance << 32 | query index
template <int NW>
__global__ __launch_bounds__(RWH_MATCH_TILE_TRAIN) void match_train_kernel(const unsigned char* __restrict__ desc_a,
                                                                           const unsigned char* __restrict__ desc_b, int nbytes,
                                                                           const int32_t* __restrict__ offsets_a,
                                                                           const int32_t* __restrict__ offsets_b, int n_problems,
                                                                           int total_a, int total_b,
                                                                           const unsigned long long* __restrict__ prefix,
                                                                           unsigned long long* __restrict__ best_b) {
    __shared__ __attribute__((aligned(16))) uint32_t q[RWH_MATCH_CHUNK_QUERY][NW];
    const int tid = threadIdx.x;
    const unsigned long long n_work = prefix[n_problems];
    for (unsigned long long w = blockIdx.x; w < n_work; w += gridDim.x) {
        int lo = 0, hi = n_problems;                                // the problem that owns block w: the last p with prefix[p] <= w
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (prefix[mid] <= w) lo = mid; else hi = mid;
        }
        const int p = lo;
        long long a0, b0; int na, nb;
        match_range(offsets_a, p, total_a, a0, na);
        match_range(offsets_b, p, total_b, b0, nb);
        const unsigned long long r = w - prefix[p];
        const unsigned tiles = (unsigned)((nb + RWH_MATCH_TILE_TRAIN - 1) / RWH_MATCH_TILE_TRAIN);
        const int seg = (int)(r / tiles), tile = (int)(r % tiles);
        const int j = tile * RWH_MATCH_TILE_TRAIN + tid;
        const bool live = j < nb;
        uint32_t t[NW];
#pragma unroll
        for (int k = 0; k < NW; ++k) t[k] = live ? desc_dword(desc_b, b0 + j, nbytes, k) : 0u;
        const int i0 = seg * RWH_MATCH_SEG_QUERY, i1 = min(na, i0 + RWH_MATCH_SEG_QUERY);
        uint32_t best = 0xFFFFFFFFu;
        for (int c = i0; c < i1; c += RWH_MATCH_CHUNK_QUERY) {
            const int n = min(RWH_MATCH_CHUNK_QUERY, i1 - c);
            __syncthreads();                                        // the chunk before this one has been read by every wave
            for (int e = tid; e < n * NW; e += RWH_MATCH_TILE_TRAIN) q[e / NW][e % NW] = desc_dword(desc_a, a0 + c + e / NW, nbytes, e % NW);
            __syncthreads();
            const uint32_t row0 = (uint32_t)(c - i0);
#pragma unroll 4
            for (int rr = 0; rr < n; ++rr) {
                uint32_t d = 0;
#pragma unroll
                for (int k = 0; k < NW; ++k) d += (uint32_t)__popc(t[k] ^ q[rr][k]);
                best = min(best, (d << 16) | (row0 + (uint32_t)rr));
            }
        }
        if (live && i1 > i0)
            atomicMin(&best_b[b0 + j], ((unsigned long long)(best >> 16) << 32) | (unsigned long long)(uint32_t)(i0 + (int)(best & 0xFFFFu)));
    }
}

// rule 2: best_a[query row q[j]] = min over the train rows j that chose it of dT[j] << 32 | j
__global__ __launch_bounds__(256) void match_cross_kernel(const int32_t* __restrict__ offsets_a, const int32_t* __restrict__ offsets_b,
                                                          int n_problems, int total_a, int total_b,
                                                          const unsigned long long* __restrict__ best_b,
                                                          unsigned long long* __restrict__ best_a) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total_b) return;
    const unsigned long long key = best_b[g];
    if (key == MATCH_NONE) return;
    int lo = 0, hi = n_problems;                                    // the last p with offsets_b[p] <= g: the non-empty problem that owns row g
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets_b[mid] <= g) lo = mid; else hi = mid;
    }
    long long a0, b0; int na, nb;
    match_range(offsets_a, lo, total_a, a0, na);
    match_range(offsets_b, lo, total_b, b0, nb);
    const long long j = g - b0;
    const uint32_t qi = (uint32_t)key;
    if (j < 0 || j >= nb || qi >= (uint32_t)na) return;
    atomicMin(&best_a[a0 + qi], (key & 0xFFFFFFFF00000000ull) | (unsigned long long)j);
}

__global__ __launch_bounds__(256) void match_emit_kernel(int total_a, const unsigned long long* __restrict__ best_a,
                                                         int32_t* __restrict__ train_idx, int32_t* __restrict__ distance) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total_a) return;
    const unsigned long long key = best_a[i];
    const bool none = key == MATCH_NONE;
    train_idx[i] = none ? -1 : (int32_t)(uint32_t)key;
    distance[i] = none ? -1 : (int32_t)(key >> 32);
}

template <int NW>
static void launch_match_train(unsigned grid, hipStream_t s, const unsigned char* a, const unsigned char* b, int nbytes, const int32_t* oa,
                               const int32_t* ob, int n_problems, int total_a, int total_b, const unsigned long long* prefix,
                               unsigned long long* best_b) {
    hipLaunchKernelGGL(match_train_kernel<NW>, dim3(grid), dim3(RWH_MATCH_TILE_TRAIN), 0, s, a, b, nbytes, oa, ob, n_problems, total_a,
                       total_b, prefix, best_b);
}

}  // namespace rwh

extern "C" int64_t rwh_match_workspace_bytes(int n_problems, int total_a, int total_b) {
    if (n_problems <= 0 || total_a < 0 || total_b < 0) return RWH_E_INVALID;
    return 8ll * ((long long)total_a + (long long)total_b + (long long)n_problems + 1);
}

extern "C" int rwh_match_hamming_batched(const uint8_t* d_desc_a, const uint8_t* d_desc_b, int nbytes, const int32_t* d_offsets_a,
                                         const int32_t* d_offsets_b, int n_problems, int total_a, int total_b, int32_t* d_train_idx,
                                         int32_t* d_distance, void* d_workspace, int64_t workspace_bytes, void* stream) {
    using namespace rwh;
    if (!d_offsets_a || !d_offsets_b || !d_workspace || n_problems <= 0 || total_a < 0 || total_b < 0) return RWH_E_INVALID;
    if ((total_a > 0 && (!d_desc_a || !d_train_idx || !d_distance)) || (total_b > 0 && !d_desc_b)) return RWH_E_INVALID;
    if (workspace_bytes < rwh_match_workspace_bytes(n_problems, total_a, total_b) || ((uintptr_t)d_workspace & 7u)) return RWH_E_INVALID;
    if (nbytes < 1 || nbytes > RWH_MATCH_MAX_BYTES) return RWH_E_UNSUPPORTED;
    if (total_a == 0) return RWH_OK;                                // no query row, nothing to write
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long* best_a = static_cast<unsigned long long*>(d_workspace);
    unsigned long long* best_b = best_a + total_a;
    unsigned long long* prefix = best_b + total_b;
    const long long rows = total_a > total_b ? total_a : total_b;
    const unsigned fill = (unsigned)((rows + 255) / 256 < 1024 ? (rows + 255) / 256 : 1024);
    hipLaunchKernelGGL(match_setup_kernel, dim3(fill), dim3(256), 0, s, d_offsets_a, d_offsets_b, n_problems, total_a, total_b, prefix,
                       best_a, best_b);
    if (total_b > 0) {
        // at most (sum of tiles) x (sum of segments) blocks exist; the grid never needs more than that
        const unsigned long long bound = ((unsigned long long)total_b / RWH_MATCH_TILE_TRAIN + (unsigned)n_problems) *
                                         ((unsigned long long)total_a / RWH_MATCH_SEG_QUERY + (unsigned)n_problems);
        const unsigned grid = (unsigned)(bound < RWH_MATCH_GRID_MAX ? bound : RWH_MATCH_GRID_MAX);
        const int nw = (nbytes + 3) / 4;
        if (nw <= 1) launch_match_train<1>(grid, s, d_desc_a, d_desc_b, nbytes, d_offsets_a, d_offsets_b, n_problems, total_a, total_b, prefix, best_b);
        else if (nw <= 2) launch_match_train<2>(grid, s, d_desc_a, d_desc_b, nbytes, d_offsets_a, d_offsets_b, n_problems, total_a, total_b, prefix, best_b);
        else if (nw <= 4) launch_match_train<4>(grid, s, d_desc_a, d_desc_b, nbytes, d_offsets_a, d_offsets_b, n_problems, total_a, total_b, prefix, best_b);
        else if (nw <= 8) launch_match_train<8>(grid, s, d_desc_a, d_desc_b, nbytes, d_offsets_a, d_offsets_b, n_problems, total_a, total_b, prefix, best_b);
        else launch_match_train<16>(grid, s, d_desc_a, d_desc_b, nbytes, d_offsets_a, d_offsets_b, n_problems, total_a, total_b, prefix, best_b);
        hipLaunchKernelGGL(match_cross_kernel, dim3((unsigned)((total_b + 255ll) / 256)), dim3(256), 0, s, d_offsets_a, d_offsets_b, n_problems,
                           total_a, total_b, best_b, best_a);
    }
    hipLaunchKernelGGL(match_emit_kernel, dim3((unsigned)((total_a + 255ll) / 256)), dim3(256), 0, s, total_a, best_a, d_train_idx, d_distance);
    return check_launch();
}

extern "C" int rwh_host_match_hamming(const uint8_t* desc_a, int na, const uint8_t* desc_b, int nb, int nbytes, int32_t* train_idx,
                                      int32_t* distance) {
    if (na < 0 || nb < 0 || (na > 0 && (!desc_a || !train_idx || !distance)) || (nb > 0 && !desc_b)) return RWH_E_INVALID;
    if (nbytes < 1 || nbytes > RWH_MATCH_MAX_BYTES) return RWH_E_UNSUPPORTED;
    for (int i = 0; i < na; ++i) train_idx[i] = distance[i] = -1;
    if (na == 0) return RWH_OK;
    for (int j = 0; j < nb; ++j) {
        const uint8_t* b = desc_b + (size_t)j * nbytes;
        int q = 0, dq = 8 * RWH_MATCH_MAX_BYTES + 1;
        for (int i = 0; i < na; ++i) {                              // rule 1: the first strict minimum is the lowest i
            const uint8_t* a = desc_a + (size_t)i * nbytes;
            int d = 0;
            for (int k = 0; k < nbytes; ++k) d += __builtin_popcount((unsigned)(a[k] ^ b[k]));
            if (d < dq) { dq = d; q = i; }
        }
        if (train_idx[q] < 0 || dq < distance[q]) { train_idx[q] = j; distance[q] = dq; }   // rule 2: j ascends, so ties keep the lowest
    }
    return RWH_OK;
}
