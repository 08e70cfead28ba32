// rwh_match_ratio.hip: the Hamming matcher with Lowe's 2-nearest ratio test over a PAIR GRAPH: N images own one block of rows each
// of ONE descriptor array, and P pairs (s, d) name the query and the train image -- no descriptor is copied per pair.  The rule
// ("the ratio rule") is stated in include/rwh.h; everything is an integer, so the result is exact and does not depend on how the
// work is split.  rwh_host_match_ratio is the same rule in plain C++ for one pair.
//
// Work: match_train_kernel (rwh_match.hip) with the roles swapped.  One block per (pair, tile of MATCH2_TILE_QUERY query rows,
// segment of MATCH2_SEG_TRAIN train rows).  A lane keeps its QUERY descriptor in NW dwords of registers; the train rows pass through
// LDS in chunks of MATCH2_CHUNK_TRAIN and are read at a wave-uniform address (a broadcast).  Per descriptor pair: NW v_xor and NW
// v_bcnt (popcount with accumulate), one shift-or for the key distance << 16 | row in segment, and the top-2 update in three
// unsigned min / max: second = min(second, max(best, key)); best = min(best, key) -- both kept as keys, no shift in the loop:
// 2 NW + 4 = 20 vector instructions at 32 bytes.  The keys of one query are distinct (the row differs), so the update is a
// commutative and associative merge of sorted pairs: a block writes its (best, second) per query row as a PARTIAL, and
// match2_merge_kernel merges a row's partials in segment order, applies the ratio on integers and claims owner[train row] with the
// 64-bit vector atomicMin on d1 << 32 | i (rule 3: the smallest d1, the lowest i).  match2_emit_kernel keeps the claimants.  No
// atomic touches the top-2 and there is no float.  The block list is built on the device (prefix sums over the pairs) and walked
// by a fixed grid: four launches, whatever P.
#include <vector>

#include "rwh_match.h"

namespace rwh {

static_assert(RWH_MATCH2_SEG_TRAIN % RWH_MATCH2_CHUNK_TRAIN == 0 && RWH_MATCH2_SEG_TRAIN <= 65536, "the row in its segment takes 16 bits");
static_assert(RWH_MATCH2_TILE_QUERY == 256, "the kernels below are launched with 256 threads, one query row per lane");

constexpr uint32_t MATCH2_NO_KEY = 0xFFFFFFFFu;

// What the setup kernel leaves per pair, P + 1 entries each (exclusive prefix sums, entry P = the total): blocks of the main kernel,
// query rows (= the pair's first output row), train rows (= its first owner slot), partials.
struct Match2Tables {
    unsigned long long* blocks;
    unsigned long long* query;
    unsigned long long* train;
    unsigned long long* partial;
};

// rows of image `img`, or 0 rows for an image outside 0 .. n_images - 1 or a range outside [0, total_rows]
__device__ __forceinline__ void match2_image(const int32_t* __restrict__ image_offsets, int n_images, int total_rows, int img,
                                             long long& base, int& n) {
    base = 0;
    n = 0;
    if (img >= 0 && img < n_images) match_range(image_offsets, img, total_rows, base, n);
}

__device__ __forceinline__ unsigned long long match2_segments(int nb) {
    return (unsigned long long)((nb + RWH_MATCH2_SEG_TRAIN - 1) / RWH_MATCH2_SEG_TRAIN);
}

// A pair is LIVE when its output rows, owner slots and partials all lie inside what the caller gave (total_query, total_train, the
// workspace): the sums run over the pairs in order, so behind the first pair that is not live none is.  Only live pairs are worked
// on; with consistent arguments every pair is live.
__device__ __forceinline__ bool match2_live(const Match2Tables& t, int p, int total_query, int total_train, unsigned long long capacity) {
    return t.query[p + 1] <= (unsigned long long)total_query && t.train[p + 1] <= (unsigned long long)total_train &&
           t.partial[p + 1] <= capacity;
}

// the last p in [0, n) with prefix[p] <= v (prefix[0] == 0): the entry that owns v when v < prefix[n]
__device__ __forceinline__ int match2_owner(const unsigned long long* __restrict__ prefix, int n, unsigned long long v) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// resets owner[] and (block 0) writes the four prefix tables
__global__ __launch_bounds__(256) void match2_setup_kernel(const int32_t* __restrict__ image_offsets, int n_images, int total_rows,
                                                           const int32_t* __restrict__ pairs, int n_pairs, int total_query, int total_train,
                                                           unsigned long long capacity, Match2Tables t,
                                                           unsigned long long* __restrict__ owner) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total_train; i += stride) owner[i] = MATCH_NONE;
    if (blockIdx.x != 0) return;
    __shared__ unsigned long long part[3][256];
    const int per = (n_pairs + 255) / 256;                          // a run of consecutive pairs per thread
    const int p0 = min(n_pairs, (int)threadIdx.x * per), p1 = min(n_pairs, p0 + per);
    unsigned long long sq = 0, st = 0, sp = 0;
    for (int p = p0; p < p1; ++p) {
        long long base; int na, nb;
        match2_image(image_offsets, n_images, total_rows, pairs[2 * p], base, na);
        match2_image(image_offsets, n_images, total_rows, pairs[2 * p + 1], base, nb);
        sq += (unsigned long long)na;
        st += (unsigned long long)nb;
        sp += (unsigned long long)na * match2_segments(nb);
    }
    part[0][threadIdx.x] = sq; part[1][threadIdx.x] = st; part[2][threadIdx.x] = sp;
    __syncthreads();
    if (threadIdx.x < 3) {                                          // 256 additions each: exclusive scans of the runs
        unsigned long long run = 0;
        for (int k = 0; k < 256; ++k) { const unsigned long long v = part[threadIdx.x][k]; part[threadIdx.x][k] = run; run += v; }
        (threadIdx.x == 0 ? t.query : threadIdx.x == 1 ? t.train : t.partial)[n_pairs] = run;
    }
    __syncthreads();
    sq = part[0][threadIdx.x]; st = part[1][threadIdx.x]; sp = part[2][threadIdx.x];
    __syncthreads();                                                // part[0] is used again for the blocks
    unsigned long long sb = 0;
    for (int p = p0; p < p1; ++p) {
        long long base; int na, nb;
        match2_image(image_offsets, n_images, total_rows, pairs[2 * p], base, na);
        match2_image(image_offsets, n_images, total_rows, pairs[2 * p + 1], base, nb);
        t.query[p] = sq; t.train[p] = st; t.partial[p] = sp;
        sq += (unsigned long long)na;
        st += (unsigned long long)nb;
        sp += (unsigned long long)na * match2_segments(nb);
        const bool live = sq <= (unsigned long long)total_query && st <= (unsigned long long)total_train && sp <= capacity;   // match2_live
        // nb < 2: rule 1 has no second distance, the pair has no candidate and no block
        const unsigned long long n_blocks = live && nb >= 2 ? (unsigned long long)((na + RWH_MATCH2_TILE_QUERY - 1) / RWH_MATCH2_TILE_QUERY) * match2_segments(nb) : 0ull;
        t.blocks[p] = n_blocks;                                     // the count now, the prefix below: this thread's own entries
        sb += n_blocks;
    }
    part[0][threadIdx.x] = sb;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int k = 0; k < 256; ++k) { const unsigned long long v = part[0][k]; part[0][k] = run; run += v; }
        t.blocks[n_pairs] = run;
    }
    __syncthreads();
    sb = part[0][threadIdx.x];
    for (int p = p0; p < p1; ++p) {
        const unsigned long long n_blocks = t.blocks[p];
        t.blocks[p] = sb;
        sb += n_blocks;
    }
}

// rule 1 inside one train segment: partial[(pair, query row, segment)] = the two smallest keys distance << 16 | row in segment
template <int NW>
__global__ __launch_bounds__(RWH_MATCH2_TILE_QUERY) void match2_query_kernel(const unsigned char* __restrict__ desc, int nbytes,
                                                                             const int32_t* __restrict__ image_offsets, int n_images,
                                                                             int total_rows, const int32_t* __restrict__ pairs, int n_pairs,
                                                                             Match2Tables tb, uint2* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) uint32_t t[RWH_MATCH2_CHUNK_TRAIN][NW];
    const int tid = threadIdx.x;
    const unsigned long long n_work = tb.blocks[n_pairs];
    for (unsigned long long w = blockIdx.x; w < n_work; w += gridDim.x) {
        const int p = match2_owner(tb.blocks, n_pairs, w);         // the pair that owns block w
        long long a0, b0; int na, nb;
        match2_image(image_offsets, n_images, total_rows, pairs[2 * p], a0, na);
        match2_image(image_offsets, n_images, total_rows, pairs[2 * p + 1], b0, nb);
        const unsigned long long r = w - tb.blocks[p];
        const unsigned segs = (unsigned)match2_segments(nb);
        const int tile = (int)(r / segs), seg = (int)(r % segs);
        const int i = tile * RWH_MATCH2_TILE_QUERY + tid;
        const bool live = i < na;
        uint32_t q[NW];
#pragma unroll
        for (int k = 0; k < NW; ++k) q[k] = live ? desc_dword(desc, a0 + i, nbytes, k) : 0u;
        const int j0 = seg * RWH_MATCH2_SEG_TRAIN, j1 = min(nb, j0 + RWH_MATCH2_SEG_TRAIN);
        uint32_t best = MATCH2_NO_KEY, second = MATCH2_NO_KEY;
        for (int c = j0; c < j1; c += RWH_MATCH2_CHUNK_TRAIN) {
            const int n = min(RWH_MATCH2_CHUNK_TRAIN, j1 - c);
            __syncthreads();                                        // the chunk before this one has been read by every wave
            for (int e = tid; e < n * NW; e += RWH_MATCH2_TILE_QUERY) t[e / NW][e % NW] = desc_dword(desc, b0 + c + e / NW, nbytes, e % NW);
            __syncthreads();
            const uint32_t row0 = (uint32_t)(c - j0);
#pragma unroll 4
            for (int rr = 0; rr < n; ++rr) {
                uint32_t d = 0;
#pragma unroll
                for (int k = 0; k < NW; ++k) d += (uint32_t)__popc(q[k] ^ t[rr][k]);
                const uint32_t key = (d << 16) | (row0 + (uint32_t)rr);
                second = min(second, max(best, key));
                best = min(best, key);
            }
        }
        if (live) partial[tb.partial[p] + (unsigned long long)i * segs + (unsigned)seg] = make_uint2(best, second);
    }
}

// rules 1 (across the segments), 2 and the claim of rule 3: per query row.  Writes (j1, d1, d2) for a candidate, -1 / -1 / -1 else.
__global__ __launch_bounds__(256) void match2_merge_kernel(const int32_t* __restrict__ image_offsets, int n_images, int total_rows,
                                                           const int32_t* __restrict__ pairs, int n_pairs, int total_query, int total_train,
                                                           unsigned long long capacity, int ratio_num, int ratio_den, Match2Tables tb,
                                                           const uint2* __restrict__ partial, unsigned long long* __restrict__ owner,
                                                           int32_t* __restrict__ train_idx, int32_t* __restrict__ distance,
                                                           int32_t* __restrict__ second_out) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total_query) return;
    int32_t out_j = -1, out_d = -1, out_s = -1;
    if ((unsigned long long)g < tb.query[n_pairs]) {
        const int p = match2_owner(tb.query, n_pairs, (unsigned long long)g);      // the non-empty pair that owns row g
        long long base; int nb;
        match2_image(image_offsets, n_images, total_rows, pairs[2 * p + 1], base, nb);
        if (nb >= 2 && match2_live(tb, p, total_query, total_train, capacity)) {
            const unsigned long long i = (unsigned long long)g - tb.query[p];
            const unsigned segs = (unsigned)match2_segments(nb);
            const uint2* mine = partial + tb.partial[p] + i * segs;
            unsigned long long best = MATCH_NONE, second = MATCH_NONE;
#pragma unroll 4                                                    // four partials in flight: a long train side is a chain of loads
            for (unsigned s = 0; s < segs; ++s) {
                const uint2 k2 = mine[s];
                const unsigned long long row0 = (unsigned long long)s * RWH_MATCH2_SEG_TRAIN;
                // distance << 32 | train row: distinct over the whole pair, so the merge gives the same two keys in any order
                const unsigned long long kb = ((unsigned long long)(k2.x >> 16) << 32) | (row0 + (k2.x & 0xFFFFu));
                const unsigned long long ks = k2.y == MATCH2_NO_KEY ? MATCH_NONE : ((unsigned long long)(k2.y >> 16) << 32) | (row0 + (k2.y & 0xFFFFu));
                second = min(second, max(best, kb));
                best = min(best, kb);
                second = min(second, ks);                           // ks > kb >= best: it can only be the runner-up
            }
            const long long d1 = (long long)(best >> 32), d2 = (long long)(second >> 32);
            if (second != MATCH_NONE && (long long)ratio_den * d1 < (long long)ratio_num * d2) {      // rule 2: integers, strict
                out_j = (int32_t)(uint32_t)best; out_d = (int32_t)d1; out_s = (int32_t)d2;
                atomicMin(&owner[tb.train[p] + (uint32_t)best], ((unsigned long long)d1 << 32) | i);
            }
        }
    }
    train_idx[g] = out_j; distance[g] = out_d; second_out[g] = out_s;
}

// rule 3: a candidate that is not the claimant of its train row has no match
__global__ __launch_bounds__(256) void match2_emit_kernel(int n_pairs, int total_query, Match2Tables tb,
                                                          const unsigned long long* __restrict__ owner, int32_t* __restrict__ train_idx,
                                                          int32_t* __restrict__ distance, int32_t* __restrict__ second_out) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total_query) return;
    const int32_t j = train_idx[g];
    if (j < 0) return;                                              // no candidate (the merge kernel wrote only candidates of live pairs)
    const int p = match2_owner(tb.query, n_pairs, (unsigned long long)g);
    const unsigned long long i = (unsigned long long)g - tb.query[p];
    if (owner[tb.train[p] + (uint32_t)j] != (((unsigned long long)(uint32_t)distance[g] << 32) | i))
        train_idx[g] = distance[g] = second_out[g] = -1;
}

template <int NW>
static void launch_match2_query(unsigned grid, hipStream_t s, const unsigned char* desc, int nbytes, const int32_t* image_offsets,
                                int n_images, int total_rows, const int32_t* pairs, int n_pairs, Match2Tables tb, uint2* partial) {
    hipLaunchKernelGGL(match2_query_kernel<NW>, dim3(grid), dim3(RWH_MATCH2_TILE_QUERY), 0, s, desc, nbytes, image_offsets, n_images,
                       total_rows, pairs, n_pairs, tb, partial);
}

static long long match2_max_segments(int max_train_rows) {
    return ((long long)(max_train_rows > 1 ? max_train_rows : 1) + RWH_MATCH2_SEG_TRAIN - 1) / RWH_MATCH2_SEG_TRAIN;
}

}  // namespace rwh

extern "C" int64_t rwh_match_ratio_workspace_bytes(int n_pairs, int total_query, int total_train, int max_train_rows) {
    if (n_pairs <= 0 || total_query < 0 || total_train < 0 || max_train_rows < 0) return RWH_E_INVALID;
    // owner[total_train], four tables of P + 1, one partial per query row and segment of the longest train side
    return 8ll * ((long long)total_train + 4ll * ((long long)n_pairs + 1) + (long long)total_query * rwh::match2_max_segments(max_train_rows));
}

extern "C" int rwh_match_ratio_graph(const uint8_t* d_desc, int nbytes, const int32_t* d_image_offsets, int n_images, int total_rows,
                                     const int32_t* d_pairs, int n_pairs, int total_query, int total_train, int ratio_num, int ratio_den,
                                     int32_t* d_train_idx, int32_t* d_distance, int32_t* d_second, void* d_workspace,
                                     int64_t workspace_bytes, void* stream) {
    using namespace rwh;
    if (!d_image_offsets || !d_pairs || !d_workspace || n_images <= 0 || n_pairs <= 0 || total_rows < 0 || total_query < 0 || total_train < 0)
        return RWH_E_INVALID;
    if (ratio_num <= 0 || ratio_num > ratio_den || ratio_den > RWH_MATCH2_RATIO_MAX) return RWH_E_INVALID;
    if ((total_rows > 0 && !d_desc) || (total_query > 0 && (!d_train_idx || !d_distance || !d_second))) return RWH_E_INVALID;
    const long long fixed = 8ll * ((long long)total_train + 4ll * ((long long)n_pairs + 1));
    if (workspace_bytes < rwh_match_ratio_workspace_bytes(n_pairs, total_query, total_train, 0) || ((uintptr_t)d_workspace & 7u)) return RWH_E_INVALID;
    if (nbytes < 1 || nbytes > RWH_MATCH_MAX_BYTES) return RWH_E_UNSUPPORTED;
    if (total_query == 0) return RWH_OK;                            // no query row, nothing to write
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long* owner = static_cast<unsigned long long*>(d_workspace);
    Match2Tables tb;
    tb.blocks = owner + total_train;
    tb.query = tb.blocks + n_pairs + 1;
    tb.train = tb.query + n_pairs + 1;
    tb.partial = tb.train + n_pairs + 1;
    uint2* partial = reinterpret_cast<uint2*>(tb.partial + n_pairs + 1);
    // the partials the workspace holds: a pair whose partials would pass it is not worked on (match2_live), so a workspace sized
    // for a smaller max_train_rows than the pairs have costs matches, never a write outside it
    const unsigned long long capacity = (unsigned long long)((workspace_bytes - fixed) / 8);
    const unsigned fill = (unsigned)(((long long)total_train + 255) / 256 < 1024 ? ((long long)total_train + 255) / 256 : 1024);
    hipLaunchKernelGGL(match2_setup_kernel, dim3(fill < 1 ? 1 : fill), dim3(256), 0, s, d_image_offsets, n_images, total_rows, d_pairs, n_pairs,
                       total_query, total_train, capacity, tb, owner);
    if (total_train > 0) {
        // at most (sum of tiles) x (sum of segments) blocks exist; the grid never needs more than that
        const unsigned long long bound = ((unsigned long long)total_query / RWH_MATCH2_TILE_QUERY + (unsigned)n_pairs) *
                                         ((unsigned long long)total_train / RWH_MATCH2_SEG_TRAIN + (unsigned)n_pairs);
        const unsigned grid = (unsigned)(bound < RWH_MATCH2_GRID_MAX ? bound : RWH_MATCH2_GRID_MAX);
        const int nw = (nbytes + 3) / 4;
        if (nw <= 1) launch_match2_query<1>(grid, s, d_desc, nbytes, d_image_offsets, n_images, total_rows, d_pairs, n_pairs, tb, partial);
        else if (nw <= 2) launch_match2_query<2>(grid, s, d_desc, nbytes, d_image_offsets, n_images, total_rows, d_pairs, n_pairs, tb, partial);
        else if (nw <= 4) launch_match2_query<4>(grid, s, d_desc, nbytes, d_image_offsets, n_images, total_rows, d_pairs, n_pairs, tb, partial);
        else if (nw <= 8) launch_match2_query<8>(grid, s, d_desc, nbytes, d_image_offsets, n_images, total_rows, d_pairs, n_pairs, tb, partial);
        else launch_match2_query<16>(grid, s, d_desc, nbytes, d_image_offsets, n_images, total_rows, d_pairs, n_pairs, tb, partial);
    }
    const unsigned rows = (unsigned)((total_query + 255ll) / 256);
    hipLaunchKernelGGL(match2_merge_kernel, dim3(rows), dim3(256), 0, s, d_image_offsets, n_images, total_rows, d_pairs, n_pairs, total_query,
                       total_train, capacity, ratio_num, ratio_den, tb, partial, owner, d_train_idx, d_distance, d_second);
    hipLaunchKernelGGL(match2_emit_kernel, dim3(rows), dim3(256), 0, s, n_pairs, total_query, tb, owner, d_train_idx, d_distance, d_second);
    return check_launch();
}

extern "C" int rwh_host_match_ratio(const uint8_t* desc_a, int na, const uint8_t* desc_b, int nb, int nbytes, int ratio_num, int ratio_den,
                                    int32_t* train_idx, int32_t* distance, int32_t* second) {
    if (na < 0 || nb < 0 || (na > 0 && (!desc_a || !train_idx || !distance || !second)) || (nb > 0 && !desc_b)) return RWH_E_INVALID;
    if (ratio_num <= 0 || ratio_num > ratio_den || ratio_den > RWH_MATCH2_RATIO_MAX) return RWH_E_INVALID;
    if (nbytes < 1 || nbytes > RWH_MATCH_MAX_BYTES) return RWH_E_UNSUPPORTED;
    for (int i = 0; i < na; ++i) train_idx[i] = distance[i] = second[i] = -1;
    if (nb < 2) return RWH_OK;                                      // rule 1: no second distance, no candidate
    std::vector<int> holder((size_t)nb, -1);                        // rule 3: the query that holds train row j so far
    for (int i = 0; i < na; ++i) {
        const uint8_t* a = desc_a + (size_t)i * nbytes;
        const int none = 8 * RWH_MATCH_MAX_BYTES + 1;
        int j1 = 0, d1 = none, d2 = none;
        for (int j = 0; j < nb; ++j) {                              // rule 1: the first strict minimum is the lowest j
            const uint8_t* b = desc_b + (size_t)j * nbytes;
            int d = 0;
            for (int k = 0; k < nbytes; ++k) d += __builtin_popcount((unsigned)(a[k] ^ b[k]));
            if (d < d1) { d2 = d1; d1 = d; j1 = j; }
            else if (d < d2) d2 = d;
        }
        if ((long long)ratio_den * d1 >= (long long)ratio_num * d2) continue;                        // rule 2
        const int h = holder[j1];                                   // i ascends: the holder has the smallest d1 so far and, on ties, the lowest i
        if (h >= 0 && distance[h] <= d1) continue;
        if (h >= 0) train_idx[h] = distance[h] = second[h] = -1;
        holder[j1] = i;
        train_idx[i] = j1; distance[i] = d1; second[i] = d2;
    }
    return RWH_OK;
}
