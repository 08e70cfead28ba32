// Sequence compositor (include/rwh.h, "The sequence rule"): N images, each warped ONCE by its own homography into the anchor's
// frame, every canvas pixel written ONCE.  The reference composites two images per call (stitchPanorama, homography.py:288-338);
// this is its paste compositor generalised to N images, plus a feather blend, and at N = 2 / paste it produces stitchPanorama's bytes.
// The sampling recipe is stitch_pixel's (rwh_stitch.hip), restated here: float64, dgemm k-order, IEEE divides, separately rounded
// lerps.  The pixel function is compiled for the device and for the host (rwh_host_stitch_sequence), so the two run one arithmetic.
#include "rwh_sequence.h"

namespace rwh {

// stitch_kernel's shape (rwh_stitch.hip): 256 lanes as 64 x 4, four consecutive pixels per lane (SEQ_PX), the 12 output bytes in
// one store.  A block's 256 x 4 tile is tested once against the n rectangles; blockIdx and the descriptor indices are wave-uniform,
// so the test and the descriptor reads of the pixel loop stay on the scalar side.
// RING: the canvas is a whole number of tiles wide (checked before the launch), so every lane has its four pixels and there is no
// tail path.
// L: the launch record, SeqWith<SeqArgs, GAIN, PROJ> or SeqWithMaps<SeqArgs, PROJ> -- one body for every state of the gain switch.
template <bool FEATHER, bool GAIN, bool PROJ, bool RING, class L>
__global__ __launch_bounds__(256) void seq_kernel(const L l) {
    static_assert(SEQ_RING_TILE == 64 * SEQ_PX, "a ring canvas is made of whole tiles");
    const SeqArgs& a = l.a;
    const int bx0 = blockIdx.x * 64 * SEQ_PX, by0 = a.row_begin + blockIdx.y * 4;
    const uint64_t cand = seq_tile_mask<RING>(a, bx0, bx0 + 64 * SEQ_PX, by0, by0 + 4);
    const int cx0 = bx0 + (threadIdx.x & 63) * SEQ_PX;
    const int cy = by0 + seq_wave_row<PROJ>(threadIdx.x >> 6);
    if ((!RING && cx0 >= a.fw) || cy >= a.row_end) return;
    unsigned char* out = a.dst + ((size_t)cy * a.fw + cx0) * 3;
    uint32_t px[SEQ_PX];
#pragma unroll
    for (int j = 0; j < SEQ_PX; ++j)
        px[j] = (RING || cx0 + j < a.fw) ? seq_pixel<FEATHER, GAIN, PROJ, RING>(a, cand, cx0 + j, cy, seq_gains(l), seq_rays(l)) : 0u;
    if (RING || cx0 + SEQ_PX <= a.fw) {
        pk3 w;
        w.a = px[0] | (px[1] << 24);
        w.b = (px[1] >> 8) | (px[2] << 16);
        w.c = (px[2] >> 16) | (px[3] << 8);
        __builtin_memcpy(out, &w, 12);
    } else {
        for (int j = 0; cx0 + j < a.fw; ++j) { out[3 * j] = (unsigned char)px[j]; out[3 * j + 1] = (unsigned char)(px[j] >> 8); out[3 * j + 2] = (unsigned char)(px[j] >> 16); }
    }
}

// A host table of the family (descriptors, the multi-band windows) travels in kernel arguments, SEQ_PUT_WORDS eight-byte words per
// launch (64 descriptors are 6.5 KB: more than one launch's 4 KB of arguments), and this kernel lays them down in the workspace:
// stream-ordered, no host buffer that has to outlive the call.
constexpr int SEQ_PUT_WORDS = 32 * SEQ_DESC_WORDS;
struct SeqPut { uint64_t w[SEQ_PUT_WORDS]; };
__global__ __launch_bounds__(256) void seq_put_kernel(const SeqPut c, uint64_t* out, int words) {
    for (int t = threadIdx.x; t < words; t += 256) out[t] = c.w[t];
}
void seq_put(const void* host, size_t words, uint64_t* dev, hipStream_t s) {
    for (size_t at = 0; at < words; at += SEQ_PUT_WORDS) {
        const int cnt = (int)(words - at < (size_t)SEQ_PUT_WORDS ? words - at : (size_t)SEQ_PUT_WORDS);
        SeqPut c;
        memset(&c, 0, sizeof(c));
        memcpy(c.w, static_cast<const uint64_t*>(host) + at, (size_t)cnt * 8);
        hipLaunchKernelGGL(seq_put_kernel, dim3(1), dim3(256), 0, s, c, dev + at, cnt);
    }
}

// ---- the gain rule's overlap statistics (include/rwh.h); the per-sample functions are rwh_sequence.h's ----
struct StatArgs {
    SeqArgs a;                  // order: 0 .. n-1 (candidate bits are image indices); dst, row_begin, row_end unused
    int stride, nsx, nsy;       // the sample grid: nsx x nsy samples, sample (u, v) is canvas pixel (u * stride, v * stride)
    unsigned long long* slabs;  // STAT_SLABS slabs of slab_words words, zeroed on the stream before the launch: count [n][n], then sum [n][n]
    int slab_words;
};
// Every block adds its pairs into ONE of STAT_SLABS copies of the two tables (a whole number of 128-byte lines each), and a second
// kernel sums the copies into the caller's tables: with one copy, the atomics of thousands of blocks queue on the one cache line
// that holds count[0][0] and sum[0][0] of a two-image strip.
constexpr int STAT_SLABS = 64;
__host__ __device__ __forceinline__ int seq_slab_words(int n) { return (2 * n * n + 15) & ~15; }

// The candidates of the samples [u0, u1) x [v0, v1): the images whose rectangles meet the canvas pixels between the first and the
// last of them.
template <bool RING = false>
__host__ __device__ __forceinline__ uint64_t seq_stat_mask(const StatArgs& s, int u0, int u1, int v0, int v1) {
    return seq_tile_mask<RING>(s.a, u0 * s.stride, (u1 - 1) * s.stride + 1, v0 * s.stride, (v1 - 1) * s.stride + 1);
}

// A block takes 256 x 4 samples (64 lanes x 4 consecutive samples, one wave per sample row) and tests their footprint once against
// the n rectangles.  Pass 1: every lane's coverage masks.  Pass 2, over the candidate pairs (block-uniform, so the loops stay on the
// scalar side): the lanes' L_i and one wave sum per live pair of (count << 20 | sum), added into 32-bit LDS accumulators of the same
// packing, indexed by candidate rank -- a block has 1024 samples: count <= 2^10 and sum <= 1024 * 765 < 2^20 -- then one 64-bit
// integer atomic add per non-zero count and sum per block, into the block's slab.  Integer adds commute: the tables do not depend
// on the order.
constexpr int STAT_W = 256, STAT_H = 4;
template <bool PROJ = false, bool RING = false>
__global__ __launch_bounds__(256) void seq_stats_kernel(const SeqWith<StatArgs, false, PROJ> l) {
    const StatArgs& s = l.a;
    static_assert(STAT_W * STAT_H * 765 < (1 << 20) && STAT_W * STAT_H < (1 << 12), "count << 20 | sum in 32 bits");
    __shared__ uint32_t acc[RWH_SEQ_MAX_IMAGES * RWH_SEQ_MAX_IMAGES];
    __shared__ unsigned char ids[RWH_SEQ_MAX_IMAGES];
    const SeqArgs& a = s.a;
    const int u0 = blockIdx.x * STAT_W, v0 = blockIdx.y * STAT_H;
    const int u1 = u0 + STAT_W < s.nsx ? u0 + STAT_W : s.nsx, v1 = v0 + STAT_H < s.nsy ? v0 + STAT_H : s.nsy;
    const uint64_t cand = seq_stat_mask<RING>(s, u0, u1, v0, v1);
    const int nc = __builtin_popcountll(cand);
    if (nc == 0) return;                                   // (block-uniform)
    for (int t = threadIdx.x; t < nc * nc; t += 256) acc[t] = 0u;
    if (threadIdx.x < RWH_SEQ_MAX_IMAGES && (cand >> threadIdx.x & 1))
        ids[__builtin_popcountll(cand & ((1ull << threadIdx.x) - 1))] = (unsigned char)threadIdx.x;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int u = u0 + lane * SEQ_PX, v = v0 + seq_wave_row<PROJ>(threadIdx.x >> 6);
    const int cy = v * s.stride;
    uint64_t cov[SEQ_PX];
#pragma unroll
    for (int k = 0; k < SEQ_PX; ++k) cov[k] = (u + k < s.nsx && v < s.nsy) ? seq_cover<PROJ, RING>(a, cand, (u + k) * s.stride, cy, seq_rays(l)) : 0ull;
    int ri = 0;
    for (uint64_t mi = cand; mi; mi &= mi - 1, ++ri) {
        const int i = __builtin_ctzll(mi);
        uint32_t L[SEQ_PX];
        bool any = false;
#pragma unroll
        for (int k = 0; k < SEQ_PX; ++k) {
            const bool c = cov[k] >> i & 1;
            L[k] = c ? seq_byte_sum<PROJ, RING>(a, i, (u + k) * s.stride, cy, seq_rays(l)) : 0u;
            any |= c;
        }
        if (!__any(any)) continue;                         // (wave-uniform)
        int rj = 0;
        for (uint64_t mj = cand; mj; mj &= mj - 1, ++rj) {
            const int j = __builtin_ctzll(mj);
            uint32_t p = 0u;
#pragma unroll
            for (int k = 0; k < SEQ_PX; ++k)
                if ((cov[k] >> i) & (cov[k] >> j) & 1) p += (1u << 20) + L[k];
            if (!__any(p != 0u)) continue;                 // (wave-uniform: i and j meet at none of the wave's samples)
            p = seq_wave_sum(p);
            if (lane == 0 && p) atomicAdd(&acc[ri * nc + rj], p);
        }
    }
    __syncthreads();
    unsigned long long* slab = s.slabs + (size_t)((blockIdx.y * gridDim.x + blockIdx.x) % STAT_SLABS) * s.slab_words;
    for (int t = threadIdx.x; t < nc * nc; t += 256) {
        const uint32_t c = acc[t] >> 20, l = acc[t] & 0xfffffu;
        if (!c) continue;
        const size_t at = (size_t)ids[t / nc] * a.n + ids[t % nc];
        atomicAdd(&slab[at], (unsigned long long)c);
        if (l) atomicAdd(&slab[(size_t)a.n * a.n + at], (unsigned long long)l);
    }
}

// count and sum (nn words each) = the sum of the slabs: writes both tables whole.
__global__ __launch_bounds__(256) void seq_stats_sum_kernel(const unsigned long long* slabs, int slab_words, int nn,
                                                            unsigned long long* count, unsigned long long* sum) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 2 * nn) return;
    unsigned long long total = 0;
    for (int r = 0; r < STAT_SLABS; ++r) total += slabs[(size_t)r * slab_words + t];
    if (t < nn) count[t] = total; else sum[t - nn] = total;
}

// What both statistics entry points check, and their arguments: rwh_stitch_sequence's checks (with the index order, no canvas
// buffer and all rows) plus the stride range.
static int seq_stat_prepare(const SeqCall& c, int stride, uint64_t* count, uint64_t* sum, SeqDesc* descs, StatArgs& s, bool device) {
    if (!count || !sum || stride < 1 || stride > 255) return RWH_E_INVALID;
    const int st = seq_prepare_indexed(c, count, descs, s.a, device);
    if (st != RWH_OK) return st;
    s.a.dst = nullptr;
    s.stride = stride;
    s.nsx = (c.canvas_w + stride - 1) / stride;
    s.nsy = (c.canvas_h + stride - 1) / stride;
    s.slabs = nullptr;
    s.slab_words = seq_slab_words(c.n);
    return RWH_OK;
}

// The device compositor behind every rwh_stitch_sequence* entry point: the three forms, the two blends and the three states of
// the gain switch.
static int seq_device(const SeqCall& c, const int32_t* order, int blend, void* d_canvas, int row_begin, int row_end, void* d_workspace,
                      int64_t workspace_bytes, void* stream, SeqGain gain) {
    SeqDesc descs[RWH_SEQ_MAX_IMAGES];
    SeqArgs a;
    const int st = seq_prepare(c, order, blend, d_canvas, row_begin, row_end, descs, a, true);
    if (st != RWH_OK) return st;
    if (!seq_gain_ok(gain, c, false)) return RWH_E_INVALID;
    if (!d_workspace || workspace_bytes < rwh_stitch_sequence_workspace_bytes(c.n) || ((uintptr_t)d_workspace & 7u)) return RWH_E_INVALID;
    if (row_begin == row_end) return RWH_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint64_t* table = static_cast<uint64_t*>(d_workspace);
    seq_put(descs, (size_t)c.n * SEQ_DESC_WORDS, table, s);
    a.desc = reinterpret_cast<const SeqDesc*>(table);
    const dim3 grid((c.canvas_w + 64 * SEQ_PX - 1) / (64 * SEQ_PX), (row_end - row_begin + 3) / 4);
    seq_form_dispatch(c.form, [&](auto form) {
        constexpr bool PROJ = decltype(form)::proj, RING = decltype(form)::ring;
        seq_dispatch<!RING>(blend == RWH_SEQ_FEATHER, gain, [&](auto feather, auto on, auto value) {
            auto l = seq_with<decltype(on)::value, PROJ>(a, value, c.n, c.rays);
            hipLaunchKernelGGL((seq_kernel<decltype(feather)::value, decltype(on)::value, PROJ, RING, decltype(l)>), grid, dim3(256), 0, s, l);
        });
    });
    return check_launch();
}

static int seq_host(const SeqCall& c, const int32_t* order, int blend, void* canvas, int row_begin, int row_end, SeqGain gain) {
    SeqDesc descs[RWH_SEQ_MAX_IMAGES];
    SeqArgs a;
    const int st = seq_prepare(c, order, blend, canvas, row_begin, row_end, descs, a, false);
    if (st != RWH_OK) return st;
    if (!seq_gain_ok(gain, c, true)) return RWH_E_INVALID;
    seq_form_dispatch(c.form, [&](auto form) {
        constexpr bool PROJ = decltype(form)::proj, RING = decltype(form)::ring;
        seq_dispatch<!RING>(blend == RWH_SEQ_FEATHER, gain, [&](auto feather, auto on, auto value) {
            seq_host_rows<decltype(feather)::value, decltype(on)::value, PROJ, RING>(a, value, c.rays);
        });
    });
    return RWH_OK;
}

static int seq_stat_device(const SeqCall& c, int stride, uint64_t* d_count, uint64_t* d_sum, void* d_workspace, int64_t workspace_bytes,
                           void* stream) {
    SeqDesc descs[RWH_SEQ_MAX_IMAGES];
    StatArgs a;
    const int n = c.n;
    const int st = seq_stat_prepare(c, stride, d_count, d_sum, descs, a, true);
    if (st != RWH_OK) return st;
    if (!d_workspace || workspace_bytes < rwh_sequence_overlap_stats_workspace_bytes(n, c.canvas_h, c.canvas_w, stride) ||
        ((uintptr_t)d_workspace & 7u) || ((uintptr_t)d_count & 7u) || ((uintptr_t)d_sum & 7u)) return RWH_E_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint64_t* table = static_cast<uint64_t*>(d_workspace);
    a.slabs = reinterpret_cast<unsigned long long*>(static_cast<char*>(d_workspace) + seq_stat_table_bytes(n));
    if (fill_async(a.slabs, 0, (size_t)STAT_SLABS * a.slab_words * sizeof(uint64_t), s) != hipSuccess) return RWH_E_LAUNCH;
    seq_put(descs, (size_t)n * SEQ_DESC_WORDS, table, s);
    a.a.desc = reinterpret_cast<const SeqDesc*>(table);
    const dim3 grid((a.nsx + STAT_W - 1) / STAT_W, (a.nsy + STAT_H - 1) / STAT_H);
    seq_form_dispatch(c.form, [&](auto form) {
        constexpr bool PROJ = decltype(form)::proj, RING = decltype(form)::ring;
        hipLaunchKernelGGL((seq_stats_kernel<PROJ, RING>), grid, dim3(256), 0, s, (seq_with<false, PROJ>(a, nullptr, n, c.rays)));
    });
    hipLaunchKernelGGL(seq_stats_sum_kernel, dim3((2 * n * n + 255) / 256), dim3(256), 0, s, a.slabs, a.slab_words, n * n,
                       reinterpret_cast<unsigned long long*>(d_count), reinterpret_cast<unsigned long long*>(d_sum));
    return check_launch();
}

static int seq_stat_host(const SeqCall& c, int stride, uint64_t* count, uint64_t* sum) {
    SeqDesc descs[RWH_SEQ_MAX_IMAGES];
    StatArgs a;
    const int n = c.n;
    const int st = seq_stat_prepare(c, stride, count, sum, descs, a, false);
    if (st != RWH_OK) return st;
    memset(count, 0, (size_t)n * n * sizeof(uint64_t));
    memset(sum, 0, (size_t)n * n * sizeof(uint64_t));
    const uint64_t all = seq_all(n);
    seq_form_dispatch(c.form, [&](auto form) {
        constexpr bool PROJ = decltype(form)::proj, RING = decltype(form)::ring;
        for (int v = 0; v < a.nsy; ++v)
            for (int u = 0; u < a.nsx; ++u) {
                const int cx = u * stride, cy = v * stride;
                const uint64_t cov = seq_cover<PROJ, RING>(a.a, all, cx, cy, c.rays);
                for (uint64_t mi = cov; mi; mi &= mi - 1) {
                    const int i = __builtin_ctzll(mi);
                    const uint64_t l = seq_byte_sum<PROJ, RING>(a.a, i, cx, cy, c.rays);
                    for (uint64_t mj = cov; mj; mj &= mj - 1) {
                        const int j = __builtin_ctzll(mj);
                        count[(size_t)i * n + j] += 1;
                        sum[(size_t)i * n + j] += l;
                    }
                }
            }
    });
    return RWH_OK;
}

}  // namespace rwh

using rwh::seq_curved;
using rwh::seq_gain_maps;
using rwh::seq_gain_n;
using rwh::seq_plane;

extern "C" int64_t rwh_stitch_sequence_workspace_bytes(int n) {
    if (n < 1 || n > RWH_SEQ_MAX_IMAGES) return RWH_E_INVALID;
    return (int64_t)n * (int64_t)sizeof(rwh::SeqDesc);
}

// Every entry point below: the geometry record of its form, then the driver.
extern "C" int rwh_stitch_sequence_ex(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                      int anchor, const int32_t* order, int blend, void* d_canvas, int canvas_h, int canvas_w,
                                      int origin_x, int origin_y, int row_begin, int row_end, void* d_workspace, int64_t workspace_bytes,
                                      void* stream, const double* gains) {
    return rwh::seq_device(seq_plane(d_images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), order, blend, d_canvas,
                           row_begin, row_end, d_workspace, workspace_bytes, stream, seq_gain_n(gains));
}

extern "C" int rwh_stitch_sequence_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                        const int32_t* order, int blend, const double* d_col, const double* d_row, void* d_canvas,
                                        int canvas_h, int canvas_w, int row_begin, int row_end, void* d_workspace, int64_t workspace_bytes,
                                        void* stream, const double* gains) {
    return rwh::seq_device(seq_curved(d_images, hw, m, rects, n, d_col, d_row, canvas_h, canvas_w), order, blend, d_canvas,
                           row_begin, row_end, d_workspace, workspace_bytes, stream, seq_gain_n(gains));
}

extern "C" int rwh_stitch_sequence_ring(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                        const int32_t* order, int blend, const double* d_col, const double* d_row, void* d_canvas,
                                        int canvas_h, int canvas_w, int row_begin, int row_end, void* d_workspace, int64_t workspace_bytes,
                                        void* stream, const double* gains) {
    return rwh::seq_device(seq_curved(d_images, hw, m, rects, n, d_col, d_row, canvas_h, canvas_w, true), order, blend, d_canvas,
                           row_begin, row_end, d_workspace, workspace_bytes, stream, seq_gain_n(gains));
}

extern "C" int rwh_stitch_sequence(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                   int anchor, const int32_t* order, int blend, void* d_canvas, int canvas_h, int canvas_w,
                                   int origin_x, int origin_y, int row_begin, int row_end, void* d_workspace, int64_t workspace_bytes,
                                   void* stream) {
    return rwh_stitch_sequence_ex(d_images, hw, inv_g, rects, n, anchor, order, blend, d_canvas, canvas_h, canvas_w, origin_x, origin_y,
                                  row_begin, row_end, d_workspace, workspace_bytes, stream, nullptr);
}

// The compositor on the gain maps of the block gain rule (rwh_blockgains.hip makes them): d_maps / maps and shift where the calls
// above take gains.  The host twins read the maps: every entry finite and > 0.
extern "C" int rwh_stitch_sequence_maps(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                        int anchor, const int32_t* order, int blend, void* d_canvas, int canvas_h, int canvas_w,
                                        int origin_x, int origin_y, int row_begin, int row_end, void* d_workspace, int64_t workspace_bytes,
                                        void* stream, const double* d_maps, int shift) {
    return rwh::seq_device(seq_plane(d_images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), order, blend, d_canvas,
                           row_begin, row_end, d_workspace, workspace_bytes, stream, seq_gain_maps(d_maps, shift));
}

extern "C" int rwh_stitch_sequence_maps_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                             const int32_t* order, int blend, const double* d_col, const double* d_row, void* d_canvas,
                                             int canvas_h, int canvas_w, int row_begin, int row_end, void* d_workspace,
                                             int64_t workspace_bytes, void* stream, const double* d_maps, int shift) {
    return rwh::seq_device(seq_curved(d_images, hw, m, rects, n, d_col, d_row, canvas_h, canvas_w), order, blend, d_canvas,
                           row_begin, row_end, d_workspace, workspace_bytes, stream, seq_gain_maps(d_maps, shift));
}

extern "C" int rwh_host_stitch_sequence_ex(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                           int anchor, const int32_t* order, int blend, void* canvas, int canvas_h, int canvas_w,
                                           int origin_x, int origin_y, int row_begin, int row_end, const double* gains) {
    return rwh::seq_host(seq_plane(images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), order, blend, canvas,
                         row_begin, row_end, seq_gain_n(gains));
}

extern "C" int rwh_host_stitch_sequence_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                             const int32_t* order, int blend, const double* col, const double* row, void* canvas,
                                             int canvas_h, int canvas_w, int row_begin, int row_end, const double* gains) {
    return rwh::seq_host(seq_curved(images, hw, m, rects, n, col, row, canvas_h, canvas_w), order, blend, canvas, row_begin, row_end,
                         seq_gain_n(gains));
}

extern "C" int rwh_host_stitch_sequence_ring(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                             const int32_t* order, int blend, const double* col, const double* row, void* canvas,
                                             int canvas_h, int canvas_w, int row_begin, int row_end, const double* gains) {
    return rwh::seq_host(seq_curved(images, hw, m, rects, n, col, row, canvas_h, canvas_w, true), order, blend, canvas, row_begin, row_end,
                         seq_gain_n(gains));
}

extern "C" int rwh_host_stitch_sequence(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                        int anchor, const int32_t* order, int blend, void* canvas, int canvas_h, int canvas_w,
                                        int origin_x, int origin_y, int row_begin, int row_end) {
    return rwh_host_stitch_sequence_ex(images, hw, inv_g, rects, n, anchor, order, blend, canvas, canvas_h, canvas_w, origin_x, origin_y,
                                       row_begin, row_end, nullptr);
}

extern "C" int rwh_host_stitch_sequence_maps(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                             int anchor, const int32_t* order, int blend, void* canvas, int canvas_h, int canvas_w,
                                             int origin_x, int origin_y, int row_begin, int row_end, const double* maps, int shift) {
    return rwh::seq_host(seq_plane(images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), order, blend, canvas,
                         row_begin, row_end, seq_gain_maps(maps, shift));
}

extern "C" int rwh_host_stitch_sequence_maps_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                                  const int32_t* order, int blend, const double* col, const double* row, void* canvas,
                                                  int canvas_h, int canvas_w, int row_begin, int row_end, const double* maps, int shift) {
    return rwh::seq_host(seq_curved(images, hw, m, rects, n, col, row, canvas_h, canvas_w), order, blend, canvas, row_begin, row_end,
                         seq_gain_maps(maps, shift));
}

extern "C" int64_t rwh_sequence_overlap_stats_workspace_bytes(int n, int canvas_h, int canvas_w, int stride) {
    if (n < 1 || n > RWH_SEQ_MAX_IMAGES || stride < 1 || stride > 255) return RWH_E_INVALID;
    if (!rwh::seq_canvas_ok(canvas_h, canvas_w)) return RWH_E_INVALID;
    return rwh::seq_stat_table_bytes(n) + (int64_t)rwh::STAT_SLABS * rwh::seq_slab_words(n) * (int64_t)sizeof(uint64_t);
}

extern "C" int rwh_sequence_overlap_stats(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                          int anchor, int canvas_h, int canvas_w, int origin_x, int origin_y, int stride,
                                          uint64_t* d_count, uint64_t* d_sum, void* d_workspace, int64_t workspace_bytes, void* stream) {
    return rwh::seq_stat_device(seq_plane(d_images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), stride, d_count,
                                d_sum, d_workspace, workspace_bytes, stream);
}

extern "C" int rwh_sequence_overlap_stats_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                               const double* d_col, const double* d_row, int canvas_h, int canvas_w, int stride,
                                               uint64_t* d_count, uint64_t* d_sum, void* d_workspace, int64_t workspace_bytes, void* stream) {
    return rwh::seq_stat_device(seq_curved(d_images, hw, m, rects, n, d_col, d_row, canvas_h, canvas_w), stride, d_count, d_sum,
                                d_workspace, workspace_bytes, stream);
}

extern "C" int rwh_sequence_overlap_stats_ring(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                               const double* d_col, const double* d_row, int canvas_h, int canvas_w, int stride,
                                               uint64_t* d_count, uint64_t* d_sum, void* d_workspace, int64_t workspace_bytes, void* stream) {
    return rwh::seq_stat_device(seq_curved(d_images, hw, m, rects, n, d_col, d_row, canvas_h, canvas_w, true), stride, d_count, d_sum,
                                d_workspace, workspace_bytes, stream);
}

extern "C" int rwh_host_sequence_overlap_stats(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                               int anchor, int canvas_h, int canvas_w, int origin_x, int origin_y, int stride,
                                               uint64_t* count, uint64_t* sum) {
    return rwh::seq_stat_host(seq_plane(images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), stride, count, sum);
}

extern "C" int rwh_host_sequence_overlap_stats_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                                    const double* col, const double* row, int canvas_h, int canvas_w, int stride,
                                                    uint64_t* count, uint64_t* sum) {
    return rwh::seq_stat_host(seq_curved(images, hw, m, rects, n, col, row, canvas_h, canvas_w), stride, count, sum);
}

extern "C" int rwh_host_sequence_overlap_stats_ring(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                                    const double* col, const double* row, int canvas_h, int canvas_w, int stride,
                                                    uint64_t* count, uint64_t* sum) {
    return rwh::seq_stat_host(seq_curved(images, hw, m, rects, n, col, row, canvas_h, canvas_w, true), stride, count, sum);
}

// The gains of the gain rule from the two tables: seq_solve_gains (rwh_sequence.h) on them.
extern "C" int rwh_host_sequence_gains(const uint64_t* count, const uint64_t* sum, int n, double sigma_n, double sigma_g, double* gains) {
    if (!count || !sum || !gains || n < 1 || n > RWH_SEQ_MAX_IMAGES) return RWH_E_INVALID;
    if (!(isfinite(sigma_n) && sigma_n > 0.0 && isfinite(sigma_g) && sigma_g > 0.0)) return RWH_E_INVALID;
    const uint64_t* cnt = count;
    const uint64_t* sm = sum;
    const double alpha = 1.0 / (sigma_n * sigma_n), beta = 1.0 / (sigma_g * sigma_g);
    auto N = [&](int i, int j) { return (double)cnt[(size_t)i * n + j]; };
    auto I = [&](int i, int j) { return cnt[(size_t)i * n + j] ? (double)sm[(size_t)i * n + j] / (3.0 * N(i, j)) : 0.0; };
    if (!rwh::seq_solve_gains(n, alpha, beta, [&](int i) { return cnt[(size_t)i * n + i] != 0; }, N, I, gains)) return RWH_E_INVALID;
    return RWH_OK;
}
