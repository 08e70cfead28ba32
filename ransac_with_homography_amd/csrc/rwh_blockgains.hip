// Block exposure gains for the sequence compositor (include/rwh.h, "The block gain rule"): the gain rule's overlap statistics taken
// per B x B cell of the canvas, a gain system solved per cell on the host, and the solutions smoothed into one gain MAP per image.
// The per-sample functions and the solver are rwh_sequence.h's: the cells sample an image with the one arithmetic of the family.
// The compositors that read the maps are the family's own (rwh_sequence.hip, rwh_multiband.hip, rwh_seams.hip), instantiated on the
// third state of the gain switch.
#include <vector>
#include "rwh_sequence.h"

namespace rwh {

struct CellArgs {
    SeqArgs a;                  // order: 0 .. n-1 (candidate bits are image indices); dst, row_begin, row_end unused
    int shift, stride;          // cells of B = 2^shift pixels; the gain rule's sample set
    int slots;                  // K: the most candidates of any cell
    int gw, gh;
    uint32_t* tables;           // [gh][gw][2][K][K]: count then sum, by candidate RANK
};


// The first sample at or after canvas coordinate c.
__host__ __device__ __forceinline__ int cell_first_sample(int c, int stride) { return (c + stride - 1) / stride; }

// One workgroup owns one cell and nobody else writes its slot: no global atomics, no slabs, no second kernel.  The clipped cell is
// tested once against the n rectangles (blockIdx is wave-uniform: the mask and the pair loops stay on the scalar side).  The cell's
// samples are walked 1024 at a time -- four per lane, consecutive lanes on consecutive samples of a sample row, rows following one
// another -- so a 16 x 16 cell fills its waves as a 128 x 128 one does.  Per pass, as seq_stats_kernel: every lane's coverage masks,
// then per candidate pair one wave sum of (count << 20 | sum) -- a wave has 256 samples a pass: count <= 2^8 and sum <= 256 * 765 <
// 2^20 -- unpacked by lane 0 into the two LDS tables, 2 x K x K uint32 indexed by rank, which hold the whole cell (16384 samples
// x 765 < 2^32).  Ranks at or above the cell's candidate count are never added to: the slot is the LDS tables, stored whole.
constexpr int CELL_PX = 4;
template <bool PROJ>
__global__ __launch_bounds__(256) void seq_cell_stats_kernel(const SeqWith<CellArgs, false, PROJ> l) {
    static_assert(64 * CELL_PX * 765 < (1 << 20) && 64 * CELL_PX < (1 << 12), "count << 20 | sum in 32 bits");
    extern __shared__ uint32_t acc[];
    const CellArgs& c = l.a;
    const SeqArgs& a = c.a;
    const int K = c.slots, KK = K * K;
    const int x0 = (int)blockIdx.x << c.shift, y0 = (int)blockIdx.y << c.shift;
    const int x1 = x0 + (1 << c.shift) < a.fw ? x0 + (1 << c.shift) : a.fw, y1 = y0 + (1 << c.shift) < a.fh ? y0 + (1 << c.shift) : a.fh;
    const uint64_t cand = seq_tile_mask(a, x0, x1, y0, y1);
    for (int t = threadIdx.x; t < 2 * KK; t += 256) acc[t] = 0u;
    __syncthreads();
    const int u0 = cell_first_sample(x0, c.stride), v0 = cell_first_sample(y0, c.stride);
    const int cols = cell_first_sample(x1, c.stride) - u0, rows = cell_first_sample(y1, c.stride) - v0;
    const int total = cand ? cols * rows : 0;                      // (block-uniform)
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < total; base += 256 * CELL_PX) {
        uint64_t cov[CELL_PX];
        int cx[CELL_PX], cy[CELL_PX];
#pragma unroll
        for (int k = 0; k < CELL_PX; ++k) {
            const int s = base + k * 256 + (int)threadIdx.x;
            const int sv = s / cols;
            cx[k] = (u0 + (s - sv * cols)) * c.stride;
            cy[k] = (v0 + sv) * c.stride;
            cov[k] = s < total ? seq_cover<PROJ>(a, cand, cx[k], cy[k], seq_rays(l)) : 0ull;
        }
        int ri = 0;
        for (uint64_t mi = cand; mi; mi &= mi - 1, ++ri) {
            const int i = __builtin_ctzll(mi);
            uint32_t L[CELL_PX];
            bool any = false;
#pragma unroll
            for (int k = 0; k < CELL_PX; ++k) {
                const bool on = cov[k] >> i & 1;
                L[k] = on ? seq_byte_sum<PROJ>(a, i, cx[k], cy[k], seq_rays(l)) : 0u;
                any |= on;
            }
            if (!__any(any)) continue;                             // (wave-uniform)
            int rj = 0;
            for (uint64_t mj = cand; mj; mj &= mj - 1, ++rj) {
                const int j = __builtin_ctzll(mj);
                uint32_t p = 0u;
#pragma unroll
                for (int k = 0; k < CELL_PX; ++k)
                    if ((cov[k] >> i) & (cov[k] >> j) & 1) p += (1u << 20) + L[k];
                if (!__any(p != 0u)) continue;                     // (wave-uniform: i and j meet at none of the wave's samples)
                p = seq_wave_sum(p);
                if (lane == 0) {
                    atomicAdd(&acc[ri * K + rj], p >> 20);
                    atomicAdd(&acc[KK + ri * K + rj], p & 0xfffffu);
                }
            }
        }
    }
    __syncthreads();
    uint32_t* out = c.tables + ((size_t)blockIdx.y * c.gw + blockIdx.x) * (size_t)(2 * KK);
    for (int t = threadIdx.x; t < 2 * KK; t += 256) out[t] = acc[t];
}

// The frame of a set of rectangles alone (seq_frame) -- what seq_tile_mask reads -- for the functions that are given no images.
static bool cell_frame(const SeqCall& c, SeqDesc* descs, SeqArgs& a) {
    const int32_t* rects = c.rects;
    const int n = c.n, canvas_h = c.canvas_h, canvas_w = c.canvas_w, origin_x = c.origin_x, origin_y = c.origin_y;
    if (!rects || n < 1 || n > RWH_SEQ_MAX_IMAGES || !seq_canvas_ok(canvas_h, canvas_w)) return false;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < n; ++i) {
        SeqDesc& d = descs[i];
        memset(&d, 0, sizeof(d));
        d.mx = rects[4 * i]; d.my = rects[4 * i + 1]; d.wt = rects[4 * i + 2]; d.ht = rects[4 * i + 3];
        const int64_t rx = (int64_t)d.mx - origin_x, ry = (int64_t)d.my - origin_y;
        if (d.wt <= 0 || d.ht <= 0 || rx < 0 || ry < 0 || rx + d.wt > canvas_w || ry + d.ht > canvas_h) return false;
        a.order[i] = (unsigned char)i;
    }
    a.desc = descs;
    a.n = n; a.ox = origin_x; a.oy = origin_y; a.fh = canvas_h; a.fw = canvas_w;
    return true;
}

// The candidates of cell (gx, gy): seq_tile_mask on the clipped cell.
static uint64_t cell_mask(const SeqArgs& a, int gx, int gy, int shift) {
    const int x0 = gx << shift, y0 = gy << shift, B = 1 << shift;
    return seq_tile_mask(a, x0, x0 + B < a.fw ? x0 + B : a.fw, y0, y0 + B < a.fh ? y0 + B : a.fh);
}

static int cell_slots(const SeqArgs& a, int shift) {
    int K = 0;
    for (int gy = 0; gy < seq_cell_count(a.fh, shift); ++gy)
        for (int gx = 0; gx < seq_cell_count(a.fw, shift); ++gx) {
            const int nc = __builtin_popcountll(cell_mask(a, gx, gy, shift));
            K = nc > K ? nc : K;
        }
    return K;
}

// What both statistics entry points check, and their arguments: the overlap statistics' checks plus the block, and K as the
// rectangles give it.  The cells have no ring form.
static int cell_prepare(const SeqCall& c, int shift, int stride, int slots, uint32_t* tables, SeqDesc* descs, CellArgs& cell, bool device) {
    if (!tables || ((uintptr_t)tables & 3u) || stride < 1 || stride > 255 || shift < SEQ_SHIFT_MIN || shift > SEQ_SHIFT_MAX) return RWH_E_INVALID;
    if (c.form == SEQ_RING) return RWH_E_INVALID;
    const int st = seq_prepare_indexed(c, tables, descs, cell.a, device);
    if (st != RWH_OK) return st;
    cell.a.dst = nullptr;
    if (slots != cell_slots(cell.a, shift)) return RWH_E_INVALID;
    cell.shift = shift; cell.stride = stride; cell.slots = slots;
    cell.gw = seq_cell_count(c.canvas_w, shift); cell.gh = seq_cell_count(c.canvas_h, shift);
    cell.tables = tables;
    return RWH_OK;
}

static int cell_device(const SeqCall& c, int shift, int stride, int slots, uint32_t* d_tables, void* d_workspace, int64_t workspace_bytes,
                       void* stream) {
    SeqDesc descs[RWH_SEQ_MAX_IMAGES];
    CellArgs cell;
    const int st = cell_prepare(c, shift, stride, slots, d_tables, descs, cell, true);
    if (st != RWH_OK) return st;
    if (!d_workspace || workspace_bytes < seq_stat_table_bytes(c.n) || ((uintptr_t)d_workspace & 7u)) return RWH_E_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint64_t* table = static_cast<uint64_t*>(d_workspace);
    seq_put(descs, (size_t)c.n * SEQ_DESC_WORDS, table, s);
    cell.a.desc = reinterpret_cast<const SeqDesc*>(table);
    seq_form_dispatch<false>(c.form, [&](auto form) {
        constexpr bool PROJ = decltype(form)::proj;
        hipLaunchKernelGGL((seq_cell_stats_kernel<PROJ>), dim3(cell.gw, cell.gh), dim3(256), (size_t)2 * slots * slots * sizeof(uint32_t), s,
                           (seq_with<false, PROJ>(cell, nullptr, c.n, c.rays)));
    });
    return check_launch();
}

static int cell_host(const SeqCall& c, int shift, int stride, int slots, uint32_t* tables) {
    SeqDesc descs[RWH_SEQ_MAX_IMAGES];
    CellArgs cell;
    const int st = cell_prepare(c, shift, stride, slots, tables, descs, cell, false);
    if (st != RWH_OK) return st;
    const SeqArgs& a = cell.a;
    const int K = slots, KK = K * K, B = 1 << shift;
    memset(tables, 0, (size_t)cell.gh * cell.gw * 2 * KK * sizeof(uint32_t));
    seq_form_dispatch<false>(c.form, [&](auto form) {
        constexpr bool PROJ = decltype(form)::proj;
        for (int gy = 0; gy < cell.gh; ++gy)
            for (int gx = 0; gx < cell.gw; ++gx) {
                const uint64_t cand = cell_mask(a, gx, gy, shift);
                uint32_t* cnt = tables + ((size_t)gy * cell.gw + gx) * (size_t)(2 * KK);
                uint32_t* sm = cnt + KK;
                const int x1 = (gx << shift) + B < a.fw ? (gx << shift) + B : a.fw, y1 = (gy << shift) + B < a.fh ? (gy << shift) + B : a.fh;
                for (int cy = cell_first_sample(gy << shift, stride) * stride; cy < y1; cy += stride)
                    for (int cx = cell_first_sample(gx << shift, stride) * stride; cx < x1; cx += stride) {
                        const uint64_t cov = seq_cover<PROJ>(a, cand, cx, cy, c.rays);
                        for (uint64_t mi = cov; mi; mi &= mi - 1) {
                            const int i = __builtin_ctzll(mi), ri = __builtin_popcountll(cand & ((1ull << i) - 1));
                            const uint32_t lsum = seq_byte_sum<PROJ>(a, i, cx, cy, c.rays);
                            for (uint64_t mj = cov; mj; mj &= mj - 1) {
                                const int rj = __builtin_popcountll(cand & ((1ull << __builtin_ctzll(mj)) - 1));
                                cnt[ri * K + rj] += 1u;
                                sm[ri * K + rj] += lsum;
                            }
                        }
                    }
            }
    });
    return RWH_OK;
}

}  // namespace rwh

extern "C" int rwh_sequence_cell_slots(const int32_t* rects, int n, int canvas_h, int canvas_w, int origin_x, int origin_y, int shift) {
    using namespace rwh;
    SeqDesc descs[RWH_SEQ_MAX_IMAGES];
    SeqArgs a;
    if (shift < SEQ_SHIFT_MIN || shift > SEQ_SHIFT_MAX || !cell_frame(seq_frame(rects, n, canvas_h, canvas_w, origin_x, origin_y), descs, a)) return RWH_E_INVALID;
    return cell_slots(a, shift);
}

extern "C" int64_t rwh_sequence_cell_stats_workspace_bytes(int n) {
    if (n < 1 || n > RWH_SEQ_MAX_IMAGES) return RWH_E_INVALID;
    return rwh::seq_stat_table_bytes(n);
}

extern "C" int64_t rwh_sequence_cell_stats_table_bytes(int canvas_h, int canvas_w, int shift, int slots) {
    using namespace rwh;
    if (shift < SEQ_SHIFT_MIN || shift > SEQ_SHIFT_MAX || slots < 1 || slots > RWH_SEQ_MAX_IMAGES || !seq_canvas_ok(canvas_h, canvas_w)) return RWH_E_INVALID;
    return (int64_t)seq_cell_count(canvas_h, shift) * seq_cell_count(canvas_w, shift) * 2 * slots * slots * (int64_t)sizeof(uint32_t);
}

extern "C" int rwh_sequence_cell_stats(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                       int anchor, int canvas_h, int canvas_w, int origin_x, int origin_y, int shift, int stride, int slots,
                                       uint32_t* d_tables, void* d_workspace, int64_t workspace_bytes, void* stream) {
    return rwh::cell_device(rwh::seq_plane(d_images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), shift, stride,
                            slots, d_tables, d_workspace, workspace_bytes, stream);
}

extern "C" int rwh_sequence_cell_stats_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                            const double* d_col, const double* d_row, int canvas_h, int canvas_w, int shift, int stride,
                                            int slots, uint32_t* d_tables, void* d_workspace, int64_t workspace_bytes, void* stream) {
    return rwh::cell_device(rwh::seq_curved(d_images, hw, m, rects, n, d_col, d_row, canvas_h, canvas_w), shift, stride, slots, d_tables,
                            d_workspace, workspace_bytes, stream);
}

extern "C" int rwh_host_sequence_cell_stats(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                            int anchor, int canvas_h, int canvas_w, int origin_x, int origin_y, int shift, int stride,
                                            int slots, uint32_t* tables) {
    return rwh::cell_host(rwh::seq_plane(images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), shift, stride, slots,
                          tables);
}

extern "C" int rwh_host_sequence_cell_stats_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                                 const double* col, const double* row, int canvas_h, int canvas_w, int shift, int stride,
                                                 int slots, uint32_t* tables) {
    return rwh::cell_host(rwh::seq_curved(images, hw, m, rects, n, col, row, canvas_h, canvas_w), shift, stride, slots, tables);
}

// Cell gains, smoothing and maps of the block gain rule.  Host only, plain C++: the cell solves are seq_solve_gains, the solver of
// the gain rule, on the candidates' sub-tables.
extern "C" int rwh_host_sequence_block_gains(const uint32_t* tables, const int32_t* rects, int n, int canvas_h, int canvas_w, int origin_x,
                                             int origin_y, int shift, int slots, const double* base, double sigma_n, double sigma_g,
                                             int smooth, double* maps) {
    using namespace rwh;
    SeqDesc descs[RWH_SEQ_MAX_IMAGES];
    SeqArgs a;
    if (!tables || !maps || shift < SEQ_SHIFT_MIN || shift > SEQ_SHIFT_MAX || smooth < 0 || smooth > 8) return RWH_E_INVALID;
    if (!cell_frame(seq_frame(rects, n, canvas_h, canvas_w, origin_x, origin_y), descs, a) || slots != cell_slots(a, shift)) return RWH_E_INVALID;
    if (!(isfinite(sigma_n) && sigma_n > 0.0 && isfinite(sigma_g) && sigma_g > 0.0) || (base && !seq_gains_ok(base, n))) return RWH_E_INVALID;
    const double alpha = 1.0 / (sigma_n * sigma_n), beta = 1.0 / (sigma_g * sigma_g);
    const int gw = seq_cell_count(canvas_w, shift), gh = seq_cell_count(canvas_h, shift), K = slots, KK = K * K;
    const size_t plane = (size_t)gw * gh;
    for (size_t t = 0; t < plane * n; ++t) maps[t] = 1.0;                       // r: 1.0 for an image that is no candidate
    for (int gy = 0; gy < gh; ++gy)
        for (int gx = 0; gx < gw; ++gx) {
            const uint64_t cand = cell_mask(a, gx, gy, shift);
            int ids[RWH_SEQ_MAX_IMAGES], nc = 0;
            for (uint64_t m = cand; m; m &= m - 1) ids[nc++] = __builtin_ctzll(m);
            if (!nc) continue;
            const uint32_t* cnt = tables + ((size_t)gy * gw + gx) * (size_t)(2 * KK);
            const uint32_t* sm = cnt + KK;
            auto N = [&](int i, int j) { return (double)cnt[i * K + j]; };
            auto I = [&](int i, int j) { return cnt[i * K + j] ? (double)sm[i * K + j] / (3.0 * N(i, j)) * (base ? base[ids[i]] : 1.0) : 0.0; };
            double r[RWH_SEQ_MAX_IMAGES];
            if (!seq_solve_gains(nc, alpha, beta, [&](int i) { return cnt[i * K + i] != 0u; }, N, I, r)) return RWH_E_INVALID;
            for (int k = 0; k < nc; ++k) maps[ids[k] * plane + (size_t)gy * gw + gx] = r[k];
        }
    std::vector<double> tmp(plane);
    for (int i = 0; i < n; ++i) {
        double* r = maps + i * plane;
        for (int it = 0; it < smooth; ++it) {
            for (int y = 0; y < gh; ++y)                                        // along x, edges replicated
                for (int x = 0; x < gw; ++x) {
                    const double* row = r + (size_t)y * gw;
                    tmp[(size_t)y * gw + x] = ((row[x > 0 ? x - 1 : 0] + 2.0 * row[x]) + row[x + 1 < gw ? x + 1 : gw - 1]) * 0.25;
                }
            for (int y = 0; y < gh; ++y)                                        // then along y
                for (int x = 0; x < gw; ++x)
                    r[(size_t)y * gw + x] = ((tmp[(size_t)(y > 0 ? y - 1 : 0) * gw + x] + 2.0 * tmp[(size_t)y * gw + x]) +
                                             tmp[(size_t)(y + 1 < gh ? y + 1 : gh - 1) * gw + x]) * 0.25;
        }
        for (size_t t = 0; t < plane; ++t) {
            r[t] = (base ? base[i] : 1.0) * r[t];
            if (!(isfinite(r[t]) && r[t] > 0.0)) return RWH_E_INVALID;
        }
    }
    return RWH_OK;
}

