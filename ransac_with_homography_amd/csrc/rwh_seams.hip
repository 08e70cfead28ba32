// Seam finding for the sequence compositor (include/rwh.h, "The seam rule"): which image owns a canvas pixel, decided by what the
// images show.  Every image grows outward from the pixels it owns beyond dispute (its seeds), slowly where the covering images agree
// and fast where they disagree, and a pixel goes to the image that reaches it first: a geodesic, watershed-style seam.  The result is
// the unique fixed point of an integer shortest-path problem, so the device's chaotic relaxation, the host twin's Dijkstra and a
// restatement by Jacobi sweeps give the same integers.
//
// The plan ("Seam finding"): image i works in one WINDOW, its rectangle, a row-major uint32 plane of distances.
//   1. sm_survey_kernel: one pass over the canvas; a pixel samples its candidates once and stores its cost, the feather winner and
//      the seed flag in one dword, and its coverage set as the candidate mask.
//   2. sm_init_kernel, blockIdx.z the image: 0 at the image's seeds, SM_WALL where it does not cover, SM_UNREACHED elsewhere.
//   3. sm_relax_kernel, all images in one launch, as many passes as it takes: a block stages its SM_TW x SM_TH tile of distances with
//      a one-pixel halo and the tile's costs in LDS, relaxes there in place until the tile stops changing (or SM_INNER sweeps),
//      stores the pixels that changed and raises the device flag.  A tile that did not change in the previous pass and whose four
//      neighbours did not either leaves at once (a dirty byte per tile, two arrays in turn).
//   4. sm_label_kernel: one pass over the canvas, the argmin over the covering images' windows.
// sm_paste_kernel is label paste: the bytes of the labelled winner (seq_label_winner_pixel, which the labelled multi-band winner
// pass of rwh_multiband.hip shares).
#include <stdlib.h>
#include <new>
#include <queue>
#include <utility>
#include <vector>
#include "rwh_sequence.h"

namespace rwh {

constexpr uint32_t SM_WALL = 0xffffffffu;        // the image does not cover the pixel (or the pixel lies outside its window)
constexpr uint32_t SM_UNREACHED = 0xfffffffeu;   // covered, no path from a seed yet; every real distance is <= 2^32 - 3
constexpr int SM_TW = RWH_SEAM_TILE_W, SM_TH = RWH_SEAM_TILE_H;
constexpr int SM_ROWS = SM_TH / 4;               // rows of the tile per lane: 256 lanes as SM_TW columns x 4 row groups
constexpr int SM_INNER = 64;                     // most sweeps (one down, one up) of a tile per pass
constexpr int SM_BATCH = 4;                      // passes between two reads of the flag
static_assert(SM_TW == 64 && SM_TH % 4 == 0, "a wave takes one row group of the tile");

// The survey dword: bits 0 .. 9 the cost c (1 .. 766), bit 10 the seed flag, bits 24 .. 31 the feather winner (0xff: nobody covers).
constexpr uint32_t SM_COST_MASK = 0x3ffu, SM_SEED = 1u << 10;

// Image i's window: its rectangle in canvas coordinates, row-major at `off` (in dwords) of the distance area; tx x ty tiles, whose
// dirty bytes start at `toff`.
struct SmWin { int x0, y0, w, h, tx, ty; int64_t off, toff; };
static_assert(sizeof(SmWin) == 40, "SmWin is copied as 8-byte words");

struct SmArgs {
    SeqArgs a;                  // order: 0 .. n-1 (candidate bits are image indices); dst: the label plane, fh x fw
    const SmWin* win;           // [n]
    uint32_t* sv;               // fh x fw survey dwords
    uint64_t* cov;              // fh x fw coverage sets
    uint32_t* dist;             // the windows
    unsigned char* dirty;       // [2][tiles]: pass k reads array (k + 1) & 1 and writes array k & 1
    uint32_t* flag;             // the last pass that changed a distance (0: none has)
    int64_t tiles;
    double margin;
    int tau;
};

// ---- the per-pixel functions ----
// Cost, feather winner, seed flag and coverage set of canvas pixel (cx, cy).  best is the greatest feather weight and rest the
// greatest among the others: the pixel is a seed of the winner when rest <= margin (g >= 1 wherever an image covers, so rest = 0
// says that nobody else does).
template <bool GAIN, bool PROJ>
__host__ __device__ __forceinline__ void sm_survey_pixel(const SeqArgs& a, uint64_t cand, int cx, int cy, double margin, int tau,
                                                         const double* gains, SeqRays rays, uint32_t& sv, uint64_t& cov) {
    const int fx = a.ox + cx, fy = a.oy + cy;
    SeqRay ray;
    if constexpr (PROJ) ray = seq_ray(rays, cx, cy);
    double best = 0.0, rest = 0.0;
    uint32_t w = SEQ_LABEL_NONE;
    int lo[3] = {255, 255, 255}, hi[3] = {0, 0, 0};
    cov = 0;
    for (uint64_t m = cand; m; m &= m - 1) {
        const int i = __builtin_ctzll(m);
        double v[3], g = 0.0, gain = 1.0;
        if constexpr (GAIN) gain = gains[i];
        if (!seq_sample<true, GAIN, PROJ>(a.desc[i], i == a.anchor, fx, fy, v, g, gain, &ray, a.fw)) continue;
        cov |= 1ull << i;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int b = (int)(unsigned char)(int)v[k];
            lo[k] = b < lo[k] ? b : lo[k];
            hi[k] = b > hi[k] ? b : hi[k];
        }
        if (g > best) { rest = best; best = g; w = (uint32_t)i; }
        else if (g > rest) rest = g;
    }
    int c = tau;
    if (cov) c -= (hi[0] - lo[0]) + (hi[1] - lo[1]) + (hi[2] - lo[2]);
    c = c < 1 ? 1 : c;
    sv = (uint32_t)c | ((cov && rest <= margin) ? SM_SEED : 0u) | (w << 24);
}

// Image i's first distance at a pixel of its window.
__host__ __device__ __forceinline__ uint32_t sm_init_pixel(int i, uint32_t sv, uint64_t cov) {
    if (!((cov >> i) & 1)) return SM_WALL;
    return ((sv & SM_SEED) && (sv >> 24) == (uint32_t)i) ? 0u : SM_UNREACHED;
}

// One relaxation: cur, the pixel's distance (a seed's 0 and SM_WALL never change), nb the least of its four neighbours', c its cost.
// nb + c < cur is tested without forming a sum that could wrap.
__host__ __device__ __forceinline__ bool sm_relax(uint32_t& cur, uint32_t nb, uint32_t c) {
    if (cur == SM_WALL || nb >= SM_UNREACHED || nb >= cur || c >= cur - nb) return false;
    cur = nb + c;
    return true;
}
__host__ __device__ __forceinline__ uint32_t sm_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// The label: the covering image with the least (distance, index) among the reached, else the feather winner (0xff: nobody covers).
__host__ __device__ __forceinline__ unsigned char sm_label_pixel(const SmArgs& m, int x, int y) {
    const int64_t p = (int64_t)y * m.a.fw + x;
    uint32_t best = SM_UNREACHED, lab = m.sv[p] >> 24;
    for (uint64_t c = m.cov[p]; c; c &= c - 1) {
        const int i = __builtin_ctzll(c);
        const SmWin& w = m.win[i];
        const uint32_t d = m.dist[w.off + (int64_t)(y - w.y0) * w.w + (x - w.x0)];
        if (d < best) { best = d; lab = (uint32_t)i; }
    }
    return (unsigned char)lab;
}

// ---- the kernels ----
// 256 lanes as 64 x 4, one canvas pixel each; the tile is tested once against the n rectangles (block-uniform).
template <bool GAIN, bool PROJ>
__global__ __launch_bounds__(256) void sm_survey_kernel(const SeqWith<SmArgs, GAIN, PROJ> l) {
    const SmArgs& m = l.a;
    const int bx0 = blockIdx.x * 64, by0 = blockIdx.y * 4;
    const uint64_t cand = seq_tile_mask(m.a, bx0, bx0 + 64, by0, by0 + 4);
    const int x = bx0 + (threadIdx.x & 63), y = by0 + seq_wave_row<PROJ>(threadIdx.x >> 6);
    if (x >= m.a.fw || y >= m.a.fh) return;
    uint32_t sv;
    uint64_t cov;
    sm_survey_pixel<GAIN, PROJ>(m.a, cand, x, y, m.margin, m.tau, seq_gains(l), seq_rays(l), sv, cov);
    const int64_t p = (int64_t)y * m.a.fw + x;
    m.sv[p] = sv;
    m.cov[p] = cov;
}

// blockIdx.z is the image; a block takes 64 x 4 pixels of its window (blocks beyond the window leave at once).
__global__ __launch_bounds__(256) void sm_init_kernel(const SmArgs m) {
    const int i = blockIdx.z;
    const SmWin w = m.win[i];
    const int lx = blockIdx.x * 64 + (threadIdx.x & 63), ly = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (lx >= w.w || ly >= w.h) return;
    const int64_t p = (int64_t)(w.y0 + ly) * m.a.fw + w.x0 + lx;
    m.dist[w.off + (int64_t)ly * w.w + lx] = sm_init_pixel(i, m.sv[p], m.cov[p]);
}

// One pass (pass = 1, 2, ...) over every tile of every window; blockIdx.z is the image.  The tile's distances and costs are staged
// once; a lane owns one column of SM_ROWS rows and sweeps them down and then up, in place, so a distance travels a whole row group
// per sweep vertically and one pixel horizontally.  Lanes read their neighbours' distances while those change: every value ever
// stored is the length of a real path, values only fall, and a 32-bit access is whole, so whichever value is read is an upper
// bound and the fixed point is the rule's.  The same holds for the halo, which a neighbouring block may be storing to.
__global__ __launch_bounds__(256) void sm_relax_kernel(const SmArgs m, int pass) {
    __shared__ uint32_t D[SM_TH + 2][SM_TW + 2];
    __shared__ uint16_t C[SM_TH][SM_TW];
    const int i = blockIdx.z;
    const SmWin w = m.win[i];
    const int bx = blockIdx.x, by = blockIdx.y;
    if (bx >= w.tx || by >= w.ty) return;                           // (block-uniform)
    const int64_t tile = w.toff + (int64_t)by * w.tx + bx;
    const unsigned char* was = m.dirty + ((pass & 1) ? 0 : m.tiles);
    unsigned char* now = m.dirty + ((pass & 1) ? m.tiles : 0);
    const bool live = was[tile] | (bx > 0 && was[tile - 1]) | (bx + 1 < w.tx && was[tile + 1]) | (by > 0 && was[tile - w.tx]) |
                      (by + 1 < w.ty && was[tile + w.tx]);
    if (!live) {
        if (threadIdx.x == 0) now[tile] = 0;
        return;
    }
    const int x0 = bx * SM_TW, y0 = by * SM_TH;                     // the tile's corner in the window
    for (int t = threadIdx.x; t < (SM_TH + 2) * (SM_TW + 2); t += 256) {
        const int row = t / (SM_TW + 2), col = t - row * (SM_TW + 2);
        const int lx = x0 + col - 1, ly = y0 + row - 1;
        const bool in = (unsigned)lx < (unsigned)w.w && (unsigned)ly < (unsigned)w.h;
        D[row][col] = in ? m.dist[w.off + (int64_t)ly * w.w + lx] : SM_WALL;
    }
    for (int t = threadIdx.x; t < SM_TH * SM_TW; t += 256) {
        const int row = t / SM_TW, col = t - row * SM_TW;
        const int lx = x0 + col, ly = y0 + row;
        const bool in = lx < w.w && ly < w.h;
        C[row][col] = (uint16_t)(in ? m.sv[(int64_t)(w.y0 + ly) * m.a.fw + w.x0 + lx] & SM_COST_MASK : 1u);
    }
    __syncthreads();
    const int col = threadIdx.x & (SM_TW - 1), r0 = (threadIdx.x / SM_TW) * SM_ROWS;
    uint32_t first[SM_ROWS];
#pragma unroll
    for (int k = 0; k < SM_ROWS; ++k) first[k] = D[r0 + k + 1][col + 1];
    bool changed = false;
    for (int it = 0; it < SM_INNER; ++it) {
        bool ch = false;
#pragma unroll
        for (int s = 0; s < 2 * SM_ROWS; ++s) {
            const int k = s < SM_ROWS ? s : 2 * SM_ROWS - 1 - s, r = r0 + k;
            uint32_t cur = D[r + 1][col + 1];
            const uint32_t nb = sm_min(sm_min(D[r][col + 1], D[r + 2][col + 1]), sm_min(D[r + 1][col], D[r + 1][col + 2]));
            if (sm_relax(cur, nb, C[r][col])) {
                D[r + 1][col + 1] = cur;
                ch = true;
            }
        }
        if (!__syncthreads_or(ch)) break;
        changed = true;
    }
    if (changed) {
#pragma unroll
        for (int k = 0; k < SM_ROWS; ++k) {
            const uint32_t v = D[r0 + k + 1][col + 1];
            const int lx = x0 + col, ly = y0 + r0 + k;
            if (v != first[k] && lx < w.w && ly < w.h) m.dist[w.off + (int64_t)ly * w.w + lx] = v;
        }
    }
    if (threadIdx.x == 0) {
        now[tile] = changed ? 1 : 0;
        if (changed) *m.flag = (uint32_t)pass;
    }
}

__global__ __launch_bounds__(256) void sm_label_kernel(const SmArgs m) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= m.a.fw || y >= m.a.fh) return;
    m.a.dst[(int64_t)y * m.a.fw + x] = sm_label_pixel(m, x, y);
}

// Label paste: the canvas is the labelled winner's bytes (0 where nobody covers).
struct SmPasteArgs { SeqArgs a; const unsigned char* labels; };
__host__ __device__ __forceinline__ void sm_paste_store(const SeqArgs& a, int x, int y, uint32_t px) {
    unsigned char* out = a.dst + ((size_t)y * a.fw + x) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = (unsigned char)(px >> (8 * k));
}
// L: the launch record on SmPasteArgs, SeqWith or (on the gain maps of the block gain rule) SeqWithMaps.
template <bool GAIN, bool PROJ, class L>
__global__ __launch_bounds__(256) void sm_paste_kernel(const L l) {
    const SeqArgs& a = l.a.a;
    const int bx0 = blockIdx.x * 64, by0 = blockIdx.y * 4;
    const uint64_t cand = seq_tile_mask(a, bx0, bx0 + 64, by0, by0 + 4);
    const int x = bx0 + (threadIdx.x & 63), y = by0 + seq_wave_row<PROJ>(threadIdx.x >> 6);
    if (x >= a.fw || y >= a.fh) return;
    const uint32_t px = seq_label_winner_pixel<GAIN, PROJ>(a, cand, x, y, l.a.labels[(int64_t)y * a.fw + x], seq_gains(l), seq_rays(l));
    sm_paste_store(a, x, y, px & 0xffffffu);
}

// ---- the plan: windows and workspace layout ----
struct SmPlan {
    SmWin win[RWH_SEQ_MAX_IMAGES];
    int maxw, maxh, maxtx, maxty;
    int64_t tiles, desc_at, win_at, sv_at, cov_at, dist_at, dirty_at, flag_at, bytes;   // byte offsets, 128-byte aligned
};

static int64_t sm_align(int64_t v) { return (v + 127) & ~(int64_t)127; }

// What the size function and both entry points check of the geometry, and the plan.  tau: the main calls' (the size function
// passes 1): wt * ht * tau <= 2^32 - 3 for every image, so that no distance reaches SM_UNREACHED and no sum wraps.
static int sm_plan(const SeqCall& c, int tau, SmPlan& p) {
    const int32_t* rects = c.rects;
    const int n = c.n, canvas_h = c.canvas_h, canvas_w = c.canvas_w, origin_x = c.origin_x, origin_y = c.origin_y;
    if (!rects || n < 1 || n > RWH_SEQ_MAX_IMAGES || !seq_canvas_ok(canvas_h, canvas_w)) return RWH_E_INVALID;
    p.maxw = p.maxh = p.maxtx = p.maxty = 0;
    int64_t px = 0, tiles = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t wt = rects[4 * i + 2], ht = rects[4 * i + 3];
        const int64_t rx = (int64_t)rects[4 * i] - origin_x, ry = (int64_t)rects[4 * i + 1] - origin_y;
        if (wt <= 0 || ht <= 0) return RWH_E_INVALID;
        if ((uint64_t)wt * (uint64_t)ht > (0xfffffffdull / (uint64_t)tau)) return RWH_E_INVALID;    // (wt, ht < 2^31: no wrap here)
        if (rx < 0 || ry < 0 || rx + wt > canvas_w || ry + ht > canvas_h) return RWH_E_INVALID;
        SmWin& w = p.win[i];
        w.x0 = (int)rx; w.y0 = (int)ry; w.w = (int)wt; w.h = (int)ht;
        w.tx = (w.w + SM_TW - 1) / SM_TW; w.ty = (w.h + SM_TH - 1) / SM_TH;
        w.off = px; w.toff = tiles;
        px += wt * ht;
        tiles += (int64_t)w.tx * w.ty;
        if (w.w > p.maxw) p.maxw = w.w;
        if (w.h > p.maxh) p.maxh = w.h;
        if (w.tx > p.maxtx) p.maxtx = w.tx;
        if (w.ty > p.maxty) p.maxty = w.ty;
    }
    p.tiles = tiles;
    const int64_t canvas = (int64_t)canvas_h * canvas_w;
    int64_t at = 0;
    p.desc_at = at;  at = sm_align(at + (int64_t)n * (int64_t)sizeof(SeqDesc));
    p.win_at = at;   at = sm_align(at + (int64_t)n * (int64_t)sizeof(SmWin));
    p.flag_at = at;  at = sm_align(at + 8);
    p.cov_at = at;   at = sm_align(at + canvas * 8);
    p.sv_at = at;    at = sm_align(at + canvas * 4);
    p.dist_at = at;  at = sm_align(at + px * 4);
    p.dirty_at = at; at = sm_align(at + 2 * tiles);
    p.bytes = at;
    return RWH_OK;
}

// Everything both entry points check, the descriptors and the plan.  The seam rule has no ring form.
static int sm_prepare(const SeqCall& c, const double* gains, double margin, int tau, void* labels, SeqDesc* descs, SmArgs& m, SmPlan& p,
                      bool device) {
    if (c.form == SEQ_RING) return RWH_E_INVALID;
    int st = seq_prepare_indexed(c, labels, descs, m.a, device);
    if (st != RWH_OK) return st;
    if (gains && !seq_gains_ok(gains, c.n)) return RWH_E_INVALID;
    if (!(margin >= 0.0) || tau < 1 || tau > 766) return RWH_E_INVALID;          // (a NaN margin is not >= 0)
    st = sm_plan(c, tau, p);
    if (st != RWH_OK) return st;
    m.margin = margin; m.tau = tau; m.tiles = p.tiles;
    return RWH_OK;
}

static void sm_bind(SmArgs& m, const SmPlan& p, char* base) {
    m.a.desc = reinterpret_cast<const SeqDesc*>(base + p.desc_at);
    m.win = reinterpret_cast<const SmWin*>(base + p.win_at);
    m.flag = reinterpret_cast<uint32_t*>(base + p.flag_at);
    m.cov = reinterpret_cast<uint64_t*>(base + p.cov_at);
    m.sv = reinterpret_cast<uint32_t*>(base + p.sv_at);
    m.dist = reinterpret_cast<uint32_t*>(base + p.dist_at);
    m.dirty = reinterpret_cast<unsigned char*>(base + p.dirty_at);
}

// The host twin's distances of one image: Dijkstra with a binary heap over the image's window -- on purpose not the device's
// algorithm.  A popped entry that is no longer the pixel's distance is stale and skipped.
static void sm_host_dijkstra(const SmArgs& m, int i) {
    const SmWin& w = m.win[i];
    uint32_t* d = m.dist + w.off;
    typedef std::pair<uint32_t, uint32_t> Entry;                    // (distance, pixel of the window)
    std::priority_queue<Entry, std::vector<Entry>, std::greater<Entry> > heap;
    for (int ly = 0; ly < w.h; ++ly)
        for (int lx = 0; lx < w.w; ++lx) {
            const int64_t p = (int64_t)(w.y0 + ly) * m.a.fw + w.x0 + lx;
            const uint32_t v = sm_init_pixel(i, m.sv[p], m.cov[p]);
            d[(int64_t)ly * w.w + lx] = v;
            if (v == 0) heap.push(Entry(0u, (uint32_t)((int64_t)ly * w.w + lx)));
        }
    while (!heap.empty()) {
        const Entry e = heap.top();
        heap.pop();
        if (d[e.second] != e.first) continue;
        const int ly = (int)(e.second / (uint32_t)w.w), lx = (int)(e.second % (uint32_t)w.w);
        const int nx[4] = {lx - 1, lx + 1, lx, lx}, ny[4] = {ly, ly, ly - 1, ly + 1};
        for (int k = 0; k < 4; ++k) {
            if ((unsigned)nx[k] >= (unsigned)w.w || (unsigned)ny[k] >= (unsigned)w.h) continue;
            const uint32_t q = (uint32_t)((int64_t)ny[k] * w.w + nx[k]);
            const uint32_t c = m.sv[(int64_t)(w.y0 + ny[k]) * m.a.fw + w.x0 + nx[k]] & SM_COST_MASK;
            if (sm_relax(d[q], e.first, c)) heap.push(Entry(d[q], q));
        }
    }
}

template <bool GAIN, bool PROJ>
static void sm_host_run(const SmArgs& m, const double* gains, SeqRays rays) {
    const uint64_t all = seq_all(m.a.n);
    for (int y = 0; y < m.a.fh; ++y)
        for (int x = 0; x < m.a.fw; ++x) {
            const int64_t p = (int64_t)y * m.a.fw + x;
            sm_survey_pixel<GAIN, PROJ>(m.a, all, x, y, m.margin, m.tau, gains, rays, m.sv[p], m.cov[p]);
        }
    for (int i = 0; i < m.a.n; ++i) sm_host_dijkstra(m, i);
    for (int y = 0; y < m.a.fh; ++y)
        for (int x = 0; x < m.a.fw; ++x) m.a.dst[(int64_t)y * m.a.fw + x] = sm_label_pixel(m, x, y);
}

// The device call behind rwh_sequence_seams and rwh_sequence_seams_proj.  The seam rule's gain switch has two states (no maps).
// The host loop reads the flag after every SM_BATCH passes and so synchronises the stream.
static int sm_device(const SeqCall& c, const double* gains, double margin, int tau, unsigned char* d_labels, void* d_workspace,
                     int64_t workspace_bytes, void* stream, int32_t* passes) {
    SeqDesc descs[RWH_SEQ_MAX_IMAGES];
    SmArgs m;
    SmPlan p;
    const int n = c.n;
    const int st = sm_prepare(c, gains, margin, tau, d_labels, descs, m, p, true);
    if (st != RWH_OK) return st;
    if (!d_workspace || workspace_bytes < p.bytes || ((uintptr_t)d_workspace & 7u)) return RWH_E_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(d_workspace);
    seq_put(descs, (size_t)n * SEQ_DESC_WORDS, reinterpret_cast<uint64_t*>(base + p.desc_at), s);
    seq_put(p.win, (size_t)n * (sizeof(SmWin) / 8), reinterpret_cast<uint64_t*>(base + p.win_at), s);
    sm_bind(m, p, base);
    if (fill_async(m.flag, 0, 8, s) != hipSuccess) return RWH_E_LAUNCH;
    if (fill_async(m.dirty, 1, (size_t)p.tiles, s) != hipSuccess) return RWH_E_LAUNCH;      // pass 1 reads array 0: every tile live
    seq_form_dispatch<false>(c.form, [&](auto form) {
        seq_gain_dispatch<false>(seq_gain_n(gains), [&](auto on, const double* value) {
            constexpr bool GAIN = decltype(on)::value, PROJ = decltype(form)::proj;
            hipLaunchKernelGGL((sm_survey_kernel<GAIN, PROJ>), dim3((m.a.fw + 63) / 64, (m.a.fh + 3) / 4), dim3(256), 0, s,
                               seq_with<GAIN, PROJ>(m, value, n, c.rays));
        });
    });
    hipLaunchKernelGGL(sm_init_kernel, dim3((p.maxw + 63) / 64, (p.maxh + 3) / 4, n), dim3(256), 0, s, m);
    uint32_t last = 0;
    int launched = 0;
    do {
        for (int b = 0; b < SM_BATCH; ++b)
            hipLaunchKernelGGL(sm_relax_kernel, dim3(p.maxtx, p.maxty, n), dim3(256), 0, s, m, ++launched);
        if (hipMemcpyAsync(&last, m.flag, 4, hipMemcpyDeviceToHost, s) != hipSuccess) return RWH_E_LAUNCH;
        if (hipStreamSynchronize(s) != hipSuccess) return RWH_E_LAUNCH;
    } while ((int64_t)last >= (int64_t)launched);                   // the last pass launched still changed something
    if (passes) *passes = (int32_t)last;
    hipLaunchKernelGGL(sm_label_kernel, dim3((c.canvas_w + 63) / 64, (c.canvas_h + 3) / 4), dim3(256), 0, s, m);
    return check_launch();
}

static int sm_host(const SeqCall& c, const double* gains, double margin, int tau, unsigned char* labels) {
    SeqDesc descs[RWH_SEQ_MAX_IMAGES];
    SmArgs m;
    SmPlan p;
    const int st = sm_prepare(c, gains, margin, tau, labels, descs, m, p, false);
    if (st != RWH_OK) return st;
    char* base = static_cast<char*>(malloc((size_t)p.bytes));
    if (!base) return RWH_E_LAUNCH;
    memcpy(base + p.desc_at, descs, (size_t)c.n * sizeof(SeqDesc));
    memcpy(base + p.win_at, p.win, (size_t)c.n * sizeof(SmWin));
    sm_bind(m, p, base);
    int out = RWH_OK;
    try {
        seq_form_dispatch<false>(c.form, [&](auto form) {
            seq_gain_dispatch<false>(seq_gain_n(gains), [&](auto on, const double* value) {
                sm_host_run<decltype(on)::value, decltype(form)::proj>(m, value, c.rays);
            });
        });
    } catch (const std::bad_alloc&) {
        out = RWH_E_LAUNCH;
    }
    free(base);
    return out;
}

// ---- label paste ----
// What both label-paste entry points check, and their arguments.  Label paste has no ring form.
static int sm_paste_prepare(const SeqCall& c, SeqGain& gain, const unsigned char* labels, void* canvas, SeqDesc* descs, SeqArgs& a, bool device) {
    if (!labels || c.form == SEQ_RING) return RWH_E_INVALID;
    const int st = seq_prepare_indexed(c, canvas, descs, a, device);
    if (st != RWH_OK) return st;
    return seq_gain_ok(gain, c, !device) ? RWH_OK : RWH_E_INVALID;
}

static int sm_paste_device(const SeqCall& c, SeqGain gain, const unsigned char* d_labels, void* d_canvas, void* d_workspace,
                           int64_t workspace_bytes, void* stream) {
    SeqDesc descs[RWH_SEQ_MAX_IMAGES];
    SmPasteArgs m;
    const int st = sm_paste_prepare(c, gain, d_labels, d_canvas, descs, m.a, true);
    if (st != RWH_OK) return st;
    if (!d_workspace || workspace_bytes < (int64_t)c.n * (int64_t)sizeof(SeqDesc) || ((uintptr_t)d_workspace & 7u)) return RWH_E_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    seq_put(descs, (size_t)c.n * SEQ_DESC_WORDS, static_cast<uint64_t*>(d_workspace), s);
    m.a.desc = static_cast<const SeqDesc*>(d_workspace);
    m.labels = d_labels;
    const dim3 grid((c.canvas_w + 63) / 64, (c.canvas_h + 3) / 4);
    seq_form_dispatch<false>(c.form, [&](auto form) {
        seq_gain_dispatch(gain, [&](auto on, auto value) {
            constexpr bool GAIN = decltype(on)::value, PROJ = decltype(form)::proj;
            auto l = seq_with<GAIN, PROJ>(m, value, c.n, c.rays);
            hipLaunchKernelGGL((sm_paste_kernel<GAIN, PROJ, decltype(l)>), grid, dim3(256), 0, s, l);
        });
    });
    return check_launch();
}

static int sm_paste_host(const SeqCall& c, SeqGain gain, const unsigned char* labels, void* canvas) {
    SeqDesc descs[RWH_SEQ_MAX_IMAGES];
    SeqArgs a;
    const int st = sm_paste_prepare(c, gain, labels, canvas, descs, a, false);
    if (st != RWH_OK) return st;
    const uint64_t all = seq_all(c.n);
    seq_form_dispatch<false>(c.form, [&](auto form) {
        seq_gain_dispatch(gain, [&](auto on, auto value) {
            for (int y = 0; y < c.canvas_h; ++y)
                for (int x = 0; x < c.canvas_w; ++x) {
                    const uint32_t lab = labels[(int64_t)y * c.canvas_w + x];
                    const uint32_t px = seq_label_winner_pixel<decltype(on)::value, decltype(form)::proj>(a, all, x, y, lab, value, c.rays);
                    sm_paste_store(a, x, y, px & 0xffffffu);
                }
        });
    });
    return RWH_OK;
}

}  // namespace rwh

using rwh::seq_curved;
using rwh::seq_gain_maps;
using rwh::seq_gain_n;
using rwh::seq_plane;

extern "C" int64_t rwh_sequence_seams_workspace_bytes(const int32_t* rects, int n, int canvas_h, int canvas_w, int origin_x, int origin_y) {
    rwh::SmPlan p;
    const int st = rwh::sm_plan(rwh::seq_frame(rects, n, canvas_h, canvas_w, origin_x, origin_y), 1, p);
    return st == RWH_OK ? p.bytes : (int64_t)st;
}

// Every entry point below: the geometry record of its form, then the driver.
extern "C" int rwh_sequence_seams(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                  int anchor, const double* gains, double margin, int tau, unsigned char* d_labels, int canvas_h,
                                  int canvas_w, int origin_x, int origin_y, void* d_workspace, int64_t workspace_bytes, void* stream,
                                  int32_t* passes) {
    return rwh::sm_device(seq_plane(d_images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), gains, margin, tau,
                          d_labels, d_workspace, workspace_bytes, stream, passes);
}

extern "C" int rwh_sequence_seams_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                       const double* gains, double margin, int tau, const double* d_col, const double* d_row,
                                       unsigned char* d_labels, int canvas_h, int canvas_w, void* d_workspace, int64_t workspace_bytes,
                                       void* stream, int32_t* passes) {
    return rwh::sm_device(seq_curved(d_images, hw, m, rects, n, d_col, d_row, canvas_h, canvas_w), gains, margin, tau, d_labels,
                          d_workspace, workspace_bytes, stream, passes);
}

extern "C" int rwh_host_sequence_seams(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                       int anchor, const double* gains, double margin, int tau, unsigned char* labels, int canvas_h,
                                       int canvas_w, int origin_x, int origin_y) {
    return rwh::sm_host(seq_plane(images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), gains, margin, tau, labels);
}

extern "C" int rwh_host_sequence_seams_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                            const double* gains, double margin, int tau, const double* col, const double* row,
                                            unsigned char* labels, int canvas_h, int canvas_w) {
    return rwh::sm_host(seq_curved(images, hw, m, rects, n, col, row, canvas_h, canvas_w), gains, margin, tau, labels);
}

extern "C" int rwh_stitch_sequence_labels(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                          int anchor, const double* gains, const unsigned char* d_labels, void* d_canvas, int canvas_h,
                                          int canvas_w, int origin_x, int origin_y, void* d_workspace, int64_t workspace_bytes,
                                          void* stream) {
    return rwh::sm_paste_device(seq_plane(d_images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), seq_gain_n(gains),
                                d_labels, d_canvas, d_workspace, workspace_bytes, stream);
}

extern "C" int rwh_stitch_sequence_labels_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                               const double* gains, const unsigned char* d_labels, const double* d_col,
                                               const double* d_row, void* d_canvas, int canvas_h, int canvas_w, void* d_workspace,
                                               int64_t workspace_bytes, void* stream) {
    return rwh::sm_paste_device(seq_curved(d_images, hw, m, rects, n, d_col, d_row, canvas_h, canvas_w), seq_gain_n(gains), d_labels,
                                d_canvas, d_workspace, workspace_bytes, stream);
}

extern "C" int rwh_host_stitch_sequence_labels(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects,
                                               int n, int anchor, const double* gains, const unsigned char* labels, void* canvas,
                                               int canvas_h, int canvas_w, int origin_x, int origin_y) {
    return rwh::sm_paste_host(seq_plane(images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), seq_gain_n(gains),
                              labels, canvas);
}

extern "C" int rwh_host_stitch_sequence_labels_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects,
                                                    int n, const double* gains, const unsigned char* labels, const double* col,
                                                    const double* row, void* canvas, int canvas_h, int canvas_w) {
    return rwh::sm_paste_host(seq_curved(images, hw, m, rects, n, col, row, canvas_h, canvas_w), seq_gain_n(gains), labels, canvas);
}

// Label paste on the gain maps of the block gain rule: d_maps / maps and shift where the calls above take gains.  The host twins
// read the maps: every entry finite and > 0.
extern "C" int rwh_stitch_sequence_labels_maps(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                               int anchor, const double* d_maps, int shift, const unsigned char* d_labels, void* d_canvas,
                                               int canvas_h, int canvas_w, int origin_x, int origin_y, void* d_workspace,
                                               int64_t workspace_bytes, void* stream) {
    return rwh::sm_paste_device(seq_plane(d_images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y),
                                seq_gain_maps(d_maps, shift), d_labels, d_canvas, d_workspace, workspace_bytes, stream);
}

extern "C" int rwh_stitch_sequence_labels_maps_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                                    const double* d_maps, int shift, const unsigned char* d_labels, const double* d_col,
                                                    const double* d_row, void* d_canvas, int canvas_h, int canvas_w, void* d_workspace,
                                                    int64_t workspace_bytes, void* stream) {
    return rwh::sm_paste_device(seq_curved(d_images, hw, m, rects, n, d_col, d_row, canvas_h, canvas_w), seq_gain_maps(d_maps, shift),
                                d_labels, d_canvas, d_workspace, workspace_bytes, stream);
}

extern "C" int rwh_host_stitch_sequence_labels_maps(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects,
                                                    int n, int anchor, const double* maps_in, int shift, const unsigned char* labels,
                                                    void* canvas, int canvas_h, int canvas_w, int origin_x, int origin_y) {
    return rwh::sm_paste_host(seq_plane(images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y),
                              seq_gain_maps(maps_in, shift), labels, canvas);
}

extern "C" int rwh_host_stitch_sequence_labels_maps_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects,
                                                         int n, const double* maps_in, int shift, const unsigned char* labels,
                                                         const double* col, const double* row, void* canvas, int canvas_h, int canvas_w) {
    return rwh::sm_paste_host(seq_curved(images, hw, m, rects, n, col, row, canvas_h, canvas_w), seq_gain_maps(maps_in, shift), labels, canvas);
}
