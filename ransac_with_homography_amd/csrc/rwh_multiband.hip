// Multi-band blending for the sequence compositor (include/rwh.h, "The multi-band rule"; Burt & Adelson 1983 as Brown & Lowe 2007,
// section 7, use it): every image gets a Gaussian pyramid of its bytes (its own where it covers, the winner's elsewhere) and of its
// winner mask, the Laplacian bands are averaged with the mask pyramids as weights, and the blended bands are collapsed into the
// canvas.  From the planes onward everything is integer arithmetic; the per-pixel and per-stencil functions below are compiled for
// the device and for the host twin (rwh_host_stitch_multiband), so the two run one arithmetic.
//
// The plan ("Multi-band blending"): image i works in one WINDOW per level, the interval the rule can read of it
// (mb_plan), all windows of a level batched into one launch (blockIdx.z is the image).
//   1. mb_winner_kernel: one pass over the padded canvas, P and the winner's index in one dword per pixel.
//   2. mb_level0_kernel: G_i^0 = (I_i, W_i) as four int16 over image i's level-0 window.
//   3. mb_down_kernel, K times: the 5 x 5 reduce; a block stages its (2 * 32 + 3) x (2 * 8 + 3) source tile in LDS, even and odd
//      columns apart, so that the stride-2 taps of neighbouring lanes are neighbouring 8-byte words.
//   4. mb_collapse_kernel, from level K down to 0, one pass over the CANVAS plane of the level: a pixel visits the images whose
//      window holds it, forms L_i^l = G_i^l - up(G_i^{l+1}) where W_i^l > 0, sums num and den in registers, normalises, adds
//      up(R^{l+1}) and stores R^l -- at level 0 the clamped bytes.  num and den never reach memory: no atomics, no zeroing, and the
//      sums are integers, so their order does not matter.
#include <stdlib.h>
#include "rwh_sequence.h"

namespace rwh {

// One pixel of a pyramid plane: three channels and the weight (G planes) or three channels and a spare (R planes).
struct __attribute__((aligned(8))) MbPx { int16_t c[4]; };
static_assert(sizeof(MbPx) == 8, "a plane pixel is one 8-byte word");
constexpr int MB_ONE = 16384;                  // the weight of a winner
constexpr uint32_t MB_NONE = 0xffu;            // the winner byte of a pixel nobody covers

// Image i at level l: columns [x0, x0 + w) and rows [y0, y0 + h) of the level's plane, row-major at `off` (in pixels) of the G area.
struct MbWin { int x0, y0, w, h; int64_t off; };
static_assert(sizeof(MbWin) == 24, "MbWin is copied as 8-byte words");
constexpr int MB_LEVELS = RWH_SEQ_MAX_BANDS + 1;

struct MbArgs {
    SeqArgs a;                  // order: 0 .. n-1 (candidate bits are image indices); dst: the canvas; row_begin, row_end unused
    const MbWin* win;           // [n][K + 1]
    uint32_t* pw;               // PH x PW: P as 0x00BBGGRR, the winner's index (MB_NONE: nobody) in the top byte
    MbPx* g;                    // the G windows
    MbPx* r[MB_LEVELS];         // R^l, the whole (PH >> l) x (PW >> l) plane, l = 1 .. K (r[0] unused: R^0 is the canvas)
    int K, PW, PH;
};
// The labelled winner pass's arguments: MbArgs stays the record the other kernels take.
struct MbLabelArgs { MbArgs m; const unsigned char* labels; };   // labels: fh x fw, the label plane of the seam rule

// ---- the per-pixel functions ----
// P and the winner at canvas pixel (cx, cy): the covering image with the greatest feather weight g, the lowest index on equal
// weights (candidates are visited in index order and only a greater g replaces the best; g >= 1 wherever an image covers).
// rays: the ray tables of the projection rule, read with PROJ only.
template <bool GAIN, bool PROJ = false, bool RING = false, class G = const double*>
__host__ __device__ __forceinline__ uint32_t mb_winner_pixel(const SeqArgs& a, uint64_t cand, int cx, int cy, G gains,
                                                             SeqRays rays = SeqRays{nullptr, nullptr}) {
    const int fx = a.ox + cx, fy = a.oy + cy;
    SeqRay ray;
    if constexpr (PROJ) ray = seq_ray(rays, cx, cy);
    [[maybe_unused]] const auto site = seq_gain_site(gains, cx, cy);
    double best = 0.0;
    uint32_t out = MB_NONE << 24;
    for (uint64_t m = cand; m; m &= m - 1) {
        const int i = __builtin_ctzll(m);
        double v[3], g = 0.0, gain = 1.0;
        if constexpr (GAIN) gain = seq_gain_of(site, i);
        if (!seq_sample<true, GAIN, PROJ, RING>(a.desc[i], i == a.anchor, fx, fy, v, g, gain, &ray, a.fw)) continue;
        if (g > best) {
            best = g;
            out = (uint32_t)i << 24;
#pragma unroll
            for (int k = 0; k < 3; ++k) out |= (uint32_t)(unsigned char)(int)v[k] << (8 * k);
        }
    }
    return out;
}

// (I_i, W_i) at plane pixel (x, y) of level 0: image i's bytes where it covers, P elsewhere; MB_ONE where i is the winner.
template <bool GAIN, bool PROJ = false, bool RING = false, class G = const double*>
__host__ __device__ __forceinline__ MbPx mb_level0_pixel(const SeqArgs& a, int i, uint32_t pwv, int x, int y, G gains,
                                                         SeqRays rays = SeqRays{nullptr, nullptr}) {
    MbPx o;
#pragma unroll
    for (int k = 0; k < 3; ++k) o.c[k] = (int16_t)((pwv >> (8 * k)) & 0xffu);
    o.c[3] = (int16_t)((pwv >> 24) == (uint32_t)i ? MB_ONE : 0);
    if (x < a.fw && y < a.fh) {
        double v[3], g = 0.0, gain = 1.0;
        if constexpr (GAIN) gain = seq_gain_of(seq_gain_site(gains, x, y), i);
        SeqRay ray;
        if constexpr (PROJ) ray = seq_ray(rays, x, y);
        if (seq_sample<false, GAIN, PROJ, RING>(a.desc[i], i == a.anchor, a.ox + x, a.oy + y, v, g, gain, &ray, a.fw)) {
#pragma unroll
            for (int k = 0; k < 3; ++k) o.c[k] = (int16_t)(unsigned char)(int)v[k];
        }
    }
    return o;
}

// A window's pixel at plane coordinates (x, y); 0 outside the window (beyond the plane's edge the rule reads 0, and inside the plane
// the windows are made so that nothing outside them is ever needed: mb_plan).
// RING (the ring rule): the level's plane is periodic in x with `period` columns and the window is an interval of the unwrapped
// axis, x0 possibly negative or x0 + w past the period; x may be any tap, left of 0 or past the period.  The one place where a ring
// window is indexed: a non-negative modulo, then the same bounds test.
__host__ __device__ __forceinline__ int mb_mod(int x, int period) {
    if ((unsigned)x < (unsigned)period) return x;       // (most taps; a wave away from the seam never divides)
    x %= period;
    return x + (x < 0 ? period : 0);
}
template <bool RING = false>
__host__ __device__ __forceinline__ MbPx mb_fetch(const MbPx* g, const MbWin& w, int x, int y, int period = 0) {
    x -= w.x0; y -= w.y0;
    if constexpr (RING) x = mb_mod(x, period);
    if ((unsigned)x >= (unsigned)w.w || (unsigned)y >= (unsigned)w.h) return MbPx{{0, 0, 0, 0}};
    return g[w.off + (int64_t)y * w.w + x];
}

// Reduce: at(ky, kx) is S[2y + ky][2x + kx].  All four channels are non-negative; 256 * 16384 fits int32.
template <class F>
__host__ __device__ __forceinline__ MbPx mb_down(const F& at) {
    int s[4] = {0, 0, 0, 0};
#pragma unroll
    for (int ky = -2; ky <= 2; ++ky) {
        const int wy = ky == 0 ? 6 : (ky == 1 || ky == -1) ? 4 : 1;
#pragma unroll
        for (int kx = -2; kx <= 2; ++kx) {
            const int wx = kx == 0 ? 6 : (kx == 1 || kx == -1) ? 4 : 1;
            const MbPx p = at(ky, kx);
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] += wy * wx * (int)p.c[k];
        }
    }
    MbPx o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o.c[k] = (int16_t)((s[k] + 128) >> 8);
    return o;
}

// Expand at (x, y): at(yy, xx) is S[yy][xx] of the level above.  The taps with y + ky and x + kx even: an even coordinate c reads
// c/2 - 1, c/2, c/2 + 1 with weights 1 6 1, an odd one (c-1)/2 and (c+1)/2 with 4 4.  The shift is arithmetic: floor for negative sums.
template <class F>
__host__ __device__ __forceinline__ void mb_up(const F& at, int x, int y, int out[3]) {
    int s[3] = {0, 0, 0};
    const int bx = x >> 1, by = y >> 1;
#pragma unroll
    for (int j = -1; j <= 1; ++j) {
        const int wy = (y & 1) ? (j < 0 ? 0 : 4) : (j == 0 ? 6 : 1);
        if (!wy) continue;
#pragma unroll
        for (int i = -1; i <= 1; ++i) {
            const int wx = (x & 1) ? (i < 0 ? 0 : 4) : (i == 0 ? 6 : 1);
            if (!wx) continue;
            const MbPx p = at(by + j, bx + i);
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] += wy * wx * (int)p.c[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = (s[k] + 32) >> 6;
}

struct MbWinAt {                // a G window as mb_up's source
    const MbPx* g; const MbWin& w;
    __host__ __device__ __forceinline__ MbPx operator()(int y, int x) const { return mb_fetch(g, w, x, y); }
};
struct MbPlaneAt {              // a whole R plane as mb_up's source, 0 beyond its edge
    const MbPx* r; int w, h;
    __host__ __device__ __forceinline__ MbPx operator()(int y, int x) const {
        if ((unsigned)x >= (unsigned)w || (unsigned)y >= (unsigned)h) return MbPx{{0, 0, 0, 0}};
        return r[(int64_t)y * w + x];
    }
};

template <bool RING> struct MbRingWinAt {     // MbWinAt with the accessor's form (RING: on a ring of `period` columns)
    const MbPx* g; const MbWin& w; int period;
    __host__ __device__ __forceinline__ MbPx operator()(int y, int x) const { return mb_fetch<RING>(g, w, x, y, period); }
};
struct MbRingPlaneAt {          // a whole R plane of the ring rule: periodic in x, 0 above and below
    const MbPx* r; int w, h;
    __host__ __device__ __forceinline__ MbPx operator()(int y, int x) const {
        if ((unsigned)y >= (unsigned)h) return MbPx{{0, 0, 0, 0}};
        return r[(int64_t)y * w + mb_mod(x, w)];
    }
};

// R^l at plane pixel (x, y) of level l: bands, accumulate, normalise and one collapse step.  cand: the images whose level-l window
// may hold the pixel.
template <bool RING = false>
__host__ __device__ __forceinline__ void mb_collapse_pixel(const MbArgs& m, int l, uint64_t cand, int x, int y, int R[3]) {
    int num[3] = {0, 0, 0}, den = 0;
    for (uint64_t c = cand; c; c &= c - 1) {
        const int i = __builtin_ctzll(c);
        const MbWin* w = m.win + (size_t)i * (m.K + 1) + l;
        const MbPx gp = mb_fetch<RING>(m.g, w[0], x, y, m.PW >> l);
        const int wt = gp.c[3];
        if (wt <= 0) continue;
        int L[3] = {gp.c[0], gp.c[1], gp.c[2]};
        if (l < m.K) {
            int u[3];
            if constexpr (RING) mb_up(MbRingWinAt<true>{m.g, w[1], m.PW >> (l + 1)}, x, y, u);
            else mb_up(MbWinAt{m.g, w[1]}, x, y, u);
#pragma unroll
            for (int k = 0; k < 3; ++k) L[k] -= u[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) num[k] += L[k] * wt;
        den += wt;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int b = 0;
        if (den) {
            const int mag = ((num[k] < 0 ? -num[k] : num[k]) + den / 2) / den;
            b = num[k] < 0 ? -mag : mag;
        }
        R[k] = b;
    }
    if (l < m.K) {
        int u[3];
        if constexpr (RING) mb_up(MbRingPlaneAt{m.r[l + 1], m.PW >> (l + 1), m.PH >> (l + 1)}, x, y, u);
        else mb_up(MbPlaneAt{m.r[l + 1], m.PW >> (l + 1), m.PH >> (l + 1)}, x, y, u);
#pragma unroll
        for (int k = 0; k < 3; ++k) R[k] += u[k];
    }
}

// R^l stored: an R plane's pixel, or at level 0 the canvas bytes (0 where nobody covers; outside the canvas nothing is written).
__host__ __device__ __forceinline__ void mb_store(const MbArgs& m, int l, int x, int y, const int R[3]) {
    if (l) {
        m.r[l][(int64_t)y * (m.PW >> l) + x] = MbPx{{(int16_t)R[0], (int16_t)R[1], (int16_t)R[2], 0}};
        return;
    }
    if (x >= m.a.fw || y >= m.a.fh) return;
    const bool covered = (m.pw[(int64_t)y * m.PW + x] >> 24) != MB_NONE;
    unsigned char* out = m.a.dst + ((size_t)y * m.a.fw + x) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = (unsigned char)(covered ? (R[k] < 0 ? 0 : R[k] > 255 ? 255 : R[k]) : 0);
}

// The images whose level-l window meets columns [x0, x1) and rows [y0, y1) of the level's plane.
// RING: a window is an interval of the unwrapped axis that starts within one period of the plane (mb_plan), so it is also tested
// shifted by the level's period either way.
template <bool RING = false>
__host__ __device__ __forceinline__ uint64_t mb_window_mask(const MbArgs& m, int l, int x0, int x1, int y0, int y1) {
    uint64_t c = 0;
    for (int i = 0; i < m.a.n; ++i) {
        const MbWin& w = m.win[(size_t)i * (m.K + 1) + l];
        bool cols = (w.x0 < x1) & (w.x0 + w.w > x0);
        if constexpr (RING) {
            const int period = m.PW >> l;
            cols |= ((w.x0 + period < x1) & (w.x0 + period + w.w > x0)) | ((w.x0 - period < x1) & (w.x0 - period + w.w > x0));
        }
        if (cols & (w.y0 < y1) & (w.y0 + w.h > y0)) c |= 1ull << i;
    }
    return c;
}

// ---- the kernels ----
// The three head kernels take their launch record as L -- SeqWith<.., GAIN, PROJ>, or SeqWithMaps<.., PROJ> on the gain maps of the
// block gain rule -- so each is one body for every state of the gain switch.
// 256 lanes as 64 x 4, one pixel of the padded canvas each; the tile is tested once against the n rectangles (block-uniform).
template <bool GAIN, bool PROJ, bool RING, class L>
__global__ __launch_bounds__(256) void mb_winner_kernel(const L l) {
    const MbArgs& m = l.a;
    const int bx0 = blockIdx.x * 64, by0 = blockIdx.y * 4;
    const uint64_t cand = seq_tile_mask<RING>(m.a, bx0, bx0 + 64, by0, by0 + 4);
    const int x = bx0 + (threadIdx.x & 63), y = by0 + seq_wave_row<PROJ>(threadIdx.x >> 6);
    if (x >= m.PW || y >= m.PH) return;
    const bool on = x < m.a.fw && y < m.a.fh;
    m.pw[(int64_t)y * m.PW + x] = on ? mb_winner_pixel<GAIN, PROJ, RING>(m.a, cand, x, y, seq_gains(l), seq_rays(l)) : MB_NONE << 24;
}

// mb_winner_kernel under a label plane (the seam rule, "Using labels"): the pixel's label names the winner where that image covers
// the pixel, the multi-band rule's own Winner stands everywhere else.  A kernel of its own: the unlabelled pass stays the code it was.
// L is a record on MbLabelArgs.  No ring form.
template <bool GAIN, bool PROJ, class L>
__global__ __launch_bounds__(256) void mb_label_winner_kernel(const L l) {
    const MbArgs& m = l.a.m;
    const int bx0 = blockIdx.x * 64, by0 = blockIdx.y * 4;
    const uint64_t cand = seq_tile_mask(m.a, bx0, bx0 + 64, by0, by0 + 4);
    const int x = bx0 + (threadIdx.x & 63), y = by0 + seq_wave_row<PROJ>(threadIdx.x >> 6);
    if (x >= m.PW || y >= m.PH) return;
    uint32_t out = MB_NONE << 24;
    if (x < m.a.fw && y < m.a.fh) out = seq_label_winner_pixel<GAIN, PROJ>(m.a, cand, x, y, l.a.labels[(int64_t)y * m.a.fw + x], seq_gains(l), seq_rays(l));
    m.pw[(int64_t)y * m.PW + x] = out;
}

// blockIdx.z is the image; a block takes 64 x 4 pixels of its level-0 window (blocks beyond the window leave at once).
// RING: the window's columns are taken modulo the period (PW).
template <bool GAIN, bool PROJ, bool RING, class L>
__global__ __launch_bounds__(256) void mb_level0_kernel(const L l) {
    const MbArgs& m = l.a;
    const int i = blockIdx.z;
    const MbWin w = m.win[(size_t)i * (m.K + 1)];
    const int lx = blockIdx.x * 64 + (threadIdx.x & 63), ly = blockIdx.y * 4 + seq_wave_row<PROJ>(threadIdx.x >> 6);
    if (lx >= w.w || ly >= w.h) return;
    const int x = RING ? mb_mod(w.x0 + lx, m.PW) : w.x0 + lx, y = w.y0 + ly;
    m.g[w.off + (int64_t)ly * w.w + lx] = mb_level0_pixel<GAIN, PROJ, RING>(m.a, i, m.pw[(int64_t)y * m.PW + x], x, y, seq_gains(l), seq_rays(l));
}

// The reduce from level l to l + 1 of image blockIdx.z.  A block makes MB_TW x MB_TH outputs from a (2 MB_TW + 3) x (2 MB_TH + 3)
// source tile staged in LDS with whole-pixel (8-byte) loads, coalesced along the row.  Source column 2 X0 - 2 + j goes to E[j / 2]
// (j even) or O[j / 2] (j odd): output tx then reads E[tx], O[tx], E[tx + 1], O[tx + 1], E[tx + 2], and the 32 lanes of a tile
// row -- one lane group of ds_read_b64 -- read 32 consecutive 8-byte words, one 256-byte bank row: no conflict, whatever the pitch.
constexpr int MB_TW = 32, MB_TH = 8, MB_SH = 2 * MB_TH + 3, MB_SW = 2 * MB_TW + 3, MB_EW = MB_TW + 2;
struct MbLdsAt {
    const MbPx (*E)[MB_EW]; const MbPx (*O)[MB_EW]; int tx, ty;
    __device__ __forceinline__ MbPx operator()(int ky, int kx) const {
        const int row = 2 * ty + ky + 2;
        return (kx & 1) ? O[row][tx + ((kx + 1) >> 1)] : E[row][tx + ((kx + 2) >> 1)];
    }
};
template <bool RING = false>
__global__ __launch_bounds__(256) void mb_down_kernel(const MbArgs m, int l) {
    __shared__ MbPx E[MB_SH][MB_EW], O[MB_SH][MB_EW];
    const int i = blockIdx.z;
    const MbWin src = m.win[(size_t)i * (m.K + 1) + l], dst = m.win[(size_t)i * (m.K + 1) + l + 1];
    const int ox0 = blockIdx.x * MB_TW, oy0 = blockIdx.y * MB_TH;
    if (ox0 >= dst.w || oy0 >= dst.h) return;                      // (block-uniform)
    const int c0 = 2 * (dst.x0 + ox0) - 2, r0 = 2 * (dst.y0 + oy0) - 2;
    for (int t = threadIdx.x; t < MB_SH * MB_SW; t += 256) {
        const int row = t / MB_SW, j = t - row * MB_SW;
        const MbPx v = mb_fetch<RING>(m.g, src, c0 + j, r0 + row, m.PW >> l);
        if (j & 1) O[row][j >> 1] = v; else E[row][j >> 1] = v;
    }
    __syncthreads();
    const int tx = threadIdx.x & (MB_TW - 1), ty = threadIdx.x / MB_TW;
    if (ox0 + tx >= dst.w || oy0 + ty >= dst.h) return;
    m.g[dst.off + (int64_t)(oy0 + ty) * dst.w + ox0 + tx] = mb_down(MbLdsAt{E, O, tx, ty});
}

template <bool RING = false>
struct MbWinTap {               // the host twin's source of mb_down: the window itself (RING: on a ring of `period` columns)
    const MbPx* g; const MbWin& w; int x, y, period;
    __host__ __device__ __forceinline__ MbPx operator()(int ky, int kx) const { return mb_fetch<RING>(g, w, 2 * x + kx, 2 * y + ky, period); }
};

// One pass over the plane of level l, 64 x 4 pixels per block; the tile is tested once against the n windows of the level.
template <bool RING = false>
__global__ __launch_bounds__(256) void mb_collapse_kernel(const MbArgs m, int l) {
    const int bx0 = blockIdx.x * 64, by0 = blockIdx.y * 4;
    const uint64_t cand = mb_window_mask<RING>(m, l, bx0, bx0 + 64, by0, by0 + 4);
    const int x = bx0 + (threadIdx.x & 63), y = by0 + (threadIdx.x >> 6);
    if (x >= (m.PW >> l) || y >= (m.PH >> l)) return;
    int R[3];
    mb_collapse_pixel<RING>(m, l, cand, x, y, R);
    mb_store(m, l, x, y, R);
}

// ---- the plan: windows and workspace layout (include/rwh.h, "Working in windows") ----
struct MbPlan {
    int K, PW, PH;
    MbWin win[RWH_SEQ_MAX_IMAGES * MB_LEVELS];   // [n][K + 1]
    int maxw[MB_LEVELS], maxh[MB_LEVELS];
    int64_t desc_at, win_at, pw_at, r_at[MB_LEVELS], g_at, bytes;   // byte offsets into the workspace, 128-byte aligned
};

// One axis of one image's windows.  [a, b) are the rectangle's canvas coordinates, P the padded side; lo[l], hi[l] (inclusive)
// come out clipped to the level's plane.
//   D_l, where W^l can be non-zero: D_0 = [a, b); 2x + k meets D_l for a k in -2 .. 2  <=>  x in [floor((a_l - 1) / 2), floor((b_l + 1) / 2)].
//   E_l, where G^l is read by the bands: D_l, and for l >= 1 the expand taps of D_{l-1}: [floor(a_{l-1} / 2) - 1, floor((b_{l-1} - 1) / 2) + 1].
//   N_l, where G^l has to be the rule's value: N_K = E_K, N_l = E_l united with the reduce taps of N_{l+1}: [2 lo - 2, 2 hi + 2].
// Every set is an interval (hulls are taken), N_l holds all taps of N_{l+1}, and level 0 is exact everywhere, so every value stored
// in a window is the rule's; what lies outside a window is never needed, or lies beyond the plane and is 0.  N_0 reaches less than
// 6 * 2^K + 2 pixels beyond the rectangle.
// ring (the ring rule's x axis): no clip -- an interval shorter than the level's period P >> l stays as it is, on the unwrapped
// axis, and one that would reach the period is the whole ring, [0, P >> l).
static void mb_axis(int a, int b, int P, int K, int* lo, int* hi, bool ring = false) {
    int dl[MB_LEVELS], dh[MB_LEVELS];            // D_l, inclusive
    dl[0] = a; dh[0] = b - 1;
    for (int l = 0; l < K; ++l) { dl[l + 1] = (dl[l] - 1) >> 1; dh[l + 1] = (dh[l] + 2) >> 1; }
    for (int l = K; l >= 0; --l) {
        int nl = dl[l], nh = dh[l];
        if (l > 0) {
            const int el = (dl[l - 1] >> 1) - 1, eh = (dh[l - 1] >> 1) + 1;
            nl = nl < el ? nl : el; nh = nh > eh ? nh : eh;
        }
        if (l < K) {
            const int rl = 2 * lo[l + 1] - 2, rh = 2 * hi[l + 1] + 2;     // (of the unclipped N_{l+1}: kept in lo / hi until clipped below)
            nl = nl < rl ? nl : rl; nh = nh > rh ? nh : rh;
        }
        lo[l] = nl; hi[l] = nh;
    }
    for (int l = 0; l <= K; ++l) {
        if (ring) {
            if (hi[l] - lo[l] + 1 >= (P >> l)) { lo[l] = 0; hi[l] = (P >> l) - 1; }
            continue;
        }
        if (lo[l] < 0) lo[l] = 0;
        if (hi[l] > (P >> l) - 1) hi[l] = (P >> l) - 1;
    }
}

static int64_t mb_align(int64_t v) { return (v + 127) & ~(int64_t)127; }

// What the size function and both entry points check of the geometry, and the plan.
// SEQ_RING: the ring rule -- canvas_w is the period (PW = canvas_w), a rectangle may pass the canvas's edge.
static int mb_plan(const SeqCall& c, int bands, MbPlan& p) {
    const int32_t* rects = c.rects;
    const int n = c.n, canvas_h = c.canvas_h, canvas_w = c.canvas_w, origin_x = c.origin_x, origin_y = c.origin_y;
    const bool ring = c.form == SEQ_RING;
    if (!rects || n < 1 || n > RWH_SEQ_MAX_IMAGES || bands < 1 || bands > RWH_SEQ_MAX_BANDS) return RWH_E_INVALID;
    if (!seq_canvas_ok(canvas_h, canvas_w) || (ring && !seq_period_ok(canvas_w))) return RWH_E_INVALID;
    const int K = bands, mask = (1 << K) - 1;
    p.K = K; p.PW = (canvas_w + mask) & ~mask; p.PH = (canvas_h + mask) & ~mask;
    for (int l = 0; l <= K; ++l) p.maxw[l] = p.maxh[l] = 0;
    int64_t px = 0;
    for (int i = 0; i < n; ++i) {
        const int wt = rects[4 * i + 2], ht = rects[4 * i + 3];
        const int64_t rx = (int64_t)rects[4 * i] - origin_x, ry = (int64_t)rects[4 * i + 1] - origin_y;
        if (wt <= 0 || ht <= 0 || rx < 0 || ry < 0 || ry + ht > canvas_h) return RWH_E_INVALID;
        if (ring ? (rx >= canvas_w || wt > canvas_w) : (rx + wt > canvas_w)) return RWH_E_INVALID;
        int xl[MB_LEVELS], xh[MB_LEVELS], yl[MB_LEVELS], yh[MB_LEVELS];
        mb_axis((int)rx, (int)rx + wt, p.PW, K, xl, xh, ring);
        mb_axis((int)ry, (int)ry + ht, p.PH, K, yl, yh);
        for (int l = 0; l <= K; ++l) {
            MbWin& w = p.win[i * (K + 1) + l];
            w.x0 = xl[l]; w.y0 = yl[l]; w.w = xh[l] - xl[l] + 1; w.h = yh[l] - yl[l] + 1; w.off = px;
            if (w.w < 1 || w.h < 1) return RWH_E_INVALID;          // (cannot happen: a window holds its rectangle's corner)
            px += (int64_t)w.w * w.h;
            if (w.w > p.maxw[l]) p.maxw[l] = w.w;
            if (w.h > p.maxh[l]) p.maxh[l] = w.h;
        }
    }
    int64_t at = 0;
    p.desc_at = at; at = mb_align(at + (int64_t)n * (int64_t)sizeof(SeqDesc));
    p.win_at = at;  at = mb_align(at + (int64_t)n * (K + 1) * (int64_t)sizeof(MbWin));
    p.pw_at = at;   at = mb_align(at + (int64_t)p.PH * p.PW * 4);
    p.r_at[0] = 0;
    for (int l = 1; l <= K; ++l) { p.r_at[l] = at; at = mb_align(at + (int64_t)(p.PH >> l) * (p.PW >> l) * 8); }
    p.g_at = at;    at = mb_align(at + px * 8);
    p.bytes = at;
    return RWH_OK;
}

// Everything both entry points check, the descriptors and the plan.  labelled: the call is one of the seam rule's, which has a
// label plane and no ring form; the calls on maps may have a plane.
static int mb_prepare(const SeqCall& c, int bands, SeqGain& gain, const unsigned char* labels, bool labelled, void* canvas, SeqDesc* descs,
                      MbArgs& m, MbPlan& p, bool device) {
    if (labelled && !labels) return RWH_E_INVALID;
    if (labels && c.form == SEQ_RING) return RWH_E_INVALID;        // labels on the ring: no such form (include/rwh.h)
    int st = seq_prepare_indexed(c, canvas, descs, m.a, device);
    if (st != RWH_OK) return st;
    if (!seq_gain_ok(gain, c, !device)) return RWH_E_INVALID;
    st = mb_plan(c, bands, p);
    if (st != RWH_OK) return st;
    m.K = p.K; m.PW = p.PW; m.PH = p.PH;
    return RWH_OK;
}

// The workspace's areas as pointers (the device's, or the host twin's own buffer).
static void mb_bind(MbArgs& m, const MbPlan& p, char* base) {
    m.a.desc = reinterpret_cast<const SeqDesc*>(base + p.desc_at);
    m.win = reinterpret_cast<const MbWin*>(base + p.win_at);
    m.pw = reinterpret_cast<uint32_t*>(base + p.pw_at);
    m.g = reinterpret_cast<MbPx*>(base + p.g_at);
    m.r[0] = nullptr;
    for (int l = 1; l < MB_LEVELS; ++l) m.r[l] = l <= p.K ? reinterpret_cast<MbPx*>(base + p.r_at[l]) : nullptr;
}

// The winner pass (labelled where the call has a label plane; never on the ring: mb_prepare) and level 0.  gains: the gain switch's
// value as seq_gain_dispatch hands it out.
template <bool GAIN, bool PROJ, bool RING, class G>
static void mb_launch_head(const MbArgs& m, const MbPlan& p, G gains, SeqRays rays, hipStream_t s, const unsigned char* labels) {
    auto l = seq_with<GAIN, PROJ>(m, gains, m.a.n, rays);
    const dim3 grid((p.PW + 63) / 64, (p.PH + 3) / 4);
    if constexpr (!RING) {
        if (labels) {
            auto ll = seq_with<GAIN, PROJ>(MbLabelArgs{m, labels}, gains, m.a.n, rays);
            hipLaunchKernelGGL((mb_label_winner_kernel<GAIN, PROJ, decltype(ll)>), grid, dim3(256), 0, s, ll);
        }
    }
    if (RING || !labels) hipLaunchKernelGGL((mb_winner_kernel<GAIN, PROJ, RING, decltype(l)>), grid, dim3(256), 0, s, l);
    hipLaunchKernelGGL((mb_level0_kernel<GAIN, PROJ, RING, decltype(l)>), dim3((p.maxw[0] + 63) / 64, (p.maxh[0] + 3) / 4, m.a.n), dim3(256), 0, s, l);
}

template <bool GAIN, bool PROJ, bool RING, class G>
static void mb_host_run(const MbArgs& m, const MbPlan& p, G gains, SeqRays rays, const unsigned char* labels) {
    const int n = m.a.n, K = p.K;
    const uint64_t all = seq_all(n);
    for (int y = 0; y < p.PH; ++y)
        for (int x = 0; x < p.PW; ++x) {
            uint32_t out = MB_NONE << 24;
            if (x < m.a.fw && y < m.a.fh) {
                if constexpr (!RING) {
                    if (labels) out = seq_label_winner_pixel<GAIN, PROJ>(m.a, all, x, y, labels[(int64_t)y * m.a.fw + x], gains, rays);
                }
                if (RING || !labels) out = mb_winner_pixel<GAIN, PROJ, RING>(m.a, all, x, y, gains, rays);
            }
            m.pw[(int64_t)y * p.PW + x] = out;
        }
    for (int i = 0; i < n; ++i) {
        const MbWin& w = m.win[i * (K + 1)];
        for (int ly = 0; ly < w.h; ++ly)
            for (int lx = 0; lx < w.w; ++lx) {
                const int x = RING ? mb_mod(w.x0 + lx, p.PW) : w.x0 + lx;
                m.g[w.off + (int64_t)ly * w.w + lx] = mb_level0_pixel<GAIN, PROJ, RING>(m.a, i, m.pw[(int64_t)(w.y0 + ly) * p.PW + x], x, w.y0 + ly, gains, rays);
            }
        for (int l = 0; l < K; ++l) {
            const MbWin& src = m.win[i * (K + 1) + l];
            const MbWin& dst = m.win[i * (K + 1) + l + 1];
            for (int ly = 0; ly < dst.h; ++ly)
                for (int lx = 0; lx < dst.w; ++lx)
                    m.g[dst.off + (int64_t)ly * dst.w + lx] = mb_down(MbWinTap<RING>{m.g, src, dst.x0 + lx, dst.y0 + ly, p.PW >> l});
        }
    }
    for (int l = K; l >= 0; --l)
        for (int y = 0; y < (p.PH >> l); ++y)
            for (int x = 0; x < (p.PW >> l); ++x) {
                int R[3];
                mb_collapse_pixel<RING>(m, l, all, x, y, R);
                mb_store(m, l, x, y, R);
            }
}

// The device call behind every rwh_stitch_multiband* entry point.  The head passes are instantiated on the form and the gain switch;
// the reduce and collapse passes work on canvas planes and know only the ring.
static int mb_device(const SeqCall& c, int bands, SeqGain gain, const unsigned char* d_labels, bool labelled, void* d_canvas,
                     void* d_workspace, int64_t workspace_bytes, void* stream) {
    SeqDesc descs[RWH_SEQ_MAX_IMAGES];
    MbArgs m;
    MbPlan p;
    const int n = c.n;
    const int st = mb_prepare(c, bands, gain, d_labels, labelled, d_canvas, descs, m, p, true);
    if (st != RWH_OK) return st;
    if (!d_workspace || workspace_bytes < p.bytes || ((uintptr_t)d_workspace & 7u)) return RWH_E_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(d_workspace);
    seq_put(descs, (size_t)n * SEQ_DESC_WORDS, reinterpret_cast<uint64_t*>(base + p.desc_at), s);
    seq_put(p.win, (size_t)n * (p.K + 1) * (sizeof(MbWin) / 8), reinterpret_cast<uint64_t*>(base + p.win_at), s);
    mb_bind(m, p, base);
    seq_form_dispatch(c.form, [&](auto form) {
        constexpr bool PROJ = decltype(form)::proj, RING = decltype(form)::ring;
        seq_gain_dispatch<!RING>(gain, [&](auto on, auto value) { mb_launch_head<decltype(on)::value, PROJ, RING>(m, p, value, c.rays, s, d_labels); });
        for (int l = 0; l < p.K; ++l)
            hipLaunchKernelGGL(mb_down_kernel<RING>, dim3((p.maxw[l + 1] + MB_TW - 1) / MB_TW, (p.maxh[l + 1] + MB_TH - 1) / MB_TH, n), dim3(256), 0, s, m, l);
        for (int l = p.K; l >= 0; --l)
            hipLaunchKernelGGL(mb_collapse_kernel<RING>, dim3(((p.PW >> l) + 63) / 64, ((p.PH >> l) + 3) / 4), dim3(256), 0, s, m, l);
    });
    return check_launch();
}

static int mb_host(const SeqCall& c, int bands, SeqGain gain, const unsigned char* labels, bool labelled, void* canvas) {
    SeqDesc descs[RWH_SEQ_MAX_IMAGES];
    MbArgs m;
    MbPlan p;
    const int st = mb_prepare(c, bands, gain, labels, labelled, canvas, descs, m, p, false);
    if (st != RWH_OK) return st;
    char* base = static_cast<char*>(malloc((size_t)p.bytes));
    if (!base) return RWH_E_LAUNCH;
    memcpy(base + p.desc_at, descs, (size_t)c.n * sizeof(SeqDesc));
    memcpy(base + p.win_at, p.win, (size_t)c.n * (p.K + 1) * sizeof(MbWin));
    mb_bind(m, p, base);
    seq_form_dispatch(c.form, [&](auto form) {
        constexpr bool PROJ = decltype(form)::proj, RING = decltype(form)::ring;
        seq_gain_dispatch<!RING>(gain, [&](auto on, auto value) { mb_host_run<decltype(on)::value, PROJ, RING>(m, p, value, c.rays, labels); });
    });
    free(base);
    return RWH_OK;
}

}  // namespace rwh

using rwh::seq_curved;
using rwh::seq_gain_maps;
using rwh::seq_gain_n;
using rwh::seq_plane;

extern "C" int64_t rwh_stitch_multiband_workspace_bytes(const int32_t* rects, int n, int canvas_h, int canvas_w, int origin_x, int origin_y,
                                                        int bands) {
    rwh::MbPlan p;
    const int st = rwh::mb_plan(rwh::seq_frame(rects, n, canvas_h, canvas_w, origin_x, origin_y), bands, p);
    return st == RWH_OK ? p.bytes : (int64_t)st;
}

extern "C" int64_t rwh_stitch_multiband_ring_workspace_bytes(const int32_t* rects, int n, int canvas_h, int canvas_w, int bands) {
    rwh::MbPlan p;
    const int st = rwh::mb_plan(rwh::seq_frame(rects, n, canvas_h, canvas_w, 0, 0, true), bands, p);
    return st == RWH_OK ? p.bytes : (int64_t)st;
}

// Every entry point below: the geometry record of its form, then the driver.
extern "C" int rwh_stitch_multiband(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                    int anchor, int bands, const double* gains, void* d_canvas, int canvas_h, int canvas_w,
                                    int origin_x, int origin_y, void* d_workspace, int64_t workspace_bytes, void* stream) {
    return rwh::mb_device(seq_plane(d_images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), bands, seq_gain_n(gains),
                          nullptr, false, d_canvas, d_workspace, workspace_bytes, stream);
}

extern "C" int rwh_stitch_multiband_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                         int bands, const double* gains, const double* d_col, const double* d_row, void* d_canvas,
                                         int canvas_h, int canvas_w, void* d_workspace, int64_t workspace_bytes, void* stream) {
    return rwh::mb_device(seq_curved(d_images, hw, m, rects, n, d_col, d_row, canvas_h, canvas_w), bands, seq_gain_n(gains), nullptr, false,
                          d_canvas, d_workspace, workspace_bytes, stream);
}

extern "C" int rwh_stitch_multiband_ring(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                         int bands, const double* gains, const double* d_col, const double* d_row, void* d_canvas,
                                         int canvas_h, int canvas_w, void* d_workspace, int64_t workspace_bytes, void* stream) {
    return rwh::mb_device(seq_curved(d_images, hw, m, rects, n, d_col, d_row, canvas_h, canvas_w, true), bands, seq_gain_n(gains), nullptr,
                          false, d_canvas, d_workspace, workspace_bytes, stream);
}

extern "C" int rwh_host_stitch_multiband(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                         int anchor, int bands, const double* gains, void* canvas, int canvas_h, int canvas_w,
                                         int origin_x, int origin_y) {
    return rwh::mb_host(seq_plane(images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), bands, seq_gain_n(gains),
                        nullptr, false, canvas);
}

extern "C" int rwh_host_stitch_multiband_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                              int bands, const double* gains, const double* col, const double* row, void* canvas,
                                              int canvas_h, int canvas_w) {
    return rwh::mb_host(seq_curved(images, hw, m, rects, n, col, row, canvas_h, canvas_w), bands, seq_gain_n(gains), nullptr, false, canvas);
}

extern "C" int rwh_host_stitch_multiband_ring(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                              int bands, const double* gains, const double* col, const double* row, void* canvas,
                                              int canvas_h, int canvas_w) {
    return rwh::mb_host(seq_curved(images, hw, m, rects, n, col, row, canvas_h, canvas_w, true), bands, seq_gain_n(gains), nullptr, false,
                        canvas);
}

// The multi-band rule with the seam rule's Winner (include/rwh.h, "Using labels"): the calls above with a label plane.
extern "C" int rwh_stitch_multiband_labels(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                           int anchor, int bands, const double* gains, const unsigned char* d_labels, void* d_canvas,
                                           int canvas_h, int canvas_w, int origin_x, int origin_y, void* d_workspace,
                                           int64_t workspace_bytes, void* stream) {
    return rwh::mb_device(seq_plane(d_images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), bands, seq_gain_n(gains),
                          d_labels, true, d_canvas, d_workspace, workspace_bytes, stream);
}

extern "C" int rwh_stitch_multiband_labels_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                                int bands, const double* gains, const unsigned char* d_labels, const double* d_col,
                                                const double* d_row, void* d_canvas, int canvas_h, int canvas_w, void* d_workspace,
                                                int64_t workspace_bytes, void* stream) {
    return rwh::mb_device(seq_curved(d_images, hw, m, rects, n, d_col, d_row, canvas_h, canvas_w), bands, seq_gain_n(gains), d_labels, true,
                          d_canvas, d_workspace, workspace_bytes, stream);
}

extern "C" int rwh_host_stitch_multiband_labels(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                                int anchor, int bands, const double* gains, const unsigned char* labels, void* canvas,
                                                int canvas_h, int canvas_w, int origin_x, int origin_y) {
    return rwh::mb_host(seq_plane(images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), bands, seq_gain_n(gains),
                        labels, true, canvas);
}

extern "C" int rwh_host_stitch_multiband_labels_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                                     int bands, const double* gains, const unsigned char* labels, const double* col,
                                                     const double* row, void* canvas, int canvas_h, int canvas_w) {
    return rwh::mb_host(seq_curved(images, hw, m, rects, n, col, row, canvas_h, canvas_w), bands, seq_gain_n(gains), labels, true, canvas);
}

// The multi-band rule on the gain maps of the block gain rule: d_maps / maps and shift where the calls above take gains; labels may
// be NULL (the multi-band rule's Winner) or a label plane (the seam rule's).  The host twins read the maps: every entry finite and > 0.
extern "C" int rwh_stitch_multiband_maps(const void* const* d_images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                         int anchor, int bands, const double* d_maps, int shift, const unsigned char* d_labels,
                                         void* d_canvas, int canvas_h, int canvas_w, int origin_x, int origin_y, void* d_workspace,
                                         int64_t workspace_bytes, void* stream) {
    return rwh::mb_device(seq_plane(d_images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), bands,
                          seq_gain_maps(d_maps, shift), d_labels, false, d_canvas, d_workspace, workspace_bytes, stream);
}

extern "C" int rwh_stitch_multiband_maps_proj(const void* const* d_images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                              int bands, const double* d_maps, int shift, const unsigned char* d_labels,
                                              const double* d_col, const double* d_row, void* d_canvas, int canvas_h, int canvas_w,
                                              void* d_workspace, int64_t workspace_bytes, void* stream) {
    return rwh::mb_device(seq_curved(d_images, hw, m, rects, n, d_col, d_row, canvas_h, canvas_w), bands, seq_gain_maps(d_maps, shift),
                          d_labels, false, d_canvas, d_workspace, workspace_bytes, stream);
}

extern "C" int rwh_host_stitch_multiband_maps(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n,
                                              int anchor, int bands, const double* maps_in, int shift, const unsigned char* labels,
                                              void* canvas, int canvas_h, int canvas_w, int origin_x, int origin_y) {
    return rwh::mb_host(seq_plane(images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y), bands,
                        seq_gain_maps(maps_in, shift), labels, false, canvas);
}

extern "C" int rwh_host_stitch_multiband_maps_proj(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n,
                                                   int bands, const double* maps_in, int shift, const unsigned char* labels,
                                                   const double* col, const double* row, void* canvas, int canvas_h, int canvas_w) {
    return rwh::mb_host(seq_curved(images, hw, m, rects, n, col, row, canvas_h, canvas_w), bands, seq_gain_maps(maps_in, shift), labels,
                        false, canvas);
}
