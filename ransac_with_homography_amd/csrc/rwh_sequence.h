// The sequence rule's shared pieces (include/rwh.h, "The sequence rule"): the image descriptor, the sampling recipe, the pixel
// function and the argument checks.  rwh_sequence.hip (paste, feather, overlap statistics), rwh_multiband.hip (the multi-band
// rule), rwh_seams.hip (the seam rule) and rwh_blockgains.hip (the block gain rule) include this, so every compositor samples an
// image with one arithmetic, on the device and in the host twins.  The host side of a call is three records: its geometry
// (SeqCall), its gain switch (SeqGain) and the launch record made of them (SeqWith / SeqWithMaps).
#ifndef RWH_SEQUENCE_H
#define RWH_SEQUENCE_H
#include <math.h>
#include <string.h>
#include <type_traits>
#include "rwh_common.h"

namespace rwh {

// One image of the sequence, 13 eight-byte words: the kernels read it from a device table with wave-uniform indices.
struct SeqDesc {
    const unsigned char* src;   // h x w x 3 uint8
    double ih[9];               // inv(G): frame point -> source coordinates
    int h, w;
    int mx, my, wt, ht;         // its rectangle in the anchor's frame
};
constexpr int SEQ_DESC_WORDS = 13;
static_assert(sizeof(SeqDesc) == 8 * SEQ_DESC_WORDS, "SeqDesc is copied as 8-byte words");

struct SeqArgs {
    const SeqDesc* desc;        // n descriptors (device table; host array in the host twin)
    unsigned char* dst;         // canvas fh x fw x 3 uint8
    int n, anchor;
    int ox, oy;                 // canvas pixel (cx, cy) is frame point (ox + cx, oy + cy)
    int fh, fw;
    int row_begin, row_end;     // canvas rows this call produces
    unsigned char order[RWH_SEQ_MAX_IMAGES];   // paste: priority order; feather: 0 .. n-1
};

// The ray tables of the projection rule (include/rwh.h): col[cx] = (sin, cos) of the canvas column's angle, fw pairs; row[cy] = the
// canvas row's pair, fh pairs; float64, 16-byte aligned on the device.  Both null in the planar forms.
struct SeqRays { const double* col; const double* row; };

// The arguments of one launch: A, with GAIN the N gains of the gain rule behind it (512 B: the arguments stay under 4 KB), and with
// PROJ the ray tables of the projection rule last.  The forms without PROJ are laid out as they were before there was one.
template <class A, bool GAIN, bool PROJ = false> struct SeqWith { A a; };
template <class A> struct SeqWith<A, true, false> { A a; double gains[RWH_SEQ_MAX_IMAGES]; };
template <class A> struct SeqWith<A, false, true> { A a; SeqRays rays; };
template <class A> struct SeqWith<A, true, true> { A a; double gains[RWH_SEQ_MAX_IMAGES]; SeqRays rays; };
template <class A, bool GAIN, bool PROJ> __host__ __device__ __forceinline__ const double* seq_gains(const SeqWith<A, GAIN, PROJ>& l) {
    if constexpr (GAIN) return l.gains; else return nullptr;
}
template <class A, bool GAIN, bool PROJ> __host__ __device__ __forceinline__ SeqRays seq_rays(const SeqWith<A, GAIN, PROJ>& l) {
    if constexpr (PROJ) return l.rays; else return SeqRays{nullptr, nullptr};
}
template <bool GAIN, bool PROJ = false, class A>
static SeqWith<A, GAIN, PROJ> seq_with(const A& a, const double* gains, int n, SeqRays rays = SeqRays{nullptr, nullptr}) {
    SeqWith<A, GAIN, PROJ> l;
    l.a = a;
    if constexpr (GAIN) {
        memset(l.gains, 0, sizeof(l.gains));
        memcpy(l.gains, gains, (size_t)n * sizeof(double));
    }
    if constexpr (PROJ) l.rays = rays;
    return l;
}

// The third state of the gain switch (include/rwh.h, the block gain rule): gain MAPS instead of N gains.  m: float64 [n][gh][gw] (a
// device pointer in a launch, host memory in the host twins), cells of 2^shift canvas pixels.  The pointer and three ints travel
// where gains[64] travels, in a record of their own, so the arguments of the other two states lie where they lay.  A head kernel
// takes its record as a template parameter L and reads it through seq_gains(l) and seq_rays(l): one body per role, instantiated
// on SeqWith or SeqWithMaps.
struct SeqMaps { const double* m; int gw, gh, shift; };
template <class A, bool PROJ = false> struct SeqWithMaps { A a; SeqMaps maps; };
template <class A> struct SeqWithMaps<A, true> { A a; SeqMaps maps; SeqRays rays; };
template <class A, bool PROJ> __host__ __device__ __forceinline__ SeqMaps seq_gains(const SeqWithMaps<A, PROJ>& l) { return l.maps; }
template <class A, bool PROJ> __host__ __device__ __forceinline__ SeqRays seq_rays(const SeqWithMaps<A, PROJ>& l) {
    if constexpr (PROJ) return l.rays; else return SeqRays{nullptr, nullptr};
}
template <bool GAIN, bool PROJ = false, class A>
static SeqWithMaps<A, PROJ> seq_with(const A& a, const SeqMaps& maps, int, SeqRays rays = SeqRays{nullptr, nullptr}) {
    static_assert(GAIN, "maps are gains");
    SeqWithMaps<A, PROJ> l;
    l.a = a;
    l.maps = maps;
    if constexpr (PROJ) l.rays = rays;
    return l;
}

// The cells of the block gain rule: B = 2^shift of 16 .. 128, ceil(side / B) cells along a side.
constexpr int SEQ_SHIFT_MIN = 4, SEQ_SHIFT_MAX = 7;
static int seq_cell_count(int side, int shift) { return (side + (1 << shift) - 1) >> shift; }
// The maps of a call as the pixel functions take them; false: no maps, a misaligned pointer or another block.
static bool seq_maps_of(const double* maps, int shift, int canvas_h, int canvas_w, SeqMaps& m) {
    if (!maps || ((uintptr_t)maps & 7u) || shift < SEQ_SHIFT_MIN || shift > SEQ_SHIFT_MAX) return false;
    m.m = maps; m.shift = shift;
    m.gw = seq_cell_count(canvas_w, shift); m.gh = seq_cell_count(canvas_h, shift);
    return true;
}
// Host maps are read before they are used (the host twins): every entry finite and > 0, as the gain rule asks of a gain.
static bool seq_maps_ok(const SeqMaps& m, int n) {
    for (size_t t = 0, end = (size_t)n * m.gw * m.gh; t < end; ++t)
        if (!(isfinite(m.m[t]) && m.m[t] > 0.0)) return false;
    return true;
}

// Where a pixel function gets the gain of image i at canvas pixel (cx, cy): seq_gain_site(gains, cx, cy) once per pixel, then
// seq_gain_of(site, i) per image.  N gains: the site is the array and the gain gains[i].  Maps ("Applying maps" of the block gain
// rule): the site is the pixel's four cells and two fractions -- u = ((double)cx + 0.5) / B - 0.5 is exact, B a power of two -- and
// the gain the two-step lerp of image i's plane, every product and sum rounded on its own.
struct SeqMapSite { const double* m; size_t plane; int o00, o01, o10, o11; double t, q; };
__host__ __device__ __forceinline__ void seq_map_axis(int c, int cells, double inv_b, int& c0, int& c1, double& t) {
    const double u = ((double)c + 0.5) * inv_b - 0.5;
    if (u <= 0.0) { c0 = c1 = 0; t = 0.0; }
    else if (u >= (double)(cells - 1)) { c0 = c1 = cells - 1; t = 0.0; }
    else { c0 = (int)u; c1 = c0 + 1; t = u - (double)c0; }
}
__host__ __device__ __forceinline__ const double* seq_gain_site(const double* gains, int, int) { return gains; }
__host__ __device__ __forceinline__ double seq_gain_of(const double* gains, int i) { return gains[i]; }
__host__ __device__ __forceinline__ SeqMapSite seq_gain_site(const SeqMaps& g, int cx, int cy) {
    const double inv_b = 1.0 / (double)(1 << g.shift);
    int x0, x1, y0, y1;
    SeqMapSite s;
    seq_map_axis(cx, g.gw, inv_b, x0, x1, s.t);
    seq_map_axis(cy, g.gh, inv_b, y0, y1, s.q);
    s.m = g.m; s.plane = (size_t)g.gw * g.gh;
    s.o00 = y0 * g.gw + x0; s.o01 = y0 * g.gw + x1; s.o10 = y1 * g.gw + x0; s.o11 = y1 * g.gw + x1;
    return s;
}
__host__ __device__ __forceinline__ double seq_gain_of(const SeqMapSite& s, int i) {
    const double* p = s.m + (size_t)i * s.plane;
    const double top = p[s.o00] * (1.0 - s.t) + p[s.o01] * s.t;
    const double bot = p[s.o10] * (1.0 - s.t) + p[s.o11] * s.t;
    return top * (1.0 - s.q) + bot * s.q;
}

// The ray of canvas pixel (cx, cy) on the curved canvas: three products of table entries, no transcendental function.  Both
// indices lie inside the canvas (the callers' bounds tests come first).  The column pair is one 16-byte load per lane; cy is
// wave-uniform in every kernel, so the row pair is a scalar load.
struct SeqRay { double r0, r1, r2; };
__host__ __device__ __forceinline__ SeqRay seq_ray(const SeqRays& t, int cx, int cy) {
#ifdef __HIP_DEVICE_COMPILE__
    struct __attribute__((aligned(16))) Pair { double s, c; };     // (checked before the launch)
#else
    struct Pair { double s, c; };
#endif
    const Pair col = reinterpret_cast<const Pair*>(t.col)[cx], row = reinterpret_cast<const Pair*>(t.row)[cy];
    return SeqRay{col.s * row.c, row.s, col.c * row.c};
}

// A wave's row (threadIdx.x >> 6 in every kernel of the family), which the compiler cannot see to be wave-uniform: told so in the
// projected forms, whose row entry of the ray tables then comes by a scalar load.  The planar forms keep the expression, and the
// code, they had.
template <bool PROJ> __device__ __forceinline__ int seq_wave_row(int row) {
    if constexpr (PROJ) return __builtin_amdgcn_readfirstlane(row); else return row;
}

// One RGB texel as a dword: an unaligned 4-byte load (3 bytes used) unless that would step past the image's last byte.
__host__ __device__ __forceinline__ uint32_t seq_rgb_at(const unsigned char* base, size_t off, size_t img_bytes) {
    if (off + 4 <= img_bytes) { uint32_t v; __builtin_memcpy(&v, base + off, 4); return v; }
    return (uint32_t)base[off] | ((uint32_t)base[off + 1] << 8) | ((uint32_t)base[off + 2] << 16);
}
__host__ __device__ __forceinline__ double seq_chan(uint32_t texel, int k) { return (double)((texel >> (8 * k)) & 0xffu); }
__host__ __device__ __forceinline__ double seq_min(double a, double b) { return a < b ? a : b; }

// Image d at frame point (fx, fy): false where it does not cover the point; else its value v (float64 per channel) and, for the
// feather blend, its weight g.  The anchor enters unwarped: its own bytes, texel (0,0) included.  GAIN (the gain rule): v is
// min(v * gain, 255.0), the product rounded on its own; without GAIN `gain` is not read.
// PROJ (the projection rule): (fx, fy) is the canvas pixel, `ray` its ray and d.ih the image's M; X, Y and W are M's rows on the
// ray, a ray behind the camera (W <= 0) is not valid, and no image enters unwarped (is_anchor is not read).
// RING (the ring rule, with PROJ): the canvas is periodic in x with `period` columns and the rectangle may pass its edge; the
// containment is one conditional add, and nothing else of the recipe changes.
template <bool FEATHER, bool GAIN = false, bool PROJ = false, bool RING = false>
__host__ __device__ __forceinline__ bool seq_sample(const SeqDesc& d, bool is_anchor, int fx, int fy, double v[3], double& g,
                                                    double gain = 1.0, const SeqRay* ray = nullptr, int period = 0) {
    static_assert(PROJ || !RING, "the ring rule is stated on the projection rule");
    int tx = fx - d.mx;
    const int ty = fy - d.my;
    if constexpr (RING) tx += tx < 0 ? period : 0;      // (0 <= fx, mx < period: tx lands in [0, period))
    if (!((tx >= 0) & (tx < d.wt) & (ty >= 0) & (ty < d.ht))) return false;
    const size_t bytes = (size_t)d.h * d.w * 3;
    double sx, sy;
    if (!PROJ && is_anchor) {   // (its rectangle is (0, 0, w, h): checked before the launch)
        const uint32_t p = seq_rgb_at(d.src, ((size_t)ty * d.w + tx) * 3, bytes);
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = seq_chan(p, k);
        sx = (double)tx; sy = (double)ty;
    } else {
        double X, Y, W;
        if constexpr (PROJ) {
            X = fma(d.ih[2], ray->r2, fma(d.ih[1], ray->r1, d.ih[0] * ray->r0));
            Y = fma(d.ih[5], ray->r2, fma(d.ih[4], ray->r1, d.ih[3] * ray->r0));
            W = fma(d.ih[8], ray->r2, fma(d.ih[7], ray->r1, d.ih[6] * ray->r0));
        } else {
            const double x = (double)fx, y = (double)fy;
            X = fma(d.ih[1], y, d.ih[0] * x) + d.ih[2];
            Y = fma(d.ih[4], y, d.ih[3] * x) + d.ih[5];
            W = fma(d.ih[7], y, d.ih[6] * x) + d.ih[8];
        }
        sx = X / W; sy = Y / W;
        bool valid = (sx >= 0.0) & (sx <= (double)(d.w - 1)) & (sy >= 0.0) & (sy <= (double)(d.h - 1));   // a NaN is not valid
        if constexpr (PROJ) valid &= W > 0.0;
        if (!valid) return false;
        const int ix = (int)sx, iy = (int)sy;
        const double fx_ = sx - (double)ix, fy_ = sy - (double)iy;
        const double gx = 1.0 - fx_, gy = 1.0 - fy_;
        const int ix1 = ix + 1 < d.w ? ix + 1 : d.w - 1, iy1 = iy + 1 < d.h ? iy + 1 : d.h - 1;
        // texel (0,0) reads as 0: the caller's image is never written
        const uint32_t p00 = (ix | iy) ? seq_rgb_at(d.src, ((size_t)iy * d.w + ix) * 3, bytes) : 0u;
        const uint32_t p01 = (ix1 | iy) ? seq_rgb_at(d.src, ((size_t)iy * d.w + ix1) * 3, bytes) : 0u;
        const uint32_t p10 = (ix | iy1) ? seq_rgb_at(d.src, ((size_t)iy1 * d.w + ix) * 3, bytes) : 0u;
        const uint32_t p11 = seq_rgb_at(d.src, ((size_t)iy1 * d.w + ix1) * 3, bytes);      // (h, w >= 2: never texel (0,0))
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double top = seq_chan(p00, k) * gx + seq_chan(p01, k) * fx_;
            const double bot = seq_chan(p10, k) * gx + seq_chan(p11, k) * fx_;
            v[k] = top * gy + bot * fy_;
        }
    }
    if constexpr (GAIN) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = seq_min(v[k] * gain, 255.0);
    }
    if constexpr (FEATHER) g = seq_min(seq_min(sx, (double)(d.w - 1) - sx), seq_min(sy, (double)(d.h - 1) - sy)) + 1.0;
    return true;
}

// One canvas pixel as 0x00BBGGRR.  cand: bit k set = image order[k] may cover the pixel (its rectangle meets the pixel's tile).
// gains: the N gains of the gain rule or the maps of the block gain rule (SeqMaps), read with GAIN only.  rays: the ray tables, read with PROJ only (then ox = oy = 0).
// RING: a.fw is the period.
template <bool FEATHER, bool GAIN = false, bool PROJ = false, bool RING = false, class G = const double*>
__host__ __device__ __forceinline__ uint32_t seq_pixel(const SeqArgs& a, uint64_t cand, int cx, int cy, G gains = nullptr,
                                                       SeqRays rays = SeqRays{nullptr, nullptr}) {
    const int fx = a.ox + cx, fy = a.oy + cy;
    SeqRay ray;
    if constexpr (PROJ) ray = seq_ray(rays, cx, cy);
    [[maybe_unused]] const auto site = seq_gain_site(gains, cx, cy);
    double num[3] = {0.0, 0.0, 0.0}, den = 0.0;
    bool covered = false;
    for (uint64_t m = cand; m; m &= m - 1) {
        const int i = a.order[__builtin_ctzll(m)];
        double v[3], g = 0.0;
        double gain = 1.0;
        if constexpr (GAIN) gain = seq_gain_of(site, i);
        if (!seq_sample<FEATHER, GAIN, PROJ, RING>(a.desc[i], i == a.anchor, fx, fy, v, g, gain, &ray, a.fw)) continue;
        if constexpr (!FEATHER) {       // paste: the first image in `order` that covers the pixel
            uint32_t out = 0u;
#pragma unroll
            for (int k = 0; k < 3; ++k) out |= (uint32_t)(unsigned char)(int)v[k] << (8 * k);
            return out;
        } else {
            covered = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) num[k] += g * v[k];
            den += g;
        }
    }
    uint32_t out = 0u;
    if (FEATHER && covered) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out |= (uint32_t)(unsigned char)(int)(num[k] / den) << (8 * k);
    }
    return out;
}

// The Winner of the multi-band rule under a label plane (include/rwh.h, the seam rule, "Using labels"): image `label` where it is
// one of the candidates and covers the pixel, otherwise the covering image with the greatest feather weight g, the lowest index on
// equal weights.  -> the winner's bytes as 0x00BBGGRR with its index in the top byte, SEQ_LABEL_NONE there where nobody covers.
// cand: candidate bits are image indices (order is 0 .. n-1), so a label of n or more meets no candidate and indexes nothing.
constexpr uint32_t SEQ_LABEL_NONE = 0xffu;
template <bool GAIN, bool PROJ = false, class G = const double*>
__host__ __device__ __forceinline__ uint32_t seq_label_winner_pixel(const SeqArgs& a, uint64_t cand, int cx, int cy, uint32_t label,
                                                                    G gains, SeqRays rays = SeqRays{nullptr, nullptr}) {
    const int fx = a.ox + cx, fy = a.oy + cy;
    SeqRay ray;
    if constexpr (PROJ) ray = seq_ray(rays, cx, cy);
    [[maybe_unused]] const auto site = seq_gain_site(gains, cx, cy);
    double best = 0.0;
    uint32_t out = SEQ_LABEL_NONE << 24;
    for (uint64_t m = cand; m; m &= m - 1) {
        const int i = __builtin_ctzll(m);
        double v[3], g = 0.0, gain = 1.0;
        if constexpr (GAIN) gain = seq_gain_of(site, i);
        if (!seq_sample<true, GAIN, PROJ>(a.desc[i], i == a.anchor, fx, fy, v, g, gain, &ray, a.fw)) continue;
        const bool named = (uint32_t)i == label;
        if (named || g > best) {
            best = g;
            out = (uint32_t)i << 24;
#pragma unroll
            for (int k = 0; k < 3; ++k) out |= (uint32_t)(unsigned char)(int)v[k] << (8 * k);
            if (named) break;
        }
    }
    return out;
}

// The images whose rectangles meet canvas columns [x0, x1) and rows [y0, y1), as bits in `order`'s numbering.
// RING: a rectangle that passes the canvas's edge comes back in at column 0, so the rectangle shifted by -period (a.fw) is tested
// as well; it starts left of every tile, which leaves one compare of wave-uniform values.
template <bool RING = false>
__host__ __device__ __forceinline__ uint64_t seq_tile_mask(const SeqArgs& a, int x0, int x1, int y0, int y1) {
    uint64_t m = 0;
    for (int k = 0; k < a.n; ++k) {
        const SeqDesc& d = a.desc[a.order[k]];
        const int rx = d.mx - a.ox, ry = d.my - a.oy;
        bool cols = (rx < x1) & (rx + d.wt > x0);
        if constexpr (RING) cols |= rx + d.wt - a.fw > x0;
        if (cols & (ry < y1) & (ry + d.ht > y0)) m |= 1ull << k;
    }
    return m;
}

// "All n images" as candidate bits.
static uint64_t seq_all(int n) { return n == 64 ? ~0ull : (1ull << n) - 1; }

// The canvas every rule of the family takes: sides of 1 .. 65535, byte offsets within int32.
static bool seq_canvas_ok(int h, int w) { return h >= 1 && w >= 1 && h <= 65535 && w <= 65535 && (int64_t)h * w * 3 <= INT32_MAX; }

// The period of the ring rule: a whole number of the kernels' 256-column tiles (and so of 2^RWH_SEQ_MAX_BANDS).
constexpr int SEQ_RING_TILE = 256;
static bool seq_period_ok(int w) { return w >= SEQ_RING_TILE && w % SEQ_RING_TILE == 0; }

// Lays `words` eight-byte words of a host table down at `dev` on the stream (rwh_sequence.hip).
void seq_put(const void* host, size_t words, uint64_t* dev, hipStream_t s);

// The projected forms have no anchor: every image is warped, every matrix checked, and the frame is the canvas (origin (0, 0)).
constexpr int SEQ_NO_ANCHOR = -1;

// The ray tables of a projected call: both given, 16-byte aligned where the device loads a pair at once.
static bool seq_rays_ok(const double* col, const double* row, bool device) {
    const uintptr_t mask = device ? 15u : 7u;
    return col && row && !((uintptr_t)col & mask) && !((uintptr_t)row & mask);
}

// The geometry of one call, as the Python layer's SeqGeometry holds it: the images with their matrices and rectangles, the canvas
// and the form.  Every driver of the family takes one, and every entry point makes it with seq_plane or seq_curved.
//   SEQ_PLANE: mats holds the inv(G_i), the anchor enters unwarped, no rays.
//   SEQ_CURVED (the projection rule): mats holds the M_i, anchor is SEQ_NO_ANCHOR and the origin (0, 0).
//   SEQ_RING (the ring rule, on the projection rule): canvas_w is the period, a multiple of SEQ_RING_TILE; a rectangle starts on
//   the canvas, is at most one period wide and may pass the canvas's edge.
enum SeqForm { SEQ_PLANE, SEQ_CURVED, SEQ_RING };
struct SeqCall {
    const void* const* images; const int32_t* hw; const double* mats; const int32_t* rects;
    int n, anchor, canvas_h, canvas_w, origin_x, origin_y;
    SeqRays rays;
    SeqForm form;
};
static SeqCall seq_plane(const void* const* images, const int32_t* hw, const double* inv_g, const int32_t* rects, int n, int anchor,
                         int canvas_h, int canvas_w, int origin_x, int origin_y) {
    return SeqCall{images, hw, inv_g, rects, n, anchor, canvas_h, canvas_w, origin_x, origin_y, SeqRays{nullptr, nullptr}, SEQ_PLANE};
}
static SeqCall seq_curved(const void* const* images, const int32_t* hw, const double* m, const int32_t* rects, int n, const double* col,
                          const double* row, int canvas_h, int canvas_w, bool ring = false) {
    return SeqCall{images, hw, m, rects, n, SEQ_NO_ANCHOR, canvas_h, canvas_w, 0, 0, SeqRays{col, row}, ring ? SEQ_RING : SEQ_CURVED};
}
// The rectangles alone, for the functions that are given no images (the size functions, the cells of the block gain rule).
static SeqCall seq_frame(const int32_t* rects, int n, int canvas_h, int canvas_w, int origin_x, int origin_y, bool ring = false) {
    SeqCall c = seq_plane(nullptr, nullptr, nullptr, rects, n, 0, canvas_h, canvas_w, origin_x, origin_y);
    if (ring) c.form = SEQ_RING;
    return c;
}

// f(form), form a SeqFormOf: where PROJ and RING have to be compile-time.  RINGS false: an operation that has no ring form (its
// prepare refuses SEQ_RING), so none is instantiated.
template <bool PROJ, bool RING> struct SeqFormOf { static constexpr bool proj = PROJ, ring = RING; };
template <bool RINGS = true, class F> static void seq_form_dispatch(SeqForm form, const F& f) {
    if (form == SEQ_PLANE) f(SeqFormOf<false, false>{});
    else if (form == SEQ_CURVED) f(SeqFormOf<true, false>{});
    else if constexpr (RINGS) f(SeqFormOf<true, true>{});
}

// Everything both entry points check, and the descriptors / arguments they share.  descs: room for RWH_SEQ_MAX_IMAGES.
// device: the images, the canvas and the ray tables are the device's (the tables 16-byte aligned).
static int seq_prepare(const SeqCall& c, const int32_t* order, int blend, void* canvas, int row_begin, int row_end, SeqDesc* descs,
                       SeqArgs& a, bool device) {
    const void* const* images = c.images;
    const int32_t *hw = c.hw, *rects = c.rects;
    const int n = c.n, anchor = c.anchor, canvas_h = c.canvas_h, canvas_w = c.canvas_w, origin_x = c.origin_x, origin_y = c.origin_y;
    const bool proj = c.form != SEQ_PLANE, ring = c.form == SEQ_RING;
    if (!images || !hw || !c.mats || !rects || !order || !canvas) return RWH_E_INVALID;
    if (proj ? (anchor != SEQ_NO_ANCHOR || origin_x || origin_y) : (anchor < 0 || anchor >= n)) return RWH_E_INVALID;
    if (proj && !seq_rays_ok(c.rays.col, c.rays.row, device)) return RWH_E_INVALID;
    if (n < 1 || n > RWH_SEQ_MAX_IMAGES || (blend != RWH_SEQ_PASTE && blend != RWH_SEQ_FEATHER)) return RWH_E_INVALID;
    if (!seq_canvas_ok(canvas_h, canvas_w) || (ring && !seq_period_ok(canvas_w))) return RWH_E_INVALID;
    if (row_begin < 0 || row_end > canvas_h || row_begin > row_end) return RWH_E_INVALID;
    uint64_t seen = 0;
    for (int k = 0; k < n; ++k) {
        if (order[k] < 0 || order[k] >= n || (seen >> order[k] & 1)) return RWH_E_INVALID;
        seen |= 1ull << order[k];
    }
    for (int i = 0; i < n; ++i) {
        SeqDesc& d = descs[i];
        d.src = static_cast<const unsigned char*>(images[i]);
        d.h = hw[2 * i]; d.w = hw[2 * i + 1];
        d.mx = rects[4 * i]; d.my = rects[4 * i + 1]; d.wt = rects[4 * i + 2]; d.ht = rects[4 * i + 3];
        if (!d.src || d.h < 2 || d.w < 2 || d.wt <= 0 || d.ht <= 0) return RWH_E_INVALID;
        // the rectangle lies on the canvas (so no frame coordinate leaves int32), the anchor's is its own image
        const int64_t rx = (int64_t)d.mx - origin_x, ry = (int64_t)d.my - origin_y;
        if (rx < 0 || ry < 0 || ry + d.ht > canvas_h) return RWH_E_INVALID;
        if (ring ? (rx >= canvas_w || d.wt > canvas_w) : (rx + d.wt > canvas_w)) return RWH_E_INVALID;
        if (i == anchor && (d.mx != 0 || d.my != 0 || d.wt != d.w || d.ht != d.h)) return RWH_E_INVALID;
        for (int j = 0; j < 9; ++j) {
            d.ih[j] = c.mats[9 * i + j];
            if (i != anchor && !isfinite(d.ih[j])) return RWH_E_INVALID;
        }
    }
    a.desc = descs;
    a.dst = static_cast<unsigned char*>(canvas);
    a.n = n; a.anchor = anchor; a.ox = origin_x; a.oy = origin_y; a.fh = canvas_h; a.fw = canvas_w;
    a.row_begin = row_begin; a.row_end = row_end;
    memset(a.order, 0, sizeof(a.order));
    for (int k = 0; k < n; ++k) a.order[k] = (unsigned char)(blend == RWH_SEQ_FEATHER ? k : order[k]);   // feather: index order
    return RWH_OK;
}

// seq_prepare for the rules that take the images in index order over the whole canvas: the identity order, feather, all rows.
static int seq_prepare_indexed(const SeqCall& c, void* canvas, SeqDesc* descs, SeqArgs& a, bool device) {
    if (c.n < 1 || c.n > RWH_SEQ_MAX_IMAGES) return RWH_E_INVALID;     // (before order[] is filled)
    int32_t order[RWH_SEQ_MAX_IMAGES];
    for (int k = 0; k < c.n; ++k) order[k] = k;
    return seq_prepare(c, order, RWH_SEQ_FEATHER, canvas, 0, c.canvas_h, descs, a, device);
}

// The gains of the gain rule: N values, each finite and > 0.
static bool seq_gains_ok(const double* gains, int n) {
    for (int i = 0; i < n; ++i)
        if (!(isfinite(gains[i]) && gains[i] > 0.0)) return false;
    return true;
}

// The gain switch of one call, host side: no gains, the N gains of the gain rule, or the maps of the block gain rule with their
// shift (gw and gh come from the canvas in seq_gain_ok).
struct SeqGain {
    enum Kind { NONE, GAINS, MAPS } kind;
    const double* gains;
    SeqMaps maps;
};
static SeqGain seq_gain_n(const double* gains) { return SeqGain{gains ? SeqGain::GAINS : SeqGain::NONE, gains, SeqMaps{nullptr, 0, 0, 0}}; }
static SeqGain seq_gain_maps(const double* maps, int shift) { return SeqGain{SeqGain::MAPS, nullptr, SeqMaps{maps, 0, 0, shift}}; }

// What a call checks of its gains, after its geometry (n and the canvas are in range).  host: the maps are host memory and read
// here, as the N gains always are.  Maps on the ring: there is no such form (include/rwh.h), and this is where it is refused.
static bool seq_gain_ok(SeqGain& g, const SeqCall& c, bool host) {
    if (g.kind == SeqGain::GAINS) return seq_gains_ok(g.gains, c.n);
    if (g.kind == SeqGain::NONE) return true;
    if (c.form == SEQ_RING || !seq_maps_of(g.maps.m, g.maps.shift, c.canvas_h, c.canvas_w, g.maps)) return false;
    return !host || seq_maps_ok(g.maps, c.n);
}

// f(gain, value): gain is std::false_type with a null pointer, or std::true_type with the N gains (const double*) or the maps
// (SeqMaps) -- what seq_with and the pixel functions take.  MAPS false: the call's form has no maps (the ring, refused in
// seq_gain_ok), so none is instantiated.
template <bool MAPS = true, class F> static void seq_gain_dispatch(const SeqGain& g, const F& f) {
    if (g.kind == SeqGain::NONE) f(std::false_type{}, (const double*)nullptr);
    else if (g.kind == SeqGain::GAINS) f(std::true_type{}, g.gains);
    else if constexpr (MAPS) f(std::true_type{}, g.maps);
}

// f(feather, gain, value): the forms of the compositor over the blend and the gain switch, device and host.
template <bool MAPS = true, class F> static void seq_dispatch(bool feather, const SeqGain& g, const F& f) {
    seq_gain_dispatch<MAPS>(g, [&](auto gain, auto value) {
        if (feather) f(std::true_type{}, gain, value); else f(std::false_type{}, gain, value);
    });
}

// The compositor's shape -- stitch_kernel's (rwh_stitch.hip): 256 lanes as 64 x 4, four consecutive pixels per lane, the 12 output
// bytes in one store.
constexpr int SEQ_PX = 4;

__device__ __forceinline__ uint32_t seq_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = RWH_WAVE / 2; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

template <bool FEATHER, bool GAIN, bool PROJ = false, bool RING = false, class G = const double*>
static void seq_host_rows(const SeqArgs& a, G gains, SeqRays rays = SeqRays{nullptr, nullptr}) {
    const uint64_t all = seq_all(a.n);
    for (int cy = a.row_begin; cy < a.row_end; ++cy)
        for (int cx = 0; cx < a.fw; ++cx) {
            const uint32_t p = seq_pixel<FEATHER, GAIN, PROJ, RING>(a, all, cx, cy, gains, rays);
            unsigned char* out = a.dst + ((size_t)cy * a.fw + cx) * 3;
            out[0] = (unsigned char)p; out[1] = (unsigned char)(p >> 8); out[2] = (unsigned char)(p >> 16);
        }
}

// ---- the per-sample functions of the gain rule's statistics (include/rwh.h), which the block gain rule's cells share ----
// The images that cover canvas pixel (cx, cy), bit i = image i (cand: bits of image indices), by the sequence rule's Coverage:
// seq_sample's own test, its taps unused.  rays: the ray tables, read with PROJ only.
template <bool PROJ = false, bool RING = false>
__host__ __device__ __forceinline__ uint64_t seq_cover(const SeqArgs& a, uint64_t cand, int cx, int cy, SeqRays rays = SeqRays{nullptr, nullptr}) {
    const int fx = a.ox + cx, fy = a.oy + cy;
    SeqRay ray;
    if constexpr (PROJ) ray = seq_ray(rays, cx, cy);
    uint64_t cov = 0;
    for (uint64_t m = cand; m; m &= m - 1) {
        const int i = __builtin_ctzll(m);
        double v[3], g = 0.0;
        if (seq_sample<false, false, PROJ, RING>(a.desc[i], i == a.anchor, fx, fy, v, g, 1.0, &ray, a.fw)) cov |= 1ull << i;
    }
    return cov;
}

// L_i of the gain rule: the sum of the three bytes paste would write for image i at a canvas pixel that it covers.
template <bool PROJ = false, bool RING = false>
__host__ __device__ __forceinline__ uint32_t seq_byte_sum(const SeqArgs& a, int i, int cx, int cy, SeqRays rays = SeqRays{nullptr, nullptr}) {
    double v[3], g = 0.0;
    SeqRay ray;
    if constexpr (PROJ) ray = seq_ray(rays, cx, cy);
    if (!seq_sample<false, false, PROJ, RING>(a.desc[i], i == a.anchor, a.ox + cx, a.oy + cy, v, g, 1.0, &ray, a.fw)) return 0u;
    return (uint32_t)(unsigned char)(int)v[0] + (uint32_t)(unsigned char)(int)v[1] + (uint32_t)(unsigned char)(int)v[2];
}

// the descriptor table at the head of a statistics workspace, a whole number of 128-byte lines
static int64_t seq_stat_table_bytes(int n) { return ((int64_t)n * (int64_t)sizeof(SeqDesc) + 127) & ~(int64_t)127; }

// The Gains step of the gain rule (include/rwh.h) on n images: A and b built in the rule's order from N(i, j) and I(i, j), the
// square-root-free Cholesky A = L D L^T on the lower triangle, forward and back substitution.  Host only, float64, no LAPACK.
// meets(i): count[i][i] > 0.  false: a non-positive pivot or a non-finite solution.  The gain rule calls it on its two tables, the
// block gain rule on every cell's.
template <class FM, class FN, class FI>
static bool seq_solve_gains(int n, double alpha, double beta, const FM& meets, const FN& N, const FI& I, double* gains) {
    static_assert(RWH_SEQ_MAX_IMAGES == 64, "A, b and y live on the stack");
    double A[64 * 64], b[64], y[64];
    memset(A, 0, sizeof(double) * (size_t)n * n);
    memset(b, 0, sizeof(double) * (size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!meets(i)) { A[i * n + i] = 1.0; b[i] = 1.0; continue; }
        for (int j = 0; j < n; ++j) {
            A[i * n + i] += beta * N(i, j);
            b[i] += beta * N(i, j);
            if (j != i) {
                A[i * n + i] += 2.0 * alpha * I(i, j) * I(i, j) * N(i, j);
                A[i * n + j] -= 2.0 * alpha * I(i, j) * I(j, i) * N(i, j);
            }
        }
    }
    // A = L D L^T, L unit lower (kept below A's diagonal), D on the diagonal: a row that meets nobody (zeros off its diagonal,
    // b_i == A_ii) comes out as b_i / A_ii = 1.0 exactly.
    for (int j = 0; j < n; ++j) {
        double d = A[j * n + j];
        for (int k = 0; k < j; ++k) d -= A[j * n + k] * A[j * n + k] * A[k * n + k];
        if (!(d > 0.0) || !isfinite(d)) return false;
        A[j * n + j] = d;
        for (int i = j + 1; i < n; ++i) {
            double t = A[i * n + j];
            for (int k = 0; k < j; ++k) t -= A[i * n + k] * A[j * n + k] * A[k * n + k];
            A[i * n + j] = t / d;
        }
    }
    for (int i = 0; i < n; ++i) {
        double t = b[i];
        for (int k = 0; k < i; ++k) t -= A[i * n + k] * y[k];
        y[i] = t;
    }
    for (int i = n - 1; i >= 0; --i) {
        double t = y[i] / A[i * n + i];
        for (int k = i + 1; k < n; ++k) t -= A[k * n + i] * gains[k];
        gains[i] = t;
    }
    for (int i = 0; i < n; ++i)
        if (!isfinite(gains[i])) return false;
    return true;
}

}  // namespace rwh
#endif  // RWH_SEQUENCE_H
