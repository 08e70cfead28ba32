// rwh_orb.hip: the feature extractor in front of the matcher (the reference's cv2.ORB_create().detectAndCompute, ransac.py:252-257)
// for a batch of images: FAST-9 corners with non-maximum suppression, intensity-centroid orientation in 12-degree bins, steered
// BRIEF.  The rule is stated in include/rwh.h -- it is NOT OpenCV's ORB and parity with it is not claimed; everything is an
// integer, so the result is exact and does not depend on the order in which the blocks find the keypoints.
// rwh_host_orb_extract (rwh_host.hip) is the same rule in plain C++ for one image.
//
// orb_detect_kernel: one block of 256 lanes per tile of RWH_ORB_TILE_W x RWH_ORB_TILE_H pixels (the tile list is built on the
// device, where the shapes live: a prefix sum of tiles per image that a fixed grid walks with a stride).  The tile and a halo of 4
// (3 for the circle, 1 for the suppression) are converted to gray once and staged as bytes in LDS; the scores of the tile and a halo
// of 1 go to a second LDS plane; a lane then decides four pixels and the survivors of a wave are appended with ONE atomic add of
// their number (ballot + popcount), each lane storing its key at the wave's base + its rank among the survivors.
// A score at or below the threshold is stored as 0: such a pixel is no keypoint and, being below every keypoint's score, never
// suppresses one, so the keypoints and their scores are those of the rule; this lets the high-speed test skip the 16 arcs -- every
// arc of 9 holds two of the four compass pixels 0, 4, 8, 12, so a score above the threshold needs two of them beyond it on one side.
//
// orb_describe_kernel: one wavefront per keypoint.  The 31 x 31 gray patch goes to LDS; the moments are summed per lane and reduced
// across the wave; lanes 0 .. 29 each test one sector and a ballot names the bin; the 5 x 5 box sums of all 27 x 27 test positions
// are built separably in LDS (31 x 27 row sums, then 27 x 27 boxes: 125 byte / halfword reads per lane instead of 25 per test
// point); lane l evaluates tests l, l + 64, ... -- two LDS reads each --, a ballot makes a 64-bit word of the descriptor and eight
// lanes store its bytes.
//
// orb_pyramid_kernel (rule 6): one block of 256 lanes per tile of RWH_ORB_PYR_TILE_W x RWH_ORB_PYR_TILE_H = 64 x 16 pixels of a level
// plane; the tile list runs over (image, level) and is built by orb_pyramid_setup_kernel as orb_setup_kernel builds the detector's:
// a prefix sum that a fixed grid walks with a stride, all levels of all images in ONE launch.  The source window of the tile -- at
// most 4 * 64 + 2 = 258 columns x 4 * 16 + 2 = 66 rows at the largest scale, 1024 -- is read once, a wave per row, converted to gray on
// the way (rule 1) with indices clamped to the last column and row (the edge rule), and staged as bytes: 66 rows at a stride of 260 =
// 17160 bytes of LDS.  The area average is evaluated separably out of LDS, which rule 6 allows because nothing is rounded before
// the end: lane X of a wave forms the row sum sum_j wx_j g of its column for one staged row at a time (its at most five weights
// are per-tile registers), into a plane of 66 x 68 uint32 = 17952 bytes; then a lane takes four adjacent columns of one output row,
// sums at most five rows of row sums (one 16-byte LDS read each), divides by s^2 -- a 32-bit unsigned division by a per-level
// constant; no 64-bit arithmetic inside the loops -- and stores the four bytes as one word where the address is a multiple of 4.
// 35112 bytes of LDS per block in all.  The 16 scales travel by value as a kernel argument.
#include "rwh_common.h"

#define RWH_ORB_GRID_MAX 16384

namespace rwh {

constexpr int ORB_HALO = 4;
constexpr int ORB_LW = RWH_ORB_TILE_W + 2 * ORB_HALO, ORB_LH = RWH_ORB_TILE_H + 2 * ORB_HALO;     // the staged gray tile
constexpr int ORB_SW = RWH_ORB_TILE_W + 2, ORB_SH = RWH_ORB_TILE_H + 2;                           // the score plane
constexpr int ORB_PATCH = 2 * RWH_ORB_PATCH_RADIUS + 1;                                           // 31
constexpr int ORB_BOX = 2 * RWH_ORB_TEST_RADIUS + 1;                                              // 27
static_assert(RWH_ORB_TILE_W * RWH_ORB_TILE_H == 4 * 256 && RWH_ORB_TILE_W == RWH_WAVE, "a lane decides four pixels, a wave one tile row");
static_assert(RWH_ORB_TEST_RADIUS + 2 == RWH_ORB_PATCH_RADIUS && RWH_ORB_BORDER == RWH_ORB_PATCH_RADIUS + 1, "the boxes end at the patch");
static_assert(RWH_ORB_BINS <= RWH_WAVE, "one lane per sector");

struct OrbImage { long long src, gray; int h, w, c; };

// row i of the table, or an image without pixels where the row does not describe one inside the two buffers
__device__ __forceinline__ OrbImage orb_image(const int64_t* __restrict__ table, int i, long long images_bytes, long long gray_bytes) {
    const long long src = table[5 * i], gray = table[5 * i + 1], h = table[5 * i + 2], w = table[5 * i + 3], c = table[5 * i + 4];
    const bool shape = h >= 1 && w >= 1 && h <= 65536 && w <= 65536 && (c == 1 || c == 3 || c == 4);
    const bool ok = shape && src >= 0 && gray >= 0 && (images_bytes < 0 || src + h * w * c <= images_bytes) && gray + h * w <= gray_bytes;
    OrbImage im;
    im.src = ok ? src : 0; im.gray = ok ? gray : 0; im.h = ok ? (int)h : 0; im.w = ok ? (int)w : 0; im.c = ok ? (int)c : 1;
    return im;
}

__device__ __forceinline__ unsigned long long orb_tiles(const OrbImage& im) {
    return (unsigned long long)((im.w + RWH_ORB_TILE_W - 1) / RWH_ORB_TILE_W) * (unsigned long long)((im.h + RWH_ORB_TILE_H - 1) / RWH_ORB_TILE_H);
}

// prefix[i] = tiles of the images before i, prefix[n_images] = all (one block)
__global__ __launch_bounds__(256) void orb_setup_kernel(const int64_t* __restrict__ table, int n_images, long long images_bytes,
                                                        long long gray_bytes, unsigned long long* __restrict__ prefix) {
    __shared__ unsigned long long part[256];
    const int per = (n_images + 255) / 256;
    const int i0 = min(n_images, (int)threadIdx.x * per), i1 = min(n_images, i0 + per);
    unsigned long long sum = 0;
    for (int i = i0; i < i1; ++i) sum += orb_tiles(orb_image(table, i, images_bytes, gray_bytes));
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < 256; ++t) { const unsigned long long v = part[t]; part[t] = run; run += v; }
        prefix[n_images] = run;
    }
    __syncthreads();
    sum = part[threadIdx.x];
    for (int i = i0; i < i1; ++i) { prefix[i] = sum; sum += orb_tiles(orb_image(table, i, images_bytes, gray_bytes)); }
}

// rule 2 at the LDS byte `p` (row stride ORB_LW), or 0 where the score cannot exceed `threshold`
__device__ __forceinline__ int orb_fast_score(const unsigned char* p, int threshold) {
    const int c = p[0];
    const int d0 = p[-3 * ORB_LW] - c, d4 = p[3] - c, d8 = p[3 * ORB_LW] - c, d12 = p[-3] - c;
    const int hi = (d0 > threshold) + (d4 > threshold) + (d8 > threshold) + (d12 > threshold);
    const int lo = (d0 < -threshold) + (d4 < -threshold) + (d8 < -threshold) + (d12 < -threshold);
    if (hi < 2 && lo < 2) return 0;
    int d[16];
    d[0] = d0; d[4] = d4; d[8] = d8; d[12] = d12;
    d[1] = p[-3 * ORB_LW + 1] - c; d[2] = p[-2 * ORB_LW + 2] - c; d[3] = p[-ORB_LW + 3] - c;
    d[5] = p[ORB_LW + 3] - c; d[6] = p[2 * ORB_LW + 2] - c; d[7] = p[3 * ORB_LW + 1] - c;
    d[9] = p[3 * ORB_LW - 1] - c; d[10] = p[2 * ORB_LW - 2] - c; d[11] = p[ORB_LW - 3] - c;
    d[13] = p[-ORB_LW - 3] - c; d[14] = p[-2 * ORB_LW - 2] - c; d[15] = p[-3 * ORB_LW - 1] - c;
    // min / max over the 9 pixels from i on, by doubling: 2, 4, 8, then one more
    int mn[16], mx[16], t[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { mn[i] = min(d[i], d[(i + 1) & 15]); mx[i] = max(d[i], d[(i + 1) & 15]); }
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = min(mn[i], mn[(i + 2) & 15]);
#pragma unroll
    for (int i = 0; i < 16; ++i) mn[i] = min(t[i], t[(i + 4) & 15]);
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = max(mx[i], mx[(i + 2) & 15]);
#pragma unroll
    for (int i = 0; i < 16; ++i) mx[i] = max(t[i], t[(i + 4) & 15]);
    int s = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) s = max(s, max(min(mn[i], d[(i + 8) & 15]), -max(mx[i], d[(i + 8) & 15])));
    return s > threshold ? s : 0;
}

__global__ __launch_bounds__(256) void orb_detect_kernel(const unsigned char* __restrict__ images, long long images_bytes,
                                                         const int64_t* __restrict__ table, int n_images, int threshold,
                                                         unsigned char* __restrict__ gray_out, long long gray_bytes,
                                                         const unsigned long long* __restrict__ prefix,
                                                         unsigned long long* __restrict__ keys, int capacity, int* __restrict__ counts) {
    __shared__ unsigned char g[ORB_LH * ORB_LW];
    __shared__ unsigned char sc[ORB_SH * ORB_SW];
    const int tid = threadIdx.x, lane = tid & (RWH_WAVE - 1);
    const unsigned long long n_work = prefix[n_images];
    for (unsigned long long wk = blockIdx.x; wk < n_work; wk += gridDim.x) {
        int lo = 0, hi = n_images;                                  // the image that owns tile wk: the last i with prefix[i] <= wk
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (prefix[mid] <= wk) lo = mid; else hi = mid;
        }
        const int img = lo;
        const OrbImage im = orb_image(table, img, images_bytes, gray_bytes);
        const unsigned tiles_x = (unsigned)((im.w + RWH_ORB_TILE_W - 1) / RWH_ORB_TILE_W);
        const unsigned long long r = wk - prefix[img];
        const int x0 = (int)(r % tiles_x) * RWH_ORB_TILE_W, y0 = (int)(r / tiles_x) * RWH_ORB_TILE_H;
        const unsigned char* src = images + im.src;
        __syncthreads();                                            // the tile before this one has been read by every wave
        for (int e = tid; e < ORB_LH * ORB_LW; e += 256) {
            const int ly = e / ORB_LW, lx = e % ORB_LW;
            const int x = x0 - ORB_HALO + lx, y = y0 - ORB_HALO + ly;
            int v = 0;
            if (x >= 0 && x < im.w && y >= 0 && y < im.h) {
                const long long px = (long long)y * im.w + x;
                if (im.c == 1) v = src[px];
                else {
                    const unsigned char* q = src + px * im.c;
                    v = (4899 * q[0] + 9617 * q[1] + 1868 * q[2] + 8192) >> 14;
                }
                if (lx >= ORB_HALO && lx < ORB_HALO + RWH_ORB_TILE_W && ly >= ORB_HALO && ly < ORB_HALO + RWH_ORB_TILE_H)
                    gray_out[im.gray + px] = (unsigned char)v;
            }
            g[e] = (unsigned char)v;
        }
        __syncthreads();
        for (int e = tid; e < ORB_SH * ORB_SW; e += 256) {
            const int ly = e / ORB_SW, lx = e % ORB_SW;
            const int x = x0 - 1 + lx, y = y0 - 1 + ly;
            int s = 0;
            if (x >= 3 && x < im.w - 3 && y >= 3 && y < im.h - 3) s = orb_fast_score(&g[(ly + ORB_HALO - 1) * ORB_LW + lx + ORB_HALO - 1], threshold);
            sc[e] = (unsigned char)s;
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int ly = it * 4 + (tid >> 6), lx = lane;          // a wave takes one row of the tile at a time
            const int x = x0 + lx, y = y0 + ly;
            const unsigned char* p = &sc[(ly + 1) * ORB_SW + lx + 1];
            const int s = p[0];
            const int nb = max(max(max((int)p[-ORB_SW - 1], (int)p[-ORB_SW]), max((int)p[-ORB_SW + 1], (int)p[-1])),
                               max(max((int)p[1], (int)p[ORB_SW - 1]), max((int)p[ORB_SW], (int)p[ORB_SW + 1])));
            const bool kp = s > threshold && s > nb && x >= RWH_ORB_BORDER && x <= im.w - 1 - RWH_ORB_BORDER && y >= RWH_ORB_BORDER &&
                            y <= im.h - 1 - RWH_ORB_BORDER;
            const unsigned long long found = __ballot(kp);
            if (found) {
                const int first = __ffsll((long long)found) - 1;
                int base = 0;
                if (lane == first) base = atomicAdd(&counts[img], __popcll(found));
                base = __shfl(base, first);
                const long long slot = (long long)base + __popcll(found & ((1ull << lane) - 1ull));
                if (kp && slot < capacity)
                    keys[(long long)img * capacity + slot] = ((unsigned long long)(255 - s) << 32) | ((unsigned long long)y << 16) | (unsigned long long)x;
            }
        }
    }
}

__global__ __launch_bounds__(RWH_WAVE) void orb_describe_kernel(const unsigned char* __restrict__ gray, long long gray_bytes,
                                                                const int64_t* __restrict__ table, const unsigned long long* __restrict__ keys,
                                                                int key_stride, const int* __restrict__ counts, int n_features,
                                                                const int* __restrict__ bin_table, const signed char* __restrict__ pattern,
                                                                int nbytes, float* __restrict__ kps, unsigned char* __restrict__ desc,
                                                                int* __restrict__ score, int* __restrict__ bins) {
    __shared__ unsigned char patch[ORB_PATCH * 32];                  // rows of 31 at a stride of 32
    __shared__ unsigned short rows5[ORB_PATCH * ORB_BOX];            // sums of 5 along x
    __shared__ unsigned short box[ORB_BOX * ORB_BOX];
    const int lane = threadIdx.x;
    const int img = blockIdx.x / n_features, slot = blockIdx.x % n_features;
    if (slot >= min(min(counts[img], n_features), key_stride)) return;
    const OrbImage im = orb_image(table, img, -1, gray_bytes);
    const unsigned long long key = keys[(long long)img * key_stride + slot];
    const int x = (int)(key & 0xFFFFu), y = (int)((key >> 16) & 0xFFFFu), s = 255 - (int)((key >> 32) & 0xFFu);
    if ((key >> 40) != 0 || x < RWH_ORB_BORDER || x > im.w - 1 - RWH_ORB_BORDER || y < RWH_ORB_BORDER || y > im.h - 1 - RWH_ORB_BORDER) return;
    const unsigned char* src = gray + im.gray + (long long)(y - RWH_ORB_PATCH_RADIUS) * im.w + (x - RWH_ORB_PATCH_RADIUS);
    int m10 = 0, m01 = 0;
    for (int e = lane; e < ORB_PATCH * ORB_PATCH; e += RWH_WAVE) {
        const int r = e / ORB_PATCH, c = e % ORB_PATCH;
        const int v = src[(long long)r * im.w + c];
        patch[r * 32 + c] = (unsigned char)v;
        const int dx = c - RWH_ORB_PATCH_RADIUS, dy = r - RWH_ORB_PATCH_RADIUS;
        if (dx * dx + dy * dy <= RWH_ORB_PATCH_RADIUS * RWH_ORB_PATCH_RADIUS) { m10 += dx * v; m01 += dy * v; }
    }
#pragma unroll
    for (int o = RWH_WAVE / 2; o > 0; o >>= 1) { m10 += __shfl_xor(m10, o); m01 += __shfl_xor(m01, o); }
    // rule 4: lane k < 30 tests sector k
    bool mine = false;
    if (lane < RWH_ORB_BINS) {
        const int k1 = lane + 1 == RWH_ORB_BINS ? 0 : lane + 1;
        const long long c0 = (long long)bin_table[2 * lane] * m01 - (long long)bin_table[2 * lane + 1] * m10;
        const long long c1 = (long long)bin_table[2 * k1] * m01 - (long long)bin_table[2 * k1 + 1] * m10;
        mine = c0 >= 0 && c1 < 0;
    }
    const unsigned long long sector = __ballot(mine);
    const int bin = sector ? __ffsll((long long)sector) - 1 : 0;
    __syncthreads();
    for (int e = lane; e < ORB_PATCH * ORB_BOX; e += RWH_WAVE) {
        const int r = e / ORB_BOX, c = e % ORB_BOX;
        const unsigned char* p = &patch[r * 32 + c];
        rows5[e] = (unsigned short)(p[0] + p[1] + p[2] + p[3] + p[4]);
    }
    __syncthreads();
    for (int e = lane; e < ORB_BOX * ORB_BOX; e += RWH_WAVE) {
        const unsigned short* p = &rows5[e];                        // e = r * 27 + c: the five rows r .. r + 4 of column c
        box[e] = (unsigned short)(p[0] + p[ORB_BOX] + p[2 * ORB_BOX] + p[3 * ORB_BOX] + p[4 * ORB_BOX]);
    }
    __syncthreads();
    const int nbits = 8 * nbytes;
    const long long out = (long long)img * n_features + slot;
    const signed char* pat = pattern + (long long)bin * nbits * 4;
    for (int w0 = 0; w0 < nbits; w0 += RWH_WAVE) {
        const int t = w0 + lane;
        bool bit = false;
        if (t < nbits) {
            const uint32_t q = ld4(reinterpret_cast<const unsigned char*>(pat + 4 * t));
            const int R = RWH_ORB_TEST_RADIUS;
            const int x1 = min(max((int)(signed char)(q & 0xFF), -R), R), y1 = min(max((int)(signed char)((q >> 8) & 0xFF), -R), R);
            const int x2 = min(max((int)(signed char)((q >> 16) & 0xFF), -R), R), y2 = min(max((int)(signed char)(q >> 24), -R), R);
            bit = box[(y1 + R) * ORB_BOX + x1 + R] < box[(y2 + R) * ORB_BOX + x2 + R];
        }
        const unsigned long long word = __ballot(bit);
        const int b = (w0 >> 3) + lane;
        if (lane < 8 && b < nbytes) desc[out * nbytes + b] = (unsigned char)(word >> (8 * lane));
    }
    if (lane == 0) {
        kps[2 * out] = (float)x; kps[2 * out + 1] = (float)y;
        score[out] = s; bins[out] = bin;
    }
}

// ---- rule 6: the levels of the pyramid ----
constexpr int PYR_TW = RWH_ORB_PYR_TILE_W, PYR_TH = RWH_ORB_PYR_TILE_H;
constexpr int PYR_MAXQ = RWH_ORB_SCALE_MAX / RWH_ORB_SCALE_ONE;                                   // source pixels per level pixel, per axis: 4
constexpr int PYR_WW = PYR_MAXQ * PYR_TW + 2, PYR_WH = PYR_MAXQ * PYR_TH + 2;                     // the staged window: 258 x 66
constexpr int PYR_WS = (PYR_WW + 3) & ~3;                                                         // its row stride: 260
constexpr int PYR_RS = PYR_TW + 4;                                                                // row stride of the row sums, in words
constexpr int PYR_TAPS = PYR_MAXQ + 1;                                                            // source pixels a footprint can touch: 5
static_assert(PYR_TW == RWH_WAVE && PYR_TW * PYR_TH == 4 * 256 && PYR_RS % 4 == 0, "a wave sums one staged row, a lane stores four columns");

struct OrbScales { int s[RWH_ORB_LEVELS_MAX]; };
struct OrbLevel { long long src, dst; int h, w, c, hl, wl, s; };

// row `row` of the table as level row % n_levels of image row / n_levels: hl = wl = 0 (no pixels to make) for level 0, for a level
// whose image's row does not describe an image inside [0, planes_offset), and for a row that is not that level's plane inside
// [planes_offset, images_bytes)
__device__ __forceinline__ OrbLevel orb_level(const int64_t* __restrict__ table, int row, int n_levels, const OrbScales& sc,
                                              long long images_bytes, long long planes_offset) {
    OrbLevel L;
    L.src = L.dst = 0; L.h = L.w = 1; L.c = 1; L.hl = L.wl = 0; L.s = RWH_ORB_SCALE_ONE;
    const int l = row % n_levels;
    if (l == 0) return L;
    const long long i0 = 5ll * (row - l), i = 5ll * row;
    const long long src = table[i0], h = table[i0 + 2], w = table[i0 + 3], c = table[i0 + 4];
    if (!(h >= 1 && w >= 1 && h <= 65536 && w <= 65536 && (c == 1 || c == 3 || c == 4) && src >= 0 && src + h * w * c <= planes_offset)) return L;
    const int s = sc.s[l];
    const int hl = orb_level_side((int)h, s), wl = orb_level_side((int)w, s);
    const long long dst = table[i];
    if (!(hl >= 1 && wl >= 1 && table[i + 2] == hl && table[i + 3] == wl && table[i + 4] == 1 && dst >= planes_offset &&
          dst + (long long)hl * wl <= images_bytes))
        return L;
    L.src = src; L.dst = dst; L.h = (int)h; L.w = (int)w; L.c = (int)c; L.hl = hl; L.wl = wl; L.s = s;
    return L;
}

__device__ __forceinline__ unsigned long long orb_level_tiles(const OrbLevel& L) {
    return (unsigned long long)((L.wl + PYR_TW - 1) / PYR_TW) * (unsigned long long)((L.hl + PYR_TH - 1) / PYR_TH);
}

// prefix[r] = output tiles of the table rows before r, prefix[n_rows] = all (one block)
__global__ __launch_bounds__(256) void orb_pyramid_setup_kernel(const int64_t* __restrict__ table, int n_rows, int n_levels, OrbScales sc,
                                                                long long images_bytes, long long planes_offset,
                                                                unsigned long long* __restrict__ prefix) {
    __shared__ unsigned long long part[256];
    const int per = (n_rows + 255) / 256;
    const int i0 = (int)min((long long)n_rows, (long long)threadIdx.x * per), i1 = (int)min((long long)n_rows, (long long)i0 + per);
    unsigned long long sum = 0;
    for (int i = i0; i < i1; ++i) sum += orb_level_tiles(orb_level(table, i, n_levels, sc, images_bytes, planes_offset));
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < 256; ++t) { const unsigned long long v = part[t]; part[t] = run; run += v; }
        prefix[n_rows] = run;
    }
    __syncthreads();
    sum = part[threadIdx.x];
    for (int i = i0; i < i1; ++i) { prefix[i] = sum; sum += orb_level_tiles(orb_level(table, i, n_levels, sc, images_bytes, planes_offset)); }
}

// the footprint [a, a + s) of a level pixel on one axis: its first source pixel and the overlap with that one and the next four
// (0 past the footprint's end), in Q8
__device__ __forceinline__ int orb_taps(unsigned a, unsigned s, unsigned (&wgt)[PYR_TAPS]) {
    const unsigned b = a + s, j0 = a >> 8;
#pragma unroll
    for (int k = 0; k < PYR_TAPS; ++k) {
        const unsigned lo = max(a, (j0 + k) << 8), hi = min(b, (j0 + k + 1) << 8);
        wgt[k] = hi > lo ? hi - lo : 0u;
    }
    return (int)j0;
}

__global__ __launch_bounds__(256) void orb_pyramid_kernel(unsigned char* __restrict__ images, long long images_bytes, long long planes_offset,
                                                          const int64_t* __restrict__ table, int n_rows, int n_levels, OrbScales sc,
                                                          const unsigned long long* __restrict__ prefix) {
    __shared__ unsigned char g[PYR_WH * PYR_WS];
    __shared__ __attribute__((aligned(16))) unsigned rsum[PYR_WH * PYR_RS];
    const int tid = threadIdx.x, lane = tid & (RWH_WAVE - 1), wave = tid >> 6;
    const unsigned long long n_work = prefix[n_rows];
    for (unsigned long long wk = blockIdx.x; wk < n_work; wk += gridDim.x) {
        int lo = 0, hi = n_rows;                                    // the row that owns tile wk: the last r with prefix[r] <= wk
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (prefix[mid] <= wk) lo = mid; else hi = mid;
        }
        const OrbLevel L = orb_level(table, lo, n_levels, sc, images_bytes, planes_offset);
        if (L.wl == 0) continue;                                    // uniform over the block; cannot happen for a tile the prefix counted
        const unsigned tiles_x = (unsigned)((L.wl + PYR_TW - 1) / PYR_TW);
        const unsigned long long r = wk - prefix[lo];
        const int X0 = (int)(r % tiles_x) * PYR_TW, Y0 = (int)(r / tiles_x) * PYR_TH;
        const int Xe = min(X0 + PYR_TW, L.wl), Ye = min(Y0 + PYR_TH, L.hl);
        const unsigned s = (unsigned)L.s;
        // the source window of the tile; level sides are below 2^16 and s <= 2^10, so every product is below 2^27
        const int jb = (int)(((unsigned)X0 * s) >> 8), ib = (int)(((unsigned)Y0 * s) >> 8);
        const int nw = min((int)(((unsigned)Xe * s - 1u) >> 8) - jb + 1, PYR_WW), nh = min((int)(((unsigned)Ye * s - 1u) >> 8) - ib + 1, PYR_WH);
        const unsigned char* src = images + L.src;
        __syncthreads();                                            // the tile before this one has been read by every wave
        for (int ly = wave; ly < nh; ly += 4) {                     // a wave stages one row at a time
            const long long row = (long long)min(ib + ly, L.h - 1) * L.w;
            for (int lx = lane; lx < nw; lx += RWH_WAVE) {
                const long long px = row + min(jb + lx, L.w - 1);
                int v;
                if (L.c == 1) v = src[px];
                else {
                    const unsigned char* q = src + px * L.c;
                    v = (4899 * q[0] + 9617 * q[1] + 1868 * q[2] + 8192) >> 14;
                }
                g[ly * PYR_WS + lx] = (unsigned char)v;
            }
        }
        unsigned wgt[PYR_TAPS];
        {                                                           // lane X: column X0 + X of the level, the same taps for every staged row
            const int j0 = orb_taps((unsigned)(X0 + lane) * s, s, wgt) - jb;
            int at[PYR_TAPS];
#pragma unroll
            for (int k = 0; k < PYR_TAPS; ++k) at[k] = min(j0 + k, nw - 1);
            __syncthreads();
            if (X0 + lane < Xe)
                for (int ly = wave; ly < nh; ly += 4) {
                    const unsigned char* p = &g[ly * PYR_WS];
                    unsigned sum = 0;
#pragma unroll
                    for (int k = 0; k < PYR_TAPS; ++k) sum += wgt[k] * p[at[k]];
                    rsum[ly * PYR_RS + lane] = sum;
                }
        }
        __syncthreads();
        const int Y = Y0 + (tid >> 4), X = X0 + 4 * (tid & 15);      // four adjacent columns of one output row
        if (Y < Ye && X < Xe) {
            const int i0 = orb_taps((unsigned)Y * s, s, wgt) - ib;
            unsigned acc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < PYR_TAPS; ++k) {
                const uint4 v = *reinterpret_cast<const uint4*>(&rsum[min(i0 + k, nh - 1) * PYR_RS + (X - X0)]);
                acc[0] += wgt[k] * v.x; acc[1] += wgt[k] * v.y; acc[2] += wgt[k] * v.z; acc[3] += wgt[k] * v.w;
            }
            const unsigned s2 = s * s;
            unsigned o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = (acc[k] + s2 / 2u) / s2;
            unsigned char* out = images + L.dst + (long long)Y * L.wl + X;
            if (X + 3 < Xe && ((uintptr_t)out & 3u) == 0)
                *reinterpret_cast<uint32_t*>(out) = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
            else
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (X + k < Xe) out[k] = (unsigned char)o[k];
        }
    }
}

}  // namespace rwh

extern "C" int64_t rwh_orb_pyramid_bytes(int h, int w, const int32_t* scales, int n_levels) {
    if (!rwh::orb_scales_ok(scales, n_levels) || h < 1 || w < 1 || h > 65536 || w > 65536) return RWH_E_INVALID;
    int64_t bytes = 0;
    for (int l = 1; l < n_levels; ++l) bytes += (int64_t)rwh::orb_level_side(h, scales[l]) * rwh::orb_level_side(w, scales[l]);
    return bytes;
}

extern "C" int rwh_orb_pyramid_batched(uint8_t* d_images, int64_t images_bytes, int64_t planes_offset, const int64_t* d_table, int n_images,
                                       const int32_t* scales, int n_levels, void* d_workspace, int64_t workspace_bytes, void* stream) {
    using namespace rwh;
    if (!d_images || !d_table || !d_workspace || n_images <= 0 || !orb_scales_ok(scales, n_levels) || planes_offset < 0 ||
        planes_offset > images_bytes || (long long)n_images * n_levels >= (1ll << 31))
        return RWH_E_INVALID;
    const int n_rows = n_images * n_levels;
    if (workspace_bytes < rwh_orb_workspace_bytes(n_rows) || ((uintptr_t)d_workspace & 7u)) return RWH_E_INVALID;
    if (n_levels == 1) return RWH_OK;                               // level 0 is the image: nothing to make
    OrbScales sc;
    for (int l = 0; l < RWH_ORB_LEVELS_MAX; ++l) sc.s[l] = l < n_levels ? scales[l] : RWH_ORB_SCALE_MAX;
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long* prefix = static_cast<unsigned long long*>(d_workspace);
    hipLaunchKernelGGL(orb_pyramid_setup_kernel, dim3(1), dim3(256), 0, s, d_table, n_rows, n_levels, sc, (long long)images_bytes,
                       (long long)planes_offset, prefix);
    // the planes hold one byte per pixel inside the tail, which bounds the output pixels; a plane adds at most one partial tile per
    // tile row and column it has -- the grid walks the tile list with a stride, so any size is correct
    const long long want = (images_bytes - planes_offset) / (PYR_TW * PYR_TH) * 2 + n_rows;
    const unsigned grid = (unsigned)(want < RWH_ORB_GRID_MAX ? want : RWH_ORB_GRID_MAX);
    hipLaunchKernelGGL(orb_pyramid_kernel, dim3(grid), dim3(256), 0, s, d_images, (long long)images_bytes, (long long)planes_offset, d_table,
                       n_rows, n_levels, sc, prefix);
    return check_launch();
}

extern "C" int64_t rwh_orb_workspace_bytes(int n_images) {
    if (n_images <= 0) return RWH_E_INVALID;
    return 8ll * ((long long)n_images + 1);
}

extern "C" int rwh_orb_detect_batched(const uint8_t* d_images, int64_t images_bytes, const int64_t* d_table, int n_images, int threshold,
                                      uint8_t* d_gray, int64_t gray_bytes, uint64_t* d_keys, int capacity, int32_t* d_counts,
                                      void* d_workspace, int64_t workspace_bytes, void* stream) {
    using namespace rwh;
    if (!d_images || !d_table || !d_gray || !d_keys || !d_counts || !d_workspace || n_images <= 0 || capacity <= 0 || images_bytes < 0 ||
        gray_bytes < 0 || threshold < 0 || threshold > 254)
        return RWH_E_INVALID;
    if (workspace_bytes < rwh_orb_workspace_bytes(n_images) || ((uintptr_t)d_workspace & 7u)) return RWH_E_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned long long* prefix = static_cast<unsigned long long*>(d_workspace);
    if (rwh::fill_async(d_keys, (int)(RWH_ORB_KEY_NONE & 0xFF), 8ull * (size_t)n_images * (size_t)capacity, s) != hipSuccess) return RWH_E_LAUNCH;
    if (rwh::fill_async(d_counts, 0, 4ull * (size_t)n_images, s) != hipSuccess) return RWH_E_LAUNCH;
    hipLaunchKernelGGL(orb_setup_kernel, dim3(1), dim3(256), 0, s, d_table, n_images, (long long)images_bytes, (long long)gray_bytes, prefix);
    // the gray planes hold one byte per pixel, so gray_bytes bounds the pixels; an image adds at most one partial tile per tile row and
    // column it has -- the grid walks the tile list with a stride, so any size is correct
    const long long want = gray_bytes / (RWH_ORB_TILE_W * RWH_ORB_TILE_H) * 2 + n_images;
    const unsigned grid = (unsigned)(want < RWH_ORB_GRID_MAX ? want : RWH_ORB_GRID_MAX);
    hipLaunchKernelGGL(orb_detect_kernel, dim3(grid), dim3(256), 0, s, d_images, (long long)images_bytes, d_table, n_images, threshold, d_gray,
                       (long long)gray_bytes, prefix, reinterpret_cast<unsigned long long*>(d_keys), capacity, d_counts);
    return check_launch();
}

extern "C" int rwh_orb_describe_batched(const uint8_t* d_gray, int64_t gray_bytes, const int64_t* d_table, int n_images,
                                        const uint64_t* d_keys, int key_stride, const int32_t* d_counts, int n_features,
                                        const int32_t* d_bin_table, const int8_t* d_pattern, int nbytes, float* d_kps, uint8_t* d_desc,
                                        int32_t* d_score, int32_t* d_bin, void* stream) {
    using namespace rwh;
    if (!d_gray || !d_table || !d_keys || !d_counts || !d_bin_table || !d_pattern || !d_kps || !d_desc || !d_score || !d_bin || n_images <= 0 ||
        n_features <= 0 || key_stride <= 0 || gray_bytes < 0 || (long long)n_images * n_features >= (1ll << 31))
        return RWH_E_INVALID;
    if (nbytes < 1 || nbytes > RWH_MATCH_MAX_BYTES) return RWH_E_UNSUPPORTED;
    hipLaunchKernelGGL(orb_describe_kernel, dim3((unsigned)(n_images * n_features)), dim3(RWH_WAVE), 0, static_cast<hipStream_t>(stream), d_gray,
                       (long long)gray_bytes, d_table, reinterpret_cast<const unsigned long long*>(d_keys), key_stride, d_counts, n_features,
                       d_bin_table, reinterpret_cast<const signed char*>(d_pattern), nbytes, d_kps, d_desc, d_score, d_bin);
    return check_launch();
}
