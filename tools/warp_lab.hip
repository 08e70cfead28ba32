// Developer microbenchmark for the warp kernels (NOT part of the product, not built by build()).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude -ffp-contract=off tools/warp_lab.hip ransac_with_homography_amd/csrc/rwh_api.hip -o tools/warp_lab
//   ./tools/warp_lab [frames] [case-filter]
// Times the RGB-u8 bilinear kernels on the BASELINE geometry (3840x2160 -> 2028x3771 auto-bounds grid and a
// 3840x2160 fixed grid) and reports how many output bytes differ from the generic (reference-order,
// texel-exact) kernel.
#include "../ransac_with_homography_amd/csrc/rwh_warp.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

using namespace rwh;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

__global__ void fill_random(uint32_t* p, size_t n_words, uint32_t seed) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n_words; i += stride) {
        uint32_t x = (uint32_t)i * 2654435761u ^ seed;
        x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
        p[i] = x;
    }
}

__global__ void diff_count(const unsigned char* a, const unsigned char* b, size_t n, unsigned long long* out) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    unsigned long long d1 = 0, d2 = 0;
    for (; i < n; i += stride) { const int d = abs((int)a[i] - (int)b[i]); d1 += d == 1; d2 += d > 1; }
    if (d1) atomicAdd(out, d1);
    if (d2) atomicAdd(out + 1, d2);
}

// calibration: plain copies of the same volume (what the memory system delivers with no arithmetic)

// Memory-pattern twin of warp_rgb8_fast8: the same grid, the same staging-load and output-store instruction shapes
// (6 source rows x 132 texels in, 4 rows x 128 px out per wave), LDS round trip, and ALU work replaced by NALU
// dependent FMAs per lane.  Answers: what does this access pattern cost with no / with the real amount of arithmetic?
constexpr int F8_PITCH = 688;   // the twin keeps the fixed 128 x 4 patch / 9 x 172 texel slab geometry
template <int NALU, int MODE = 0>   // MODE 1: loads only, 2: stores only
__global__ __launch_bounds__(256) void pattern_twin(const FastArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char slab[4][FP_ROWS * F8_PITCH];
    const unsigned b = blockIdx.x;
    const unsigned logical = (b & 7u) * a.cpx + (b >> 3);
    if (logical >= a.nblocks) return;
    const unsigned t = a.tiles_x_magic ? __umulhi(logical, a.tiles_x_magic) : logical;
    const unsigned tx = logical - t * a.tiles_x;
    const unsigned img = a.tiles_y_magic ? __umulhi(t, a.tiles_y_magic) : t;
    const unsigned ty = t - img * a.tiles_y;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63, prow = lane >> 4, pq = lane & 15;
    const int rr = min(((int)ty * 4 + wave) * 4 + prow, a.rows - 1);
    const int tcol = min((int)tx * 128, a.out_w - 128);
    const unsigned char* simg = a.src + (long long)img * a.src_img_stride;
    unsigned char* drow = a.dst + (long long)img * a.dst_img_stride + ((uint32_t)rr * (uint32_t)a.out_w + (uint32_t)(tcol + 4 * pq)) * 3u;
    const uint32_t pitch = (uint32_t)a.src_w * 3u;
    const int srow = (lane * 49) >> 10, scol = lane - 21 * srow;
    const int r0 = min(((int)ty * 4 + wave) * 4 + 5, a.src_h - 8), x0 = tcol + 3;   // footprint origin (like the warp: a few px off)
    const unsigned char* gbase = simg + (size_t)((uint32_t)r0 * pitch + (uint32_t)x0 * 3u);
    const uint32_t goff = (uint32_t)srow * pitch + (uint32_t)scol * 12u;
    pk3 va[2], vb[2];
    const bool ona = srow < 3, onb = (srow < 3) & (4 * scol + 84 < 132);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        va[k] = pk3{0, 0, 0}; vb[k] = pk3{0, 0, 0};
        if (MODE != 2) {
            if (ona) __builtin_memcpy(&va[k], gbase + (size_t)(3 * k) * pitch + goff, 12);
            if (onb) __builtin_memcpy(&vb[k], gbase + (size_t)(3 * k) * pitch + goff + 252, 12);
        } else { va[k] = pk3{goff, goff * 3u, goff * 5u}; vb[k] = pk3{goff * 7u, goff * 11u, goff * 13u}; }
    }
    float f = (float)lane;
#pragma unroll 16
    for (int i = 0; i < NALU / 2; ++i) f = fmaf(f, 1.0001f, 0.5f);
    unsigned char* my = slab[wave];
    unsigned char* wlds = my + srow * F8_PITCH + scol * 16;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (ona) *reinterpret_cast<uint4*>(wlds + 3 * k * F8_PITCH) = uint4{va[k].a, va[k].b, va[k].c, va[k].a};
        if (onb) *reinterpret_cast<uint4*>(wlds + 3 * k * F8_PITCH + 336) = uint4{vb[k].a, vb[k].b, vb[k].c, vb[k].a};
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 16
    for (int i = 0; i < NALU / 2; ++i) f = fmaf(f, 1.0001f, 0.5f);
    const uint32_t fx = __float_as_uint(f) & 1u;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t* t0 = reinterpret_cast<const uint32_t*>(my + prow * F8_PITCH + (64 * h + 4 * pq) * 4);
        pk3 w = {t0[0] ^ fx, t0[1], t0[2] + t0[F8_PITCH / 4]};
        if (MODE != 1 || w.a + w.b + w.c == 0x12345u) __builtin_memcpy(drow + 192 * h, &w, 12);
    }
}

__global__ __launch_bounds__(256) void copy16(const uint4* __restrict__ s, uint4* __restrict__ d, size_t n) {
    size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i < n) d[i] = s[i];
}
__global__ __launch_bounds__(256) void copy12(const unsigned char* __restrict__ s, unsigned char* __restrict__ d, size_t n12) {
    size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i < n12) { pk3 v; __builtin_memcpy(&v, s + i * 12, 12); __builtin_memcpy(d + i * 12, &v, 12); }
}

int main(int argc, char** argv) {
    const int B = argc > 1 ? atoi(argv[1]) : 16;
    const char* filter = argc > 2 ? argv[2] : nullptr;
    const int SH = 2160, SW = 3840;
    double H[9] = {1.02, 0.01, 5.0, 0.015, 0.98, 7.0, 1e-5, 2e-5, 1.0};
    if (const char* rot = getenv("LAB_ROT")) {   // rotation by LAB_ROT degrees about the image centre, scale LAB_SCALE (default 1)
        const double th = atof(rot) * 3.14159265358979323846 / 180.0, sc = getenv("LAB_SCALE") ? atof(getenv("LAB_SCALE")) : 1.0;
        const double c = sc * cos(th), sn = sc * sin(th), cx = 0.5 * (SW - 1), cy = 0.5 * (SH - 1);
        const double R[9] = {c, -sn, cx - c * cx + sn * cy, sn, c, cy - sn * cx - c * cy, 0, 0, 1};
        for (int i = 0; i < 9; ++i) H[i] = R[i];
        printf("H = rotation %s deg, scale %.3f about the centre\n", rot, sc);
    }
    double A[3][6], ih[9];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { A[i][j] = H[3 * i + j]; A[i][3 + j] = i == j; }
    for (int c = 0; c < 3; ++c) {
        int p = c; for (int i = c + 1; i < 3; ++i) if (fabs(A[i][c]) > fabs(A[p][c])) p = i;
        for (int j = 0; j < 6; ++j) { double t = A[c][j]; A[c][j] = A[p][j]; A[p][j] = t; }
        const double d = A[c][c]; for (int j = 0; j < 6; ++j) A[c][j] /= d;
        for (int i = 0; i < 3; ++i) if (i != c) { const double f = A[i][c]; for (int j = 0; j < 6; ++j) A[i][j] -= f * A[c][j]; }
    }
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) ih[3 * i + j] = A[i][3 + j];
    const size_t src_bytes = (size_t)SH * SW * 3;
    unsigned char *src, *dst, *ref;
    CK(hipMalloc(&src, src_bytes * B + 64));
    CK(hipMalloc(&dst, (size_t)3840 * 2160 * 3 * B + 64));
    CK(hipMalloc(&ref, (size_t)3840 * 2160 * 3 * B + 64));
    fill_random<<<4096, 256>>>(reinterpret_cast<uint32_t*>(src), src_bytes * B / 4, 1234u);
    CK(hipDeviceSynchronize());
    unsigned long long* d_diff; CK(hipMalloc(&d_diff, 16));
    hipEvent_t e0s, e1s; CK(hipEventCreate(&e0s)); CK(hipEventCreate(&e1s));
    {
        const size_t nbytes = (size_t)2028 * 3771 * 3 * B;   // copy as many bytes as one launch writes (reads the same amount)
        for (int which = 0; which < 2; ++which) {
            float best = 1e9f;
            for (int rep = 0; rep < 5; ++rep) {
                CK(hipEventRecord(e0s));
                if (which == 0) copy16<<<(unsigned)((nbytes / 16 + 255) / 256), 256>>>((const uint4*)src, (uint4*)dst, nbytes / 16);
                else copy12<<<(unsigned)((nbytes / 12 + 255) / 256), 256>>>(src, dst, nbytes / 12);
                CK(hipEventRecord(e1s)); CK(hipEventSynchronize(e1s));
                float ms; CK(hipEventElapsedTime(&ms, e0s, e1s)); best = ms < best ? ms : best;
            }
            printf("copy %s: %zu MB read + same written: %.3f ms = %.1f GB/s\n", which ? "12 B/lane" : "16 B/lane", nbytes >> 20, best, 2.0 * nbytes / best / 1e6);
        }
    }
    struct Geo { int x0, y0, w, h; const char* name; } geo[2] = {{5, 7, 3771, 2028, "auto 3771x2028"}, {0, 0, 3840, 2160, "fixed 3840x2160"}};
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int g = 0; g < 2; ++g) {
        const Geo G = geo[g];
        auto args = [&] {
            return make_warp_args(src, SH, SW, (long long)src_bytes, ih, G.x0, 1.0, G.x0 + G.w - 1, G.y0, 1.0, G.y0 + G.h - 1, G.h, G.w, SH, SW,
                                  dst, (long long)G.w * G.h * 3, 0, G.h);
        };
        auto call = [&](int interp, int dst_dtype, bool generic) {
            // the C ABI picks the fast kernel; `generic` forces the generic one by going through launch()
            if (!generic)
                return rwh_warp_backward(src, SH, SW, 3, RWH_U8, (int64_t)src_bytes, B, ih, 1, G.x0, 1.0, G.x0 + G.w - 1, G.y0, 1.0,
                                         G.y0 + G.h - 1, G.h, G.w, SH, SW, interp, dst, dst_dtype, (int64_t)G.w * G.h * 3, 0, G.h, 0, nullptr);
            WarpArgs a = args();
            if (!tile_grid(a, PX, B)) return (int)RWH_E_UNSUPPORTED;
            return launch(pick_generic<unsigned char, 3, unsigned char, RWH_BILINEAR>(), a.cpx, (hipStream_t)0, a);
        };
        // kind Custom: the memory-pattern twin number `group` on the 8 px kernel's tiling
        auto fast = [&](FastKind kind, int group = 1) {
            FastRequest q{kind};
            q.batch = B;
            if (kind == FastKind::Custom) {
                q.group = group;
                q.custom = group == 0 ? pattern_twin<0> : group == 1 ? pattern_twin<220> : group == 2 ? pattern_twin<440> : group == 3 ? pattern_twin<0, 1> : pattern_twin<0, 2>;
            }
            return launch_fast(args(), q, (hipStream_t)0);
        };
        struct Case { const char* name; std::function<int()> run; };
        std::vector<Case> cases = {
            {"generic u8 (reference order)", [&] { return call(RWH_BILINEAR, RWH_U8, true); }},
            {"fast u8 (C ABI default)", [&] { return call(RWH_BILINEAR, RWH_U8, false); }},
            {"nearest u8 (C ABI)", [&] { return call(RWH_NEAREST, RWH_U8, false); }},
            {"exact u8 (float64, RWH_WARP_EXACT)", [&] {
                return rwh_warp_backward(src, SH, SW, 3, RWH_U8, (int64_t)src_bytes, B, ih, 1, G.x0, 1.0, G.x0 + G.w - 1, G.y0, 1.0,
                                         G.y0 + G.h - 1, G.h, G.w, SH, SW, RWH_BILINEAR, dst, RWH_U8, (int64_t)G.w * G.h * 3, 0, G.h, RWH_WARP_EXACT, nullptr); }},
            {"fast u8 px4", [&] { return fast(FastKind::Bilinear4); }},
            {"fast u8 px8", [&] { return fast(FastKind::Bilinear8); }},
            {"fast u8 px8 shape 128x4", [&] { rwh_lab_tune(RWH_TUNE_WARP_SHAPE, 7); int r = fast(FastKind::Bilinear8); rwh_lab_tune(RWH_TUNE_WARP_SHAPE, 0); return r; }},
            {"fast u8 px8 shape 64x8", [&] { rwh_lab_tune(RWH_TUNE_WARP_SHAPE, 6); int r = fast(FastKind::Bilinear8); rwh_lab_tune(RWH_TUNE_WARP_SHAPE, 0); return r; }},
            {"fast u8 px8 shape 32x16", [&] { rwh_lab_tune(RWH_TUNE_WARP_SHAPE, 5); int r = fast(FastKind::Bilinear8); rwh_lab_tune(RWH_TUNE_WARP_SHAPE, 0); return r; }},
            {"twin: px8 access pattern, no ALU", [&] { return fast(FastKind::Custom, 0); }},
            {"twin: px8 access pattern + 220 FMA", [&] { return fast(FastKind::Custom, 1); }},
            {"twin: px8 access pattern + 440 FMA", [&] { return fast(FastKind::Custom, 2); }},
            {"twin: loads only", [&] { return fast(FastKind::Custom, 3); }},
            {"twin: stores only", [&] { return fast(FastKind::Custom, 4); }},
        };
        const double bytes = (double)B * (src_bytes + (double)G.w * G.h * 3);
        const size_t nbytes = (size_t)G.w * G.h * 3 * B;
        printf("== geometry %s, %d frames, %.1f MB algorithmic ==\n", G.name, B, bytes / 1e6);
        for (auto& c : cases) {
            if (filter && &c != &cases[0] && !strstr(c.name, filter)) continue;
            CK(hipMemset(dst, 0, nbytes));
            for (int i = 0; i < 2; ++i) if (c.run() != 0) { printf("launch failed\n"); return 1; }
            CK(hipEventRecord(e0));
            const int reps = getenv("LAB_REPS") ? atoi(getenv("LAB_REPS")) : 10;
            for (int i = 0; i < reps; ++i) c.run();
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1)); ms /= reps;
            if (&c == &cases[0]) CK(hipMemcpy(ref, dst, nbytes, hipMemcpyDeviceToDevice));
            CK(hipMemset(d_diff, 0, 16));
            diff_count<<<2048, 256>>>(dst, ref, nbytes, d_diff);
            unsigned long long hd[2]; CK(hipMemcpy(hd, d_diff, 16, hipMemcpyDeviceToHost));
            printf("%-30s %8.3f ms  %7.1f GB/s  %6.2f us/frame  diff1=%llu diff>1=%llu of %zu\n", c.name, ms, bytes / ms / 1e6, ms * 1e3 / B, hd[0], hd[1], nbytes);
        }
    }
    return 0;
}
