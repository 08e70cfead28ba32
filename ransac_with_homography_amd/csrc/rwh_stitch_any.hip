// Any-dtype panorama compositor (rwh_stitch_panorama_ex): stitchPanorama (homography.py:288-338) on images of every numeric
// element type, imgT with 3 or 4 channels and imgQ with 1, 3 or 4.  The same per-pixel float64 recipe as stitch_pixel
// (rwh_stitch.hip), in the same operation order, with the element conversions of the reference's numpy code (rwh_cast.h):
//   paste  -- bilinear() lerps the texels of the caller's imgT in float64 (numpy promotes every integer to float64), the warp is
//             cast to uint8 into a C_T-channel canvas, imgQ is assigned over it (integers by low byte, floats by the uint8 cast;
//             a 1-channel imgQ broadcasts);
//   blend  -- addAlpha's float32 copy of imgT (C_T + 1 channels) is warped in float64; imgQ enters as float32; the float32 canvas
//             is cast to uint8.  With C_T == 4 the weight of imgT is its own channel 3, warped (img_t[:, :, 3:4] of the 5-channel
//             warp); bilinear() blanks channels 0..2 of texel (0,0) of the 5-channel copy, not channel 3.
// Texels are read in their own type (with_elem on the dtype code per launch: one instance per imgT type), imgQ through the
// same switch per pixel, uniform across the launch (a scalar branch).  Four canvas pixels per lane, one 12- or 16-byte store per lane, as stitch_kernel.
#include "rwh_common.h"
#include "rwh_cast.h"

namespace rwh {
namespace {

using half_t = _Float16;

struct AnyArgs {
    const unsigned char* src_t;   // imgT, t_h x t_w x C_T elements of t_dtype
    const unsigned char* src_q;   // imgQ, q_h x q_w x q_c elements of q_dtype
    unsigned char* dst;           // canvas fh x fw x (blend ? 3 : C_T) uint8
    double ih[9];                 // inv(H)
    int t_h, t_w, q_h, q_w, fh, fw;
    int tsx, tsy, wt, ht;         // warped-T rectangle on the canvas and its size (= the warp's output grid)
    int gx0, gy0;                 // warp grid origin (min_x, min_y)
    int qsx, qsy;                 // imgQ rectangle origin on the canvas
    int q_c, q_dtype;
    int blend;                    // 0 paste, 1 'Rate', 2 'Gradient', 3 any other truthy `blending` (as rwh_stitch_panorama)
    int blank;                    // blend + RWH_WARP_ZERO_ORIGIN: texel (0,0) read with channels 0..2 (and, C_T 3, its alpha) zero
    float alpha_t;                // C_T 3: the constant alpha plane ('Rate': float32(rate + 1e-10); mode 3: 0)
    double ramp_den;              // C_T 3, 'Gradient': w + h of imgT
    float alpha_q_in, alpha_q_out;
    int row_begin, row_end;
};

// element conversions by source type (rwh_cast.h): -> float64 (paste lerps), -> float32 (blend's float32 copies), -> uint8
using rwh_cast::as_f64;
template <class T> __device__ __forceinline__ float as_f32(T v) { return (float)v; }
template <> __device__ __forceinline__ float as_f32<int64_t>(int64_t v) { return rwh_cast::f32_of_i64(v); }
template <> __device__ __forceinline__ float as_f32<uint64_t>(uint64_t v) { return rwh_cast::f32_of_u64(v); }
template <> __device__ __forceinline__ float as_f32<double>(double v) { return rwh_cast::f32_of_f64(v); }
template <class T> __device__ __forceinline__ uint8_t as_u8(T v) { return rwh_cast::u8_of_i64((int64_t)v); }
template <> __device__ __forceinline__ uint8_t as_u8<uint64_t>(uint64_t v) { return rwh_cast::u8_of_u64(v); }
template <> __device__ __forceinline__ uint8_t as_u8<float>(float v) { return rwh_cast::u8_of_f32(v); }
template <> __device__ __forceinline__ uint8_t as_u8<double>(double v) { return rwh_cast::u8_of_f64(v); }
template <> __device__ __forceinline__ uint8_t as_u8<half_t>(half_t v) { return rwh_cast::u8_of_f32((float)v); }

// one texel of C elements in a single (12-byte float32 RGB: dwordx3; 24-byte float64 RGB: dwordx4 + dwordx2) load
template <class T, int C> struct alignas(sizeof(T)) Texel { T v[C]; };
template <class T, int C> __device__ __forceinline__ Texel<T, C> ld_texel(const unsigned char* base, size_t idx) {
    Texel<T, C> t;
    __builtin_memcpy(&t, reinterpret_cast<const Texel<T, C>*>(base) + idx, sizeof(t));
    return t;
}

// imgQ's pixel: channel k of the canvas takes imgQ's channel k, or channel 0 when imgQ has 1 channel (numpy broadcasting)
template <int CT>
__device__ __forceinline__ uint32_t q_bytes(const AnyArgs& a, size_t pix) {      // paste: uint8, 0x(AA)BBGGRR
    uint32_t out = 0u;
    with_elem(a.q_dtype, [&](auto tag, const char*) {
        using T = decltype(tag);
        const T* p = reinterpret_cast<const T*>(a.src_q) + pix * a.q_c;
#pragma unroll
        for (int k = 0; k < CT; ++k) out |= (uint32_t)as_u8<T>(p[a.q_c == 1 ? 0 : k]) << (8 * k);
    });
    return out;
}
__device__ __forceinline__ void q_floats(const AnyArgs& a, size_t pix, float q[3]) {   // blend: imgQ[:, :, :3].astype(np.float32)
    with_elem(a.q_dtype, [&](auto tag, const char*) {
        using T = decltype(tag);
        const T* p = reinterpret_cast<const T*>(a.src_q) + pix * a.q_c;
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = as_f32<T>(p[a.q_c == 1 ? 0 : k]);
    });
}

// One canvas pixel (paste: C_T bytes, blend: 3), packed as 0x(AA)BBGGRR.
template <class TT, int CT, bool BLEND>
__device__ __forceinline__ uint32_t any_pixel(const AnyArgs& a, int cx, int cy) {
    const int qx = cx - a.qsx, qy = cy - a.qsy;
    const bool in_q = (qx >= 0) & (qx < a.q_w) & (qy >= 0) & (qy < a.q_h);
    const size_t qpix = in_q ? (size_t)qy * a.q_w + qx : 0;
    const int tx = cx - a.tsx, ty = cy - a.tsy;
    const bool in_t = (tx >= 0) & (tx < a.wt) & (ty >= 0) & (ty < a.ht);
    if (!BLEND && in_q) return q_bytes<CT>(a, qpix);       // paste: imgQ is written last (homography.py:337-338)

    constexpr int NV = BLEND ? 4 : CT;                     // lerped values: paste C_T channels; blend rgb + alpha
    double t[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) t[k] = 0.0;
    if (in_t) {
        // warp_exact's coordinate recipe: dgemm k-order, IEEE divides
        const double x = (double)(a.gx0 + tx), y = (double)(a.gy0 + ty);
        const double X = fma(a.ih[1], y, a.ih[0] * x) + a.ih[2];
        const double Y = fma(a.ih[4], y, a.ih[3] * x) + a.ih[5];
        const double W = fma(a.ih[7], y, a.ih[6] * x) + a.ih[8];
        double sx = X / W, sy = Y / W;
        // bilinear()'s mask moves a coordinate outside the image to (0, 0) and still lerps the four texels there (weights 1, 0,
        // 0, 0: a NaN or inf texel next to the origin makes the pixel NaN, imgT's own alpha at (0,0) weights the blend)
        const bool valid = (sx >= 0.0) & (sx <= (double)(a.t_w - 1)) & (sy >= 0.0) & (sy <= (double)(a.t_h - 1));
        if (!valid) { sx = 0.0; sy = 0.0; }
        const int ix = (int)sx, iy = (int)sy;              // NaN: the index check reports it, any texel will do
        const double fx = sx - (double)ix, fy = sy - (double)iy;
        const double gx = 1.0 - fx, gy = 1.0 - fy;
        const int jx = max(0, min(ix, a.t_w - 1)), jy = max(0, min(iy, a.t_h - 1));
        const int jx1 = min(jx + 1, a.t_w - 1), jy1 = min(jy + 1, a.t_h - 1);
        const int tap_x[4] = {jx, jx1, jx, jx1}, tap_y[4] = {jy, jy, jy1, jy1};
        double v[4][NV];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const Texel<TT, CT> p = ld_texel<TT, CT>(a.src_t, (size_t)tap_y[n] * a.t_w + tap_x[n]);
            const bool origin = (tap_x[n] | tap_y[n]) == 0;
            if constexpr (!BLEND) {
#pragma unroll
                for (int k = 0; k < CT; ++k) v[n][k] = as_f64<TT>(p.v[k]);     // texel (0,0): blanked in memory
            } else {
                const bool z = a.blank && origin;
#pragma unroll
                for (int k = 0; k < 3; ++k) v[n][k] = z ? 0.0 : (double)as_f32<TT>(p.v[k]);
                if constexpr (CT == 4) {
                    v[n][3] = (double)as_f32<TT>(p.v[3]);                         // never blanked (5-channel copy)
                } else if (z) {
                    v[n][3] = 0.0;
                } else {
                    // the alpha plane is never read from memory: 'Rate' a constant, 'Gradient' the float32 ramp (as stitch_pixel)
                    v[n][3] = a.blend == 2 ? (double)(float)(((double)tap_x[n] + (double)tap_y[n]) / a.ramp_den * 0.5) : (double)a.alpha_t;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const double top = v[0][k] * gx + v[1][k] * fx;
            const double bot = v[2][k] * gx + v[3][k] * fx;
            t[k] = top * gy + bot * fy;
        }
    }
    uint32_t out = 0u;
    if constexpr (!BLEND) {          // paste, outside imgQ: the warp cast to uint8, or 0
#pragma unroll
        for (int k = 0; k < CT; ++k) out |= (uint32_t)rwh_cast::u8_of_f64(t[k]) << (8 * k);
        return out;
    } else {
        // float32 canvas: rgb = imgQ (or 0), alpha = alpha_q_in / alpha_q_out; blended inside the warped rectangle
        float q[3] = {0.0f, 0.0f, 0.0f};
        if (in_q) q_floats(a, qpix, q);
        const double qa = (double)(in_q ? a.alpha_q_in : a.alpha_q_out);
        const double base = qa + t[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float c = q[k];
            if (in_t) c = (float)((qa / base) * (double)q[k] + (t[3] / base) * t[k]);   // assignment into the float32 canvas
            out |= (uint32_t)rwh_cast::u8_of_f32(c) << (8 * k);
        }
        return out;
    }
}

constexpr int SA_PX = 4;   // canvas pixels per lane
template <class TT, int CT, bool BLEND>
__global__ __launch_bounds__(256) void stitch_any_kernel(const AnyArgs a) {
    constexpr int CC = BLEND ? 3 : CT;                    // canvas channels
    const int cx0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * SA_PX;
    const int cy = a.row_begin + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (cx0 >= a.fw || cy >= a.row_end) return;
    unsigned char* out = a.dst + ((size_t)cy * a.fw + cx0) * CC;
    uint32_t px[SA_PX];
#pragma unroll
    for (int j = 0; j < SA_PX; ++j) px[j] = cx0 + j < a.fw ? any_pixel<TT, CT, BLEND>(a, cx0 + j, cy) : 0u;
    if (cx0 + SA_PX <= a.fw) {
        if constexpr (CC == 4) {
            pk4 w{px[0], px[1], px[2], px[3]};
            __builtin_memcpy(out, &w, 16);
        } else {
            pk3 w;
            w.a = px[0] | (px[1] << 24);
            w.b = (px[1] >> 8) | (px[2] << 16);
            w.c = (px[2] >> 16) | (px[3] << 8);
            __builtin_memcpy(out, &w, 12);
        }
    } else {
        for (int j = 0; cx0 + j < a.fw; ++j)
#pragma unroll
            for (int k = 0; k < CC; ++k) out[CC * j + k] = (unsigned char)(px[j] >> (8 * k));
    }
}

template <class TT>
int launch_any(const AnyArgs& a, int t_c, dim3 grid, hipStream_t s) {
    if (a.blend) {
        if (t_c == 4) hipLaunchKernelGGL((stitch_any_kernel<TT, 4, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((stitch_any_kernel<TT, 3, true>), grid, dim3(256), 0, s, a);
    } else {
        if (t_c == 4) hipLaunchKernelGGL((stitch_any_kernel<TT, 4, false>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((stitch_any_kernel<TT, 3, false>), grid, dim3(256), 0, s, a);
    }
    return check_launch();
}

}  // namespace
}  // namespace rwh

extern "C" int rwh_stitch_panorama_ex(const void* d_img_t, int t_h, int t_w, int t_c, int t_dtype,
                                      const void* d_img_q, int q_h, int q_w, int q_c, int q_dtype,
                                      const double* inv_h, int grid_x0, int grid_y0, int warp_w, int warp_h,
                                      int tsx, int tsy, int qsx, int qsy, int canvas_h, int canvas_w, int canvas_c,
                                      int blend, double rate, void* d_canvas, int row_begin, int row_end, unsigned flags, void* stream) {
    using namespace rwh;
    if (!d_img_t || !d_img_q || !d_canvas || !inv_h) return RWH_E_INVALID;
    const int t_esz = elem_size(t_dtype);
    if (!t_esz || !elem_size(q_dtype) || blend < 0 || blend > 3 || (flags & ~RWH_WARP_ZERO_ORIGIN)) return RWH_E_INVALID;
    if (t_h <= 0 || t_w <= 0 || q_h <= 0 || q_w <= 0 || warp_w <= 0 || warp_h <= 0 || canvas_h <= 0 || canvas_w <= 0) return RWH_E_INVALID;
    if (row_begin < 0 || row_end > canvas_h || row_begin > row_end) return RWH_E_INVALID;
    if ((t_c != 3 && t_c != 4) || (q_c != 1 && q_c != 3 && q_c != 4)) return RWH_E_UNSUPPORTED;
    if (blend ? canvas_c != 3 : (canvas_c != t_c || (q_c != t_c && q_c != 1))) return RWH_E_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((flags & RWH_WARP_ZERO_ORIGIN) && !blend) {      // bilinear() on the caller's imgT: texel (0,0), every channel (C_T 3 or 4)
        if (rwh::fill_async(const_cast<void*>(d_img_t), 0, (size_t)t_esz * t_c, s) != hipSuccess) return RWH_E_LAUNCH;
    }
    if (row_begin == row_end) return RWH_OK;
    AnyArgs a;
    a.src_t = static_cast<const unsigned char*>(d_img_t);
    a.src_q = static_cast<const unsigned char*>(d_img_q);
    a.dst = static_cast<unsigned char*>(d_canvas);
    for (int i = 0; i < 9; ++i) a.ih[i] = inv_h[i];
    a.t_h = t_h; a.t_w = t_w; a.q_h = q_h; a.q_w = q_w; a.fh = canvas_h; a.fw = canvas_w;
    a.tsx = tsx; a.tsy = tsy; a.wt = warp_w; a.ht = warp_h; a.gx0 = grid_x0; a.gy0 = grid_y0; a.qsx = qsx; a.qsy = qsy;
    a.q_c = q_c; a.q_dtype = q_dtype;
    a.blend = blend;
    a.blank = blend && (flags & RWH_WARP_ZERO_ORIGIN) ? 1 : 0;
    a.row_begin = row_begin; a.row_end = row_end;
    a.ramp_den = (double)(t_w + t_h);
    a.alpha_t = blend == 3 ? 0.0f : (float)(rate + 1e-10);                    // as rwh_stitch_panorama_rows
    a.alpha_q_in = blend >= 2 ? 1.0f : (float)(1 + 1e-10 - rate);
    a.alpha_q_out = (float)1e-10;
    const dim3 grid((canvas_w + 64 * SA_PX - 1) / (64 * SA_PX), (row_end - row_begin + 3) / 4);
    int st = RWH_E_INVALID;
    with_elem(t_dtype, [&](auto tag, const char*) { st = launch_any<decltype(tag)>(a, t_c, grid, s); });
    return st;
}
