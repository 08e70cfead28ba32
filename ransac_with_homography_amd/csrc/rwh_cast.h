// rwh_cast.h: numpy's element conversions as the reference meets them in stitchPanorama (homography.py:288-338) and in its
// interpolators (homography.py:123-138), for the any-dtype compositor (rwh_stitch_any.hip) and the any-dtype warp (rwh_warp.hip).  Compiles as plain C++ too (no HIP include): the CPU suite builds it with g++ through
// tests/cabi/stitch_cast_shim.cpp and checks it against numpy (tests/test_stitch_any_dtype_cpu.py).
//
// numpy on x86-64 (numpy 2.x) casts a float to uint8 through a truncating conversion to int32 (cvttsd2si) and keeps the low byte;
// a value whose truncation does not fit int32 -- NaN, +-inf, |v| >= 2^31 -- gives the "integer indefinite" 0x80000000, low byte 0.
// Every helper below is plain C++ on in-range values and takes the out-of-range ones on an explicit branch: the GPU's own
// conversions saturate where x86 returns 0x80000000, so nothing may depend on what a conversion does out of range.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RWH_HD __host__ __device__
#else
#define RWH_HD
#endif

namespace rwh_cast {

// float64 -> uint8 (astype(np.uint8), or assignment into a uint8 array): truncate toward zero, low byte of the int32; 0 outside int32
RWH_HD inline uint8_t u8_of_f64(double v) {
    if (v > -2147483649.0 && v < 2147483648.0) return (uint8_t)(uint32_t)(int32_t)v;   // truncation fits int32 (NaN fails both tests)
    return 0;
}
// float32 / float16 -> uint8: the same rule (every such value is exact in float64)
RWH_HD inline uint8_t u8_of_f32(float v) { return u8_of_f64((double)v); }
// integer -> uint8: the low byte (two's complement)
RWH_HD inline uint8_t u8_of_i64(int64_t v) { return (uint8_t)(uint64_t)v; }
RWH_HD inline uint8_t u8_of_u64(uint64_t v) { return (uint8_t)v; }

// -> float32 (addAlpha's float32 copy of imgT, imgQ.astype(np.float32)): round to nearest even, one rounding from the source type
// (int64 / uint64 go to float32 directly: through float64 they would be rounded twice)
RWH_HD inline float f32_of_i64(int64_t v) { return (float)v; }
RWH_HD inline float f32_of_u64(uint64_t v) { return (float)v; }
RWH_HD inline float f32_of_f64(double v) { return (float)v; }     // beyond float32's range: +-inf, NaN stays NaN

// -> float64 (a texel times the float64 weights of bilinear(): numpy promotes every integer, bool and float to float64): exact but
// for int64 / uint64, which round to nearest even like numpy's conversion
template <class T> RWH_HD inline double as_f64(T v) { return (double)v; }
#if defined(__HIPCC__)
template <> RWH_HD inline double as_f64<_Float16>(_Float16 v) { return (double)(float)v; }   // every float16 is exact in float32
#endif

}  // namespace rwh_cast
