// Shared device/host helpers for librwh_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rwh.h"

#define RWH_WAVE 64

// hipcc contracts a*b+c into FMA by default; the parity recipes in this library
// state every rounding explicitly, so contraction is switched off file-wide and
// fused operations are written as fma()/fmaf() where they are wanted.
#pragma clang fp contract(off)

namespace rwh {

// Packed (alignment 1) views for byte-addressed texel traffic.  gfx950 runs in
// unaligned-access mode: these lower to single global_load_dwordx2 /
// global_store_dwordx3 instructions at any byte address.
struct __attribute__((packed)) pk2 { uint32_t a, b; };
struct __attribute__((packed)) pk3 { uint32_t a, b, c; };
struct __attribute__((packed)) pk4 { uint32_t a, b, c, d; };

__device__ __forceinline__ pk2 ld8(const unsigned char* p) { pk2 v; __builtin_memcpy(&v, p, 8); return v; }
__device__ __forceinline__ uint32_t ld4(const unsigned char* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }

extern int g_force_warp_shape, g_force_score_hpw, g_score_exact_only, g_force_warp_frames;   // rwh_api.hip (rwh_lab_tune)

// The element types of image planes, one row each: C++ type, its RWH_* code (rwh.h; a bool plane is RWH_U8) and the name the
// demangled kernel names spell for it.  elem<T>, with_elem and elem_size below are all made from this one list.
// RWH_ELSE marks the type an unknown code reads as in device code, where the code was validated on the host before the launch.
#if defined(__HIP_DEVICE_COMPILE__)
#define RWH_ELSE default:
#else
#define RWH_ELSE
#endif
#define RWH_ELEM_TYPES(X)                                                                                                          \
    X(uint8_t, RWH_U8, "unsigned char", ) X(int8_t, RWH_I8, "signed char", ) X(uint16_t, RWH_U16, "unsigned short", )              \
    X(int16_t, RWH_I16, "short", ) X(int32_t, RWH_I32, "int", ) X(uint32_t, RWH_U32, "unsigned int", ) X(int64_t, RWH_I64, "long", ) \
    X(uint64_t, RWH_U64, "unsigned long", ) X(_Float16, RWH_F16, "_Float16", ) X(float, RWH_F32, "float", )                        \
    X(double, RWH_F64, "double", RWH_ELSE)

template <class T> struct elem;
#define RWH_X(T, CODE, NAME, ELSE) template <> struct elem<T> { static constexpr int dtype = CODE; static constexpr const char* name = NAME; };
RWH_ELEM_TYPES(RWH_X)
#undef RWH_X

// f(T{}, elem<T>::name) with T the element type of `code` (uniform across a launch: a scalar branch in device code).
// false, and f not called: an unknown code, on the host.
template <class F> __host__ __device__ __forceinline__ bool with_elem(int code, F&& f) {
    switch (code) {
#define RWH_X(T, CODE, NAME, ELSE) ELSE case CODE: f(T{}, NAME); return true;
        RWH_ELEM_TYPES(RWH_X)
#undef RWH_X
    }
    return false;
}

// the same for the unsigned integer of `esz` bytes (nearest neighbour copies elements as raw bits)
template <class F> void with_raw(int esz, F&& f) {
    switch (esz) {
        case 1: f(uint8_t{}, elem<uint8_t>::name); break;
        case 2: f(uint16_t{}, elem<uint16_t>::name); break;
        case 4: f(uint32_t{}, elem<uint32_t>::name); break;
        default: f(uint64_t{}, elem<uint64_t>::name); break;
    }
}

// bytes per element of an RWH_U8 .. RWH_F16 code; 0 for an unknown code
inline int elem_size(int code) {
    int n = 0;
    with_elem(code, [&](auto tag, const char*) { n = (int)sizeof(tag); });
    return n;
}

// The extractor's pyramid (include/rwh.h, rule 6): the side of level s (Q8) of an image side n, and the check of a scales table --
// scales[0] == 256, strictly increasing, <= 1024, 1 .. 16 levels.
__host__ __device__ __forceinline__ int orb_level_side(int n, int s) { return (int)((256u * (unsigned)n + (unsigned)s / 2u) / (unsigned)s); }

inline bool orb_scales_ok(const int32_t* scales, int n_levels) {
    if (!scales || n_levels < 1 || n_levels > RWH_ORB_LEVELS_MAX || scales[0] != RWH_ORB_SCALE_ONE) return false;
    for (int l = 1; l < n_levels; ++l)
        if (scales[l] <= scales[l - 1] || scales[l] > RWH_ORB_SCALE_MAX) return false;
    return true;
}

// A fill of device memory enqueued as a kernel; every driver that clears device memory on its stream uses it, none uses
// hipMemsetAsync.  What was observed (tests/test_stream_contract_gpu.py, ROCm 7 under torch, one MI355X): a call captured alone, on
// a side stream, into a torch.cuda.CUDAGraph and replayed through torch left other values in the words its hipMemsetAsync was
// asked to clear -- on the first or second replay, never eagerly -- in seq_stat_device (the slabs), the chunked scorer (the counts)
// and the detector (keys and counts); with this kernel in their place the same records replay to the reference.  The cause
// inside the runtime was not looked for, and nothing is claimed about memset nodes in general.
static __global__ void fill_words_kernel(uint32_t* p, uint32_t v, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

static __global__ void fill_bytes_kernel(uint8_t* p, uint8_t v, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

// `bytes` bytes at p set to `byte` on stream s: whole 32-bit words where p and bytes are multiples of four, else byte by byte.
inline hipError_t fill_async(void* p, int byte, size_t bytes, hipStream_t s) {
    if (bytes == 0) return hipSuccess;
    const bool words = (((uintptr_t)p | bytes) & 3u) == 0;
    const size_t n = words ? bytes / 4 : bytes;
    const unsigned blocks = (unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    if (words) hipLaunchKernelGGL(fill_words_kernel, dim3(blocks), dim3(256), 0, s, static_cast<uint32_t*>(p), 0x01010101u * (uint32_t)(byte & 0xFF), n);
    else hipLaunchKernelGGL(fill_bytes_kernel, dim3(blocks), dim3(256), 0, s, static_cast<uint8_t*>(p), (uint8_t)(byte & 0xFF), n);
    return hipGetLastError();
}

inline int check_launch() {
    return hipGetLastError() == hipSuccess ? RWH_OK : RWH_E_LAUNCH;
}

}  // namespace rwh
