// What the two matchers share (rwh_match.hip: cross-check; rwh_match_ratio.hip: the ratio rule over a pair graph): how a descriptor
// row is read and how a row range is taken from an offsets table.
#pragma once
#include "rwh_common.h"

namespace rwh {

static_assert(8 * RWH_MATCH_MAX_BYTES < 65536, "the distance takes the other 16 bits of the 32-bit key");

constexpr unsigned long long MATCH_NONE = ~0ull;

// dword k of descriptor `row` (rows of nbytes bytes, any alignment); bytes past the row's end read as 0 on both sides, so they
// add nothing to a distance
__device__ __forceinline__ uint32_t desc_dword(const unsigned char* __restrict__ desc, long long row, int nbytes, int k) {
    const unsigned char* p = desc + row * nbytes + 4 * k;
    const int left = nbytes - 4 * k;
    if (left >= 4) return ld4(p);
    uint32_t v = 0;
    for (int b = 0; b < left; ++b) v |= (uint32_t)p[b] << (8 * b);
    return v;
}

// rows of problem p on one side, or 0 rows where the offsets table does not describe a range inside [0, total]
__device__ __forceinline__ void match_range(const int32_t* __restrict__ offsets, int p, int total, long long& base, int& n) {
    const long long o0 = offsets[p], o1 = offsets[p + 1];
    const bool ok = o0 >= 0 && o1 >= o0 && o1 <= total;
    base = ok ? o0 : 0;
    n = ok ? (int)(o1 - o0) : 0;
}

}  // namespace rwh
