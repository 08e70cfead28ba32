// rwh_bundle.h: the arithmetic of the bundle rule (include/rwh.h) for one correspondence of one edge, and the layout of an edge's
// block, written once for the kernel and its host twin (csrc/rwh_bundle.hip).  Everything is float64, no operation is contracted
// beyond the two fma() of each component of p.
#pragma once
#include <stdint.h>

#include "rwh.h"

#pragma clang fp contract(off)

#ifndef RWH_HD
#define RWH_HD __host__ __device__ __forceinline__
#endif

namespace rwh_bundle {

static constexpr int PARAMS = 16;                           // columns of J: delta_s (0 .. 7), delta_d (8 .. 15)
static constexpr int ROW = 2 * PARAMS + 2;                  // J[0][0 .. 15], J[1][0 .. 15], r0, r1
static constexpr int N_S = PARAMS * (PARAMS + 1) / 2;       // 136: upper triangle of S, row-major
static constexpr int BLOCK = RWH_BUNDLE_BLOCK;              // 153 = 136 + 16 + 1
static constexpr int PARTIALS = 4;                          // partial sums over rows with index = 0, 1, 2, 3 (mod 4)
static constexpr int CHUNK = 128;                           // rows the kernel stages in LDS at a time (a multiple of PARTIALS)
static constexpr int THREADS = 64 * PARTIALS;               // one wave per partial
static constexpr int STRIDE = ROW + 1;                      // doubles per staged row: 35, so that 16 lanes' 8-byte stores meet no bank twice

// One correspondence a = (x, y) -> b = (bx, by) under the transfer T (row-major 3 x 3): the row's 34 values at out[0 .. 33].
// Returns false, with out unspecified, for a correspondence that is not valid (p2 not finite or <= 0, or q not finite).
//   p_i = fma(T[3i+1], y, T[3i] * x) + T[3i+2]      (rounded multiply, fma, fma with w = 1: the k-order of rwh_project_points_ex)
//   q = (p0 / p2, p1 / p2), r = q - b
//   column k = 3 rho + c of delta_s: dp = a~[c] * T[:, rho], a~ = (x, y, 1), each product rounded (exact for c = 2)
//   column k = 3 rho + c of delta_d: dp = -p[c] e_rho
//   J[0][k] = (dp0 - q0 * dp2) / p2, J[1][k] = (dp1 - q1 * dp2) / p2: product, difference and quotient each rounded.  Where a dp is
//   an exact zero the operations on it are left out: x - q * 0 = x and 0 - q * 0 = +0 for finite q, so the bits are the same.
RWH_HD bool row_values(const double* T, float xf, float yf, float bxf, float byf, double* out) {
    const double at[3] = {(double)xf, (double)yf, 1.0};
    double p[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = fma(T[3 * i + 1], at[1], T[3 * i] * at[0]) + T[3 * i + 2];
    const double q0 = p[0] / p[2], q1 = p[1] / p[2];
    if (!(__builtin_isfinite(p[2]) && p[2] > 0.0 && __builtin_isfinite(q0) && __builtin_isfinite(q1))) return false;
#pragma unroll
    for (int rho = 0; rho < 3; ++rho)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int k = 3 * rho + c;
            if (k >= 8) continue;
            const double dp0 = c == 2 ? T[rho] : at[c] * T[rho], dp1 = c == 2 ? T[3 + rho] : at[c] * T[3 + rho];
            const double dp2 = c == 2 ? T[6 + rho] : at[c] * T[6 + rho];
            out[k] = (dp0 - q0 * dp2) / p[2];
            out[PARAMS + k] = (dp1 - q1 * dp2) / p[2];
            const double m = -p[c];
            out[8 + k] = rho == 0 ? m / p[2] : rho == 1 ? 0.0 : (0.0 - q0 * m) / p[2];
            out[PARAMS + 8 + k] = rho == 0 ? 0.0 : rho == 1 ? m / p[2] : (0.0 - q1 * m) / p[2];
        }
    out[2 * PARAMS] = q0 - (double)bxf;
    out[2 * PARAMS + 1] = q1 - (double)byf;
    return true;
}

// Entry e of a block is the sum over the edge's rows of row[i0] * row[j0] + row[i1] * row[j1]:
//   e < 136: S[a][b], a <= b, row-major upper triangle: J[0][a] J[0][b] + J[1][a] J[1][b]
//   136 <= e < 152: g[k], k = e - 136: J[0][k] r0 + J[1][k] r1
//   e == 152: c = r0 r0 + r1 r1
struct Entry { int i0, j0, i1, j1; };

RWH_HD Entry entry_of(int e) {
    if (e >= N_S + PARAMS) return {2 * PARAMS, 2 * PARAMS, 2 * PARAMS + 1, 2 * PARAMS + 1};
    if (e >= N_S) return {e - N_S, 2 * PARAMS, PARAMS + e - N_S, 2 * PARAMS + 1};
    int a = 0, left = e;
    while (left >= PARAMS - a) { left -= PARAMS - a; ++a; }
    return {a, a + left, PARAMS + a, PARAMS + a + left};
}

// one step of an accumulator: both products rounded, their sum rounded, then the addition
RWH_HD double step(double acc, const double* row, const Entry& t) {
    return acc + (row[t.i0] * row[t.j0] + row[t.i1] * row[t.j1]);
}

}  // namespace rwh_bundle
