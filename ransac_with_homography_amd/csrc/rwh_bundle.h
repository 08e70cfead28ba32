// rwh_bundle.h: the bundle rule (include/rwh.h) as a rule of csrc/rwh_edge_blocks.h: the arithmetic for one correspondence of one
// edge, written once for the kernel and its host twin (csrc/rwh_bundle.hip).  Everything is float64, no operation is contracted
// beyond the two fma() of each component of p.
#pragma once
#include "rwh_edge_blocks.h"

#pragma clang fp contract(off)

namespace rwh {

struct BundleRule {
    static constexpr int PARAMS = 16;                       // columns of J: delta_s (0 .. 7), delta_d (8 .. 15)
    static constexpr int RECORD = 9;                        // the transfer T, row-major 3 x 3

    // One correspondence a = (x, y) -> b = (bx, by) under the transfer T (row-major 3 x 3): the row's 34 values at out[0 .. 33].
    // Returns false, with out unspecified, for a correspondence that is not valid (p2 not finite or <= 0, or q not finite).
    //   p_i = fma(T[3i+1], y, T[3i] * x) + T[3i+2]      (rounded multiply, fma, fma with w = 1: the k-order of rwh_project_points_ex)
    //   q = (p0 / p2, p1 / p2), r = q - b
    //   column k = 3 rho + c of delta_s: dp = a~[c] * T[:, rho], a~ = (x, y, 1), each product rounded (exact for c = 2)
    //   column k = 3 rho + c of delta_d: dp = -p[c] e_rho
    //   J[0][k] = (dp0 - q0 * dp2) / p2, J[1][k] = (dp1 - q1 * dp2) / p2: product, difference and quotient each rounded.  Where a dp is
    //   an exact zero the operations on it are left out: x - q * 0 = x and 0 - q * 0 = +0 for finite q, so the bits are the same.
    static RWH_HD bool row_values(const double* T, float xf, float yf, float bxf, float byf, double* out) {
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
};

static_assert(rwh_edge::Layout<BundleRule>::BLOCK == RWH_BUNDLE_BLOCK && BundleRule::RECORD == 9, "the block and record of include/rwh.h");

}  // namespace rwh
