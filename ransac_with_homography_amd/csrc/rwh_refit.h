// rwh_refit.h: the arithmetic of the N-point refit (rwh_refit_batched / rwh_host_refit, csrc/rwh_refit.hip), written once for the
// kernel and its host twin.  The least-squares problem is the reference's (calc_correspLinearCollective, homography.py:48-69:
// two rows per correspondence, h33 == 1), solved by float64 normal equations instead of the reference's float32 ones:
//   row 1 = [x, y, 1, 0, 0, 0, -x x', -y x' | x'],  row 2 = [0, 0, 0, x, y, 1, -x y', -y y' | y'],
// every entry a float32 input or the float64 product of two of them (exact: 24 + 24 bits).  A^T A is symmetric with two equal
// 3 x 3 blocks and a zero block, so A^T A and A^T b together are N_MOMENTS = 23 distinct sums.
// The normal equations alone lose the square of cond(A): with G the equilibrated A^T A their relative error is of the order of
// 2^-53 |G^-1|, on four inliers of a narrow strip far from the origin 1e-4 px, more than an SVD of A loses.  Where they may have
// lost more than half of the 53 bits -- trace(G^-1) >= CORRECT_ABOVE = 2^27; the trace is |G^-1|_2 to within a factor 8 and comes
// from the Cholesky factor -- the solution is corrected once (Bjorck's corrected normal equations): the residual b - A h is taken
// from the correspondences themselves, its N_RESIDUALS = 8 sums A^T (b - A h) go through the factor already at hand, and the
// result is added to h; the error left is of the order of cond(A) 2^-53, not its square.  Below the threshold the first solution
// stands, and the second pass over the correspondences is not made.
#pragma once
#include <stdint.h>

#include "rwh.h"

#pragma clang fp contract(off)

#define RWH_HD __host__ __device__ __forceinline__

namespace rwh_refit {

static constexpr int N_MOMENTS = 23;
static constexpr int N_RESIDUALS = 8;
static constexpr int THREADS = 256;     // lanes of one problem's workgroup; the host twin sums in the same 256 strided partials
static constexpr int WAVES = THREADS / 64;

// moment indices, with a = x x', b = y x', c = x y', d = y y':
//   0 xx  1 xy  2 x  3 yy  4 y  5 n            6 x a  7 x b  8 y b  9 a  10 b          11 x c  12 x d  13 y d  14 c  15 d
//   16 aa + cc  17 ab + cd  18 bb + dd         19 x'  20 y'  21 a x' + c y'  22 b x' + d y'
RWH_HD void moment_update(double* s, float xf, float yf, float xpf, float ypf) {
    const double x = xf, y = yf, xp = xpf, yp = ypf;
    const double a = x * xp, b = y * xp, c = x * yp, d = y * yp;
    s[0] += x * x;  s[1] += x * y;  s[2] += x;  s[3] += y * y;  s[4] += y;  s[5] += 1.0;
    s[6] += x * a;  s[7] += x * b;  s[8] += y * b;  s[9] += a;  s[10] += b;
    s[11] += x * c; s[12] += x * d; s[13] += y * d; s[14] += c; s[15] += d;
    s[16] += a * a + c * c;  s[17] += a * b + c * d;  s[18] += b * b + d * d;
    s[19] += xp;  s[20] += yp;  s[21] += a * xp + c * yp;  s[22] += b * xp + d * yp;
}

// t += A^T (b - A h) of one correspondence, h = the eight unknowns of a solution with h33 == 1
RWH_HD void residual_update(double* t, const double* h, float xf, float yf, float xpf, float ypf) {
    const double x = xf, y = yf, xp = xpf, yp = ypf;
    const double a = x * xp, b = y * xp, c = x * yp, d = y * yp;
    const double r1 = xp - ((((x * h[0] + y * h[1]) + h[2]) - a * h[6]) - b * h[7]);
    const double r2 = yp - ((((x * h[3] + y * h[4]) + h[5]) - c * h[6]) - d * h[7]);
    t[0] += x * r1;  t[1] += y * r1;  t[2] += r1;  t[3] += x * r2;  t[4] += y * r2;  t[5] += r2;
    t[6] -= a * r1 + c * r2;  t[7] -= b * r1 + d * r2;
}

// what solve() leaves for correct(): L (lower triangle) of the equilibrated A^T A, and the equilibration D
struct Factor {
    double l[8][8], dd[8];
};

static constexpr double CORRECT_ABOVE = 134217728.0;    // 2^27

// trace(G^-1) = |L^-1|_F^2 for G = L L^T: L^-1 column by column
RWH_HD double inverse_trace(const Factor& f) {
    double sum = 0.0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        double x[8];
#pragma unroll
        for (int i = c; i < 8; ++i) {
            double v = i == c ? 1.0 : 0.0;
#pragma unroll
            for (int k = c; k < i; ++k) v -= f.l[i][k] * x[k];
            x[i] = v / f.l[i][i];
            sum += x[i] * x[i];
        }
    }
    return sum;
}

RWH_HD void fill_nan(double* h9) {
    for (int i = 0; i < 9; ++i) h9[i] = __builtin_nan("");
}

// The 8 x 8 solve of (A^T A) h = A^T b from the moments: symmetric diagonal equilibration (G -> D G D with D = diag(G)^-1/2: unit
// diagonal, the solution D^-1 h of the scaled system scaled back, so h is unchanged in exact arithmetic), Cholesky, two triangular
// solves.  h9 = row-major 3 x 3 with h9[8] == 1.  Returns RWH_REFIT_OK, RWH_REFIT_FEW (fewer than 4 inliers) or RWH_REFIT_SINGULAR
// (a diagonal entry or Cholesky pivot that is not a positive finite number, or a non-finite solution); h9 is all NaN unless OK.
// f holds the factor when the status is OK.
RWH_HD int solve(const double* s, Factor& f, double* h9) {
    if (!(s[5] >= 4.0)) { fill_nan(h9); return RWH_REFIT_FEW; }
    double (&g)[8][8] = f.l;
    double (&dd)[8] = f.dd;
    double r[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) g[i][j] = 0.0;
    g[0][0] = g[3][3] = s[0];  g[1][0] = g[4][3] = s[1];  g[2][0] = g[5][3] = s[2];      // lower triangle only
    g[1][1] = g[4][4] = s[3];  g[2][1] = g[5][4] = s[4];  g[2][2] = g[5][5] = s[5];
    g[6][0] = -s[6];   g[7][0] = -s[7];   g[6][1] = -s[7];   g[7][1] = -s[8];   g[6][2] = -s[9];   g[7][2] = -s[10];
    g[6][3] = -s[11];  g[7][3] = -s[12];  g[6][4] = -s[12];  g[7][4] = -s[13];  g[6][5] = -s[14];  g[7][5] = -s[15];
    g[6][6] = s[16];   g[7][6] = s[17];   g[7][7] = s[18];
    r[0] = s[9];  r[1] = s[10];  r[2] = s[19];  r[3] = s[14];  r[4] = s[15];  r[5] = s[20];  r[6] = -s[21];  r[7] = -s[22];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        ok = ok && g[i][i] > 0.0 && __builtin_isfinite(g[i][i]);
        dd[i] = 1.0 / __builtin_sqrt(g[i][i]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        r[i] *= dd[i];
#pragma unroll
        for (int j = 0; j <= i; ++j) g[i][j] = (g[i][j] * dd[i]) * dd[j];
    }
    // Cholesky, column by column: g becomes L (lower triangle)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        double piv = g[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) piv -= g[j][k] * g[j][k];
        ok = ok && piv > 0.0 && __builtin_isfinite(piv);
        const double l = __builtin_sqrt(piv);
        g[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < 8; ++i) {
            double v = g[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= g[i][k] * g[j][k];
            g[i][j] = v / l;
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {       // L z = r
        double v = r[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= g[i][k] * r[k];
        r[i] = v / g[i][i];
    }
#pragma unroll
    for (int i = 7; i >= 0; --i) {      // L^T y = z
        double v = r[i];
#pragma unroll
        for (int k = i + 1; k < 8; ++k) v -= g[k][i] * r[k];
        r[i] = v / g[i][i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        r[i] *= dd[i];
        ok = ok && __builtin_isfinite(r[i]);
    }
    if (!ok) { fill_nan(h9); return RWH_REFIT_SINGULAR; }
#pragma unroll
    for (int i = 0; i < 8; ++i) h9[i] = r[i];
    h9[8] = 1.0;
    return RWH_REFIT_OK;
}

// The corrected step: h9 += D L^-T L^-1 D t for t = A^T (b - A h9) summed over the inliers (residual_update).  Returns
// RWH_REFIT_OK, or RWH_REFIT_SINGULAR with h9 all NaN when the corrected solution is not finite.
RWH_HD int correct(const Factor& f, const double* t, double* h9) {
    double r[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {       // L z = D t
        double v = t[i] * f.dd[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= f.l[i][k] * r[k];
        r[i] = v / f.l[i][i];
    }
#pragma unroll
    for (int i = 7; i >= 0; --i) {      // L^T y = z
        double v = r[i];
#pragma unroll
        for (int k = i + 1; k < 8; ++k) v -= f.l[k][i] * r[k];
        r[i] = v / f.l[i][i];
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        h9[i] += r[i] * f.dd[i];
        ok = ok && __builtin_isfinite(h9[i]);
    }
    if (!ok) { fill_nan(h9); return RWH_REFIT_SINGULAR; }
    return RWH_REFIT_OK;
}

// lane 0's value of the wave's shuffle-down tree (offsets 32, 16, .. 1) over v[0 .. 63], as the kernel computes it
inline double wave_tree(double* v) {
    for (int off = 32; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l) v[l] += v[l + off];
    return v[0];
}

}  // namespace rwh_refit
