// rwh_camera.h: the arithmetic of the camera rule (include/rwh.h) for one correspondence of one edge, and the layout of an edge's
// block, written once for the kernel and its host twin (csrc/rwh_camera.hip).  Everything is float64, no operation is contracted
// beyond the fma() written out.
#pragma once
#include <stdint.h>

#include "rwh.h"

#pragma clang fp contract(off)

#ifndef RWH_HD
#define RWH_HD __host__ __device__ __forceinline__
#endif

namespace rwh_camera {

static constexpr int PARAMS = 8;                            // columns of J: omega_s (0 .. 2), phi_s (3), omega_d (4 .. 6), phi_d (7)
static constexpr int ROW = 2 * PARAMS + 2;                  // J[0][0 .. 7], J[1][0 .. 7], r0, r1
static constexpr int N_S = PARAMS * (PARAMS + 1) / 2;       // 36: upper triangle of S, row-major
static constexpr int BLOCK = RWH_CAMERA_BLOCK;              // 45 = 36 + 8 + 1
static constexpr int RECORD = RWH_CAMERA_RECORD;            // 15: R (9, row-major), f_s, cx_s, cy_s, f_d, cx_d, cy_d
static constexpr int PARTIALS = 4;                          // partial sums over rows with index = 0, 1, 2, 3 (mod 4)
static constexpr int CHUNK = 128;                           // rows the kernel stages in LDS at a time (a multiple of PARTIALS)
static constexpr int THREADS = 64 * PARTIALS;               // one wave per partial
static constexpr int STRIDE = ROW + 1;                      // doubles per staged row: 19, odd, so that 16 lanes' 8-byte stores meet no bank twice

static_assert(BLOCK == N_S + PARAMS + 1 && BLOCK <= 64, "one lane of a wave per block entry");

// One correspondence a = (x, y) -> b = (bx, by) under the edge record E: the row's 18 values at out[0 .. 17].  Returns false, with
// out unspecified, for a correspondence that is not valid (v2 not finite or <= 0, or q not finite).  The operations, each rounded
// once, in the order of the camera rule:
//   u = (x - cx_s, y - cy_s, f_s)
//   v_i = fma(R[i][2], u2, fma(R[i][1], u1, R[i][0] * u0))
//   m = (v0 / v2, v1 / v2), q = (fma(f_d, m0, cx_d), fma(f_d, m1, cy_d)), r = q - b
//   dv of omega_s,0: fma(R[i][2], u1, R[i][1] * -u2); omega_s,1: fma(R[i][2], -u0, R[i][0] * u2); omega_s,2: fma(R[i][1], u0,
//   R[i][0] * -u1); phi_s: R[i][2] * u2; omega_d,0: (0, v2, -v1); omega_d,1: (-v2, 0, v0); omega_d,2: (v1, -v0, 0)
//   J[c][k] = (f_d * (dv_c - m_c * dv2)) / v2 for these seven columns, the zeros taken as +0.0 like any other operand
//   J[c][7] = f_d * m_c
RWH_HD bool row_values(const double* E, float xf, float yf, float bxf, float byf, double* out) {
    const double fs = E[9], fd = E[12];
    const double u0 = (double)xf - E[10], u1 = (double)yf - E[11], u2 = fs;
    double v[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = fma(E[3 * i + 2], u2, fma(E[3 * i + 1], u1, E[3 * i] * u0));
    const double m0 = v[0] / v[2], m1 = v[1] / v[2];
    const double q0 = fma(fd, m0, E[13]), q1 = fma(fd, m1, E[14]);
    if (!(__builtin_isfinite(v[2]) && v[2] > 0.0 && __builtin_isfinite(q0) && __builtin_isfinite(q1))) return false;
    double dv[7][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        dv[0][i] = fma(E[3 * i + 2], u1, E[3 * i + 1] * -u2);
        dv[1][i] = fma(E[3 * i + 2], -u0, E[3 * i] * u2);
        dv[2][i] = fma(E[3 * i + 1], u0, E[3 * i] * -u1);
        dv[3][i] = E[3 * i + 2] * u2;
    }
    dv[4][0] = 0.0;   dv[4][1] = v[2];  dv[4][2] = -v[1];
    dv[5][0] = -v[2]; dv[5][1] = 0.0;   dv[5][2] = v[0];
    dv[6][0] = v[1];  dv[6][1] = -v[0]; dv[6][2] = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        out[k] = (fd * (dv[k][0] - m0 * dv[k][2])) / v[2];
        out[PARAMS + k] = (fd * (dv[k][1] - m1 * dv[k][2])) / v[2];
    }
    out[7] = fd * m0;
    out[PARAMS + 7] = fd * m1;
    out[2 * PARAMS] = q0 - (double)bxf;
    out[2 * PARAMS + 1] = q1 - (double)byf;
    return true;
}

// Entry e of a block is the sum over the edge's rows of row[i0] * row[j0] + row[i1] * row[j1]:
//   e < 36: S[a][b], a <= b, row-major upper triangle: J[0][a] J[0][b] + J[1][a] J[1][b]
//   36 <= e < 44: g[k], k = e - 36: J[0][k] r0 + J[1][k] r1
//   e == 44: c = r0 r0 + r1 r1
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

}  // namespace rwh_camera
