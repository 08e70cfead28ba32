// rwh_camera.h: the camera rule (include/rwh.h) as a rule of csrc/rwh_edge_blocks.h: the arithmetic for one correspondence of one
// edge, written once for the kernel and its host twin (csrc/rwh_camera.hip).  Everything is float64, no operation is contracted
// beyond the fma() written out.
#pragma once
#include "rwh_edge_blocks.h"

#pragma clang fp contract(off)

namespace rwh {

struct CameraRule {
    static constexpr int PARAMS = 8;                        // columns of J: omega_s (0 .. 2), phi_s (3), omega_d (4 .. 6), phi_d (7)
    static constexpr int RECORD = 15;                       // R (9, row-major), f_s, cx_s, cy_s, f_d, cx_d, cy_d

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
    static RWH_HD bool row_values(const double* E, float xf, float yf, float bxf, float byf, double* out) {
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
};

static_assert(rwh_edge::Layout<CameraRule>::BLOCK == RWH_CAMERA_BLOCK && CameraRule::RECORD == RWH_CAMERA_RECORD,
              "the block and record of include/rwh.h");

}  // namespace rwh
