// mfx_normals.h — smooth shading (mfx_set_normals): the normal record of a primitive and the shading normal
// of a hit point, one statement shared by the host (mfx_set_normals, mfx_normal_table, mfx_shading_normal)
// and the gfx950 kernels (k_shadow, k_aov). The rule is the contract in include/mafrix_rt.h;
// mafrixraytracing_amd/normals.py states it in Python floats.
//
// FP64, one rounding per operation in the order written (every file that includes this is compiled
// with -ffp-contract=off), + - * / sqrt only, so the host and the device give the same bits.
#ifndef MFX_NORMALS_H
#define MFX_NORMALS_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MFX_SN_HD __host__ __device__ __forceinline__
#else
#define MFX_SN_HD inline
#endif

#define MFX_SN_RECORD_DOUBLES 12  // g_0[3], k_0, g_1[3], k_1, g_2[3], k_2

// The device tables of a context with normals (WfParams::sn, AovParams::sn; both null without).
struct MfxSnTables {
    const double* rec;    // [world primitives][12] the normal records
    const int32_t* flag;  // [world primitives] 1: a smooth primitive, 0: it keeps its face normal
};

MFX_SN_HD double mfx_sn_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// finite and > 0 (a NaN fails both comparisons)
MFX_SN_HD bool mfx_sn_length_ok(double l) { return l > 0.0 && l <= 1.7976931348623157e308; }

// The shading normal at hit point hp of a smooth primitive with record r, whose vertex has the normal ng today:
// the interpolated normal normalized (ng itself where it has no length), on ng's side.
MFX_SN_HD void mfx_sn_shade(const double* r, const double* hp, const double* ng, double* ns) {
    const double r0 = mfx_sn_dot(hp, r) + r[3];
    const double r1 = mfx_sn_dot(hp, r + 4) + r[7];
    const double r2 = mfx_sn_dot(hp, r + 8) + r[11];
    const double l = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
    if (mfx_sn_length_ok(l)) {
        ns[0] = r0 / l;
        ns[1] = r1 / l;
        ns[2] = r2 / l;
    } else {
        ns[0] = ng[0];
        ns[1] = ng[1];
        ns[2] = ng[2];
    }
    if (mfx_sn_dot(ns, ng) < 0.0) {
        ns[0] = -ns[0];
        ns[1] = -ns[1];
        ns[2] = -ns[2];
    }
}

// The normal record of a primitive with world corners v0, v1, v2 and their normals n[0..2]: per component c,
// out[4c .. 4c+3] = g_c[3], k_c, so that component c of the interpolated normal is dot(p, g_c) + k_c on the
// primitive's plane (the UV record's affine solve, mfx_texture.h). A degenerate primitive (det == 0, or a value
// that is not finite) gets 0,0,0,n[0][c]: its first corner's normal.
inline void mfx_sn_record(const double v0[3], const double v1[3], const double v2[3], const double n[3][3], double out[12]) {
    double e1[3], e2[3];
    for (int c = 0; c < 3; ++c) {
        e1[c] = v1[c] - v0[c];
        e2[c] = v2[c] - v0[c];
    }
    const double d11 = mfx_sn_dot(e1, e1), d12 = mfx_sn_dot(e1, e2), d22 = mfx_sn_dot(e2, e2);
    const double det = d11 * d22 - d12 * d12;
    bool ok = det != 0.0;
    for (int c = 0; c < 3; ++c) {
        const double w0 = n[0][c], w1 = n[1][c], w2 = n[2][c];
        const double dw1 = w1 - w0, dw2 = w2 - w0;
        const double a = (d22 * dw1 - d12 * dw2) / det;
        const double b = (d11 * dw2 - d12 * dw1) / det;
        double* g = out + 4 * c;
        for (int k = 0; k < 3; ++k) g[k] = e1[k] * a + e2[k] * b;
        g[3] = w0 - mfx_sn_dot(v0, g);
        for (int k = 0; k < 4; ++k) ok = ok && isfinite(g[k]);
    }
    if (!ok)
        for (int c = 0; c < 3; ++c) {
            double* g = out + 4 * c;
            g[0] = g[1] = g[2] = 0.0;
            g[3] = n[0][c];
        }
}

#endif
