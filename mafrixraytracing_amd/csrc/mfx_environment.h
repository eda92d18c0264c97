// mfx_environment.h — the sky (mfx_set_environment): the texel of a ray direction in a square octahedral
// map, one statement shared by the host (mfx_env_texel_index) and the gfx950 kernels (k_extend, k_camera,
// k_resolve). The rule is the contract in include/mafrix_rt.h; mafrixraytracing_amd/environment.py states it
// in Python floats.
//
// FP64, one rounding per operation in the order written (every file that includes this is compiled
// with -ffp-contract=off), + - * / abs floor and comparisons only, so the host and the device give the
// same bits. +y is the pole (the camera's up).
#ifndef MFX_ENVIRONMENT_H
#define MFX_ENVIRONMENT_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MFX_ENV_HD __host__ __device__ __forceinline__
#else
#define MFX_ENV_HD inline
#endif

#define MFX_ENV_SIZE_MAX 4096        // MFX_MAX_ENV_SIZE: size * size <= 2^24, so a texel id is 24 bits
#define MFX_ENV_NONE 0xFFFFFFFFu     // a path slot's miss record when its path did not end in a miss
#define MFX_ENV_ID_MASK 0x00FFFFFFu  // the record of a miss: texel id | vertices before the miss << 24
#define MFX_ENV_NV_SHIFT 24

MFX_ENV_HD double mfx_env_sg(double x) { return x >= 0.0 ? 1.0 : -1.0; }

// floor(w * n) clamped into [0, n - 1]
MFX_ENV_HD int mfx_env_coord(double w, int n) {
    const double f = floor(w * (double)n);
    return !(f >= 0.0) ? 0 : (f >= (double)n ? n - 1 : (int)f);
}

// the texel of unit direction (dx, dy, dz) in a size x size map
MFX_ENV_HD uint32_t mfx_env_texel(double dx, double dy, double dz, int size) {
    const double s = (fabs(dx) + fabs(dy)) + fabs(dz);
    const double px = dx / s, pz = dz / s;
    double a = px, b = pz;
    if (!(dy >= 0.0)) {  // the lower half folds outwards
        a = (1.0 - fabs(pz)) * mfx_env_sg(px);
        b = (1.0 - fabs(px)) * mfx_env_sg(pz);
    }
    const double u = a * 0.5 + 0.5, v = b * 0.5 + 0.5;
    const int xi = mfx_env_coord(u, size), yi = mfx_env_coord(v, size);
    return (uint32_t)(yi * size + xi);
}

#endif
