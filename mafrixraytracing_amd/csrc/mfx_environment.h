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

// ---- the sky as a light (mfx_set_environment_sampled): the sampling table and the direction rule -----------
// One entry per texel, 16 B: the alias pair of entry k (q, alias) and the probability prob of texel k that the
// whole table implies. A sky vertex reads entry k for its pick and entry t for its pdf.
struct MfxSkyEntry {
    float q;         // in [0, 1]: draw r2 < q returns k, otherwise alias
    uint32_t alias;
    double prob;     // (q_t + sum over k != t with alias[k] == t of (1 - q_k)) / n, in increasing k
};
static_assert(sizeof(MfxSkyEntry) == 16, "MfxSkyEntry: 16 B a texel");

// the extension ray's far bound (Integrators.fs:108): the sky's shadow query ends there too
#define MFX_ENV_FAR 99999999.

// The direction of (texel t, jitter ju, jv) in a size x size map, the inverse of mfx_env_texel: out = the unit
// direction, len2 and len of the unnormalised point (the pdf's Jacobian factor is len2 * len).
MFX_ENV_HD void mfx_env_sample_dir(uint32_t t, double ju, double jv, int size, double out[3], double& len2, double& len) {
    const int xi = (int)(t % (uint32_t)size), yi = (int)(t / (uint32_t)size);
    const double u = ((double)xi + ju) / (double)size, a = u * 2.0 - 1.0;
    const double v = ((double)yi + jv) / (double)size, b = v * 2.0 - 1.0;
    const double py = (1.0 - fabs(a)) - fabs(b);
    double px = a, pz = b;
    if (!((fabs(a) + fabs(b)) <= 1.0)) {
        px = (1.0 - fabs(b)) * mfx_env_sg(a);
        pz = (1.0 - fabs(a)) * mfx_env_sg(b);
    }
    len2 = (px * px + py * py) + pz * pz;
    len = sqrt(len2);
    out[0] = px / len;
    out[1] = py / len;
    out[2] = pz / len;
}

// the entry index of draw r1 among n entries: floor(r1 * n) clamped into [0, n - 1]
MFX_ENV_HD uint32_t mfx_env_sample_entry(double r1, uint32_t n) {
    const double f = floor(r1 * (double)n);
    return !(f >= 0.0) ? 0u : (f >= (double)n ? n - 1u : (uint32_t)f);
}

// pdf_v of a sky vertex: (((prob * n) * 0.25) * (len2 * len)) / (N + 1)
MFX_ENV_HD double mfx_env_sample_pdf(double prob, int size, double len2, double len, int nlights) {
    return (((prob * (double)(size * size)) * 0.25) * (len2 * len)) / (double)(nlights + 1);
}

#endif
