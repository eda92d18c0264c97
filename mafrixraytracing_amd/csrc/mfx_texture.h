// mfx_texture.h — albedo textures (mfx_create_textured): the UV record of a primitive, the texel rule and
// the albedo of a textured vertex, one statement shared by the host (creation, mfx_uv_table,
// mfx_texel_index) and the gfx950 kernels (k_shadow, k_resolve, k_aov). The rule is the contract in
// include/mafrix_rt.h; mafrixraytracing_amd/textures.py states it in Python floats.
//
// FP64, one rounding per operation in the order written (every file that includes this is compiled
// with -ffp-contract=off), + - * / floor only, so the host and the device give the same bits.
#ifndef MFX_TEXTURE_H
#define MFX_TEXTURE_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MFX_TX_HD __host__ __device__ __forceinline__
#else
#define MFX_TX_HD inline
#endif

#define MFX_TEXEL_NONE 0xFFFFFFFFu  // a path vertex's texel id on an untextured primitive
#define MFX_TEX_DIM_MAX 16384       // a texture's width and height at most
#define MFX_TEX_COUNT_MAX 4096      // textures of a context at most
#define MFX_TEXELS_MAX 0x7FFFFFFEll // texels of a context at most: 2^31 - 2 (an id is below MFX_TEXEL_NONE in 32 bits)
#define MFX_UV_RECORD_DOUBLES 8     // gu[3], cu, gv[3], cv

// one texture of the concatenated texel array: its first texel, width and height
struct MfxTexDesc {
    int32_t base, width, height, pad;
};

// The device tables of a textured context (WfParams::tx, AovParams::tx; all null without textures).
struct MfxTexTables {
    const double* uvrec;     // [world primitives][8] the UV records
    const int32_t* ptex;     // [world primitives] the primitive's texture, -1: untextured
    const MfxTexDesc* desc;  // [textures]
    const uint32_t* texels;  // the textures' RGBA8 texels, rows top to bottom, one after the other
};

MFX_TX_HD double mfx_tx_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// floor((w - floor(w)) * n) clamped into [0, n - 1] (w - floor(w) is exactly 1.0 for a tiny negative w)
MFX_TX_HD int mfx_tx_coord(double w, int n) {
    const double t = w - floor(w);
    const double f = floor(t * (double)n);
    return !(f >= 0.0) ? 0 : (f >= (double)n ? n - 1 : (int)f);
}

// the texel of (u, v) in texture d: OBJ's v points up, rows run top to bottom
MFX_TX_HD uint32_t mfx_tx_texel(const MfxTexDesc& d, double u, double v) {
    const int xi = mfx_tx_coord(u, d.width), yi = mfx_tx_coord(v, d.height);
    const int row = (d.height - 1) - yi;
    return (uint32_t)(d.base + row * d.width + xi);
}

// (u, v) of hit point hp under UV record r
MFX_TX_HD void mfx_tx_uv(const double* r, const double* hp, double& u, double& v) {
    u = mfx_tx_dot(hp, r) + r[3];
    v = mfx_tx_dot(hp, r + 4) + r[7];
}

// one channel of the albedo at a textured vertex: albedo * (byte / 255); a 255 byte gives albedo itself
MFX_TX_HD double mfx_tx_albedo(double albedo, uint32_t texel, int c) {
    return albedo * ((double)((texel >> (8 * c)) & 0xffu) / 255.0);
}

// The UV record of a primitive with world corners v0, v1, v2 and their (u, v): out = gu[3], cu, gv[3], cv,
// so that u = dot(p, gu) + cu on the primitive's plane. A degenerate primitive (det == 0, or a value that
// is not finite) gets 0,0,0,u0, 0,0,0,v0: the texel of its first corner.
inline void mfx_tx_record(const double v0[3], const double v1[3], const double v2[3], const double uv[3][2], double out[8]) {
    double e1[3], e2[3];
    for (int c = 0; c < 3; ++c) {
        e1[c] = v1[c] - v0[c];
        e2[c] = v2[c] - v0[c];
    }
    const double d11 = mfx_tx_dot(e1, e1), d12 = mfx_tx_dot(e1, e2), d22 = mfx_tx_dot(e2, e2);
    const double det = d11 * d22 - d12 * d12;
    bool ok = det != 0.0;
    for (int k = 0; k < 2; ++k) {
        const double w0 = uv[0][k], w1 = uv[1][k], w2 = uv[2][k];
        const double dw1 = w1 - w0, dw2 = w2 - w0;
        const double a = (d22 * dw1 - d12 * dw2) / det;
        const double b = (d11 * dw2 - d12 * dw1) / det;
        double* g = out + 4 * k;
        for (int c = 0; c < 3; ++c) g[c] = e1[c] * a + e2[c] * b;
        g[3] = w0 - mfx_tx_dot(v0, g);
        for (int c = 0; c < 4; ++c) ok = ok && isfinite(g[c]);
    }
    if (!ok) {
        for (int c = 0; c < 8; ++c) out[c] = 0.0;
        out[3] = uv[0][0];
        out[7] = uv[0][1];
    }
}

#endif
