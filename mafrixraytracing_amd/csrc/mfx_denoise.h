// mfx_denoise.h — parameter blocks and launchers of the feature-buffer and denoising kernels
// (mfx_denoise.hip: mfx_aov, mfx_denoise, mfx_denoise_var). A translation unit of its own, so the trace kernels' code
// objects do not change with it.
#ifndef MFX_DENOISE_H
#define MFX_DENOISE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfx_layout.h"
#include "mfx_lens.h"
#include "mfx_normals.h"
#include "mfx_texture.h"

#define MFX_AOV_PLANES 8  // normal xyz, hit t, albedo rgb, hit fraction

// k_aov: the first hit of the film's own camera rays, averaged over a sample range
struct AovParams {
    const MfxNode* nodes;
    const MfxSlot* slots;
    const int32_t* slot_ref;
    const uint8_t* ref_blob;
    const MfxShade* shade;
    const MfxInstance* inst;  // two-level scenes (null for a flat scene)
    double tslack;            // MfxHostScene::tslack (SceneView::tslack)
    MfxCamera cam;            // by value: scalar-loaded
    uint64_t seed;
    int64_t sample_base;      // first global sample
    int32_t spp;
    int32_t width, height;
    int32_t stack_size;       // LDS traversal stack entries per lane
    double* feat;             // [MFX_AOV_PLANES][w*h], x-major pixels
    double* out;              // null, or [w*h][MFX_AOV_PLANES] (the caller's layout)
    MfxTexTables tx;          // albedo textures (all null without: the untextured instances run)
    MfxLensRec lens;          // a thin lens (mfx_set_lens; lens_on runs the LENS instances: the film's own lens rays)
    int32_t lens_on;
    MfxSnTables sn;           // smooth shading (mfx_set_normals; both null without: the instances without run)
};

// k_atrous: one iteration of the edge-avoiding a-trous filter (the rule: include/mafrix_rt.h)
struct AtrousParams {
    const double* src;   // [3][w*h] the current colour
    double* dst;         // [3][w*h] the iteration's output
    const double* feat;  // [MFX_AOV_PLANES][w*h]
    int32_t width, height;
    int32_t step;        // 2^i
    int32_t terms;       // bit 0 normal, 1 depth, 2 albedo, 3 colour: the terms whose sigma is > 0
    double sn2, sz2, sa2;  // sigma * sigma
    double sc2;            // (sigma_color * sigma_color) * 0.25^i
};

// k_atrous_var: one iteration of the variance-guided filter (mfx_denoise_var; the rule: include/mafrix_rt.h)
struct AtrousVarParams {
    const double* src;   // [3][w*h] the current colour
    const double* vsrc;  // [w*h] the current variance of the pixel's mean luminance
    double* dst;         // [3][w*h] the iteration's colour
    double* vdst;        // [w*h] and its variance
    const double* feat;  // [MFX_AOV_PLANES][w*h]
    int32_t width, height;
    int32_t step;        // 2^i
    int32_t terms;       // bit 0 normal, 1 depth, 2 albedo, 3 luminance: the terms whose sigma is > 0
    double sn2, sz2, sa2;  // sigma * sigma
    double sl2;            // sigma_luma * sigma_luma
    double luma_floor;
};

// A temporal history buffer's planes ([MFX_TP_PLANES][w*h], x-major pixels): the merged colour, the
// variance of its mean luminance, its effective sample count, and the features of the view it was
// merged in (normal, depth, hit fraction). Colour first, so the three planes are an a-trous source.
#define MFX_TP_COLOR 0
#define MFX_TP_VAR 3
#define MFX_TP_COUNT 4
#define MFX_TP_NORMAL 5
#define MFX_TP_DEPTH 8
#define MFX_TP_HIT 9
#define MFX_TP_PLANES 10

// k_temporal: reproject the history into the current view and merge (mfx_temporal; the rule: include/mafrix_rt.h)
struct TemporalParams {
    const double* color;      // [3][w*h] this frame's colour
    const double* var;        // [w*h] the variance of its mean luminance
    const double* count;      // [w*h] its sample counts, or null: tile_spp
    const int32_t* tile_spp;  // [tiles] the adaptive sampler's counts (count == null)
    const double* feat;       // [MFX_AOV_PLANES][w*h] the current view's features
    const double* hist;       // [MFX_TP_PLANES][w*h] the history, or null: none (every pixel passes through)
    double* hist_out;         // [MFX_TP_PLANES][w*h] the history after the call
    unsigned long long* accepted;  // [1] += pixels that took history
    MfxCamera cam, hcam;      // the current view's and the history's, by value: scalar-loaded
    int32_t width, height;
    double tol_depth2;        // tol_depth * tol_depth
    double tol_normal2;
    double max_history;
};

hipError_t mfx_launch_aov(const AovParams& P, hipStream_t st);
// resident blocks per CU of k_aov's instance (two-level, textured, lens, normals) with stack_size stack entries per lane in LDS
hipError_t mfx_aov_occupancy(bool inst, bool tx, bool lens, int stack_size, int* blocks_per_cu, bool sn = false);
hipError_t mfx_launch_temporal(const TemporalParams& P, hipStream_t st);
hipError_t mfx_launch_atrous(const AtrousParams& P, hipStream_t st);
hipError_t mfx_launch_atrous_var(const AtrousVarParams& P, hipStream_t st);
// colour planes <- accum / n, variance plane <- max(0, S2 - S1*S1/n) / (n (n - 1)), n = tile_spp[the pixel's tile]
hipError_t mfx_launch_dn_from_adaptive(const double* accum, const double* mom, const int32_t* tile_spp, int w, int h,
                                       double* dst, double* vdst, hipStream_t st);
// colour planes <- accum / n (mfx_accum_read_mean's value)
hipError_t mfx_launch_dn_from_accum(const double* accum, int64_t npix, double n, double* dst, hipStream_t st);
// colour planes <- an x-major RGBA frame (alpha dropped)
hipError_t mfx_launch_dn_from_frame(const double* frame, int64_t npix, double* dst, hipStream_t st);
// colour planes -> x-major RGBA doubles (alpha 1.0) and / or posted y-major RGBA8; either may be null
hipError_t mfx_launch_dn_post(const double* src, int w, int h, double* out, uint8_t* rgba, hipStream_t st);

#endif
