// mfx_lens.h — the thin lens (mfx_set_lens): the lens record of a camera and the camera ray through it, one
// statement shared by the host (mfx_lens_derive, mfx_lens_rays) and the gfx950 kernels (k_extend's and k_aov's
// LENS instances). The rule is the contract in include/mafrix_rt.h; mafrixraytracing_amd/lens.py states it in
// Python floats.
//
// FP64, one rounding per operation in the order written (every file that includes this is compiled with
// -ffp-contract=off), + - * / sqrt and comparisons only, and 64-bit integer arithmetic for the draws, so the host
// and the device give the same bits. dot(a, b) = (a0*b0 + a1*b1) + a2*b2.
#ifndef MFX_LENS_H
#define MFX_LENS_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MFX_LENS_HD __host__ __device__ __forceinline__
#else
#define MFX_LENS_HD inline
#endif

// The lens record: the lens disk's axes, aperture long (U along the camera's right, V along its down), and
// s = focus / dplane, which scales a pinhole ray's vector to the film plane onto the focus plane.
struct MfxLensRec {
    double U[3], V[3], s;
};
static_assert(sizeof(MfxLensRec) == 56, "MfxLensRec: seven doubles");

// the lens stream's first counter: draws 2^31 + 1, 2^31 + 2, ... of the path's own key (a path's counter stays
// far below 2^31, and goes on at 2 after the camera ray)
#define MFX_LENS_COUNTER0 0x80000000ULL

MFX_LENS_HD uint64_t mfx_lens_mix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xbf58476d1ce4e5b9ULL;
    z ^= z >> 27;
    z *= 0x94d049bb133111ebULL;
    z ^= z >> 31;
    return z;
}
// draw m of key: rng_unit(mix64(key + m * 0x9e3779b97f4a7c15)), as rng_next with counter m
MFX_LENS_HD double mfx_lens_draw(uint64_t key, uint64_t m) {
    const uint64_t z = mfx_lens_mix64(key + m * 0x9e3779b97f4a7c15ULL);
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
MFX_LENS_HD double mfx_lens_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// what mfx_lens_record refuses, in the order it looks
enum { MFX_LENS_OK = 0, MFX_LENS_BAD_APERTURE, MFX_LENS_BAD_FOCUS, MFX_LENS_BAD_RIGHT, MFX_LENS_BAD_DOWN, MFX_LENS_BAD_FORWARD,
       MFX_LENS_BAD_DPLANE, MFX_LENS_BAD_SCALE };

// The record of the derived camera cam = {P0, TL, R, D} (MfxCamera's twelve doubles) under (aperture, focus);
// *dplane gets the film plane's distance along the forward axis. Host only.
inline int mfx_lens_record(const double cam[12], double aperture, double focus, MfxLensRec& rec, double* dplane) {
    const double *P0 = cam, *TL = cam + 3, *R = cam + 6, *D = cam + 9;
    if (!(aperture >= 0.0) || !isfinite(aperture)) return MFX_LENS_BAD_APERTURE;
    if (!(focus > 0.0) || !isfinite(focus)) return MFX_LENS_BAD_FOCUS;
    const double lr = sqrt(mfx_lens_dot(R, R)), ld = sqrt(mfx_lens_dot(D, D));
    if (!(lr > 0.0) || !isfinite(lr)) return MFX_LENS_BAD_RIGHT;
    if (!(ld > 0.0) || !isfinite(ld)) return MFX_LENS_BAD_DOWN;
    for (int c = 0; c < 3; ++c) {
        rec.U[c] = (R[c] / lr) * aperture;
        rec.V[c] = (D[c] / ld) * aperture;
    }
    const double n[3] = {R[1] * D[2] - R[2] * D[1], R[2] * D[0] - R[0] * D[2], R[0] * D[1] - R[1] * D[0]};
    const double ln = sqrt(mfx_lens_dot(n, n));
    if (!(ln > 0.0) || !isfinite(ln)) return MFX_LENS_BAD_FORWARD;
    const double f[3] = {n[0] / ln, n[1] / ln, n[2] / ln};
    const double t[3] = {TL[0] - P0[0], TL[1] - P0[1], TL[2] - P0[2]};
    const double dp = mfx_lens_dot(t, f);
    if (dplane) *dplane = dp;
    if (!(dp > 0.0) || !isfinite(dp)) return MFX_LENS_BAD_DPLANE;
    rec.s = focus / dp;
    if (!isfinite(rec.s)) return MFX_LENS_BAD_SCALE;
    return MFX_LENS_OK;
}

// The camera ray of (u, v), the path's first two draws, through the lens: origin o on the lens disk around P0,
// unit direction d through the point where the pinhole ray of (u, v) meets the focus plane. a, b: the accepted
// point of the unit disk; the return value is the number of trials it took (two lens draws each).
MFX_LENS_HD int mfx_lens_ray(const double cam[12], const MfxLensRec& L, uint64_t key, double u, double v, double o[3],
                             double d[3], double& a, double& b) {
    const double *P0 = cam, *TL = cam + 3, *R = cam + 6, *D = cam + 9;
    uint64_t m = MFX_LENS_COUNTER0;
    int trials = 0;
    do {  // rejection, as the reference's GetRandomInUnitSphere: no trigonometry
        const double r1 = mfx_lens_draw(key, m + 1), r2 = mfx_lens_draw(key, m + 2);
        m += 2;
        trials += 1;
        a = r1 * 2.0 - 1.0;
        b = r2 * 2.0 - 1.0;
    } while (!((a * a + b * b) < 1.0));
    double w[3];
    for (int c = 0; c < 3; ++c) {
        const double target = (TL[c] + R[c] * u) + D[c] * v;  // the pinhole's expression
        const double pin = target - P0[c];
        o[c] = (P0[c] + L.U[c] * a) + L.V[c] * b;
        const double fp = P0[c] + pin * L.s;
        w[c] = fp - o[c];
    }
    const double l = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);  // the camera ray's own vnormalize
    for (int c = 0; c < 3; ++c) d[c] = l == 0.0 ? 0.0 : w[c] / l;
    return trials;
}

#endif
