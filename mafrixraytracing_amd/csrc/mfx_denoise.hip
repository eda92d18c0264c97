// mfx_denoise.hip — gfx950 kernels of mfx_aov (first-hit feature buffers of the film's own camera
// rays), mfx_denoise (the edge-avoiding a-trous filter they guide) and mfx_denoise_var (that filter
// with a variance-guided luminance term, fed by the adaptive sampler's moments) and mfx_temporal (the
// previous result reprojected into the current view and merged by sample counts). The rule of each is
// stated in include/mafrix_rt.h and, in numpy, in mafrixraytracing_amd/denoise.py and temporal.py.
//
// Compiled with -ffp-contract=off like the rest of the library: every FP64 expression below has one
// rounding per operation in the order written, so the device gives the host statement's bits. The
// filter's weights are rational (+ - * / only): no exp whose last bit differs between libraries.
//
// A translation unit of its own: the trace kernels' code objects (mfx_kernels.hip, mfx_wavefront.hip)
// do not change with it.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "mfx_layout.h"
#include "mfx_denoise.h"
#include "mfx_lens.h"
#include "mfx_trace_common.h"

// ----------------------------------------------------------------------------------------------
// k_aov: one lane per pixel, x-major (a wave's 64 pixels are 64 consecutive rows of one column, or
// the end of one column and the start of the next: neighbouring rays), the samples looped in
// registers. The ray is the path's own camera ray (k_camera / trace_kernel: key pixel x*h + y, draws
// 0 and 1), the hit Bvh.Hit(ray, 1e-6, 99999999.) by the per-lane walk of closest_kernel.
// ----------------------------------------------------------------------------------------------
// TX: the instances for albedo textures (mfx_create_textured): the albedo planes take the material's albedo
// times the texel of the hit point, by the rule and the functions the path vertices use (mfx_texture.h).
// LENS: the instances for a thin lens (mfx_set_lens): the ray is the film's own lens ray (mfx_lens.h), so plane [3]
// is t along it.
// SN: the twins for smooth shading (mfx_set_normals): on a smooth primitive the normal planes take the shading normal
// of the hit point, by the rule and the function the path vertices use (mfx_normals.h).
template <bool INST, bool TX = false, bool LENS = false, bool SN = false>
__global__ void __launch_bounds__(256) k_aov(AovParams P) {
    extern __shared__ int lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int* stack = lds + wave * P.stack_size * 64 + lane;
    const int64_t npix = (int64_t)P.width * P.height;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= npix) return;
    const SceneView S{P.nodes, P.slots, P.slot_ref, P.ref_blob, P.inst, nullptr, 0, nullptr, 0, nullptr, P.tslack};
    const MfxCamera& CAM = P.cam;
    const int x = (int)(q / P.height), y = (int)(q - (int64_t)x * P.height);
    double f[MFX_AOV_PLANES];
#pragma unroll
    for (int k = 0; k < MFX_AOV_PLANES; ++k) f[k] = 0.0;
    for (int32_t s = 0; s < P.spp; ++s) {
        // PixelIntegrator.Sample (Integrators.fs:166-169) + PinholeCamera.GetRay (Camera.fs:134-139)
        const uint64_t key = path_key(P.seed, (uint64_t)q, (uint64_t)(P.sample_base + s));
        uint32_t rn = 0;
        const double u = ((double)x + rng_next(key, rn)) / (double)P.width;
        const double v = ((double)y + rng_next(key, rn)) / (double)P.height;
        DV o, d;
        if constexpr (LENS) {
            double lo[3], ldir[3], la, lb;
            mfx_lens_ray(CAM.position, P.lens, key, u, v, lo, ldir, la, lb);
            o = dv(lo[0], lo[1], lo[2]);
            d = dv(ldir[0], ldir[1], ldir[2]);
        } else {
            const DV target = vadd(vadd(ld3(CAM.topleft), vmul(ld3(CAM.right), u)), vmul(ld3(CAM.down), v));
            o = ld3(CAM.position);
            d = vnormalize(vsub(target, o));
        }
        Best B;
        Stats st{0, 0, 0};
        if (!traverse<false, false, INST>(S, o, d, 1e-6, 99999999., stack, B, st)) continue;  // a miss adds nothing
        const MfxShade sh = P.shade[B.info & MFX_INFO_SHADE_MASK];
        DV nm;
        if ((sh.prim_kind & 3) == MFX_KIND_SPHERE)
            nm = vnormalize(vsub(vadd(o, vmul(d, B.t)), ld3(sh.n)));  // Sphere.fs:39-43
        else
            nm = ld3(sh.n);
        if constexpr (SN) {
            const int prim = sh.prim_kind >> 2;
            if (P.sn.flag[prim]) {
                const DV hp = vadd(o, vmul(d, B.t));  // Ray.PointAtParameter: the point k_extend stores
                const double* r = P.sn.rec + (int64_t)MFX_SN_RECORD_DOUBLES * prim;
                const double rec[12] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11]};
                const double h3[3] = {hp.x, hp.y, hp.z}, g3[3] = {nm.x, nm.y, nm.z};
                double s3[3];
                mfx_sn_shade(rec, h3, g3, s3);
                nm = dv(s3[0], s3[1], s3[2]);
            }
        }
        f[0] = f[0] + nm.x;
        f[1] = f[1] + nm.y;
        f[2] = f[2] + nm.z;
        f[3] = f[3] + B.t;
        double a0 = sh.albedo[0], a1 = sh.albedo[1], a2 = sh.albedo[2];
        if constexpr (TX) {
            const int prim = sh.prim_kind >> 2;
            const int tex = P.tx.ptex[prim];
            if (tex >= 0) {
                const DV hp = vadd(o, vmul(d, B.t));  // Ray.PointAtParameter: the point k_extend stores
                const double* r = P.tx.uvrec + (int64_t)MFX_UV_RECORD_DOUBLES * prim;
                const double h3[3] = {hp.x, hp.y, hp.z};
                const double rec[8] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
                double tu, tv;
                mfx_tx_uv(rec, h3, tu, tv);
                const uint32_t texel = P.tx.texels[mfx_tx_texel(P.tx.desc[tex], tu, tv)];
                a0 = mfx_tx_albedo(a0, texel, 0);
                a1 = mfx_tx_albedo(a1, texel, 1);
                a2 = mfx_tx_albedo(a2, texel, 2);
            }
        }
        f[4] = f[4] + a0;
        f[5] = f[5] + a1;
        f[6] = f[6] + a2;
        f[7] = f[7] + 1.0;
    }
    const double n = (double)P.spp;
#pragma unroll
    for (int k = 0; k < MFX_AOV_PLANES; ++k) {
        f[k] = f[k] / n;
        P.feat[k * npix + q] = f[k];
    }
    if (P.out) {
        double2* o = (double2*)(P.out + MFX_AOV_PLANES * q);
#pragma unroll
        for (int k = 0; k < MFX_AOV_PLANES / 2; ++k) o[k] = make_double2(f[2 * k], f[2 * k + 1]);
    }
}

// ----------------------------------------------------------------------------------------------
// k_atrous: one thread per pixel, x-major; colour and features are planes, so a wave's 64 pixels
// (consecutive y at one x) read every tap as one coalesced run of 64 doubles per plane. No LDS
// tiling: at steps 1 and 2 neighbouring threads' taps overlap in L1 / L2.
// ----------------------------------------------------------------------------------------------
__device__ __forceinline__ double d2(double a0, double a1, double a2, double b0, double b1, double b2) {
    return ((a0 - b0) * (a0 - b0) + (a1 - b1) * (a1 - b1)) + (a2 - b2) * (a2 - b2);
}

__global__ void __launch_bounds__(256) k_atrous(AtrousParams P) {
    const int W = P.width, H = P.height;
    const int64_t npix = (int64_t)W * H;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const int x = (int)(p / H), y = (int)(p - (int64_t)x * H);
    const double* __restrict__ C0 = P.src;
    const double* __restrict__ C1 = P.src + npix;
    const double* __restrict__ C2 = P.src + 2 * npix;
    const double* __restrict__ F = P.feat;
    const bool tn = P.terms & 1, tz = P.terms & 2, ta = P.terms & 4, tc = P.terms & 8;
    const double cp0 = C0[p], cp1 = C1[p], cp2 = C2[p];
    double np0 = 0, np1 = 0, np2 = 0, zp = 0, ap0 = 0, ap1 = 0, ap2 = 0;
    if (tn) { np0 = F[p]; np1 = F[npix + p]; np2 = F[2 * npix + p]; }
    if (tz) zp = F[3 * npix + p];
    if (ta) { ap0 = F[4 * npix + p]; ap1 = F[5 * npix + p]; ap2 = F[6 * npix + p]; }
    double n0 = 0.0, n1 = 0.0, n2 = 0.0, den = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = y + dy * P.step;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int xx = x + dx * P.step;
            if (xx < 0 || xx >= W) continue;
            const int64_t q = (int64_t)xx * H + yy;  // inside the film: 0 <= q < npix
            const double cq0 = C0[q], cq1 = C1[q], cq2 = C2[q];
            double g = 1.0;
            if (tn) {
                const double term = d2(np0, np1, np2, F[q], F[npix + q], F[2 * npix + q]) / P.sn2;
                g = g * (1.0 / (1.0 + term));
            }
            if (tz) {
                const double zq = F[3 * npix + q];
                const double dz = zp - zq;
                const double dd = P.sz2 * (zp * zp + zq * zq);
                const double term = dd > 0.0 ? (dz * dz) / dd : 0.0;
                g = g * (1.0 / (1.0 + term));
            }
            if (ta) {
                const double term = d2(ap0, ap1, ap2, F[4 * npix + q], F[5 * npix + q], F[6 * npix + q]) / P.sa2;
                g = g * (1.0 / (1.0 + term));
            }
            if (tc) {
                const double term = d2(cp0, cp1, cp2, cq0, cq1, cq2) / P.sc2;
                g = g * (1.0 / (1.0 + term));
            }
            const double kx = dx == 0 ? 0.375 : (dx == 1 || dx == -1) ? 0.25 : 0.0625;
            const double ky = dy == 0 ? 0.375 : (dy == 1 || dy == -1) ? 0.25 : 0.0625;
            const double wt = (kx * ky) * g;
            n0 = n0 + wt * cq0;
            n1 = n1 + wt * cq1;
            n2 = n2 + wt * cq2;
            den = den + wt;
        }
    }
    // the centre tap has g = 1: den >= 9/64
    P.dst[p] = n0 / den;
    P.dst[npix + p] = n1 / den;
    P.dst[2 * npix + p] = n2 / den;
}

// ----------------------------------------------------------------------------------------------
// k_atrous_var: k_atrous with the variance plane beside the colour (mfx_denoise_var). Thread
// mapping, tap order and the feature terms are k_atrous's, statement for statement, so with the
// luminance term off the colour is k_atrous's without its colour term, bit for bit. Before the taps a
// thread smooths its own pixel's variance over the 3x3 pixels around it (always one pixel apart: the
// prefilter follows the image's grid, not the iteration's step); a wave reads each of those nine taps,
// like the 25 of every plane, as one coalesced run.
// ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_atrous_var(AtrousVarParams P) {
    const int W = P.width, H = P.height;
    const int64_t npix = (int64_t)W * H;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const int x = (int)(p / H), y = (int)(p - (int64_t)x * H);
    const double* __restrict__ C0 = P.src;
    const double* __restrict__ C1 = P.src + npix;
    const double* __restrict__ C2 = P.src + 2 * npix;
    const double* __restrict__ V = P.vsrc;
    const double* __restrict__ F = P.feat;
    const bool tn = P.terms & 1, tz = P.terms & 2, ta = P.terms & 4, tl = P.terms & 8;
    const double cp0 = C0[p], cp1 = C1[p], cp2 = C2[p];
    double np0 = 0, np1 = 0, np2 = 0, zp = 0, ap0 = 0, ap1 = 0, ap2 = 0;
    if (tn) { np0 = F[p]; np1 = F[npix + p]; np2 = F[2 * npix + p]; }
    if (tz) zp = F[3 * npix + p];
    if (ta) { ap0 = F[4 * npix + p]; ap1 = F[5 * npix + p]; ap2 = F[6 * npix + p]; }
    double lp = 0.0, lden = 1.0;
    if (tl) {
        double pn = 0.0, pd = 0.0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= H) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int xx = x + dx;
                if (xx < 0 || xx >= W) continue;
                const double kk = (dx == 0 ? 0.5 : 0.25) * (dy == 0 ? 0.5 : 0.25);
                pn = pn + kk * V[(int64_t)xx * H + yy];  // inside the film
                pd = pd + kk;
            }
        }
        const double vf = pn / pd;  // the centre tap: pd >= 1/4
        lden = P.sl2 * vf + P.luma_floor;
        lp = (cp0 + cp1) + cp2;
    }
    double n0 = 0.0, n1 = 0.0, n2 = 0.0, den = 0.0, vn = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = y + dy * P.step;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int xx = x + dx * P.step;
            if (xx < 0 || xx >= W) continue;
            const int64_t q = (int64_t)xx * H + yy;  // inside the film: 0 <= q < npix
            const double cq0 = C0[q], cq1 = C1[q], cq2 = C2[q];
            const double vq = V[q];
            double g = 1.0;
            if (tn) {
                const double term = d2(np0, np1, np2, F[q], F[npix + q], F[2 * npix + q]) / P.sn2;
                g = g * (1.0 / (1.0 + term));
            }
            if (tz) {
                const double zq = F[3 * npix + q];
                const double dz = zp - zq;
                const double dd = P.sz2 * (zp * zp + zq * zq);
                const double term = dd > 0.0 ? (dz * dz) / dd : 0.0;
                g = g * (1.0 / (1.0 + term));
            }
            if (ta) {
                const double term = d2(ap0, ap1, ap2, F[4 * npix + q], F[5 * npix + q], F[6 * npix + q]) / P.sa2;
                g = g * (1.0 / (1.0 + term));
            }
            if (tl) {
                const double dl = lp - ((cq0 + cq1) + cq2);
                const double term = (dl * dl) / lden;
                g = g * (1.0 / (1.0 + term));
            }
            const double kx = dx == 0 ? 0.375 : (dx == 1 || dx == -1) ? 0.25 : 0.0625;
            const double ky = dy == 0 ? 0.375 : (dy == 1 || dy == -1) ? 0.25 : 0.0625;
            const double wt = (kx * ky) * g;
            n0 = n0 + wt * cq0;
            n1 = n1 + wt * cq1;
            n2 = n2 + wt * cq2;
            den = den + wt;
            vn = vn + (wt * wt) * vq;
        }
    }
    // the centre tap has g = 1: den >= 9/64
    P.dst[p] = n0 / den;
    P.dst[npix + p] = n1 / den;
    P.dst[2 * npix + p] = n2 / den;
    P.vdst[p] = vn / (den * den);
}

// ----------------------------------------------------------------------------------------------
// k_temporal: one thread per pixel, x-major planes as k_atrous (mfx_temporal; the rule, step by step:
// include/mafrix_rt.h). The pixel's world point from the current view's depth is projected into the
// history's view; the nearest history pixel is taken if it shows the same surface (hit fraction 1 on
// both sides, depth and normal within the tolerances) and merged by sample counts. Both cameras come
// in the kernel arguments (scalar loads); a wave reads its own pixels' planes as coalesced runs of 64
// doubles and gathers the history nearly so: neighbours reproject to neighbours. The history's view
// features are written beside the merged result, so the two history buffers swap by pointer. A wave
// counts its accepted pixels by ballot and adds them with one vector atomic. No lane leaves before the
// ballot: a lane past the film only loads and stores nothing.
// ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_temporal(TemporalParams P) {
    const int W = P.width, H = P.height;
    const int64_t npix = (int64_t)W * H;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool inside = p < npix;
    bool accept = false;
    if (inside) {
        const int x = (int)(p / H), y = (int)(p - (int64_t)x * H);
        const double* __restrict__ F = P.feat;
        const double* __restrict__ HB = P.hist;
        const double c0 = P.color[p], c1 = P.color[npix + p], c2 = P.color[2 * npix + p];
        const double vp = P.var[p];
        const double n = P.count ? P.count[p] : (double)P.tile_spp[(y >> 3) * ((W + 7) >> 3) + (x >> 3)];
        const double np0 = F[p], np1 = F[npix + p], np2 = F[2 * npix + p];
        const double zp = F[3 * npix + p], fp = F[7 * npix + p];
        double o0 = c0, o1 = c1, o2 = c2, ov = vp, on = n;
        if (HB && fp == 1.0) {
            // the pixel centre's camera ray (k_aov's operations) and its world point at the view's depth
            const double u = ((double)x + 0.5) / (double)W;
            const double v = ((double)y + 0.5) / (double)H;
            const DV o = ld3(P.cam.position);
            const DV target = vadd(vadd(ld3(P.cam.topleft), vmul(ld3(P.cam.right), u)), vmul(ld3(P.cam.down), v));
            const DV dir = vnormalize(vsub(target, o));
            const DV wp = vadd(o, vmul(dir, zp));
            // into the history's view: the ray from its eye through the point meets its image plane at a + g
            const DV ho = ld3(P.hcam.position), hr = ld3(P.hcam.right), hd = ld3(P.hcam.down);
            const DV e = vsub(wp, ho);
            const DV a = vsub(ld3(P.hcam.topleft), ho);
            const DV nn = vcross(hr, hd);
            const double den = vdot(e, nn), num = vdot(a, nn);
            if (num * den > 0.0) {
                const double s = num / den;
                const DV g = vsub(vmul(e, s), a);
                const double hu = vdot(g, hr) / vdot(hr, hr);
                const double hv = vdot(g, hd) / vdot(hd, hd);
                if (hu >= 0.0 && hu < 1.0 && hv >= 0.0 && hv < 1.0) {
                    const int hx = min(W - 1, (int)floor(hu * (double)W));
                    const int hy = min(H - 1, (int)floor(hv * (double)H));
                    const int64_t q = (int64_t)hx * H + hy;  // inside the film: 0 <= q < npix
                    if (HB[MFX_TP_HIT * npix + q] == 1.0) {
                        const double ze = sqrt(vdot(e, e));
                        const double dz = ze - HB[MFX_TP_DEPTH * npix + q];
                        const double nd = d2(np0, np1, np2, HB[MFX_TP_NORMAL * npix + q], HB[(MFX_TP_NORMAL + 1) * npix + q],
                                             HB[(MFX_TP_NORMAL + 2) * npix + q]);
                        if (dz * dz <= P.tol_depth2 * (ze * ze) && nd <= P.tol_normal2) {
                            accept = true;
                            const double hn = HB[MFX_TP_COUNT * npix + q];
                            const double nh = hn < P.max_history ? hn : P.max_history;
                            const double nt = n + nh;
                            const double wc = n / nt, wh = nh / nt;
                            o0 = wc * c0 + wh * HB[q];
                            o1 = wc * c1 + wh * HB[npix + q];
                            o2 = wc * c2 + wh * HB[2 * npix + q];
                            ov = (wc * wc) * vp + (wh * wh) * HB[MFX_TP_VAR * npix + q];
                            on = nt;
                        }
                    }
                }
            }
        }
        double* __restrict__ O = P.hist_out;
        O[p] = o0;
        O[npix + p] = o1;
        O[2 * npix + p] = o2;
        O[MFX_TP_VAR * npix + p] = ov;
        O[MFX_TP_COUNT * npix + p] = on;
        O[MFX_TP_NORMAL * npix + p] = np0;
        O[(MFX_TP_NORMAL + 1) * npix + p] = np1;
        O[(MFX_TP_NORMAL + 2) * npix + p] = np2;
        O[MFX_TP_DEPTH * npix + p] = zp;
        O[MFX_TP_HIT * npix + p] = fp;
    }
    const unsigned long long took = __ballot(accept);
    if ((threadIdx.x & 63) == 0 && took) atomicAdd(P.accepted, (unsigned long long)__popcll(took));
}

// colour planes <- accum / n and variance plane <- the tile check's v_p, n the pixel's own tile's count
// (adaptive_mean_kernel's and k_tile_check's statements)
__global__ void k_dn_from_adaptive(const double* __restrict__ accum, const double* __restrict__ mom,
                                   const int32_t* __restrict__ tile_spp, int w, int h, double* __restrict__ dst,
                                   double* __restrict__ vdst) {
    const int64_t npix = (int64_t)w * h;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= npix) return;
    const int x = (int)(q / h), y = (int)(q % h);
    const double n = (double)tile_spp[(y >> 3) * ((w + 7) >> 3) + (x >> 3)];
    dst[q] = accum[q] / n;
    dst[npix + q] = accum[npix + q] / n;
    dst[2 * npix + q] = accum[2 * npix + q] / n;
    const double s1 = mom[q], s2 = mom[npix + q];
    const double d = s2 - s1 * s1 / n;
    vdst[q] = (d > 0.0 ? d : 0.0) / (n * (n - 1.0));
}

__global__ void k_dn_from_accum(const double* __restrict__ accum, int64_t npix, double n, double* __restrict__ dst) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= npix) return;
    dst[q] = accum[q] / n;  // color / float n (mean_kernel)
    dst[npix + q] = accum[npix + q] / n;
    dst[2 * npix + q] = accum[2 * npix + q] / n;
}

__global__ void k_dn_from_frame(const double* __restrict__ frame, int64_t npix, double* __restrict__ dst) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= npix) return;
    const double2* f = (const double2*)frame + 2 * q;
    const double2 a = f[0], b = f[1];
    dst[q] = a.x;
    dst[npix + q] = a.y;
    dst[2 * npix + q] = b.x;
}

__global__ void k_dn_post(const double* __restrict__ src, int w, int h, double* __restrict__ out, uint8_t* __restrict__ rgba) {
    const int64_t npix = (int64_t)w * h;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= npix) return;
    const double r = src[q], g = src[npix + q], b = src[2 * npix + q];
    if (out) {
        double2* o = (double2*)out + 2 * q;
        o[0] = make_double2(r, g);
        o[1] = make_double2(b, 1.0);
    }
    if (rgba) {  // PostProcessAndToScreenBuffer (Scene.fs:315-330), y-major
        const int x = (int)(q / h), y = (int)(q % h);
        uint8_t* o = rgba + ((int64_t)y * w + x) * 4;
        o[0] = post_byte(r);
        o[1] = post_byte(g);
        o[2] = post_byte(b);
        o[3] = 255;
    }
}

// ----------------------------------------------------------------------------------------------
// Host-side launchers (called from mfx_denoise_api.cpp)
// ----------------------------------------------------------------------------------------------
static inline unsigned dn_grid(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

// k_aov's instance: two-level (inst), albedo textures (tx), a thin lens (lens), smooth shading (sn: the twin of each)
template <bool SN>
static const void* aov_kernel_sn(bool inst, bool tx, bool lens) {
    if (lens) {
        if (tx) return inst ? (const void*)k_aov<true, true, true, SN> : (const void*)k_aov<false, true, true, SN>;
        return inst ? (const void*)k_aov<true, false, true, SN> : (const void*)k_aov<false, false, true, SN>;
    }
    if (tx) return inst ? (const void*)k_aov<true, true, false, SN> : (const void*)k_aov<false, true, false, SN>;
    return inst ? (const void*)k_aov<true, false, false, SN> : (const void*)k_aov<false, false, false, SN>;
}
static const void* aov_kernel(bool inst, bool tx, bool lens, bool sn = false) {
    if (sn) return aov_kernel_sn<true>(inst, tx, lens);
    if (lens) {
        if (tx) return inst ? (const void*)k_aov<true, true, true> : (const void*)k_aov<false, true, true>;
        return inst ? (const void*)k_aov<true, false, true> : (const void*)k_aov<false, false, true>;
    }
    if (tx) return inst ? (const void*)k_aov<true, true> : (const void*)k_aov<false, true>;
    return inst ? (const void*)k_aov<true> : (const void*)k_aov<false>;
}
static size_t aov_lds_bytes(int stack_size) { return (size_t)4 * stack_size * 64 * sizeof(int); }  // mfx_launch_query's: a column per lane

hipError_t mfx_launch_aov(const AovParams& P, hipStream_t st) {
    const dim3 g(dn_grid((int64_t)P.width * P.height, 256));
    // albedo textures: the TX instances
    if (P.tx.texels && (!P.tx.uvrec || !P.tx.ptex || !P.tx.desc)) return hipErrorInvalidValue;
    // smooth shading: the SN twins
    if ((P.sn.rec != nullptr) != (P.sn.flag != nullptr)) return hipErrorInvalidValue;
    void* args[] = {const_cast<AovParams*>(&P)};
    const hipError_t e = hipLaunchKernel(aov_kernel(P.inst != nullptr, P.tx.texels != nullptr, P.lens_on != 0, P.sn.rec != nullptr), g, dim3(256), args,
                                         aov_lds_bytes(P.stack_size), st);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t mfx_aov_occupancy(bool inst, bool tx, bool lens, int stack_size, int* blocks_per_cu, bool sn) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, aov_kernel(inst, tx, lens, sn), 256, aov_lds_bytes(stack_size));
}

hipError_t mfx_launch_temporal(const TemporalParams& P, hipStream_t st) {
    hipLaunchKernelGGL(k_temporal, dim3(dn_grid((int64_t)P.width * P.height, 256)), dim3(256), 0, st, P);
    return hipGetLastError();
}

hipError_t mfx_launch_atrous(const AtrousParams& P, hipStream_t st) {
    hipLaunchKernelGGL(k_atrous, dim3(dn_grid((int64_t)P.width * P.height, 256)), dim3(256), 0, st, P);
    return hipGetLastError();
}

hipError_t mfx_launch_atrous_var(const AtrousVarParams& P, hipStream_t st) {
    hipLaunchKernelGGL(k_atrous_var, dim3(dn_grid((int64_t)P.width * P.height, 256)), dim3(256), 0, st, P);
    return hipGetLastError();
}

hipError_t mfx_launch_dn_from_adaptive(const double* accum, const double* mom, const int32_t* tile_spp, int w, int h,
                                       double* dst, double* vdst, hipStream_t st) {
    hipLaunchKernelGGL(k_dn_from_adaptive, dim3(dn_grid((int64_t)w * h, 256)), dim3(256), 0, st, accum, mom, tile_spp, w, h,
                       dst, vdst);
    return hipGetLastError();
}

hipError_t mfx_launch_dn_from_accum(const double* accum, int64_t npix, double n, double* dst, hipStream_t st) {
    hipLaunchKernelGGL(k_dn_from_accum, dim3(dn_grid(npix, 256)), dim3(256), 0, st, accum, npix, n, dst);
    return hipGetLastError();
}

hipError_t mfx_launch_dn_from_frame(const double* frame, int64_t npix, double* dst, hipStream_t st) {
    hipLaunchKernelGGL(k_dn_from_frame, dim3(dn_grid(npix, 256)), dim3(256), 0, st, frame, npix, dst);
    return hipGetLastError();
}

hipError_t mfx_launch_dn_post(const double* src, int w, int h, double* out, uint8_t* rgba, hipStream_t st) {
    hipLaunchKernelGGL(k_dn_post, dim3(dn_grid((int64_t)w * h, 256)), dim3(256), 0, st, src, w, h, out, rgba);
    return hipGetLastError();
}
