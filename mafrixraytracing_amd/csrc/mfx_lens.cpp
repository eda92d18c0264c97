// mfx_lens.cpp — the thin lens beside its setter (mfx_set_lens: mfx_create.cpp, with mfx_set_camera, whose steps
// it shares): what a context reports about it (mfx_lens_info) and the host-only statements of the rule
// (mfx_lens_derive, mfx_lens_rays), by the code the kernels compile (mfx_lens.h).
#include "mfx_ctx.h"

using namespace mfxh;

extern "C" {
int mfx_lens_info(mfx_ctx* c, double out[16]) {
    if (!c || !out) return fail(MFX_E_INVALID, "mfx_lens_info: null argument");
    std::fill(out, out + 16, 0.0);
    const Lens& L = c->lens;
    if (!L.on) return MFX_OK;
    out[0] = 1.0;
    out[1] = L.aperture;
    out[2] = L.focus;
    std::copy(L.rec.U, L.rec.U + 3, out + 3);
    std::copy(L.rec.V, L.rec.V + 3, out + 6);
    out[9] = L.rec.s;
    out[10] = (double)L.eps;
    out[11] = (double)L.rebuilds;
    HIPCHECK(hipSetDevice(c->device));
    const LaunchShapes& A = c->scene.shapes;
    WfLdsShape s = wf_lds_shape(c->scene, wf_textured(c), false, A.stack_lds_ext, A.ntop_ext, A.nslot_ext);
    s.env = wf_env(c);
    s.lens = true;
    int eb = 0, ab = 0;
    HIPCHECK(mfx_wf_kernel_occupancy(s, &eb));
    HIPCHECK(mfx_aov_occupancy(!c->scene.host.inst.empty(), wf_textured(c), true, c->scene.stack_size, &ab));
    out[12] = (double)eb;
    out[13] = (double)ab;
    return MFX_OK;
}

int mfx_lens_derive(const mfx_pinhole* cam, const mfx_lens* lens, double out[7]) {
    if (!cam || !lens || !out) return fail(MFX_E_INVALID, "mfx_lens_derive: null argument");
    MfxLensRec rec{};
    MFX_TRY(lens_record("mfx_lens_derive", cam, lens, rec));
    std::memcpy(out, &rec, sizeof(rec));
    return MFX_OK;
}

int mfx_lens_rays(const mfx_pinhole* cam, const mfx_lens* lens, uint64_t seed, int32_t width, int32_t height, int64_t n,
                  const int32_t* px, const int32_t* py, const int64_t* sample, double* out, int32_t* trials) {
    if (!cam || !lens) return fail(MFX_E_INVALID, "mfx_lens_rays: null argument");
    if (width < 1 || height < 1) return fail(MFX_E_INVALID, "mfx_lens_rays: width and height must be >= 1");
    if (n < 0 || (n > 0 && (!px || !py || !sample || !out || !trials)))
        return fail(MFX_E_INVALID, "mfx_lens_rays: n must be >= 0, with every array when n > 0");
    MfxLensRec rec{};
    MFX_TRY(lens_record("mfx_lens_rays", cam, lens, rec));
    MfxCamera m;
    mfx_derive_camera(*cam, m);
    for (int64_t i = 0; i < n; ++i) {
        const int x = px[i], y = py[i];
        if (x < 0 || x >= width || y < 0 || y >= height || sample[i] < 0)
            return fail(MFX_E_INVALID, "mfx_lens_rays: path " + std::to_string(i) + " lies outside the film or has a negative sample");
        // PixelIntegrator.Sample's key and first two draws, as the kernels derive them (path_key, rng_next)
        const uint64_t pixel = (uint64_t)((int64_t)x * height + y);
        const uint64_t key = mfx_lens_mix64(seed ^ mfx_lens_mix64((pixel << 32) | ((uint64_t)sample[i] & 0xffffffffULL)));
        const double u = ((double)x + mfx_lens_draw(key, 1)) / (double)width;
        const double v = ((double)y + mfx_lens_draw(key, 2)) / (double)height;
        double* r = out + 8 * i;
        trials[i] = mfx_lens_ray(m.position, rec, key, u, v, r, r + 3, r[6], r[7]);
    }
    return MFX_OK;
}
}  // extern "C"
