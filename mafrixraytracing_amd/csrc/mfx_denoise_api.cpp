// mfx_denoise_api.cpp — feature buffers, denoising and temporal reuse (mfx_temporal: k_temporal merges the
// reprojected history with the frame between two history buffers the context owns).
// mfx_aov traces the film's own camera rays once more, per lane (k_aov), into eight FP64 planes that
// stay on the device; mfx_denoise runs one k_atrous launch per iteration between two colour buffers,
// guided by those planes (the rule: include/mafrix_rt.h); mfx_denoise_var runs k_atrous_var the same way
// with a variance plane beside each colour buffer, filled from the host or from the last
// mfx_sample_adaptive's accumulator, moments and tile counts (read only). All launch on the context's
// stream and touch nothing the trace calls keep: not the accumulator, the film, the moment planes, the
// sample counter, the ray counters or held render-ahead frames.
#include "mfx_ctx.h"

using namespace mfxh;

static int dn_events(mfx_ctx* c) {
    if (!c->dn.ev0) HIPCHECK(c->dn.ev0.create());
    if (!c->dn.ev1) HIPCHECK(c->dn.ev1.create());
    return MFX_OK;
}

// the call's work has been enqueued: wait for it; ms: its kernels' device time (ev0 .. ev1)
static int dn_finish(mfx_ctx* c, double* ms) {
    HIPCHECK(hipStreamSynchronize(c->stream));
    float f = 0.f;
    if (ms) HIPCHECK(hipEventElapsedTime(&f, c->dn.ev0, c->dn.ev1));
    if (ms) *ms = f;
    return MFX_OK;
}

static int dn_alloc(DevBuf<double>& p, size_t doubles, const char* who) {
    if (p) return MFX_OK;
    if (p.alloc(doubles) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MFX_E_NOMEM, std::string(who) + ": its device buffers could not be allocated");
    }
    return MFX_OK;
}

// a sigma > 0 whose square, the divisor the kernels use, has underflowed to 0: the centre tap's term
// would be 0/0 and every pixel NaN
static bool zero_square(double s) { return s > 0.0 && s * s == 0.0; }

// the feature planes belong to the current camera (mfx_set_camera leaves them as they are: stale)
static int features_current(const mfx_ctx* c, const char* who) {
    if (c->dn.feat_epoch != c->cam_epoch)
        return fail(MFX_E_STATE, std::string(who) + ": the feature buffers are another camera's (run mfx_aov again after mfx_set_camera)");
    return MFX_OK;
}

extern "C" int mfx_aov(mfx_ctx* c, int32_t spp, int64_t sample_base, double* out, double* ms) {
    if (!c) return fail(MFX_E_INVALID, "mfx_aov: null context");
    if (spp < 1) return fail(MFX_E_INVALID, "mfx_aov: spp must be >= 1");
    if (sample_base < 0) return fail(MFX_E_INVALID, "mfx_aov: sample_base must be >= 0");
    MFX_TRY(whole_film_single_device(c, "mfx_aov"));
    HIPCHECK(hipSetDevice(c->device));
    Denoise& dn = c->dn;
    MFX_TRY(dn_alloc(dn.feat, (size_t)MFX_AOV_PLANES * (size_t)c->npix, "mfx_aov"));
    if (out) MFX_TRY(dn_alloc(dn.feat_out, (size_t)MFX_AOV_PLANES * (size_t)c->npix, "mfx_aov"));
    MFX_TRY(dn_events(c));
    AovParams P;
    std::memset(&P, 0, sizeof(P));
    fill_scene_ptrs(c, P);
    P.cam = c->scene.host.camera;
    P.seed = c->seed;
    P.sample_base = sample_base;
    P.spp = spp;
    P.width = c->scene.host.width;
    P.height = c->scene.host.height;
    P.stack_size = c->scene.stack_size;
    P.feat = dn.feat;
    P.out = out ? dn.feat_out.get() : nullptr;
    P.tx = c->tex.tables();  // albedo textures: k_aov's TX instances (all null without)
    P.lens = c->lens.rec;    // a thin lens: k_aov's LENS instances trace the film's own lens rays
    P.lens_on = wf_lens(c) ? 1 : 0;
    P.sn = wf_normals(c) ? c->nrm.tables() : MfxSnTables{};  // smooth shading: k_aov's SN twins
    HIPCHECK(hipEventRecord(dn.ev0, c->stream));
    HIPCHECK(mfx_launch_aov(P, c->stream));
    HIPCHECK(hipEventRecord(dn.ev1, c->stream));
    dn.feat_epoch = c->cam_epoch;
    if (out) MFX_TRY(host_readback(c, out, dn.feat_out, sizeof(double) * MFX_AOV_PLANES * (size_t)c->npix, c->stream));
    return dn_finish(c, ms);
}

extern "C" int mfx_denoise(mfx_ctx* c, const mfx_denoise_cfg* a, const double* color_in, double* out, uint8_t* rgba, double* ms) {
    if (!c || !a) return fail(MFX_E_INVALID, "mfx_denoise: null argument");
    if (a->iterations < 1 || a->iterations > 8 || a->reserved[0] != 0 || a->reserved[1] != 0)
        return fail(MFX_E_INVALID, "mfx_denoise: need 1 <= iterations <= 8 and reserved 0");
    if (a->source != MFX_DN_SRC_HOST && a->source != MFX_DN_SRC_ACCUM)
        return fail(MFX_E_INVALID, "mfx_denoise: unknown source");
    for (double s : {a->sigma_normal, a->sigma_depth, a->sigma_albedo, a->sigma_color})
        if (!(s >= 0.0) || !std::isfinite(s)) return fail(MFX_E_INVALID, "mfx_denoise: every sigma must be finite and >= 0");
    for (double s : {a->sigma_normal, a->sigma_depth, a->sigma_albedo})
        if (zero_square(s)) return fail(MFX_E_INVALID, "mfx_denoise: a sigma > 0 must have a non-zero square");
    if (a->sigma_color > 0.0) {  // the colour term divides by sc2 * 0.25^i: the loop's own products, below
        const double sc2 = a->sigma_color * a->sigma_color;
        double quarter = 1.0;
        for (int i = 0; i < a->iterations; ++i) {
            if (sc2 * quarter == 0.0)
                return fail(MFX_E_INVALID, "mfx_denoise: sigma_color > 0 must keep (sigma_color^2) * 0.25^i non-zero at every iteration");
            quarter = quarter * 0.25;
        }
    }
    if (a->source == MFX_DN_SRC_HOST && !color_in)
        return fail(MFX_E_INVALID, "mfx_denoise: MFX_DN_SRC_HOST needs color_in");
    if (a->source == MFX_DN_SRC_ACCUM && !(a->count > 0.0))
        return fail(MFX_E_INVALID, "mfx_denoise: MFX_DN_SRC_ACCUM needs count > 0");
    MFX_TRY(whole_film_single_device(c, "mfx_denoise"));
    Denoise& dn = c->dn;
    if (!dn.ready()) return fail(MFX_E_STATE, "mfx_denoise: no feature buffers (call mfx_aov on this context first)");
    MFX_TRY(features_current(c, "mfx_denoise"));
    HIPCHECK(hipSetDevice(c->device));
    for (int k = 0; k < 2; ++k) MFX_TRY(dn_alloc(dn.buf[k], 3 * (size_t)c->npix, "mfx_denoise"));
    MFX_TRY(dn_events(c));
    const int W = c->scene.host.width, H = c->scene.host.height;
    if (a->source == MFX_DN_SRC_HOST)  // staged through the x-major frame buffer, before the timed part
        HIPCHECK(hipMemcpyAsync(c->d_frame, color_in, 4 * sizeof(double) * (size_t)c->npix, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipEventRecord(dn.ev0, c->stream));
    if (a->source == MFX_DN_SRC_HOST) HIPCHECK(mfx_launch_dn_from_frame(c->d_frame, c->npix, dn.buf[0], c->stream));
    else HIPCHECK(mfx_launch_dn_from_accum(c->d_accum, c->npix, a->count, dn.buf[0], c->stream));
    AtrousParams P;
    std::memset(&P, 0, sizeof(P));
    P.feat = dn.feat;
    P.width = W;
    P.height = H;
    P.terms = (a->sigma_normal > 0.0 ? 1 : 0) | (a->sigma_depth > 0.0 ? 2 : 0) | (a->sigma_albedo > 0.0 ? 4 : 0) |
              (a->sigma_color > 0.0 ? 8 : 0);
    P.sn2 = a->sigma_normal * a->sigma_normal;
    P.sz2 = a->sigma_depth * a->sigma_depth;
    P.sa2 = a->sigma_albedo * a->sigma_albedo;
    const double sc2 = a->sigma_color * a->sigma_color;
    double quarter = 1.0;  // 0.25^i
    int cur = 0;
    for (int i = 0; i < a->iterations; ++i) {
        P.src = dn.buf[cur];
        P.dst = dn.buf[cur ^ 1];
        P.step = 1 << i;
        P.sc2 = sc2 * quarter;
        HIPCHECK(mfx_launch_atrous(P, c->stream));
        quarter = quarter * 0.25;
        cur ^= 1;
    }
    if (out || rgba)
        HIPCHECK(mfx_launch_dn_post(dn.buf[cur], W, H, out ? c->d_frame.get() : nullptr, rgba ? c->d_rgba.get() : nullptr,
                                    c->stream));
    HIPCHECK(hipEventRecord(dn.ev1, c->stream));
    if (out) MFX_TRY(host_readback(c, out, c->d_frame, 4 * sizeof(double) * (size_t)c->npix, c->stream));
    if (rgba) MFX_TRY(host_readback(c, rgba, c->d_rgba, 4 * (size_t)c->npix, c->stream));
    return dn_finish(c, ms);
}

extern "C" int mfx_denoise_var(mfx_ctx* c, const mfx_denoise_var_cfg* a, const double* color_in, const double* variance_in,
                               double* out, double* var_out, uint8_t* rgba, double* ms) {
    if (!c || !a) return fail(MFX_E_INVALID, "mfx_denoise_var: null argument");
    if (a->iterations < 1 || a->iterations > 8 || a->reserved[0] != 0 || a->reserved[1] != 0)
        return fail(MFX_E_INVALID, "mfx_denoise_var: need 1 <= iterations <= 8 and reserved 0");
    if (a->source != MFX_DN_SRC_HOST && a->source != MFX_DN_SRC_ADAPTIVE && a->source != MFX_DN_SRC_TEMPORAL)
        return fail(MFX_E_INVALID, "mfx_denoise_var: unknown source");
    for (double s : {a->sigma_normal, a->sigma_depth, a->sigma_albedo, a->sigma_luma})
        if (!(s >= 0.0) || !std::isfinite(s)) return fail(MFX_E_INVALID, "mfx_denoise_var: every sigma must be finite and >= 0");
    for (double s : {a->sigma_normal, a->sigma_depth, a->sigma_albedo})  // (sigma_luma's square is added to luma_floor > 0)
        if (zero_square(s)) return fail(MFX_E_INVALID, "mfx_denoise_var: a sigma > 0 must have a non-zero square");
    if (!(a->luma_floor > 0.0) || !std::isfinite(a->luma_floor))
        return fail(MFX_E_INVALID, "mfx_denoise_var: luma_floor must be finite and > 0");
    const bool host = a->source == MFX_DN_SRC_HOST;
    if (host && (!color_in || !variance_in))
        return fail(MFX_E_INVALID, "mfx_denoise_var: MFX_DN_SRC_HOST needs color_in and variance_in");
    const bool temporal = a->source == MFX_DN_SRC_TEMPORAL;
    if (!host && (color_in || variance_in))
        return fail(MFX_E_INVALID, "mfx_denoise_var: MFX_DN_SRC_ADAPTIVE and MFX_DN_SRC_TEMPORAL take no color_in or variance_in");
    MFX_TRY(whole_film_single_device(c, "mfx_denoise_var"));
    Denoise& dn = c->dn;
    if (!dn.ready()) return fail(MFX_E_STATE, "mfx_denoise_var: no feature buffers (call mfx_aov on this context first)");
    MFX_TRY(features_current(c, "mfx_denoise_var"));
    if (temporal && c->tp.cur < 0) return fail(MFX_E_STATE, "mfx_denoise_var: no temporal history (call mfx_temporal first)");
    if (temporal && c->tp.epoch != dn.feat_epoch)
        return fail(MFX_E_STATE, "mfx_denoise_var: the temporal history is another camera's than the feature buffers (call mfx_temporal again)");
    if (!host && !temporal && !c->adp.accum_valid)
        return fail(MFX_E_STATE, "mfx_denoise_var: the accumulator does not hold an mfx_sample_adaptive result");
    HIPCHECK(hipSetDevice(c->device));
    for (int k = 0; k < 2; ++k) {
        MFX_TRY(dn_alloc(dn.buf[k], 3 * (size_t)c->npix, "mfx_denoise_var"));
        MFX_TRY(dn_alloc(dn.var[k], (size_t)c->npix, "mfx_denoise_var"));
    }
    MFX_TRY(dn_events(c));
    const int W = c->scene.host.width, H = c->scene.host.height;
    if (host) {  // staged before the timed part: the frame through the x-major frame buffer, the variance as the plane it is
        HIPCHECK(hipMemcpyAsync(c->d_frame, color_in, 4 * sizeof(double) * (size_t)c->npix, hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(dn.var[0], variance_in, sizeof(double) * (size_t)c->npix, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHECK(hipEventRecord(dn.ev0, c->stream));
    if (host) HIPCHECK(mfx_launch_dn_from_frame(c->d_frame, c->npix, dn.buf[0], c->stream));
    else if (!temporal) HIPCHECK(mfx_launch_dn_from_adaptive(c->d_accum, c->adp.mom, c->adp.tile_spp, W, H, dn.buf[0], dn.var[0], c->stream));
    AtrousVarParams P;
    std::memset(&P, 0, sizeof(P));
    P.feat = dn.feat;
    P.width = W;
    P.height = H;
    P.terms = (a->sigma_normal > 0.0 ? 1 : 0) | (a->sigma_depth > 0.0 ? 2 : 0) | (a->sigma_albedo > 0.0 ? 4 : 0) |
              (a->sigma_luma > 0.0 ? 8 : 0);
    P.sn2 = a->sigma_normal * a->sigma_normal;
    P.sz2 = a->sigma_depth * a->sigma_depth;
    P.sa2 = a->sigma_albedo * a->sigma_albedo;
    P.sl2 = a->sigma_luma * a->sigma_luma;
    P.luma_floor = a->luma_floor;
    // the first iteration reads the source where it lies: buffer 0, or the temporal history's colour and variance planes
    const double* hist = temporal ? c->tp.hist[c->tp.cur].get() : nullptr;
    P.src = temporal ? hist + MFX_TP_COLOR * (size_t)c->npix : dn.buf[0].get();
    P.vsrc = temporal ? hist + MFX_TP_VAR * (size_t)c->npix : dn.var[0].get();
    int cur = temporal ? 1 : 0;  // the buffer an iteration leaves its output in is cur ^ 1
    for (int i = 0; i < a->iterations; ++i) {
        P.dst = dn.buf[cur ^ 1];
        P.vdst = dn.var[cur ^ 1];
        P.step = 1 << i;
        HIPCHECK(mfx_launch_atrous_var(P, c->stream));
        cur ^= 1;
        P.src = dn.buf[cur];
        P.vsrc = dn.var[cur];
    }
    if (out || rgba)
        HIPCHECK(mfx_launch_dn_post(dn.buf[cur], W, H, out ? c->d_frame.get() : nullptr, rgba ? c->d_rgba.get() : nullptr,
                                    c->stream));
    HIPCHECK(hipEventRecord(dn.ev1, c->stream));
    if (out) MFX_TRY(host_readback(c, out, c->d_frame, 4 * sizeof(double) * (size_t)c->npix, c->stream));
    if (var_out) MFX_TRY(host_readback(c, var_out, dn.var[cur], sizeof(double) * (size_t)c->npix, c->stream));  // x-major as it lies
    if (rgba) MFX_TRY(host_readback(c, rgba, c->d_rgba, 4 * (size_t)c->npix, c->stream));
    return dn_finish(c, ms);
}

extern "C" int mfx_temporal(mfx_ctx* c, const mfx_temporal_cfg* a, const double* color_in, const double* variance_in,
                            const double* count_in, double* out, double* var_out, double* count_out, uint8_t* rgba,
                            int64_t* accepted, double* ms) {
    if (!c || !a) return fail(MFX_E_INVALID, "mfx_temporal: null argument");
    if (a->reserved[0] != 0 || a->reserved[1] != 0) return fail(MFX_E_INVALID, "mfx_temporal: reserved must be 0");
    if (a->source != MFX_DN_SRC_HOST && a->source != MFX_DN_SRC_ADAPTIVE)
        return fail(MFX_E_INVALID, "mfx_temporal: unknown source");
    if (!(a->tol_depth >= 0.0) || !std::isfinite(a->tol_depth) || !(a->tol_normal2 >= 0.0) || !std::isfinite(a->tol_normal2))
        return fail(MFX_E_INVALID, "mfx_temporal: tol_depth and tol_normal2 must be finite and >= 0");
    if (!(a->max_history > 0.0) || !std::isfinite(a->max_history))
        return fail(MFX_E_INVALID, "mfx_temporal: max_history must be finite and > 0");
    const bool host = a->source == MFX_DN_SRC_HOST;
    if (host && (!color_in || !variance_in || !count_in))
        return fail(MFX_E_INVALID, "mfx_temporal: MFX_DN_SRC_HOST needs color_in, variance_in and count_in");
    if (!host && (color_in || variance_in || count_in))
        return fail(MFX_E_INVALID, "mfx_temporal: MFX_DN_SRC_ADAPTIVE takes no color_in, variance_in or count_in");
    if (host)
        for (int64_t q = 0; q < c->npix; ++q)
            if (!std::isfinite(count_in[q])) return fail(MFX_E_INVALID, "mfx_temporal: count_in must be finite");
    MFX_TRY(whole_film_single_device(c, "mfx_temporal"));
    // (its reprojection sends a world point through the pinhole; the history stays as it is)
    if (wf_lens(c)) return fail(MFX_E_STATE, "mfx_temporal: the context has a lens (mfx_set_lens): the reprojection is the pinhole's");
    Denoise& dn = c->dn;
    Temporal& tp = c->tp;
    if (!dn.ready()) return fail(MFX_E_STATE, "mfx_temporal: no feature buffers (call mfx_aov on this context first)");
    MFX_TRY(features_current(c, "mfx_temporal"));
    if (!host && !c->adp.accum_valid)
        return fail(MFX_E_STATE, "mfx_temporal: the accumulator does not hold an mfx_sample_adaptive result");
    HIPCHECK(hipSetDevice(c->device));
    const size_t npix = (size_t)c->npix;
    MFX_TRY(dn_alloc(dn.buf[0], 3 * npix, "mfx_temporal"));
    MFX_TRY(dn_alloc(dn.var[0], npix, "mfx_temporal"));
    for (int k = 0; k < 2; ++k) MFX_TRY(dn_alloc(tp.hist[k], (size_t)MFX_TP_PLANES * npix, "mfx_temporal"));
    MFX_TRY(dn_alloc(tp.count_in, npix, "mfx_temporal"));
    if (!tp.accepted && tp.accepted.alloc(1) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MFX_E_NOMEM, "mfx_temporal: its device buffers could not be allocated");
    }
    MFX_TRY(dn_events(c));
    const int W = c->scene.host.width, H = c->scene.host.height;
    if (host) {  // staged before the timed part, as mfx_denoise_var's
        HIPCHECK(hipMemcpyAsync(c->d_frame, color_in, 4 * sizeof(double) * npix, hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(dn.var[0], variance_in, sizeof(double) * npix, hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(tp.count_in, count_in, sizeof(double) * npix, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHECK(hipMemsetAsync(tp.accepted, 0, sizeof(unsigned long long), c->stream));
    HIPCHECK(hipEventRecord(dn.ev0, c->stream));
    if (host) HIPCHECK(mfx_launch_dn_from_frame(c->d_frame, c->npix, dn.buf[0], c->stream));
    else HIPCHECK(mfx_launch_dn_from_adaptive(c->d_accum, c->adp.mom, c->adp.tile_spp, W, H, dn.buf[0], dn.var[0], c->stream));
    const bool have = tp.cur >= 0 && a->restart == 0;
    const int dst = tp.cur >= 0 ? tp.cur ^ 1 : 0;
    TemporalParams P;
    std::memset(&P, 0, sizeof(P));
    P.color = dn.buf[0];
    P.var = dn.var[0];
    P.count = host ? tp.count_in.get() : nullptr;
    P.tile_spp = host ? nullptr : c->adp.tile_spp.get();
    P.feat = dn.feat;
    P.hist = have ? tp.hist[tp.cur].get() : nullptr;
    P.hist_out = tp.hist[dst];
    P.accepted = tp.accepted;
    P.cam = c->scene.host.camera;
    P.hcam = have ? tp.cam : c->scene.host.camera;
    P.width = W;
    P.height = H;
    P.tol_depth2 = a->tol_depth * a->tol_depth;
    P.tol_normal2 = a->tol_normal2;
    P.max_history = a->max_history;
    HIPCHECK(mfx_launch_temporal(P, c->stream));
    // the history is now the merged result in the current view (the buffers swap by index: no copy)
    tp.cur = dst;
    tp.cam = c->scene.host.camera;
    tp.epoch = c->cam_epoch;
    const double* hist = tp.hist[dst];
    if (out || rgba)
        HIPCHECK(mfx_launch_dn_post(hist + MFX_TP_COLOR * npix, W, H, out ? c->d_frame.get() : nullptr,
                                    rgba ? c->d_rgba.get() : nullptr, c->stream));
    HIPCHECK(hipEventRecord(dn.ev1, c->stream));
    if (out) MFX_TRY(host_readback(c, out, c->d_frame, 4 * sizeof(double) * npix, c->stream));
    if (var_out) MFX_TRY(host_readback(c, var_out, hist + MFX_TP_VAR * npix, sizeof(double) * npix, c->stream));
    if (count_out) MFX_TRY(host_readback(c, count_out, hist + MFX_TP_COUNT * npix, sizeof(double) * npix, c->stream));
    if (rgba) MFX_TRY(host_readback(c, rgba, c->d_rgba, 4 * npix, c->stream));
    unsigned long long took = 0;
    if (accepted) HIPCHECK(hipMemcpyAsync(&took, tp.accepted, sizeof(took), hipMemcpyDeviceToHost, c->stream));
    MFX_TRY(dn_finish(c, ms));
    if (accepted) *accepted = (int64_t)took;
    return MFX_OK;
}
