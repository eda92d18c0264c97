// mfx_environment.cpp — the sky on the host (include/mafrix_rt.h, mfx_set_environment): what is refused, the
// texels' copy to every device, what a change invalidates, mfx_environment_info and the host twin of the
// kernels' texel rule (mfx_env_texel_index; the rule itself: mfx_environment.h). And the sky as a light
// (mfx_set_environment_sampled): the sampling table, built here, mfx_sky_sampling_info and the host twins of
// the table and the direction rule (mfx_env_sample_table, mfx_env_sample_direction).
#include "mfx_ctx.h"

using namespace mfxh;

static_assert(MFX_ENV_SIZE_MAX == MFX_MAX_ENV_SIZE, "the kernels' texel id width is the ABI's bound");
static_assert((int64_t)MFX_ENV_SIZE_MAX * MFX_ENV_SIZE_MAX <= (int64_t)MFX_ENV_ID_MASK + 1, "a texel id is 24 bits");
static_assert(WF_MAX_VERTS <= 1 << (32 - MFX_ENV_NV_SHIFT) && (uint32_t)(WF_MAX_VERTS - 1) << MFX_ENV_NV_SHIFT < MFX_ENV_NONE - MFX_ENV_ID_MASK,
              "a miss record (id | nv << 24, nv < WF_MAX_VERTS) is never MFX_ENV_NONE");

static int bad_size(const char* who, int32_t size) {
    return fail(MFX_E_INVALID, std::string(who) + ": size " + std::to_string(size) + " is outside [1, " +
                                   std::to_string(MFX_MAX_ENV_SIZE) + "]");
}

// The pool's layout depends on whether there is a sky (the miss-record plane) and whether it is sampled: a change of that lets the pool
// go, and the next trace allocates the one a context in the new state has.
static void release_pool(mfx_ctx* d) {
    WfPool& wp = d->pool;
    wp.mem.reset();
    wp.slots = 0;
    wp.bytes = 0;
    wp.queues = false;
    wp.params = WfParams{};
}

// what mfx_set_environment refuses of a map (who: the entry point named in the message)
static int check_map(const char* who, const mfx_environment* env) {
    const std::string w(who);
    if (env->size < 1 || env->size > MFX_MAX_ENV_SIZE) return bad_size(who, env->size);
    if (!env->rgb) return fail(MFX_E_INVALID, w + ": rgb is NULL");
    const size_t n = (size_t)env->size * (size_t)env->size;
    for (size_t k = 0; k < 3 * n; ++k) {
        const float v = env->rgb[k];
        if (std::isfinite(v) && v >= 0.f) continue;
        const size_t id = k / 3;
        return fail(MFX_E_INVALID, w + ": texel " + std::to_string(id) + " (x " + std::to_string(id % env->size) +
                                       ", y " + std::to_string(id / env->size) + ") channel " + std::to_string(k % 3) +
                                       (std::isfinite(v) ? " is negative" : " is not finite"));
    }
    return MFX_OK;
}

// The sampling table of a checked map (include/mafrix_rt.h, mfx_set_environment_sampled): the weights
// w_t = ((r + g) + b) * (1 / (len2_c * len_c)), an alias table over them by Vose's method with its worklists in
// texel order (deterministic), q narrowed to float, and per texel the probability the two arrays imply, summed
// from the arrays themselves in increasing k.
static void build_sky_table(const mfx_environment* env, std::vector<MfxSkyEntry>& tab) {
    const int size = env->size;
    const size_t n = (size_t)size * (size_t)size;
    std::vector<double> w(n);
    bool any = false;
    for (size_t t = 0; t < n; ++t) {
        double u3[3], len2, len;
        mfx_env_sample_dir((uint32_t)t, 0.5, 0.5, size, u3, len2, len);
        const float* e = env->rgb + 3 * t;
        w[t] = (((double)e[0] + (double)e[1]) + (double)e[2]) * (1.0 / (len2 * len));
        any = any || w[t] > 0.0;
    }
    if (!any) std::fill(w.begin(), w.end(), 1.0);  // a black map: the uniform table
    double sum = 0.0;
    size_t heavy = 0;
    for (size_t t = 0; t < n; ++t) {
        sum += w[t];
        if (w[t] > w[heavy]) heavy = t;
    }
    tab.assign(n, MfxSkyEntry{1.f, 0u, 0.0});
    std::vector<double> p(n);
    std::vector<uint32_t> small, large;
    for (size_t t = 0; t < n; ++t) {
        tab[t].alias = (uint32_t)t;
        p[t] = w[t] * (double)n / sum;
        (p[t] < 1.0 ? small : large).push_back((uint32_t)t);
    }
    size_t si = 0;
    while (si < small.size() && !large.empty()) {  // (small grows as a large one falls below 1; each entry is settled once)
        const uint32_t l = small[si++], g = large.back();
        tab[l].q = (float)p[l];
        tab[l].alias = g;
        p[g] = (p[g] + p[l]) - 1.0;
        if (p[g] < 1.0) {
            large.pop_back();
            small.push_back(g);
        }
    }
    // what is left is 1 up to rounding: q = 1, its own alias. (A weightless texel left over, which only rounding
    // could do, keeps q = 0 and hands its share to the heaviest texel: it is never returned.)
    for (; si < small.size(); ++si)
        if (!(w[small[si]] > 0.0)) {
            tab[small[si]].q = 0.f;
            tab[small[si]].alias = (uint32_t)heavy;
        }
    for (size_t t = 0; t < n; ++t) tab[t].prob = (double)tab[t].q;
    for (size_t k = 0; k < n; ++k)
        if (tab[k].alias != k) tab[tab[k].alias].prob += 1.0 - (double)tab[k].q;
    for (size_t t = 0; t < n; ++t) tab[t].prob = tab[t].prob / (double)n;
}

// mfx_set_environment (sampled == false) and mfx_set_environment_sampled
static int set_env(mfx_ctx* c, const mfx_environment* env, bool sampled, const char* who) {
    const std::string w(who);
    if (!c) return fail(MFX_E_INVALID, w + ": null context");
    if (c->flags & (MFX_F_MEGAKERNEL | MFX_F_COUNT_STATS))
        return fail(MFX_E_STATE, w + ": a context created with MFX_F_MEGAKERNEL or MFX_F_COUNT_STATS "
                                     "has no environment instances");
    size_t n = 0;
    std::vector<MfxSkyEntry> tab;
    if (env) {
        MFX_TRY(check_map(who, env));
        n = (size_t)env->size * (size_t)env->size;
        if (sampled) {
            const size_t nl = c->scene.host.lights.size();
            if (nl > MFX_MAX_SKY_LIGHTS)
                return fail(MFX_E_STATE, w + ": the context has " + std::to_string(nl) + " lights; beside a sampled sky at most " +
                                             std::to_string(MFX_MAX_SKY_LIGHTS) + " (the sky takes light index N)");
            build_sky_table(env, tab);
        }
    }
    if (!env && !wf_env(c)) return MFX_OK;  // none before, none now: nothing to do
    sampled = sampled && env;
    // held render-ahead frames are the old sky's: the film comes back to d_film under it, and the frames' epoch
    // ends; then everything the context has enqueued, a background batch included, finishes
    MFX_TRY(ahead_break(c));
    MFX_TRY(mfx_sync(c));
    for (mfx_ctx* d : devs_of(c)) {
        HIPCHECK(hipSetDevice(d->device));
        const bool was = wf_env(d), was_sampled = wf_sky_sampled(d);
        if (!env) {
            d->sky = Environment{};
        } else {
            if (d->sky.size != env->size) {
                d->sky.size = 0;
                d->sky.sampled = false;
                HIP_TRY(d->sky.d_rgb.alloc(3 * n), _e == hipErrorOutOfMemory ? MFX_E_NOMEM : MFX_E_DEVICE, (w + ": ").c_str());
            }
            HIPCHECK(hipMemcpy(d->sky.d_rgb, env->rgb, 3 * n * sizeof(float), hipMemcpyHostToDevice));
            if (sampled) {
                HIP_TRY(d->sky.d_tab.alloc(n), _e == hipErrorOutOfMemory ? MFX_E_NOMEM : MFX_E_DEVICE, (w + ": ").c_str());
                HIPCHECK(hipMemcpy(d->sky.d_tab, tab.data(), n * sizeof(MfxSkyEntry), hipMemcpyHostToDevice));
            } else {
                d->sky.d_tab.reset();
            }
            d->sky.size = env->size;
            d->sky.sampled = sampled;
        }
        // the pool's layout depends on the sky's kind (the miss records; the sky vertices' texel ids, and with one
        // area light the light indices)
        if (was != wf_env(d) || was_sampled != wf_sky_sampled(d)) release_pool(d);
        if (was_sampled != wf_sky_sampled(d)) {  // the sky joins or leaves the lights: pdf_n, the table, the shapes
            set_sky_light(d->scene, wf_sky_sampled(d));
            MFX_TRY(scene_relight(d));
        }
    }
    HIPCHECK(hipSetDevice(c->device));
    c->adp.accum_valid = false;  // a resume must not mix skies
    c->ahead.dfilm_buf = -1;
    return MFX_OK;
}

extern "C" {
int mfx_set_environment(mfx_ctx* c, const mfx_environment* env) { return set_env(c, env, false, "mfx_set_environment"); }

int mfx_set_environment_sampled(mfx_ctx* c, const mfx_environment* env) {
    return set_env(c, env, true, "mfx_set_environment_sampled");
}

int mfx_sky_sampling_info(mfx_ctx* c, double out[8]) {
    if (!c || !out) return fail(MFX_E_INVALID, "mfx_sky_sampling_info: null argument");
    for (int k = 0; k < 8; ++k) out[k] = 0.0;
    if (!wf_sky_sampled(c)) return MFX_OK;
    const LaunchShapes& A = c->scene.shapes;
    const MfxHostScene& h = c->scene.host;
    int sb = 0, rb = 0;
    HIPCHECK(hipSetDevice(c->device));
    HIPCHECK(mfx_wf_kernel_occupancy(wf_lds_shape(c->scene, wf_textured(c), true, A.stack_lds_shd, A.ntop_shd, A.nslot_shd), &sb));
    HIPCHECK(mfx_wf_resolve_occupancy(true, &rb, wf_textured(c), true, true));
    const int nv = h.max_depth + 1;
    out[0] = 1.0;
    out[1] = (double)(h.lights.size() + 1);
    out[2] = (double)c->sky.size * (double)c->sky.size * (double)sizeof(MfxSkyEntry);
    // the texel ids, and with one area light the light indices a several-light context has anyway
    out[3] = (double)(WF_SKY_BYTES_PER_SLOT(nv) + (h.lights.size() < 2 ? WF_LIGHT_BYTES_PER_SLOT(nv) : 0));
    out[4] = (double)sb;
    out[5] = (double)rb;
    return MFX_OK;
}

int mfx_env_sample_table(const mfx_environment* env, float* q, uint32_t* alias, double* prob) {
    if (!env || !q || !alias || !prob) return fail(MFX_E_INVALID, "mfx_env_sample_table: null argument");
    MFX_TRY(check_map("mfx_env_sample_table", env));
    std::vector<MfxSkyEntry> tab;
    build_sky_table(env, tab);
    for (size_t t = 0; t < tab.size(); ++t) {
        q[t] = tab[t].q;
        alias[t] = tab[t].alias;
        prob[t] = tab[t].prob;
    }
    return MFX_OK;
}

int mfx_env_sample_direction(int32_t size, int64_t n, const uint32_t* texel, const double* jitter, double* out) {
    if (size < 1 || size > MFX_MAX_ENV_SIZE) return bad_size("mfx_env_sample_direction", size);
    if (n < 0 || (n > 0 && (!texel || !jitter || !out))) return fail(MFX_E_INVALID, "mfx_env_sample_direction: null argument");
    for (int64_t k = 0; k < n; ++k) {
        if (texel[k] >= (uint32_t)size * (uint32_t)size)
            return fail(MFX_E_INVALID, "mfx_env_sample_direction: texel " + std::to_string(texel[k]) + " (entry " + std::to_string(k) +
                                           ") is outside the map");
        double len2, len;
        mfx_env_sample_dir(texel[k], jitter[2 * k], jitter[2 * k + 1], size, out + 4 * k, len2, len);
        out[4 * k + 3] = len2 * len;
    }
    return MFX_OK;
}

int mfx_environment_info(mfx_ctx* c, double out[8]) {
    if (!c || !out) return fail(MFX_E_INVALID, "mfx_environment_info: null argument");
    for (int k = 0; k < 8; ++k) out[k] = 0.0;
    if (!wf_env(c)) return MFX_OK;
    const LaunchShapes& A = c->scene.shapes;
    int eb = 0, rb = 0;
    HIPCHECK(hipSetDevice(c->device));
    WfLdsShape s = wf_lds_shape(c->scene, wf_textured(c), false, A.stack_lds_ext, A.ntop_ext, A.nslot_ext);
    s.env = true;
    HIPCHECK(mfx_wf_kernel_occupancy(s, &eb));
    HIPCHECK(mfx_wf_resolve_occupancy(wf_multi_light(c), &rb, wf_textured(c), true));
    out[0] = (double)c->sky.size;
    out[1] = 1.0;
    out[2] = (double)c->sky.size * (double)c->sky.size * 3.0 * sizeof(float);
    out[3] = (double)WF_ENV_BYTES_PER_SLOT;
    out[4] = (double)eb;
    out[5] = (double)rb;
    return MFX_OK;
}

int mfx_env_texel_index(int32_t size, int64_t n, const double* dirs, uint32_t* id_out) {
    if (size < 1 || size > MFX_MAX_ENV_SIZE) return bad_size("mfx_env_texel_index", size);
    if (n < 0 || (n > 0 && (!dirs || !id_out))) return fail(MFX_E_INVALID, "mfx_env_texel_index: null argument");
    for (int64_t k = 0; k < n; ++k) id_out[k] = mfx_env_texel(dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2], size);
    return MFX_OK;
}
}  // extern "C"
