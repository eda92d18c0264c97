// mfx_environment.cpp — the sky on the host (include/mafrix_rt.h, mfx_set_environment): what is refused, the
// texels' copy to every device, what a change invalidates, mfx_environment_info and the host twin of the
// kernels' texel rule (mfx_env_texel_index; the rule itself: mfx_environment.h).
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

// The pool's layout depends on whether there is a sky (the miss-record plane): a change of that lets the pool
// go, and the next trace allocates the one a context in the new state has.
static void release_pool(mfx_ctx* d) {
    WfPool& wp = d->pool;
    wp.mem.reset();
    wp.slots = 0;
    wp.bytes = 0;
    wp.queues = false;
    wp.params = WfParams{};
}

extern "C" {
int mfx_set_environment(mfx_ctx* c, const mfx_environment* env) {
    if (!c) return fail(MFX_E_INVALID, "mfx_set_environment: null context");
    if (c->flags & (MFX_F_MEGAKERNEL | MFX_F_COUNT_STATS))
        return fail(MFX_E_STATE, "mfx_set_environment: a context created with MFX_F_MEGAKERNEL or MFX_F_COUNT_STATS "
                                 "has no environment instances");
    size_t n = 0;
    if (env) {
        if (env->size < 1 || env->size > MFX_MAX_ENV_SIZE) return bad_size("mfx_set_environment", env->size);
        if (!env->rgb) return fail(MFX_E_INVALID, "mfx_set_environment: rgb is NULL");
        n = (size_t)env->size * (size_t)env->size;
        for (size_t k = 0; k < 3 * n; ++k) {
            const float v = env->rgb[k];
            if (std::isfinite(v) && v >= 0.f) continue;
            const size_t id = k / 3;
            return fail(MFX_E_INVALID, "mfx_set_environment: texel " + std::to_string(id) + " (x " + std::to_string(id % env->size) +
                                           ", y " + std::to_string(id / env->size) + ") channel " + std::to_string(k % 3) +
                                           (std::isfinite(v) ? " is negative" : " is not finite"));
        }
    }
    if (!env && !wf_env(c)) return MFX_OK;  // none before, none now: nothing to do
    // held render-ahead frames are the old sky's: the film comes back to d_film under it, and the frames' epoch
    // ends; then everything the context has enqueued, a background batch included, finishes
    MFX_TRY(ahead_break(c));
    MFX_TRY(mfx_sync(c));
    for (mfx_ctx* d : devs_of(c)) {
        HIPCHECK(hipSetDevice(d->device));
        const bool was = wf_env(d);
        if (!env) {
            d->sky = Environment{};
        } else {
            if (d->sky.size != env->size) {
                d->sky.size = 0;
                HIP_TRY(d->sky.d_rgb.alloc(3 * n), _e == hipErrorOutOfMemory ? MFX_E_NOMEM : MFX_E_DEVICE, "mfx_set_environment: ");
            }
            HIPCHECK(hipMemcpy(d->sky.d_rgb, env->rgb, 3 * n * sizeof(float), hipMemcpyHostToDevice));
            d->sky.size = env->size;
        }
        if (was != wf_env(d)) release_pool(d);
    }
    HIPCHECK(hipSetDevice(c->device));
    c->adp.accum_valid = false;  // a resume must not mix skies
    c->ahead.dfilm_buf = -1;
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
