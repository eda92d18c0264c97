// mfx_adaptive.cpp — mfx_sample_adaptive: mfx_sample with a per-tile early stop (the rule:
// include/mafrix_rt.h). The host drives one pass at a time: a listed wavefront trace of the active
// tiles (wf_trace's TileList: `ns` samples from one sample base, k_resolve's moments instance), the
// tile check and the compaction of the tiles that go on (mfx_wf_tile_check), then a read of the 4-byte
// active count, which is the pass's only host round trip. The lists ping-pong between two buffers of
// one entry per tile; the pool is the first pass's (no pass runs larger generations), so it is
// allocated once. A pixel's samples are summed by its own k_resolve thread in sample order across the
// passes, so its sum over n samples is mfx_sample(n)'s.
// mfx_sample_adaptive_resume continues that result: the same loop with an entry check in front, the
// tiles' own counts as their sample bases (TileList::tile_n; k_tile_check_n keeps them), a pass limit,
// and a second word in the readback, the most samples a surviving tile gets, which sizes the next pass.
#include "mfx_ctx.h"

using namespace mfxh;

static int adaptive_alloc(mfx_ctx* c, int64_t ntiles) {
    Adaptive& a = c->adp;
    if (a.ready()) return MFX_OK;
    const size_t nt = (size_t)ntiles;
    const bool ok = a.mom.alloc(2 * (size_t)c->npix) == hipSuccess && a.tiles[0].alloc(nt) == hipSuccess &&
                    a.tiles[1].alloc(nt) == hipSuccess && a.tile_flags.alloc(nt) == hipSuccess &&
                    a.tile_spp.alloc(nt) == hipSuccess && a.tile_count.alloc(16) == hipSuccess &&
                    a.ev0.create() == hipSuccess && a.ev1.create() == hipSuccess;  // ev1 last: ready()
    if (!ok) {
        (void)hipGetLastError();
        return fail(MFX_E_NOMEM, "mfx_sample_adaptive: the moment planes and tile lists could not be allocated");
    }
    return MFX_OK;
}

// MFX_ADAPTIVE_CHECK=1 (debug): a pass's list as the device compacted it — n entries, strictly
// ascending, every one a tile of the film (list_tile_xy, the function the kernels map it with)
static int adaptive_check_list(mfx_ctx* c, const int32_t* d_list, int32_t n, int32_t prev_n) {
    const unsigned tiles_x = (unsigned)(c->scene.host.width + 7) / 8, tiles_y = (unsigned)(c->scene.host.height + 7) / 8;
    if (n < 0 || n > prev_n) return fail(MFX_E_DEVICE, "mfx_sample_adaptive: active tile count out of range");
    std::vector<int32_t> h((size_t)n);
    if (n > 0) HIPCHECK(hipMemcpy(h.data(), d_list, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    for (int32_t k = 0; k < n; ++k) {
        unsigned tx, ty;
        if (h[k] < 0 || !list_tile_xy((unsigned)h[k], tiles_x, tiles_y, tx, ty) || (k > 0 && h[k] <= h[k - 1]))
            return fail(MFX_E_DEVICE, "mfx_sample_adaptive: corrupt tile list at entry " + std::to_string(k));
    }
    return MFX_OK;
}

extern "C" int mfx_sample_adaptive(mfx_ctx* c, const mfx_adaptive* a, double* frame, int32_t* tile_spp, uint8_t* rgba) {
    if (!c || !a) return fail(MFX_E_INVALID, "mfx_sample_adaptive: null argument");
    if (a->min_spp < 2 || a->max_spp < a->min_spp || a->step_spp < 1 || a->reserved != 0)
        return fail(MFX_E_INVALID, "mfx_sample_adaptive: need 2 <= min_spp <= max_spp, step_spp >= 1, reserved 0");
    if (!(a->rel_error >= 0.0) || !std::isfinite(a->rel_error) || !(a->abs_floor >= 0.0) || !std::isfinite(a->abs_floor))
        return fail(MFX_E_INVALID, "mfx_sample_adaptive: rel_error and abs_floor must be finite and >= 0");
    MFX_TRY(whole_film_single_device(c, "mfx_sample_adaptive"));
    if (c->flags & MFX_F_MEGAKERNEL)
        return fail(MFX_E_STATE, "mfx_sample_adaptive runs the wavefront pipeline (context has MFX_F_MEGAKERNEL)");
    HIPCHECK(hipSetDevice(c->device));
    MFX_TRY(ahead_break(c));  // it moves the sample sequence past held frames
    const int W = c->scene.host.width, H = c->scene.host.height;
    const int64_t nt64 = (int64_t)((W + 7) / 8) * ((H + 7) / 8);
    const int32_t ntiles = (int32_t)nt64;
    MFX_TRY(adaptive_alloc(c, nt64));
    MFX_TRY(mfx_accum_clear(c));
    Adaptive& ad = c->adp;
    HIPCHECK(hipMemsetAsync(ad.mom, 0, 2 * sizeof(double) * (size_t)c->npix, c->stream));
    HIPCHECK(hipMemsetAsync(ad.tile_spp, 0, sizeof(int32_t) * (size_t)ntiles, c->stream));
    {
        std::vector<int32_t> all((size_t)ntiles);
        for (int32_t k = 0; k < ntiles; ++k) all[k] = k;
        HIPCHECK(hipMemcpy(ad.tiles[0], all.data(), sizeof(int32_t) * (size_t)ntiles, hipMemcpyHostToDevice));
    }
    c->rep_valid = false;
    c->mega_last = false;
    double counts[16] = {0}, stage[8] = {0}, ms = 0.0;
    auto lap = [&]() -> int {  // ev0 .. ev1 have completed: add their device time
        float f = 0.f;
        HIPCHECK(hipEventElapsedTime(&f, ad.ev0, ad.ev1));
        ms += f;
        return MFX_OK;
    };
    const int64_t first = nt64 * 64 * a->min_spp;
    int32_t active = ntiles, done = 0;
    int cur = 0;
    while (active > 0) {
        const int32_t ns = done == 0 ? a->min_spp : std::min(a->step_spp, a->max_spp - done);
        HIPCHECK(hipEventRecord(ad.ev0, c->stream));
        HIPCHECK(hipMemsetAsync(c->d_counters, 0, kCounterBytes, c->stream));
        MFX_TRY(wf_trace(c, ns, c->next_sample + done, TileList{ad.tiles[cur], active, ad.mom, (first + 4095) / 4096 * 4096}));
        HIPCHECK(mfx_launch_counters_add(c->d_counters_total, c->d_counters, WF_NCTR * WF_SHARDS, c->stream));
        done += ns;
        TileCheckParams K{};
        K.tiles = ad.tiles[cur];
        K.ntiles = active;
        K.n = done;
        K.max_spp = a->max_spp;
        K.width = W;
        K.height = H;
        K.rel2 = a->rel_error * a->rel_error;
        K.abs_floor = a->abs_floor;
        K.mom = ad.mom;
        K.tile_spp = ad.tile_spp;
        K.flags = ad.tile_flags;
        K.next = ad.tiles[cur ^ 1];
        K.next_count = ad.tile_count;
        HIPCHECK(mfx_wf_tile_check(K, c->stream));
        HIPCHECK(hipEventRecord(ad.ev1, c->stream));
        int32_t next_active = 0;
        HIPCHECK(hipMemcpyAsync(c->h_counters, c->d_counters, kCounterBytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(&next_active, ad.tile_count, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        sum_counters(c->h_counters, counts);
        if (c->pool.auto_pending) {  // the context's first wavefront trace settles the automatic queue start
            note_live(c, c->h_counters);
            c->pool.auto_pending = false;
            c->pool.auto_read = true;
        }
        MFX_TRY(lap());
        MFX_TRY(add_stage_times(c, stage));
        if (ad.check) MFX_TRY(adaptive_check_list(c, ad.tiles[cur ^ 1], next_active, active));
        if (next_active < 0 || next_active > active || (done >= a->max_spp && next_active != 0))
            return fail(MFX_E_DEVICE, "mfx_sample_adaptive: active tile count out of range");
        active = next_active;
        cur ^= 1;
    }
    ad.B = c->next_sample;
    ad.R = a->max_spp;
    ad.gen_paths = (first + 4095) / 4096 * 4096;
    c->next_sample += a->max_spp;
    HIPCHECK(hipEventRecord(ad.ev0, c->stream));
    HIPCHECK(mfx_launch_adaptive_mean(c->d_accum, ad.tile_spp, W, H, frame ? c->d_frame.get() : nullptr,
                                      rgba ? c->d_rgba.get() : nullptr, c->stream));
    HIPCHECK(hipEventRecord(ad.ev1, c->stream));
    if (frame) MFX_TRY(host_readback(c, frame, c->d_frame, 4 * sizeof(double) * (size_t)c->npix, c->stream));
    if (rgba) MFX_TRY(host_readback(c, rgba, c->d_rgba, 4 * (size_t)c->npix, c->stream));
    if (tile_spp)
        HIPCHECK(hipMemcpyAsync(tile_spp, ad.tile_spp, sizeof(int32_t) * (size_t)ntiles, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    MFX_TRY(lap());
    // the call's statistics: the sum over its passes (mfx_ray_counts, mfx_stats, mfx_last_trace_ms)
    counts[3] = counts[0];
    for (int k = 0; k < 16; ++k) c->rep_counts[k] = counts[k];
    for (int k = 0; k < 8; ++k) c->rep_timing[k] = stage[k];
    c->rep_ms = ms;
    c->rep_valid = true;
    ad.accum_valid = true;  // the accumulator, the moments and tile_spp belong together (mfx_denoise_var's device source)
    return MFX_OK;
}

extern "C" int mfx_sample_adaptive_resume(mfx_ctx* c, const mfx_adaptive_resume* a, double* frame, int32_t* tile_spp,
                                          uint8_t* rgba, int32_t* active_out) {
    const char* who = "mfx_sample_adaptive_resume";
    if (!c || !a) return fail(MFX_E_INVALID, "mfx_sample_adaptive_resume: null argument");
    if (a->max_spp < 2 || a->step_spp < 1 || a->max_passes < 0 || a->reserved != 0)
        return fail(MFX_E_INVALID, "mfx_sample_adaptive_resume: need max_spp >= 2, step_spp >= 1, max_passes >= 0, reserved 0");
    if (!(a->rel_error >= 0.0) || !std::isfinite(a->rel_error) || !(a->abs_floor >= 0.0) || !std::isfinite(a->abs_floor))
        return fail(MFX_E_INVALID, "mfx_sample_adaptive_resume: rel_error and abs_floor must be finite and >= 0");
    MFX_TRY(whole_film_single_device(c, who));
    if (c->flags & MFX_F_MEGAKERNEL)
        return fail(MFX_E_STATE, "mfx_sample_adaptive_resume runs the wavefront pipeline (context has MFX_F_MEGAKERNEL)");
    HIPCHECK(hipSetDevice(c->device));
    MFX_TRY(ahead_break(c));  // as mfx_sample_adaptive; a held frame's trace takes the result's validity with it
    Adaptive& ad = c->adp;
    if (!ad.ready() || !ad.accum_valid)
        return fail(MFX_E_STATE, "mfx_sample_adaptive_resume: the context holds no adaptive result (none yet, or a trace, "
                                 "mfx_accum_clear or mfx_accum_attach since)");
    if (c->next_sample != ad.B + ad.R)
        return fail(MFX_E_STATE, "mfx_sample_adaptive_resume: samples were drawn since the adaptive result (next_sample moved)");
    const int W = c->scene.host.width, H = c->scene.host.height;
    const int32_t ntiles = (int32_t)((int64_t)((W + 7) / 8) * ((H + 7) / 8));
    {
        std::vector<int32_t> all((size_t)ntiles);
        for (int32_t k = 0; k < ntiles; ++k) all[k] = k;
        HIPCHECK(hipMemcpy(ad.tiles[0], all.data(), sizeof(int32_t) * (size_t)ntiles, hipMemcpyHostToDevice));
    }
    c->rep_valid = false;
    c->mega_last = false;
    double counts[16] = {0}, stage[8] = {0}, ms = 0.0;
    auto lap = [&]() -> int {  // ev0 .. ev1 have completed: add their device time
        float f = 0.f;
        HIPCHECK(hipEventElapsedTime(&f, ad.ev0, ad.ev1));
        ms += f;
        return MFX_OK;
    };
    int32_t active = ntiles, cnt = 0;  // the current list's tiles; the most samples one of them gets in the next pass
    int cur = 0;
    // the check of list `cur` after a pass of at most pass_spp samples per tile (0: the entry check), the
    // compaction into the other list and the read of {tiles that go on, their largest share}
    auto check = [&](int32_t pass_spp) -> int {
        TileCheckParams K{};
        K.tiles = ad.tiles[cur];
        K.ntiles = active;
        K.max_spp = a->max_spp;
        K.width = W;
        K.height = H;
        K.rel2 = a->rel_error * a->rel_error;
        K.abs_floor = a->abs_floor;
        K.mom = ad.mom;
        K.tile_spp = ad.tile_spp;
        K.flags = ad.tile_flags;
        K.next = ad.tiles[cur ^ 1];
        K.next_count = ad.tile_count;
        K.per_tile = 1;
        K.pass_spp = pass_spp;
        K.step_spp = a->step_spp;
        HIPCHECK(mfx_wf_tile_check(K, c->stream));
        HIPCHECK(hipEventRecord(ad.ev1, c->stream));
        int32_t next[2] = {0, 0};
        if (pass_spp > 0) HIPCHECK(hipMemcpyAsync(c->h_counters, c->d_counters, kCounterBytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(next, ad.tile_count, sizeof(next), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        MFX_TRY(lap());
        if (ad.check) MFX_TRY(adaptive_check_list(c, ad.tiles[cur ^ 1], next[0], active));
        if (next[0] < 0 || next[0] > active || (next[0] > 0 && (next[1] < 1 || next[1] > a->step_spp)))
            return fail(MFX_E_DEVICE, "mfx_sample_adaptive_resume: active tile count or pass size out of range");
        active = next[0];
        cnt = next[1];
        cur ^= 1;
        return MFX_OK;
    };
    HIPCHECK(hipEventRecord(ad.ev0, c->stream));
    MFX_TRY(check(0));
    for (int32_t pass = 0; active > 0 && (a->max_passes == 0 || pass < a->max_passes); ++pass) {
        HIPCHECK(hipEventRecord(ad.ev0, c->stream));
        HIPCHECK(hipMemsetAsync(c->d_counters, 0, kCounterBytes, c->stream));
        MFX_TRY(wf_trace(c, cnt, ad.B, TileList{ad.tiles[cur], active, ad.mom, ad.gen_paths, ad.tile_spp, a->max_spp}));
        HIPCHECK(mfx_launch_counters_add(c->d_counters_total, c->d_counters, WF_NCTR * WF_SHARDS, c->stream));
        MFX_TRY(check(cnt));
        sum_counters(c->h_counters, counts);
        if (c->pool.auto_pending) {  // the context's first wavefront trace settles the automatic queue start
            note_live(c, c->h_counters);
            c->pool.auto_pending = false;
            c->pool.auto_read = true;
        }
        MFX_TRY(add_stage_times(c, stage));
    }
    if (a->max_spp > ad.R) {  // the budget grows: later calls draw samples no pixel has used
        c->next_sample += a->max_spp - ad.R;
        ad.R = a->max_spp;
    }
    if (active_out) *active_out = active;
    HIPCHECK(hipEventRecord(ad.ev0, c->stream));
    HIPCHECK(mfx_launch_adaptive_mean(c->d_accum, ad.tile_spp, W, H, frame ? c->d_frame.get() : nullptr,
                                      rgba ? c->d_rgba.get() : nullptr, c->stream));
    HIPCHECK(hipEventRecord(ad.ev1, c->stream));
    if (frame) MFX_TRY(host_readback(c, frame, c->d_frame, 4 * sizeof(double) * (size_t)c->npix, c->stream));
    if (rgba) MFX_TRY(host_readback(c, rgba, c->d_rgba, 4 * (size_t)c->npix, c->stream));
    if (tile_spp)
        HIPCHECK(hipMemcpyAsync(tile_spp, ad.tile_spp, sizeof(int32_t) * (size_t)ntiles, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    MFX_TRY(lap());
    counts[3] = counts[0];
    for (int k = 0; k < 16; ++k) c->rep_counts[k] = counts[k];
    for (int k = 0; k < 8; ++k) c->rep_timing[k] = stage[k];
    c->rep_ms = ms;
    c->rep_valid = true;
    ad.accum_valid = true;  // (a pass's trace cleared it)
    return MFX_OK;
}
