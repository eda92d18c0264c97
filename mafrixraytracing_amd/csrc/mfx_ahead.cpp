// mfx_ahead.cpp — render-ahead and mfx_render_rgba8.
//
// mfx_options.render_ahead = K > 1 with the whole sample set (part_count 1). Scene.Render
// (Scene.fs:331-333) asks for one sample per call: alone, a 1080p sample is ~21 rays per lane of a
// persistent grid plus the film/post launch and the readback per call. A sample's 1-spp image
// depends only on (seed, global sample index), so a call whose sample is not held traces the next K
// samples in one batched wavefront pass whose k_resolve runs, per pixel and in call order, each
// call's film add and post (the FP64 operations film_post_kernel runs per call, in the same order:
// k_resolve's frames mode) into K RGBA8 frames and the film after the last call: each call of the
// batch only copies its frame to the host. While a batch is served, the next one is traced in the
// background into the second buffer (the frame copies run on their own stream, so they overlap that
// trace). Every frame and the film are the bytes the one-sample path gives
// (tests/test_gpu_render_ahead.py). A buffer holds K frames (4 B per pixel each) and two films: no
// per-sample FP64 image is kept (round 3 kept one, 24 B per pixel per sample).
// Device lists: every device runs the same batches over its own band of tile rows, in its own
// buffers, film and copy stream, and a call copies each device's band rows of its frame straight
// into the caller's buffer: no FP64 buffer crosses devices, and the frames are the one-device bytes.
// The batch bookkeeping (base, n, expect, epoch, count0, reported) lives in the primary's ahead.ab[];
// the peers' hold their device buffers only.
// The frames assume the calls follow each other with nothing else touching the film. A reset, a
// render call of spp != 1 or an mfx_sample call (which moves the sample sequence) bumps film_epoch
// after bringing d_film up to date; a held batch whose frames belong to an older epoch is traced
// again from the sample the next call needs. d_film is brought up to date by tracing, film only,
// the served samples it lacks (ahead_materialize): from the prefix of the batch it already holds
// (dfilm_n), else from the film before the batch — after a batch's last call it is a copy of the
// film after it. So a caller that alternates Render and mfx_film_mean re-traces each sample once.
#include "mfx_ctx.h"

using namespace mfxh;

static void ahead_free_all(mfx_ctx* c) {
    for (mfx_ctx* d : devs_of(c)) {
        (void)hipSetDevice(d->device);
        d->ahead.release();
    }
    (void)hipSetDevice(c->device);
    c->ahead.dfilm_buf = -1;
}

// one device's buffers of `k` samples each, with the current device set
static hipError_t ahead_alloc_device(mfx_ctx* d, int nbuf, int64_t k) {
    const size_t npix = (size_t)d->npix;
    hipError_t e = hipSuccess;
    auto ok = [&e](hipError_t r) { return (e = r) == hipSuccess; };
    for (int b = 0; b < nbuf; ++b) {
        AheadBuf& B = d->ahead.ab[b];
        if (!ok(B.frames.alloc((size_t)k * 4 * npix)) || !ok(B.film_in.alloc(3 * npix)) ||
            !ok(B.film_out.alloc(3 * npix)) || !ok(B.counters.alloc(WF_NCTR * WF_SHARDS)) || !ok(B.t0.create()) ||
            !ok(B.t1.create()) || !ok(B.ready.create(hipEventDisableTiming)))
            return e;
    }
    if (!ok(d->ahead.counters_aux.alloc(WF_NCTR * WF_SHARDS)) || !ok(d->ahead.aux_ev0.create())) return e;
    return d->ahead.aux_ev1.create();
}

static int ahead_alloc(mfx_ctx* c) {
    const size_t plane = 3 * sizeof(double) * (size_t)c->npix, frame = 4 * (size_t)c->npix;
    const size_t per_sample = frame, fixed = 2 * plane + kCounterBytes;
    // Both buffers within MFX_RENDER_AHEAD_MAX_BYTES (default 2 GiB) and a quarter of the free HBM
    // per device (shared by the contexts a device list puts on one GPU): a context never takes more
    // than that for render-ahead, whatever K it asked for. K shrinks to fit two buffers (the
    // background batch) while at least 8 samples fit in each; below that one buffer of as many
    // samples as fit. At 1080p (8.3 MB per sample, 100 MB of films per buffer) K = 64 takes 1.26 GB
    // for both. Every device of a list gets the same K (the tightest device's).
    size_t cap = (size_t)2 << 30;
    if (const char* e = getenv("MFX_RENDER_AHEAD_MAX_BYTES")) cap = std::min(cap, (size_t)atoll(e));
    const std::vector<mfx_ctx*> ds = devs_of(c);
    size_t budget = cap;
    for (mfx_ctx* d : ds) {
        size_t fr = 0, tot = 0;
        HIPCHECK(hipSetDevice(d->device));
        HIPCHECK(hipMemGetInfo(&fr, &tot));
        size_t share = 0;  // contexts of this list on the same GPU
        for (mfx_ctx* o : ds) share += o->device == d->device ? 1 : 0;
        budget = std::min(budget, std::min(fr / 4, cap) / share);
    }
    HIPCHECK(hipSetDevice(c->device));
    int nbuf = 2;
    int64_t k = std::min<int64_t>(c->ahead.k, budget / 2 > fixed ? (int64_t)((budget / 2 - fixed) / per_sample) : 0);
    if (k < std::min(8, c->ahead.k)) {
        nbuf = 1;  // no background batch: one buffer of as many samples as fit
        k = budget > fixed ? (int64_t)((budget - fixed) / per_sample) : 0;
        k = std::min<int64_t>(k, c->ahead.k);
    }
    if (k < 2) return MFX_E_NOMEM;
    for (mfx_ctx* d : ds) {
        hipError_t e = hipSetDevice(d->device);
        if (e == hipSuccess) e = ahead_alloc_device(d, nbuf, k);
        if (e == hipSuccess) continue;
        (void)hipGetLastError();
        ahead_free_all(c);
        return e == hipErrorOutOfMemory ? MFX_E_NOMEM : fail(MFX_E_DEVICE, std::string("render-ahead: ") + hipGetErrorString(e));
    }
    HIPCHECK(hipSetDevice(c->device));
    c->ahead.nbuf = nbuf;
    c->ahead.cap = (int)k;
    return MFX_OK;
}

// d_film (every device's) = the film as of the last render call: a copy of the film after the
// buffer's last call, or the film before the buffer (or the prefix of the buffer's samples it
// already holds) with the buffer's samples up to that call traced again, film only (the same
// paths, added in the same order: the same bits). Its rays are not reported (no call asked for them).
int mfxh::ahead_materialize(mfx_ctx* c) {
    Ahead& a = c->ahead;
    if (a.film_in_dfilm) return MFX_OK;
    const int b = a.cur;
    const AheadBuf& B = a.ab[b];
    const size_t plane = 3 * sizeof(double) * (size_t)c->npix;
    const int64_t want = a.last_k + 1;  // the batch's samples the film holds
    const bool prefix = a.dfilm_buf == b && a.dfilm_n <= want;
    const int64_t from = want == B.n ? want : (prefix ? a.dfilm_n : 0);
    for (mfx_ctx* d : devs_of(c)) {
        HIPCHECK(hipSetDevice(d->device));
        const AheadBuf& D = d->ahead.ab[b];
        if (want == B.n) {
            HIPCHECK(hipMemcpyAsync(d->d_film, D.film_out, plane, hipMemcpyDeviceToDevice, d->stream));
            continue;
        }
        if (!prefix) HIPCHECK(hipMemcpyAsync(d->d_film, D.film_in, plane, hipMemcpyDeviceToDevice, d->stream));
        if (from == want || band_rows(d) == 0) continue;
        HIPCHECK(hipMemsetAsync(d->ahead.counters_aux, 0, kCounterBytes, d->stream));
        MFX_TRY(wf_trace(d, want - from, B.base + from,
                         FrameMode{d->d_film, nullptr, 0.0, d->ahead.counters_aux, d->ahead.aux_ev0, d->ahead.aux_ev1}));
    }
    HIPCHECK(hipSetDevice(c->device));
    a.dfilm_buf = b;
    a.dfilm_n = want;
    a.film_in_dfilm = true;
    return MFX_OK;
}

// the film leaves the held frames' sequence (a reset, an spp != 1 render call, mfx_sample)
int mfxh::ahead_break(mfx_ctx* c) {
    if (!c->ahead.ready()) return MFX_OK;
    MFX_TRY(ahead_materialize(c));
    c->ahead.film_epoch += 1;
    c->ahead.cur = -1;
    return MFX_OK;
}

// trace samples [base, base + cap) into buffer xi of every device: their frames from the film
// in buffer src's film_out (src < 0: d_film) with count0 = frameCount before them, and the film
// after them (enqueued only)
static int ahead_launch(mfx_ctx* c, int xi, int64_t base, int src, double count0) {
    Ahead& a = c->ahead;
    const size_t plane = 3 * sizeof(double) * (size_t)c->npix;
    AheadBuf& B = a.ab[xi];
    B.base = base;
    B.n = a.cap;
    B.reported = false;
    if (a.dfilm_buf == xi) a.dfilm_buf = -1;  // its film_in changes
    for (mfx_ctx* d : devs_of(c)) {
        HIPCHECK(hipSetDevice(d->device));
        AheadBuf& D = d->ahead.ab[xi];
        const double* film_src = src < 0 ? d->d_film : d->ahead.ab[src].film_out;
        HIPCHECK(hipMemcpyAsync(D.film_in, film_src, plane, hipMemcpyDeviceToDevice, d->stream));
        HIPCHECK(hipMemcpyAsync(D.film_out, film_src, plane, hipMemcpyDeviceToDevice, d->stream));
        HIPCHECK(hipMemsetAsync(D.counters, 0, kCounterBytes, d->stream));
        if (band_rows(d) > 0) {
            const int rc = wf_trace(d, B.n, base, FrameMode{D.film_out, D.frames, count0, D.counters, D.t0, D.t1});
            if (rc) {
                B.n = 0;
                (void)hipSetDevice(c->device);
                return rc;
            }
        } else {  // a device with no tile row: no rays in no time
            HIPCHECK(hipEventRecord(D.t0, d->stream));
            HIPCHECK(hipEventRecord(D.t1, d->stream));
        }
        HIPCHECK(hipEventRecord(D.ready, d->stream));
    }
    HIPCHECK(hipSetDevice(c->device));
    B.expect = 0;
    B.epoch = a.film_epoch;
    B.count0 = count0;
    if (src < 0) {  // film_in is d_film as it is
        a.dfilm_buf = xi;
        a.dfilm_n = 0;
    }
    return MFX_OK;
}

// A device's band rows of a y-major RGBA8 frame (device memory) into the caller's frame (host):
// one copy of the whole frame for a one-device context; on a device list two strided copies of its
// whole tile rows (band_tile_row: the even groups' rows and the odd groups' rows, each 8 rows every
// 2 * band_count * 8) plus the film's partial last tile row if it owns it.
static int copy_band_rgba(const mfx_ctx* d, uint8_t* dst, const uint8_t* src, hipStream_t st) {
    const int W = d->scene.host.width, H = d->scene.host.height;
    const size_t row = 4 * (size_t)W;
    if (d->band_count == 1) {
        HIPCHECK(hipMemcpyAsync(dst, src, row * (size_t)H, hipMemcpyDeviceToHost, st));
        return MFX_OK;
    }
    const int full = H / 8, tr = (H + 7) / 8, bi = d->band_index, bc = d->band_count;
    const int nb = band_row_count(bi, bc, tr);
    for (int k0 = 0; k0 < 2; ++k0) {
        int n = 0;  // the band's rows of this parity that are whole tile rows (a prefix: rows grow with k)
        for (int k = k0; k < nb && band_tile_row(bi, bc, k) < full; k += 2) ++n;
        if (n == 0) continue;
        const size_t off = (size_t)8 * band_tile_row(bi, bc, k0) * row, pitch = (size_t)16 * bc * row;
        HIPCHECK(hipMemcpy2DAsync(dst + off, pitch, src + off, pitch, 8 * row, (size_t)n, hipMemcpyDeviceToHost, st));
    }
    if (full < tr && nb > 0 && band_tile_row(bi, bc, nb - 1) == tr - 1) {
        const size_t off = (size_t)8 * full * row;
        HIPCHECK(hipMemcpyAsync(dst + off, src + off, (size_t)(H - 8 * full) * row, hipMemcpyDeviceToHost, st));
    }
    return MFX_OK;
}

// One render call (spp = 1) served from held frames. Returns MFX_E_NOMEM when no buffer fits (the
// caller then renders one sample per call, without render-ahead).
static int ahead_render(mfx_ctx* c, uint8_t* rgba) {
    Ahead& a = c->ahead;
    if (!a.ready()) MFX_TRY(ahead_alloc(c));
    const int64_t s = c->next_sample;
    int xi = -1;
    for (int b = 0; b < a.nbuf; ++b)
        if (a.ab[b].n > 0 && s >= a.ab[b].base && s < a.ab[b].base + a.ab[b].n) xi = b;
    if (xi < 0) {  // not held: trace a batch from this sample, its frames from the film as it is
        MFX_TRY(ahead_materialize(c));
        xi = (a.cur >= 0 && a.nbuf == 2) ? 1 - a.cur : 0;
        MFX_TRY(ahead_launch(c, xi, s, -1, c->frame_count));
    } else if (a.ab[xi].epoch != a.film_epoch || a.ab[xi].expect != s - a.ab[xi].base) {
        MFX_TRY(ahead_materialize(c));  // held, but the frames assumed another film: a batch from here
        MFX_TRY(ahead_launch(c, xi, s, -1, c->frame_count));
    }
    AheadBuf& X = a.ab[xi];
    const int64_t k = s - X.base;
    const std::vector<mfx_ctx*> ds = devs_of(c);
    // This call's frame, on each device's copy stream behind this batch's frames only: it overlaps
    // the background batch. Everything the call reads back goes there before the next batch is
    // enqueued, and the counters go to page-locked memory: a pageable copy enqueued behind the
    // background batch waited for it (r03b: 6,794 Mrays/s, 73 % of batch; r03c: 8,579, 93 %).
    const size_t frame = 4 * (size_t)c->npix;
    for (mfx_ctx* d : ds) {
        HIPCHECK(hipSetDevice(d->device));
        if (!d->rb.copy_stream) HIPCHECK(d->rb.copy_stream.create());
        HIPCHECK(hipStreamWaitEvent(d->rb.copy_stream, d->ahead.ab[xi].ready, 0));
        if (rgba) MFX_TRY(copy_band_rgba(d, rgba, d->ahead.ab[xi].frames + k * frame, d->rb.copy_stream));
    }
    for (int q = 0; q < 16; ++q) c->rep_counts[q] = 0.0;
    c->rep_ms = 0.0;
    if (!X.reported) {  // the first call served from a batch reports its rays (all devices) and device time (the slowest)
        for (mfx_ctx* d : ds) {
            HIPCHECK(hipSetDevice(d->device));
            HIPCHECK(hipMemcpyAsync(d->h_counters, d->ahead.ab[xi].counters, kCounterBytes, hipMemcpyDeviceToHost,
                                    d->rb.copy_stream));
        }
        float worst = 0.f;
        for (mfx_ctx* d : ds) {
            HIPCHECK(hipSetDevice(d->device));
            HIPCHECK(hipStreamSynchronize(d->rb.copy_stream));
            sum_counters(d->h_counters, c->rep_counts);
            note_live(d, d->h_counters);
            float f = 0.f;
            HIPCHECK(hipEventElapsedTime(&f, d->ahead.ab[xi].t0, d->ahead.ab[xi].t1));
            worst = std::max(worst, f);
        }
        c->rep_counts[3] = c->rep_counts[0];
        c->rep_ms = worst;
        X.reported = true;
    }
    for (mfx_ctx* d : ds) {
        HIPCHECK(hipSetDevice(d->device));
        HIPCHECK(hipStreamSynchronize(d->rb.copy_stream));
    }
    HIPCHECK(hipSetDevice(c->device));
    for (double& t : c->rep_timing) t = 0.0;
    c->rep_valid = true;
    a.cur = xi;
    a.last_k = k;
    X.expect = k + 1;
    a.film_in_dfilm = false;
    c->frame_count += 1.0;  // Film.AddSample: frameCount <- frameCount + 1 (Film.fs:19)
    c->next_sample += 1;
    if (a.nbuf == 2) {  // the next batch, in the background, unless the other buffer holds it
        AheadBuf& Y = a.ab[1 - xi];
        const double count_end = X.count0 + (double)X.n;  // frameCount after X's last call
        int rc = MFX_OK;
        // not held, or held but its frames assumed another film: traced (again) from X's film
        if (!(Y.n > 0 && Y.base == X.base + X.n) || Y.epoch != a.film_epoch || Y.count0 != count_end)
            rc = ahead_launch(c, 1 - xi, X.base + X.n, xi, count_end);
        // This call is served: a background batch that does not fit is not its failure (a NOMEM
        // here would make the caller render the call a second time). Y stays empty; the call
        // that needs it launches it, and falls back to one sample per call if it still fails.
        if (rc == MFX_E_NOMEM) {
            Y.n = 0;
            rc = MFX_OK;
        }
        if (rc) return rc;
    }
    return MFX_OK;
}

// Without render-ahead (or spp != 1): every device traces its band into its accumulator, adds it
// to its band of the film and post-processes it (film_post_kernel), and copies its band rows of
// the RGBA8 frame to the caller's buffer. No device buffer is reduced: each pixel's film lives on
// the device whose band holds it (mfx_film_mean merges them).
extern "C" int mfx_render_rgba8(mfx_ctx* c, int32_t spp, uint8_t* rgba) {
    if (!c) return fail(MFX_E_INVALID, "null context");
    if (c->api_part_count != 1) return fail(MFX_E_STATE, "mfx_render_rgba8 needs part_count == 1");
    if (spp < 1) return fail(MFX_E_INVALID, "spp must be >= 1");
    if (spp == 1 && c->ahead.k > 1) {
        HIPCHECK(hipSetDevice(c->device));
        const int rc = ahead_render(c, rgba);
        if (rc != MFX_E_NOMEM) return rc;
        // no room for the batch (nothing of this call was served): this context renders one
        // sample per call from now on; the film comes back to d_film and the buffers are freed
        c->ahead.k = 0;
        MFX_TRY(ahead_break(c));
        ahead_free_all(c);
    }
    MFX_TRY(ahead_break(c));
    MFX_TRY(mfx_accum_clear(c));
    MFX_TRY(mfx_trace_accumulate(c, spp, c->next_sample));
    c->next_sample += spp;
    c->frame_count += 1.0;  // Film.AddSample: frameCount <- frameCount + 1 (Film.fs:19)
    c->ahead.dfilm_buf = -1;  // d_film moves on
    for (mfx_ctx* d : devs_of(c)) {
        HIPCHECK(hipSetDevice(d->device));
        HIPCHECK(mfx_launch_film_post(d->d_accum, d->d_film, c->scene.host.width, c->scene.host.height, (double)spp, c->frame_count, 1,
                                      rgba ? d->d_rgba.get() : nullptr, d->stream));
        if (rgba) MFX_TRY(copy_band_rgba(d, rgba, d->d_rgba, d->stream));
    }
    return mfx_sync(c);
}

extern "C" int mfx_accumulate_render_rgba8(mfx_ctx* c, int32_t spp, uint8_t* rgba) { return mfx_render_rgba8(c, spp, rgba); }
