// mfx_trace.cpp — the trace calls of the extern "C" boundary: the wavefront pool and its driver
// (wf_trace), mfx_trace_accumulate, the multi-device reduce, the accumulator calls, trace timing and
// the ray counters.
#include "mfx_build.h"
#include "mfx_ctx.h"

using namespace mfxh;

// Allocate (or grow) the wavefront path-slot pool (SoA). queues: the trace runs ray queues
// (MFX_RAY_QUEUE), whose arrays (6 doubles and 7 words per slot) are allocated only then.
static int wf_ensure_pool(mfx_ctx* c, int32_t pool, bool queues) {
    WfPool& wp = c->pool;
    if (pool <= wp.slots && (!queues || wp.queues)) return MFX_OK;
    const size_t P = (size_t)pool;
    const int nv = c->scene.host.max_depth + 1;  // vertices per path
    const size_t per_slot = pool_slot_bytes(c) - (queues ? 0 : WF_QUEUE_BYTES_PER_SLOT);
    const size_t bytes = P * per_slot + 64 * 256;
    // leave the runtime its headroom (kernel scratch is allocated at launch, and the runtime gives
    // an idle queue's scratch back, so a later launch allocates it again): a pool that would take
    // the device's last min(2 GiB, a quarter of what is free) counts as out of memory, and wf_trace
    // retries with smaller generations. The check runs before the current pool is freed (its bytes
    // count as free), so a refused growth keeps it: a smaller generation may fit in it.
    // It runs again after the allocation: processes sharing the device (the one-GPU rehearsal of an
    // N-rank job) that checked at the same time must not take the headroom together (r06n: eight
    // ranks' pools left no room for a launch's scratch).
    size_t mfree = 0, mtotal = 0, headroom = 0;
    if (hipMemGetInfo(&mfree, &mtotal) == hipSuccess && mfree > 0) {
        const size_t avail = mfree + (wp.mem ? wp.bytes : 0);
        headroom = std::min<size_t>((size_t)2 << 30, avail / 4);
        if (bytes + headroom > avail)
            return fail(MFX_E_NOMEM, "wavefront pool: " + std::to_string(bytes >> 20) + " MiB with " +
                                         std::to_string(avail >> 20) + " MiB free");
    }
    wp.mem.reset();
    wp.slots = 0;
    wp.bytes = 0;
    // (MFX_POOL_FAIL_ONCE: the first request is one the device cannot hold, as another process's
    // allocation between the check above and this one would make it)
    const hipError_t e = wp.mem.alloc(wp.fail_once ? ((size_t)1 << 50) : bytes);
    wp.fail_once = false;
    if (e != hipSuccess) {
        // wf_trace recovers with smaller generations: clear the failure from the thread's last
        // error, or the next launch's hipGetLastError reports it as the launch's own (r06p: eight
        // ranks on one GPU failed "mfx_wf_iteration: out of memory" after a refused pool)
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? MFX_E_NOMEM : MFX_E_DEVICE,
                    std::string("wavefront pool: ") + hipGetErrorString(e));
    }
    if (headroom > 0 && hipMemGetInfo(&mfree, &mtotal) == hipSuccess && mfree < headroom) {
        wp.mem.reset();
        return fail(MFX_E_NOMEM, "wavefront pool: " + std::to_string(bytes >> 20) + " MiB left " +
                                     std::to_string(mfree >> 20) + " MiB free");
    }
    wp.bytes = bytes;
    char* p = wp.mem;
    auto take = [&](size_t n) { char* r = p; p += (n + 255) & ~(size_t)255; return r; };
    WfParams& A = wp.params;
    double** dbl[6] = {&A.ox, &A.oy, &A.oz, &A.dx, &A.dy, &A.dz};
    for (double** d : dbl) *d = (double*)take(P * 8);
    A.vei = (double*)take(P * 8 * nv);
    A.vls = (double*)take(P * 8 * 2 * nv);
    A.vmat = (WfMat*)take(P * sizeof(WfMat) * nv);
    A.vlt = wf_multi_light(c) ? (uint8_t*)take(P * WF_LIGHT_BYTES_PER_SLOT(nv)) : nullptr;  // (in pool_slot_bytes)
    A.vtex = wf_textured(c) ? (uint32_t*)take(P * WF_TEXEL_BYTES_PER_SLOT(nv)) : nullptr;  // (in pool_slot_bytes)
    A.vsky = wf_sky_sampled(c) ? (uint32_t*)take(P * WF_SKY_BYTES_PER_SLOT(nv)) : nullptr;  // (in pool_slot_bytes)
    // a sky: the slots' miss records, all "none" from here on (k_resolve puts the value back where it reads a miss)
    A.env_rec = wf_env(c) ? (uint32_t*)take(P * WF_ENV_BYTES_PER_SLOT) : nullptr;  // (in pool_slot_bytes)
    if (A.env_rec) {
        const hipError_t ef = hipMemsetAsync(A.env_rec, 0xff, P * WF_ENV_BYTES_PER_SLOT, c->stream);
        if (ef != hipSuccess) {
            wp.mem.reset();
            wp.bytes = 0;
            A.env_rec = nullptr;
            return fail(MFX_E_DEVICE, std::string("wavefront pool: ") + hipGetErrorString(ef));
        }
    }
    A.vstride = (int64_t)P;
    A.rn = (uint32_t*)take(P * 4);
    A.depth = (int32_t*)take(P * 4);
    A.state = (int32_t*)take(P * 4);
#if MFX_RAY_QUEUE
    if (queues) {
        // queue 0: its own arrays; queue 1: the pool's ray arrays (o, d, rn: dead once the
        // iterations run on queues) and its own depth, state and slot words
        WfQueue& q0 = wp.wq[0];
        double** q0d[6] = {&q0.ox, &q0.oy, &q0.oz, &q0.dx, &q0.dy, &q0.dz};
        for (double** d : q0d) *d = (double*)take(P * 8);
        q0.rn = (uint32_t*)take(P * 4);
        WfQueue& q1 = wp.wq[1];
        q1.ox = A.ox; q1.oy = A.oy; q1.oz = A.oz;
        q1.dx = A.dx; q1.dy = A.dy; q1.dz = A.dz;
        q1.rn = A.rn;
        for (WfQueue* q : {&q0, &q1}) {
            q->depth = (int32_t*)take(P * 4);
            q->state = (int32_t*)take(P * 4);
            q->slot = (int32_t*)take(P * 4);
        }
        q0.count = wp.ctl;                                  // WF_CTL_Q0
        q1.count = wp.ctl - WF_CTL_Q0 + WF_CTL_Q1;
    }
#endif
    wp.slots = pool;
    wp.queues = queues;
    return MFX_OK;
}

// Iteration d's arrays (MFX_RAY_QUEUE, mfx_wavefront.h WfParams): the pool itself up to iteration
// q = the queue start, whose k_shadow moves the continuing paths to queue 0; iteration d > q reads
// queue (d - q - 1) & 1 and writes the other. d = -1: the pool (k_resolve).
static void wf_queue_views(mfx_ctx* c, WfParams& P, int d) {
    const WfParams& A = c->pool.params;
    P.ox = A.ox; P.oy = A.oy; P.oz = A.oz; P.dx = A.dx; P.dy = A.dy; P.dz = A.dz;
    P.rn = A.rn; P.depth = A.depth; P.state = A.state;
    P.fstate = A.state;
    P.qslot = nullptr;
    P.qcount = nullptr;
    P.ncount = nullptr;
    const int q = c->pool.queue_start();
    if (q < 0 || d < 0) return;
    if (d > q) {
        const WfQueue& R = c->pool.wq[(d - q - 1) & 1];
        P.ox = R.ox; P.oy = R.oy; P.oz = R.oz; P.dx = R.dx; P.dy = R.dy; P.dz = R.dz;
        P.rn = R.rn; P.depth = R.depth; P.state = R.state;
        P.qslot = R.slot;
        P.qcount = R.count;
    }
    if (d >= q && d < P.max_depth) {
        const WfQueue& N = c->pool.wq[(d - q) & 1];
        P.nox = N.ox; P.noy = N.oy; P.noz = N.oz; P.ndx = N.dx; P.ndy = N.dy; P.ndz = N.dz;
        P.nrn = N.rn; P.ndepth = N.depth; P.nstate = N.state; P.nslot = N.slot;
        P.ncount = N.count;
    }
}

// what the wavefront's and the megakernel's parameters (WfParams, TraceParams) share
template <typename P>
static void fill_trace_params(mfx_ctx* c, P& p, int64_t sample_base) {
    fill_scene_ptrs(c, p);
    p.light = c->scene.host.light;
    p.cam = c->scene.host.camera;
    p.accum = c->d_accum;
    c->adp.accum_valid = false;  // a trace adds to it (mfx_sample_adaptive sets the flag after its own)
    p.seed = c->seed;
    p.sample_base = sample_base;
    p.part_index = c->part_index;
    p.part_count = c->part_count;
    p.band_index = c->band_index;
    p.band_count = c->band_count;
    p.band_rows = band_rows(c);
    p.width = c->scene.host.width;
    p.height = c->scene.host.height;
    p.max_depth = c->scene.host.max_depth;
    p.stack_size = c->scene.stack_size;
}

static void fill_scene_params(mfx_ctx* c, WfParams& P) {
#if MFX_NODE_F16
    P.nodes_h = c->scene.d_nodes_h;
#endif
    P.light_dev = c->scene.d_light;
    // several lights: the ML instances' table (set: mfx_wf_iteration and mfx_wf_resolve launch them)
    P.lights = wf_multi_light(c) ? c->scene.d_lights.get() : nullptr;
    P.nlights = wf_multi_light(c) ? (int32_t)c->scene.host.lights.size() : 0;
    // albedo textures: the TX instances' tables (vtex set, by wf_ensure_pool: the launchers run them)
    P.tx = c->tex.tables();
    // smooth shading: the SN instances' tables (set: mfx_wf_iteration launches them)
    P.sn = wf_normals(c) ? c->nrm.tables() : MfxSnTables{};
    // a sky: the ENV instances' map (env_rec set, by wf_ensure_pool: the launchers run them)
    P.env_rgb = wf_env(c) ? c->sky.d_rgb.get() : nullptr;
    P.env_size = c->sky.size;
    // a sampled sky: the SKY instances' table (vsky set, by wf_ensure_pool; the lights above are the N area lights)
    P.sky_tab = wf_sky_sampled(c) ? c->sky.d_tab.get() : nullptr;
    P.cam_dev = c->scene.d_cam;
    P.refs_dev = c->scene.d_refs;
    P.gray_light = wf_gray_light(c);
    P.lit_in_hit = wf_lit_in_hit(c);
    P.albedo = c->scene.d_albedo;
    P.nmat = (int32_t)(c->scene.host.albedo.size() / 3);
    const LaunchShapes& L = c->scene.shapes;
    P.stack_lds_ext = L.stack_lds_ext;
    P.stack_lds_shd = L.stack_lds_shd;
    P.ntop_ext = L.ntop_ext;
    P.ntop_shd = L.ntop_shd;
    P.nslot_ext = L.nslot_ext;
    P.nslot_shd = L.nslot_shd;
    P.shadow_waves = L.shadow_waves;
}

// ---- camera cuts (mfx_camera_cuts.h): the per-device table and when it is built ----
// a context whose camera rays run k_camera with cuts on (flat scenes, MFX_CAMERA_PACKETS and MFX_CAMERA_CUTS not 0)
bool mfxh::cuts_apply(const mfx_ctx* c) { return c->scene.host.inst.empty() && c->scene.wf_cam_grid > 0 && c->cuts.on; }

// The device's table for its current camera and node image, built on its stream if it is another's
// (context creation, a camera change, a scene rebuild): every later launch on the stream sees it.
// ns: the samples of the trace that asks. The slot cull makes the build three times as long (DESIGN.md §7, round
// 10), so the table is built with it only once its camera has served cull_min_samples samples, this trace's
// included: a camera that moves before every trace gets the plain table, one that stays gets the culled one
// with the trace that crosses the threshold and keeps it.
int mfxh::cuts_ensure(mfx_ctx* c, int64_t ns) {
    CamCuts& K = c->cuts;
    const bool same = K.valid && K.image_gen == c->image_gen && std::memcmp(&K.cam, &c->scene.host.camera, sizeof(MfxCamera)) == 0;
    if (!same) K.cam_samples = 0;
    K.cam_samples = ns > INT64_MAX - K.cam_samples ? INT64_MAX : K.cam_samples + std::max<int64_t>(ns, 0);
    const bool cull = K.cam_samples >= K.cull_min_samples;
    if (same && (K.culled || !cull)) return MFX_OK;
    const size_t tiles = (size_t)((c->scene.host.width + 7) / 8) * (size_t)((c->scene.host.height + 7) / 8);
    if (K.entries < tiles * K.cap) {
        HIP_TRY(K.table.alloc(tiles * K.cap), _e == hipErrorOutOfMemory ? MFX_E_NOMEM : MFX_E_DEVICE, "camera cuts: ");
        K.entries = tiles * K.cap;
    }
    if (!K.stats) {
        HIPCHECK(K.stats.alloc(1));
        HIPCHECK(K.e0.create());
        HIPCHECK(K.e1.create());
    }
    K.valid = false;
    HIPCHECK(hipEventRecord(K.e0, c->stream));
    HIPCHECK(mfx_build_cut_table(c->scene.d_nodes, cull ? (const MfxSlot*)c->scene.d_slots : nullptr, c->scene.d_cam, c->scene.host.width, c->scene.host.height, K.cap, K.table, K.stats, c->stream));
    HIPCHECK(hipEventRecord(K.e1, c->stream));
    K.cam = c->scene.host.camera;
    K.image_gen = c->image_gen;
    K.culled = cull;
    K.valid = true;
    K.builds += 1;
    K.last_read = false;
    return MFX_OK;
}

// the last build's statistics and time (waits for it)
int mfxh::cuts_read_stats(mfx_ctx* c) {
    CamCuts& K = c->cuts;
    if (K.builds == 0 || K.last_read) return MFX_OK;
    HIPCHECK(hipSetDevice(c->device));
    HIPCHECK(hipEventSynchronize(K.e1));
    HIPCHECK(hipEventElapsedTime(&K.last_ms, K.e0, K.e1));
    HIPCHECK(hipMemcpy(&K.last, K.stats, sizeof(MfxCutStats), hipMemcpyDeviceToHost));
    K.last_read = true;
    return MFX_OK;
}

// The wavefront pipeline. The frame's path indices (sample-major, 8x8 tiles) are cut into
// generations of at most pool.max paths; slot j of a generation holds path path_base + j. A
// generation is max_depth + 1 iterations of (k_extend, k_shadow) — the primary ray and the
// max_depth extension rays of PathIntegrator.TraceRay (Integrators.fs:107-137), one bounce of
// every live path per iteration — then k_resolve adds its finished paths to their pixels. Every
// launch count is known up front, so the whole call is enqueued without a host round trip.
// mode (mfx_ctx.h): none, or render-ahead's frames (FrameMode), mfx_sample's banded last resolve
// (ResolveSplit) or the adaptive sampler's listed tiles (TileList: mfx_sample_adaptive, and with per-tile counts
// mfx_sample_adaptive_resume).
int mfxh::wf_trace(mfx_ctx* c, int64_t ns, int64_t sample_base, TraceMode mode) {
    const FrameMode* fm = std::get_if<FrameMode>(&mode);
    ResolveSplit* split = std::holds_alternative<ResolveSplit*>(mode) ? std::get<ResolveSplit*>(mode) : nullptr;
    const TileList* list = std::get_if<TileList>(&mode);
    WfPool& wp = c->pool;
    const int W = c->scene.host.width, H = c->scene.host.height;
    const int brows = band_rows(c);
    if (list && (list->ntiles < 1 || !list->tiles || !list->mom)) return fail(MFX_E_INVALID, "wf_trace: bad tile list");
    // the device's band of the film, or the listed tiles
    const int64_t per_sample = list ? (int64_t)list->ntiles * 64 : (int64_t)((W + 7) / 8) * brows * 64;
    const int64_t total = per_sample * ns;
    if (total == 0) return fail(MFX_E_STATE, "wf_trace: empty band");
    // generations of whole 64-path windows (one 8x8 tile of one sample each: the camera-ray packets)
    const int qf = wp.queue_start();  // the ray-queue start
    int64_t gen_max = 0;
    int32_t pool = 0;
    int rc = MFX_OK;
    // the device short of memory (other contexts or processes on it): smaller generations, the same
    // images (a generation only bounds how many paths are in flight). The shrunk cap is kept, and a
    // later call goes back to the configured maximum once the device has room for twice that pool
    // (a one-off spike no longer shrinks a context for good; the margin keeps contexts of
    // several processes sharing a device from growing back into each other's launches, r06j)
    int64_t cap = wp.cap > 0 ? wp.cap : wp.max;
    if (cap < wp.max) {
        const double full = (double)std::min<int64_t>(total, wp.max) * pool_slot_bytes(c);
        size_t mfree = 0, mtotal = 0;
        if (hipMemGetInfo(&mfree, &mtotal) == hipSuccess && 2.0 * full < (double)(mfree + wp.bytes))
            cap = wp.max;
    }
    while (true) {
        // (a listed trace: at most the call's first pass per generation, so no later pass grows the pool)
        const int64_t gcap = list ? std::min(cap, list->gen_paths) : cap;
        gen_max = std::min<int64_t>(total, std::max<int64_t>(4096, gcap / 4096 * 4096));
        pool = (int32_t)((gen_max + 4095) / 4096 * 4096);  // 64 shards of whole windows
        rc = wf_ensure_pool(c, pool, qf >= 0);
        if (rc != MFX_E_NOMEM || cap <= (1 << 20)) break;
        cap = std::max<int64_t>(1 << 20, gen_max / 2);
    }
    if (rc) return rc;
    wp.cap = cap < wp.max ? cap : 0;
    WfParams P = wp.params;
    fill_trace_params(c, P, sample_base);
    fill_scene_params(c, P);
    P.ctl = wp.ctl - WF_CTL_Q0;
    P.counters = fm ? fm->counters : c->d_counters.get();
    const bool own_events = fm == nullptr;
    // per-iteration stage events (mfx_trace_timing's split): off with MFX_ITER_EVENTS=0 (A/B of their cost)
    const bool iter_events = own_events && c->iter_events;
    P.ninst_lds = std::min<int>((int)c->scene.host.inst.size(), WF_INST_LDS);
    P.spill = c->scene.d_spill;
    // slots per chunk fetch: 256 at every frame size. Round 3 used 1024 (512 for frames of at most
    // 2^25 paths); with the shard counters on lines of their own and the closed-shard mask the chunk
    // fetches no longer convoy, so small chunks cut the launches' tails (r04j: C2 fixed cost per
    // frame 1.67 -> 1.24 ms, 8 spp +8 %, 64 spp +1 %)
    P.chunk = c->wf_chunk;
    // (per-tile counts: a clipped tile's windows are padding too, whatever the film's size)
    P.tile_padding = (W % 8 != 0 || H % 8 != 0 || (list && list->tile_n)) ? 1 : 0;
    const int32_t chunk0 = P.chunk;
    P.film = fm ? fm->film : nullptr;
    P.frames = fm ? fm->frames : nullptr;
    P.count0 = fm ? fm->count0 : 0.0;
    P.tiles = list ? list->tiles : nullptr;
    P.ntiles = list ? list->ntiles : 0;
    P.mom = list ? list->mom : nullptr;
    P.tile_n = list ? list->tile_n : nullptr;
    P.list_max = list ? list->list_max : 0;
    const bool stats = (c->flags & MFX_F_COUNT_STATS) != 0;
    // (a lens: no packets and no cut table, which rest on one shared origin; k_extend's LENS twin starts the paths)
    P.cam_grid = c->scene.host.inst.empty() && !wf_lens(c) ? c->scene.wf_cam_grid : 0;
    if (own_events) c->cam_last = P.cam_grid > 0;
    // camera cuts: a table that is already this camera's costs nothing; a trace of fewer than min_samples
    // samples does not pay for a build and walks from the root (the break-even)
    P.cuts = nullptr;
    P.cut_cap = 0;
    if (P.cam_grid > 0 && cuts_apply(c)) {
        const CamCuts& K = c->cuts;
        const bool have = K.valid && K.image_gen == c->image_gen && std::memcmp(&K.cam, &c->scene.host.camera, sizeof(MfxCamera)) == 0;
        if (have || ns >= K.min_samples) {
            MFX_TRY(cuts_ensure(c, ns));
            P.cuts = K.table;
            P.cut_cap = K.cap;
        }
    }
    const int64_t ngen = (total + gen_max - 1) / gen_max;
    const int per_gen = P.max_depth + 1;  // bounce-synchronous iterations per generation
    const int iters = (int)ngen * per_gen;
    while (iter_events && (int)c->it_ev.size() < 3 * iters) {
        Event e;
        HIPCHECK(e.create());
        c->it_ev.push_back(std::move(e));
    }
    // MFX_DIAG_ITER=1: per-iteration ray counts and stage times on stderr
    auto diag = [&](int64_t g, const char* what, int d, float fe, float fs) -> int {
        HIPCHECK(hipStreamSynchronize(c->stream));
        unsigned long long h[WF_NCTR * WF_SHARDS];
        HIPCHECK(hipMemcpy(h, c->d_counters, sizeof(h), hipMemcpyDeviceToHost));
        double r[WF_NCTR] = {0};
        for (int k = 0; k < WF_SHARDS; ++k)
            for (int q = 0; q < WF_NCTR; ++q) r[q] += (double)h[WF_NCTR * k + q];
        for (int q = WF_CTR_ITER + 1; q < WF_CTR_ITER + WF_ITER_CTRS; ++q) r[1] += r[q];
        fprintf(stderr, "gen %lld %s %d: cumulative primary %.0f ext %.0f shadow %.0f; extend %.3f ms shadow %.3f ms;"
                " stamps %.4g %.4g %.4g %.4g outer %.4g node %.4g; cumulative traversal closest %.0f %.0f %.0f"
                " shadow %.0f %.0f %.0f; scan %.4g shade %.4g lat %.4g\n", (long long)g, what, d,
                r[0], r[1], r[2], fe, fs, r[10], r[11], r[12], r[13], r[14], r[15], r[4], r[5], r[6], r[7], r[8], r[9],
                r[16], r[17], r[3]);
        return MFX_OK;
    };
    HIPCHECK(hipEventRecord(fm ? fm->e0 : c->ev0.get(), c->stream));
    int it = 0;
    for (int64_t g = 0; g < ngen; ++g) {
        P.path_base = g * gen_max;
        P.base_smp = P.path_base / per_sample;
        P.base_q = P.path_base % per_sample;
        P.total = std::min<int64_t>(gen_max, total - P.path_base);
        P.pool = (int32_t)((P.total + 4095) / 4096 * 4096);
        HIPCHECK(hipMemsetAsync(P.state, 0, sizeof(int32_t) * (size_t)P.pool, c->stream));
        for (int d = 0; d < per_gen; ++d, ++it) {
            P.start = d == 0 ? 1 : 0;
            P.iter = d;
            wf_queue_views(c, P, d);
            // a queue's entries are all live rays: smaller chunks keep the launch's tail short
            P.chunk = P.qcount ? wp.qchunk : chunk0;
            // in place on a small frame (the strong-scaling shares), k_shadow takes half chunks: the
            // first vertex's last chunks are its launch's tail (r04u: C2 at 8 spp +2.4 %; at 64 spp
            // the same halving costs 1.5 %, so frames of more than 2^25 paths keep whole chunks)
            P.chunk_shd = (c->wf_shd_half && !P.qcount && total <= ((int64_t)1 << 25)) ? std::max(64, P.chunk / 2) : P.chunk;
            if (!iter_events) {
                HIPCHECK(mfx_wf_iteration(P, c->scene.wf_ext_grid, c->scene.wf_shd_grid, stats, c->stream, nullptr, wf_lens(c)));
                continue;
            }
            const Event* ev = c->it_ev.data() + 3 * it;
            hipEvent_t mid = ev[1];  // recorded between k_extend and k_shadow
            HIPCHECK(hipEventRecord(ev[0], c->stream));
            HIPCHECK(mfx_wf_iteration(P, c->scene.wf_ext_grid, c->scene.wf_shd_grid, stats, c->stream, &mid, wf_lens(c)));
            HIPCHECK(hipEventRecord(ev[2], c->stream));
            if (c->diag_iter) {
                HIPCHECK(hipStreamSynchronize(c->stream));
                float fe = 0.f, fs = 0.f;
                HIPCHECK(hipEventElapsedTime(&fe, ev[0], ev[1]));
                HIPCHECK(hipEventElapsedTime(&fs, ev[1], ev[2]));
                MFX_TRY(diag(g, "iter", d + 1, fe, fs));
            }
        }
        wf_queue_views(c, P, -1);  // k_resolve reads the pool's final state and depth words
        if (split && g == ngen - 1) {
            // a pixel's sum is its own thread's whatever the launch: the same bits as one launch
            const int tiles_x = (W + 7) / 8;
            for (int k = 0; k < split->nbands; ++k) {
                const int tx0 = (int)((int64_t)k * tiles_x / split->nbands);
                const int tx1 = (int)((int64_t)(k + 1) * tiles_x / split->nbands);
                P.res_tx0 = tx0;
                P.res_ntx = tx1 - tx0;
                if (P.res_ntx > 0) HIPCHECK(mfx_wf_resolve(P, c->stream));
                MFX_TRY(split->after(k, tx0, tx1 - tx0));
            }
            P.res_tx0 = P.res_ntx = 0;
            split->used = true;
        } else {
            HIPCHECK(mfx_wf_resolve(P, c->stream));
        }
    }
    if (!own_events) {
        HIPCHECK(hipEventRecord(fm->e1, c->stream));
        return MFX_OK;
    }
    HIPCHECK(hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    // The automatic queue start is taken from a trace's per-iteration counters: read once, after
    // the context's first wavefront trace (settle_queue_auto, once every device has been
    // enqueued), so a caller that never polls the counters gets the same kernels as one that does
    if (wp.queue_from == -2 && !wp.auto_read) wp.auto_pending = true;
    c->it_recorded = iter_events ? iters : 0;
    c->it_per_gen = per_gen;
    c->generations = (int)ngen;
    return MFX_OK;
}

// one device's share of mfx_trace_accumulate (its sample partition), enqueued on its stream
int mfxh::dev_trace_accumulate(mfx_ctx* c, int32_t spp, int64_t sample_base, ResolveSplit* split) {
    HIPCHECK(hipSetDevice(c->device));
    int64_t ns = spp > c->part_index ? (spp - c->part_index + c->part_count - 1) / c->part_count : 0;
    if (band_rows(c) == 0) ns = 0;  // a film too small to give this device a tile row
    HIPCHECK(hipMemsetAsync(c->d_work, 0, 64, c->stream));
    HIPCHECK(hipMemsetAsync(c->d_counters, 0, kCounterBytes, c->stream));
    // One sample per pixel on this device (Scene.Render's call): the megakernel, unless the caller
    // pins the wavefront. With one path per pixel its FP64 atomic add onto the zeroed accumulator
    // is exact, and its per-path arithmetic is the wavefront's, so the bits are the same; it does
    // not pay the wavefront's per-bounce launches over a 2 M-path frame (r02e: 1.7 vs 7.9 ms at 1080p).
    // (several lights: always the wavefront, as under MFX_F_WAVEFRONT; creation refused MFX_F_MEGAKERNEL)
    // (albedo textures, a sky, a lens: likewise; mfx_set_environment and mfx_set_lens refuse an MFX_F_MEGAKERNEL context)
    c->mega_last = !wf_multi_light(c) && !wf_textured(c) && !wf_env(c) && !wf_lens(c) && !wf_normals(c) && ((c->flags & MFX_F_MEGAKERNEL) != 0 || (ns == 1 && (c->flags & MFX_F_WAVEFRONT) == 0));
    if (ns == 0) {  // this partition has no sample in the call: zero rays in zero device time
        HIPCHECK(hipEventRecord(c->ev0, c->stream));
        HIPCHECK(hipEventRecord(c->ev1, c->stream));
        c->ev_valid = true;
        c->it_recorded = 0;
        c->generations = 0;
        return MFX_OK;
    }
    if (!c->mega_last) {
        MFX_TRY(wf_trace(c, ns, sample_base, split ? TraceMode{split} : TraceMode{}));
        HIPCHECK(mfx_launch_counters_add(c->d_counters_total, c->d_counters, WF_NCTR * WF_SHARDS, c->stream));
        return MFX_OK;
    }
    TraceParams P;
    std::memset(&P, 0, sizeof(P));
    fill_trace_params(c, P, sample_base);
    P.work_counter = c->d_work;
    P.counters = c->d_counters;
    P.nsamples = ns;
    P.vscratch = c->scene.d_vscratch;
    P.waves = c->scene.mega_waves;
    // paths per chunk: 256, halved while fewer than 16 chunks per wave remain (a 1-spp frame:
    // 64, one path per lane per fetch; r02g/r02i A/B at 1 spp: 256 -> 64 is +21 %)
    if (c->mega_chunk > 0) {
        P.chunk = c->mega_chunk;
    } else {
        const int64_t total = (int64_t)((c->scene.host.width + 7) / 8) * band_rows(c) * 64 * ns;
        int64_t ch = 256;
        while (ch > 64 && total / ch < 16 * (int64_t)c->scene.grid * 4) ch /= 2;
        P.chunk = (int)ch;
    }
    HIPCHECK(hipEventRecord(c->ev0, c->stream));
    HIPCHECK(mfx_launch_trace(P, (c->flags & MFX_F_COUNT_STATS) != 0, c->scene.grid, c->stream));
    HIPCHECK(hipEventRecord(c->ev1, c->stream));
    c->ev_valid = true;
    HIPCHECK(mfx_launch_counters_add(c->d_counters_total, c->d_counters, WF_NCTR * WF_SHARDS, c->stream));
    return MFX_OK;
}

// pool.queue_auto from the first wavefront trace's counters, read once every device of the call has
// been enqueued (a blocking read inside the per-device loop ran device 0 to completion before the
// next device was enqueued)
int mfxh::settle_queue_auto(mfx_ctx* c) {
    for (mfx_ctx* d : devs_of(c)) {
        if (!d->pool.auto_pending) continue;
        HIPCHECK(hipSetDevice(d->device));
        HIPCHECK(hipMemcpyAsync(d->h_counters, d->d_counters, kCounterBytes, hipMemcpyDeviceToHost, d->stream));
        HIPCHECK(hipStreamSynchronize(d->stream));
        note_live(d, d->h_counters);
        d->pool.auto_pending = false;
        d->pool.auto_read = true;
    }
    HIPCHECK(hipSetDevice(c->device));
    return MFX_OK;
}

// Sum every device's accumulator into the primary's, stream-ordered after each device's trace, and
// every peer's later work (a clear or trace of its accumulator) after the reduce: the RCCL reduce
// runs on each device's own stream; the repeated-device copies run on the primary's stream, so
// each peer's stream waits for them (reduce_done) before anything the caller enqueues next.
// The devices' [3][npix] buffers buf(d) summed into dst on the primary (dst may be buf(primary)).
// A device's buffer is +0.0 outside its band (image partition), so the sum is an exact merge.
int mfxh::reduce_planes(mfx_ctx* c, double* (*buf)(mfx_ctx*), double* dst, const char* what) {
    Multi& m = c->multi;
    if (!m.comms.empty()) {  // RCCL: rank g sends device g's buffer, the root reduces into dst
        const Rccl* R = rccl();  // loaded: the communicators exist
        const size_t count = 3 * (size_t)c->npix;
        const std::vector<mfx_ctx*> ds = devs_of(c);
        ncclResult_t r = R->groupStart();
        for (size_t g = 0; g < ds.size() && r == ncclSuccess; ++g) {
            HIPCHECK(hipSetDevice(ds[g]->device));
            double* src = buf(ds[g]);
            r = R->reduce(src, g == 0 ? dst : src, count, ncclFloat64, ncclSum, 0, m.comms[g], ds[g]->stream);
        }
        const ncclResult_t r2 = R->groupEnd();
        if (r == ncclSuccess) r = r2;
        if (r != ncclSuccess) return fail(MFX_E_DEVICE, std::string(what) + ": " + R->errorString(r));
        HIPCHECK(hipSetDevice(c->device));
        return MFX_OK;
    }
    // a repeated-device list: add the peers' buffers in device order (a0 + a1) + a2 ...
    const size_t bytes = 3 * sizeof(double) * (size_t)c->npix;
    HIPCHECK(hipSetDevice(c->device));
    if (dst != buf(c)) HIPCHECK(hipMemcpyAsync(dst, buf(c), bytes, hipMemcpyDeviceToDevice, c->stream));
    for (size_t k = 0; k < m.peers.size(); ++k) {
        mfx_ctx* p = m.peers[k].get();
        HIPCHECK(hipSetDevice(p->device));
        HIPCHECK(hipEventRecord(m.peer_done[k], p->stream));
        HIPCHECK(hipSetDevice(c->device));
        HIPCHECK(hipStreamWaitEvent(c->stream, m.peer_done[k], 0));
        HIPCHECK(hipMemcpyAsync(m.reduce_stage, buf(p), bytes, hipMemcpyDefault, c->stream));
        HIPCHECK(mfx_launch_accum_add(dst, m.reduce_stage, 3 * c->npix, c->stream));
    }
    if (!m.peers.empty()) {
        HIPCHECK(hipSetDevice(c->device));
        HIPCHECK(hipEventRecord(m.reduce_done, c->stream));
        for (const auto& p : m.peers) {
            HIPCHECK(hipSetDevice(p->device));
            HIPCHECK(hipStreamWaitEvent(p->stream, m.reduce_done, 0));
        }
        HIPCHECK(hipSetDevice(c->device));
    }
    return MFX_OK;
}

// The stage split of the last wavefront trace, added to out[1..7] from its per-iteration events (which
// have completed): [2] the closest-hit kernels (k_camera + k_extend), [4] k_shadow (+ memset), summed
// over iterations; [1] of [2] the k_camera launches (each generation's first iteration when camera
// rays run as packets), [3] their count; [5], [6] iterations, [7] generations
int mfxh::add_stage_times(mfx_ctx* c, double out[8]) {
    const int per_gen = std::max(1, c->it_per_gen);
    for (int it = 0; it < c->it_recorded; ++it) {
        const Event* ev = c->it_ev.data() + 3 * it;
        float fe = 0.f, fs = 0.f;
        HIPCHECK(hipEventElapsedTime(&fe, ev[0], ev[1]));
        HIPCHECK(hipEventElapsedTime(&fs, ev[1], ev[2]));
        out[2] += fe;
        out[4] += fs;
        if (c->cam_last && it % per_gen == 0) {
            out[1] += fe;
            out[3] += 1;
        }
    }
    out[5] += c->it_recorded;
    out[6] += c->it_recorded;
    out[7] += c->generations;
    return MFX_OK;
}

void mfxh::sum_counters(const unsigned long long* h, double out[16]) {
    for (int k = 0; k < 16; ++k) {
        double v = 0;
        for (int g = 0; g < WF_SHARDS; ++g) v += (double)h[WF_NCTR * g + k];
        out[k] += v;
    }
    for (int d = 1; d < WF_ITER_CTRS; ++d)  // k_extend's per-iteration extension-ray counters
        for (int g = 0; g < WF_SHARDS; ++g) out[1] += (double)h[WF_NCTR * g + WF_CTR_ITER + d];
}

// MFX_RAY_QUEUE: the share of a trace's paths still live after each iteration (its extension rays
// over its paths), from counters read back after the trace; wf_trace moves the paths to ray queues
// from the first iteration that leaves fewer than WF_QUEUE_LIVE of them (the later bounces are the
// sparse ones). The decision only moves data: images are the same either way.
#define WF_QUEUE_LIVE 0.35
void mfxh::note_live(mfx_ctx* c, const unsigned long long* h) {
    double paths = 0, it[WF_ITER_CTRS] = {0};
    for (int g = 0; g < WF_SHARDS; ++g) {
        paths += (double)h[WF_NCTR * g + 0];
        for (int d = 1; d < WF_ITER_CTRS; ++d) it[d] += (double)h[WF_NCTR * g + WF_CTR_ITER + d];
    }
    if (paths <= 0 || it[1] <= 0) return;  // no wavefront trace (megakernel), or no path went on
    int from = -1;
    for (int d = 0; d + 1 < WF_ITER_CTRS && d < c->scene.host.max_depth; ++d)
        if (it[d + 1] / paths < WF_QUEUE_LIVE) {
            from = d;
            break;
        }
    c->pool.queue_auto = from;
}

extern "C" {
// Every device enqueues its band on its own stream; nothing here waits for a device (bar the
// one-time settle_queue_auto read), so the G devices render concurrently.
int mfx_trace_accumulate(mfx_ctx* c, int32_t spp, int64_t sample_base) {
    if (!c) return fail(MFX_E_STATE, "null context");
    if (spp < 1) return fail(MFX_E_INVALID, "spp must be >= 1");
    c->rep_valid = false;  // the stats now describe this trace
    c->multi.accum_merged = false;
    for (mfx_ctx* d : devs_of(c)) MFX_TRY(dev_trace_accumulate(d, spp, sample_base));
    HIPCHECK(hipSetDevice(c->device));  // the primary stays current for what the caller enqueues next
    return settle_queue_auto(c);
}

int mfx_accum_reduce(mfx_ctx* c) {
    if (!c) return fail(MFX_E_STATE, "null context");
    if (!c->multi.any()) return MFX_OK;
    if (c->multi.accum_merged) return MFX_OK;  // merged since the last trace or clear: a second sum would add the peers twice
    MFX_TRY(reduce_planes(c, [](mfx_ctx* d) { return d->d_accum; }, c->d_accum, "mfx_accum_reduce"));
    c->multi.accum_merged = true;
    return MFX_OK;
}

int mfx_trace_timing(mfx_ctx* c, double out[8]) {
    if (!c || !out) return fail(MFX_E_INVALID, "null argument");
    if (c->rep_valid) {  // a call served from held frames: its batch's device time, no stage split;
                         // mfx_sample_adaptive: the sums over its passes
        for (int k = 0; k < 8; ++k) out[k] = c->rep_timing[k];
        out[0] = c->rep_ms;
        return MFX_OK;
    }
    double total = 0;
    MFX_TRY(mfx_last_trace_ms(c, &total));
    for (int k = 0; k < 8; ++k) out[k] = 0.0;
    out[0] = total;
    if (c->mega_last) {
        out[2] = total;
        out[5] = 1;
        out[6] = 1;
        return MFX_OK;
    }
    return add_stage_times(c, out);  // the resolve launches make up the rest of [0]
}

int mfx_last_trace_ms(mfx_ctx* c, double* ms) {
    if (!c || !ms) return fail(MFX_E_INVALID, "null argument");
    if (c->rep_valid) {
        *ms = c->rep_ms;
        return MFX_OK;
    }
    double worst = 0.0;  // the devices run concurrently: the slowest one's time
    for (mfx_ctx* d : devs_of(c)) {
        if (!d->ev_valid) return fail(MFX_E_STATE, "no trace launch recorded yet");
        HIPCHECK(hipSetDevice(d->device));
        HIPCHECK(hipEventSynchronize(d->ev1));
        float f = 0.f;
        HIPCHECK(hipEventElapsedTime(&f, d->ev0, d->ev1));
        worst = std::max(worst, (double)f);
    }
    *ms = worst;
    return MFX_OK;
}

int mfx_accum_clear(mfx_ctx* c) {
    if (!c) return fail(MFX_E_STATE, "null context");
    c->multi.accum_merged = false;
    c->adp.accum_valid = false;
    for (mfx_ctx* d : devs_of(c)) {
        HIPCHECK(hipSetDevice(d->device));
        HIPCHECK(hipMemsetAsync(d->d_accum, 0, 3 * sizeof(double) * (size_t)d->npix, d->stream));
    }
    return MFX_OK;
}

int mfx_accum_device_ptr(mfx_ctx* c, void** dptr, int64_t* nbytes) {
    if (!c || !dptr || !nbytes) return fail(MFX_E_INVALID, "null argument");
    *dptr = c->d_accum;
    *nbytes = 3 * (int64_t)sizeof(double) * c->npix;
    return MFX_OK;
}

int mfx_accum_attach(mfx_ctx* c, void* dptr, int64_t nbytes) {
    if (!c) return fail(MFX_E_STATE, "null context");
    c->adp.accum_valid = false;
    if (!dptr) {
        c->d_accum = c->d_accum_own;
        return MFX_OK;
    }
    if (nbytes < 3 * (int64_t)sizeof(double) * c->npix) return fail(MFX_E_INVALID, "attached accumulator too small");
    c->d_accum = (double*)dptr;
    c->multi.accum_merged = false;
    return MFX_OK;
}

int mfx_ray_counts_total(mfx_ctx* c, double out[16], int32_t reset) {
    if (!c || !out) return fail(MFX_E_INVALID, "null argument");
    for (int k = 0; k < 16; ++k) out[k] = 0.0;
    for (mfx_ctx* d : devs_of(c)) {  // summed over the context's devices
        HIPCHECK(hipSetDevice(d->device));
        unsigned long long h[WF_NCTR * WF_SHARDS];
        HIPCHECK(hipMemcpyAsync(h, d->d_counters_total, sizeof(h), hipMemcpyDeviceToHost, d->stream));
        HIPCHECK(hipStreamSynchronize(d->stream));
        sum_counters(h, out);
        if (reset) HIPCHECK(hipMemsetAsync(d->d_counters_total, 0, sizeof(h), d->stream));
    }
    HIPCHECK(hipSetDevice(c->device));
    out[3] = out[0];  // paths == primary rays
    return MFX_OK;
}

int mfx_ray_counts(mfx_ctx* c, double out[16]) {
    if (!c || !out) return fail(MFX_E_INVALID, "null argument");
    if (c->rep_valid) {  // a call served from held frames (render-ahead)
        for (int k = 0; k < 16; ++k) out[k] = c->rep_counts[k];
        return MFX_OK;
    }
    for (int k = 0; k < 16; ++k) out[k] = 0.0;
    for (mfx_ctx* d : devs_of(c)) {  // summed over the context's devices
        HIPCHECK(hipSetDevice(d->device));
        unsigned long long h[WF_NCTR * WF_SHARDS];  // per-shard counter sets (the megakernel uses set 0)
        HIPCHECK(hipMemcpyAsync(h, d->d_counters, sizeof(h), hipMemcpyDeviceToHost, d->stream));
        HIPCHECK(hipStreamSynchronize(d->stream));
        sum_counters(h, out);
        note_live(d, h);
    }
    out[3] = out[0];  // paths == primary rays
    return MFX_OK;
}
}  // extern "C"
