// mfx_api.cpp — the extern "C" boundary (include/mafrix_rt.h): what describes a context, and what ends one
// (mfx_create.cpp makes them and moves their cameras; mfx_ctx.h names the files that hold the other calls).
// One mfx_ctx = one `Scene` on one or more GPUs. Per device the scene images live in HBM from
// mfx_create until mfx_destroy, and every render call is the wavefront pipeline's launches on
// that device's own HIP stream. A context over G devices (mfx_options.devices) is a primary
// device context plus G - 1 peers built from the same host scene; each device renders its own
// sample partition, and one RCCL reduce (a communicator the library owns, ncclCommInitAll over
// the device list) sums the FP64 accumulators into the primary's, where film and post run. No
// call falls back to a CPU path.
#include <dlfcn.h>

#include "mfx_ctx.h"

using namespace mfxh;

namespace {
thread_local std::string g_err;  // written by fail(), read by mfx_last_error()
}  // namespace

int mfxh::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

const Rccl* mfxh::rccl() {
    static Rccl r;
    static bool tried = false, ok = false;
    if (tried) return ok ? &r : nullptr;
    tried = true;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return nullptr;
    r.commInitAll = (decltype(r.commInitAll))dlsym(h, "ncclCommInitAll");
    r.commDestroy = (decltype(r.commDestroy))dlsym(h, "ncclCommDestroy");
    r.reduce = (decltype(r.reduce))dlsym(h, "ncclReduce");
    r.groupStart = (decltype(r.groupStart))dlsym(h, "ncclGroupStart");
    r.groupEnd = (decltype(r.groupEnd))dlsym(h, "ncclGroupEnd");
    r.errorString = (decltype(r.errorString))dlsym(h, "ncclGetErrorString");
    ok = r.commInitAll && r.commDestroy && r.reduce && r.groupStart && r.groupEnd && r.errorString;
    return ok ? &r : nullptr;
}

int mfxh::whole_film_single_device(const mfx_ctx* c, const char* who) {
    if (c->api_part_count != 1 || (c->flags & MFX_F_ROW_PARTITION) || c->multi.device_list || !c->multi.peers.empty())
        return fail(MFX_E_STATE, std::string(who) + " needs one device and the whole film and sample set "
                                                    "(no device list, part_count == 1, no MFX_F_ROW_PARTITION)");
    return MFX_OK;
}

mfx_ctx::~mfx_ctx() {
    for (ncclComm_t cm : multi.comms)
        if (cm) (void)rccl()->commDestroy(cm);
    multi.comms.clear();
    multi.peers.clear();
    (void)hipSetDevice(device);
}

static void instancing_info(const MfxHostScene& h, double out[8]) {
    out[0] = (double)h.inst.size();
    out[1] = h.ntemplates;
    out[2] = h.inst.empty() ? 0 : h.tlas_nodes;
    out[3] = h.blas_nodes;
    out[4] = h.blas_slots;
    out[5] = h.top_slots;
    out[6] = h.world_slots;
    out[7] = (double)(h.nodes.size() * sizeof(MfxNode) + h.slots.size() * sizeof(MfxSlot) +
                      h.inst.size() * sizeof(MfxInstance));
}

// resident blocks per CU of the context's chosen k_shadow (*sb) and of its k_resolve (*rb), on its device
static int shadow_resolve_blocks(mfx_ctx* c, int* sb, int* rb) {
    const LaunchShapes& A = c->scene.shapes;
    HIPCHECK(hipSetDevice(c->device));
    HIPCHECK(mfx_wf_kernel_occupancy(wf_lds_shape(c->scene, wf_textured(c), true, A.stack_lds_shd, A.ntop_shd, A.nslot_shd), sb));
    if (A.shadow_waves == 3) *sb = std::min(*sb, 3);  // (the 3-wave build: scene_shapes)
    HIPCHECK(mfx_wf_resolve_occupancy(wf_multi_light(c), rb, wf_textured(c)));
    return MFX_OK;
}

extern "C" {
int mfx_pinhole_derive(const mfx_pinhole* cam, double out[12]) {
    if (!cam || !out) return fail(MFX_E_INVALID, "mfx_pinhole_derive: null argument");
    MfxCamera m;
    mfx_derive_camera(*cam, m);
    std::memcpy(out, &m, sizeof(m));
    return MFX_OK;
}

int mfx_camera_info(mfx_ctx* c, double out[16]) {
    if (!c || !out) return fail(MFX_E_INVALID, "mfx_camera_info: null argument");
    static_assert(sizeof(MfxCamera) == 12 * sizeof(double), "MfxCamera is position, topleft, right, down");
    const MfxHostScene& h = c->scene.host;
    std::memcpy(out, &h.camera, sizeof(MfxCamera));
    float eps = 0.f, eps_t = 0.f;
    mfx_camera_eps(h, h.camera.position, &eps, &eps_t);
    out[12] = (double)c->cam_epoch;
    out[13] = (double)h.eps;
    out[14] = (double)eps;
    out[15] = (double)c->cam_rebuilds;
    return MFX_OK;
}

const char* mfx_last_error(void) { return g_err.c_str(); }
int mfx_abi_version(void) { return MFX_ABI_VERSION; }

int mfx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mfx_texture_info(mfx_ctx* c, double out[8]) {
    if (!c || !out) return fail(MFX_E_INVALID, "mfx_texture_info: null argument");
    const bool tx = wf_textured(c);
    int sb = 0, rb = 0;
    MFX_TRY(shadow_resolve_blocks(c, &sb, &rb));
    const MfxTexHost& h = c->tex.host;
    const double v[8] = {tx ? (double)h.desc.size() : 0.0,
                         tx ? 1.0 : 0.0,
                         tx ? (double)h.ntexels * 4.0 : 0.0,
                         tx ? (double)(h.uvrec.size() * sizeof(double) + h.ptex.size() * sizeof(int32_t)) : 0.0,
                         tx ? (double)WF_TEXEL_BYTES_PER_SLOT(c->scene.host.max_depth + 1) : 0.0,
                         (double)sb,
                         (double)rb,
                         0.0};
    std::copy(v, v + 8, out);
    return MFX_OK;
}

int mfx_light_table(const mfx_quad_light* lights, int32_t nlights, double* out) {
    if (!out) return fail(MFX_E_INVALID, "mfx_light_table: null argument");
    std::vector<MfxLight> t;
    std::string err;
    if (!mfx_prepare_lights(lights, nlights, t, err)) return fail(MFX_E_INVALID, "mfx_light_table: " + err);
    for (int32_t n = 0; n < nlights; ++n) {
        out[4 * n + 0] = t[n].area;
        out[4 * n + 1] = 1. / t[n].area;
        out[4 * n + 2] = t[n].pdf;
        out[4 * n + 3] = 0.0;
    }
    return MFX_OK;
}

int mfx_light_info(mfx_ctx* c, double out[8]) {
    if (!c || !out) return fail(MFX_E_INVALID, "mfx_light_info: null argument");
    const bool ml = wf_multi_light(c);
    int sb = 0, rb = 0;
    MFX_TRY(shadow_resolve_blocks(c, &sb, &rb));
    const MfxHostScene& h = c->scene.host;
    const double v[8] = {(double)h.lights.size(), ml ? 1.0 : 0.0, ml ? (double)(h.lights.size() * sizeof(MfxLight)) : 0.0,
                         ml ? (double)WF_LIGHT_BYTES_PER_SLOT(h.max_depth + 1) : 0.0, (double)sb, (double)rb, 0.0, 0.0};
    std::copy(v, v + 8, out);
    return MFX_OK;
}

void mfx_destroy(mfx_ctx* ctx) { delete ctx; }

int mfx_expand_instances(const mfx_prim* prims, int64_t nprims, const mfx_instance* instances, int32_t ninstances,
                         mfx_prim* out, int64_t cap, int64_t* nout) {
    if (!nout) return fail(MFX_E_INVALID, "mfx_expand_instances: null count");
    std::vector<mfx_prim> w;
    std::string err;
    if (!mfx_expand(prims, nprims, instances, ninstances, w, err)) return fail(MFX_E_INVALID, "mfx_expand_instances: " + err);
    *nout = (int64_t)w.size();
    if (out) {
        if (cap < (int64_t)w.size()) return fail(MFX_E_INVALID, "mfx_expand_instances: output too small");
        std::copy(w.begin(), w.end(), out);
    }
    return MFX_OK;
}

int mfx_instancing_info(mfx_ctx* c, double out[8]) {
    if (!c || !out) return fail(MFX_E_INVALID, "null argument");
    instancing_info(c->scene.host, out);
    return MFX_OK;
}

int mfx_build_instanced_info(const mfx_scene_desc* scene, const mfx_instance* instances, int32_t ninstances,
                             int32_t flags, double out[8], int32_t* stack_entries) {
    if (!out) return fail(MFX_E_INVALID, "null argument");
    MfxHostScene h;
    std::string err;
    if (!scene) return fail(MFX_E_INVALID, "null argument");
    if ((flags & MFX_F_FLATTEN) && (flags & MFX_F_TWO_LEVEL))
        return fail(MFX_E_INVALID, "mfx_build_instanced_info: MFX_F_FLATTEN and MFX_F_TWO_LEVEL exclude each other");
    if (!mfx_build_scene(scene, h, err, false, instances, ninstances, flatten_instances(scene, instances, ninstances, flags)))
        return fail(MFX_E_INVALID, "mfx_build_instanced_info: " + err);
    instancing_info(h, out);
    if (stack_entries) *stack_entries = h.stack_entries;
    return MFX_OK;
}

int mfx_build_info(mfx_ctx* c, double out[8], uint64_t* digest) {
    if (!c) return fail(MFX_E_STATE, "null context");
    const MfxHostScene& h = c->scene.host;
    if (out) {
        out[0] = h.ms_ref_bvh;
        out[1] = h.ms_bvh;
        out[2] = h.ms_total;
        out[3] = h.images_gpu ? 2.0 : (h.bvh_gpu ? 1.0 : 0.0);
        out[4] = (double)h.nodes.size();
        out[5] = (double)h.slots.size();
        out[6] = h.nodes2;
        out[7] = h.bvh_levels;
    }
    if (digest) *digest = mfx_scene_digest(h);
    return MFX_OK;
}

int mfx_device_info(mfx_ctx* c, int32_t* out, int32_t cap) {
    if (!c || !out) return fail(MFX_E_INVALID, "null argument");
    const std::vector<mfx_ctx*> ds = devs_of(c);
    if (cap < 5 + (int32_t)ds.size()) return fail(MFX_E_INVALID, "mfx_device_info: cap < 5 + devices");
    out[0] = (int32_t)ds.size();
    out[1] = (int32_t)c->multi.comms.size();
    out[2] = !c->multi.comms.empty() ? 1 : (c->multi.peers.empty() ? 0 : 2);
    out[3] = c->band_index;
    out[4] = c->band_count;
    for (size_t g = 0; g < ds.size(); ++g) out[5 + g] = ds[g]->device;
    return MFX_OK;
}

int mfx_launch_info(mfx_ctx* c, int32_t* out, int32_t cap) {
    if (!c || !out) return fail(MFX_E_INVALID, "null argument");
    if (cap < MFX_LAUNCH_INFO_N) return fail(MFX_E_INVALID, "mfx_launch_info: cap < MFX_LAUNCH_INFO_N");
    const SceneImages& s = c->scene;
    const LaunchShapes& A = s.shapes;
    const bool inst = !s.host.inst.empty();
    const bool cuts = cuts_apply(c);
    if (cuts) MFX_TRY(cuts_read_stats(c));
    const CamCuts& K = c->cuts;
    const int64_t tiles = (int64_t)((s.host.width + 7) / 8) * ((s.host.height + 7) / 8);
    const int32_t v[MFX_LAUNCH_INFO_N] = {
        s.stack_size, A.stack_lds_ext, A.stack_lds_shd, A.stack_lds_ext < s.stack_size, A.stack_lds_shd < s.stack_size,
        A.ntop_ext, A.ntop_shd, A.nslot_ext, A.nslot_shd, inst ? std::min<int>((int)s.host.inst.size(), WF_INST_LDS) : 0,
        A.shadow_waves, s.mega_waves, wf_lit_in_hit(c), wf_gray_light(c), !inst && s.wf_cam_grid > 0,
        s.wf_ext_grid, s.wf_shd_grid, inst ? 0 : s.wf_cam_grid, s.spill_deep, s.spill_lanes,
        c->wf_chunk, c->wf_shd_half, c->pool.queue_from, (int32_t)std::min<int64_t>(c->pool.max, INT32_MAX),
        cuts, cuts ? K.cap : 0, cuts ? (int32_t)std::min<int64_t>(tiles * K.cap * (int64_t)sizeof(MfxCutEntry), INT32_MAX) : 0,
        (int32_t)(K.last.len_sum * 1000 / (unsigned long long)std::max<int64_t>(1, tiles)), (int32_t)K.last.len_max,
        (int32_t)K.last.root_tiles, (int32_t)std::min<int64_t>(K.builds, INT32_MAX), cuts ? K.min_samples : 0};
    std::copy(v, v + MFX_LAUNCH_INFO_N, out);
    return MFX_OK;
}

int mfx_camera_cut_table(mfx_ctx* c, void* out, int64_t cap_bytes, int64_t* nbytes, int32_t host) {
    if (!c || !nbytes) return fail(MFX_E_INVALID, "mfx_camera_cut_table: null argument");
    if (!cuts_apply(c)) return fail(MFX_E_STATE, "mfx_camera_cut_table: the context does not use camera cuts");
    const MfxHostScene& h = c->scene.host;
    const size_t tiles = (size_t)((h.width + 7) / 8) * (size_t)((h.height + 7) / 8);
    const size_t bytes = tiles * c->cuts.cap * sizeof(MfxCutEntry);
    *nbytes = (int64_t)bytes;
    if (!out) return MFX_OK;
    if (cap_bytes < (int64_t)bytes) return fail(MFX_E_INVALID, "mfx_camera_cut_table: output too small");
    if (host) {
        std::vector<MfxCutEntry> t(tiles * c->cuts.cap);
        MfxCutStats st;
        mfx_cut::table_host(h.nodes.data(), h.slots.data(), h.camera, h.width, h.height, c->cuts.cap, t.data(), st);
        std::memcpy(out, t.data(), bytes);
        return MFX_OK;
    }
    HIPCHECK(hipSetDevice(c->device));
    MFX_TRY(cuts_ensure(c, INT64_MAX));  // (the table with the slot cull, as the host twin's)
    HIPCHECK(hipMemcpyAsync(out, c->cuts.table, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return MFX_OK;
}

int mfx_camera_cut_info(mfx_ctx* c, double out[32]) {
    if (!c || !out) return fail(MFX_E_INVALID, "mfx_camera_cut_info: null argument");
    for (int k = 0; k < 32; ++k) out[k] = 0.0;
    if (!cuts_apply(c)) return MFX_OK;
    MFX_TRY(cuts_read_stats(c));
    const CamCuts& K = c->cuts;
    out[0] = (double)K.builds;
    out[1] = (double)K.last_ms;
    out[2] = (double)K.last.len_sum;
    out[3] = (double)K.last.len_max;
    out[4] = (double)K.last.root_tiles;
    out[5] = (double)K.last.empty_tiles;
    out[6] = (double)((int64_t)((c->scene.host.width + 7) / 8) * ((c->scene.host.height + 7) / 8));
    out[7] = (double)K.cap;
    for (int n = 0; n <= MFX_CUT_CAP_MAX; ++n) out[8 + n] = (double)K.last.hist[n];
    out[25] = (double)K.last.slots_seen;
    out[26] = (double)K.last.slots_culled;
    out[27] = (double)K.last.leaves_dropped;
    out[28] = (double)K.last.leaves_narrowed;
    out[29] = K.culled ? 1.0 : 0.0;
    return MFX_OK;
}

int mfx_stats(mfx_ctx* c, double* rays, double* seconds) {
    if (!c) return fail(MFX_E_INVALID, "null context");
    if (seconds) {
        double ms = 0;
        MFX_TRY(mfx_last_trace_ms(c, &ms));
        *seconds = ms * 1e-3;
    }
    if (rays) {
        double n[16];
        MFX_TRY(mfx_ray_counts(c, n));
        *rays = n[0] + n[1] + n[2];
    }
    return MFX_OK;
}

int mfx_reset(mfx_ctx* c) {
    if (!c) return fail(MFX_E_STATE, "null context");
    // stream-ordered after anything that reads the film (no wait for a background batch)
    for (mfx_ctx* d : devs_of(c)) {
        HIPCHECK(hipSetDevice(d->device));
        HIPCHECK(hipMemsetAsync(d->d_film, 0, 3 * sizeof(double) * (size_t)d->npix, d->stream));
    }
    HIPCHECK(hipSetDevice(c->device));
    c->frame_count = 0.0;
    c->ahead.film_in_dfilm = true;
    c->ahead.dfilm_buf = -1;
    if (c->ahead.ready()) {
        c->ahead.film_epoch += 1;
        c->ahead.cur = -1;
        return MFX_OK;
    }
    return mfx_sync(c);
}

int mfx_sync(mfx_ctx* c) {
    if (!c) return fail(MFX_E_STATE, "null context");
    for (mfx_ctx* d : devs_of(c)) {
        HIPCHECK(hipSetDevice(d->device));
        HIPCHECK(hipStreamSynchronize(d->stream));
    }
    return MFX_OK;
}

int mfx_stream(mfx_ctx* c, void** stream) {
    if (!c || !stream) return fail(MFX_E_INVALID, "null argument");
    *stream = (void*)c->stream.get();
    return MFX_OK;
}
}  // extern "C"
