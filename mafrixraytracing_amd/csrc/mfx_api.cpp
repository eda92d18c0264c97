// mfx_api.cpp — the extern "C" boundary (include/mafrix_rt.h): contexts and what describes them
// (mfx_ctx.h names the files that hold the other calls).
// One mfx_ctx = one `Scene` on one or more GPUs. Per device the scene images live in HBM from
// mfx_create until mfx_destroy, and every render call is the wavefront pipeline's launches on
// that device's own HIP stream. A context over G devices (mfx_options.devices) is a primary
// device context plus G - 1 peers built from the same host scene; each device renders its own
// sample partition, and one RCCL reduce (a communicator the library owns, ncclCommInitAll over
// the device list) sums the FP64 accumulators into the primary's, where film and post run. No
// call falls back to a CPU path.
#include <dlfcn.h>

#include <set>
#include <thread>

#include "mfx_ctx.h"
#include "mfx_half.h"

using namespace mfxh;

namespace {
thread_local std::string g_err;  // written by fail(), read by mfx_last_error()

using mfx_half::node_to_half;  // the per-lane kernels' FP16 nodes (mfx_half.h)

template <typename T>
hipError_t upload(DevBuf<T>& d, const std::vector<T>& v) {
    const hipError_t e = d.alloc(std::max<size_t>(1, v.size()));
    if (e != hipSuccess || v.empty()) return e;
    return hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}
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

static CreateEnv read_create_env() {
    const auto set = [](const char* name) { return getenv(name) != nullptr; };
    const auto num = [](const char* name) { return getenv(name) ? CreateEnv::Int(atoi(getenv(name))) : std::nullopt; };
    CreateEnv v;
    v.node_f32 = set("MFX_NODE_F32");
    v.diag_iter = set("MFX_DIAG_ITER");
    v.no_gray_light = set("MFX_NO_GRAY_LIGHT");
    v.no_lit_in_hit = set("MFX_NO_LIT_IN_HIT");
    v.mega_waves = num("MFX_MEGA_WAVES");
    v.shadow_target_blocks = num("MFX_SHADOW_TARGET_BLOCKS");
    v.stack_lds = num("MFX_STACK_LDS");
    v.ntop = num("MFX_NTOP");
    v.slot_lds = num("MFX_SLOT_LDS");
    v.shadow_waves = num("MFX_SHADOW_WAVES");
    v.blocks_per_cu = num("MFX_BLOCKS_PER_CU");
    v.camera_packets = num("MFX_CAMERA_PACKETS");
    v.cam_blocks = num("MFX_CAM_BLOCKS");
    v.camera_cuts = num("MFX_CAMERA_CUTS");
    v.camera_cut_cap = num("MFX_CAMERA_CUT_CAP");
    v.camera_cut_min_samples = num("MFX_CAMERA_CUT_MIN_SAMPLES");
    v.camera_cut_cull_min_samples = num("MFX_CAMERA_CUT_CULL_MIN_SAMPLES");
    v.pool_fail_once = num("MFX_POOL_FAIL_ONCE");
    v.adaptive_check = num("MFX_ADAPTIVE_CHECK");
    v.iter_events = num("MFX_ITER_EVENTS");
    v.queue_from = num("MFX_QUEUE_FROM");
    v.qchunk = num("MFX_QCHUNK");
    v.ray_queue = num("MFX_RAY_QUEUE");
    v.mega_chunk = num("MFX_MEGA_CHUNK");
    v.shd_half = num("MFX_SHD_HALF");
    v.chunk = num("MFX_CHUNK");
    if (const char* e = getenv("MFX_POOL")) v.pool = atoll(e);
    return v;
}

// the largest v in [lo, hi] that keeps(v) holds for; lo is taken to keep it, and no v above one that does not
template <typename F>
static int largest_keeping(int lo, int hi, F keeps) {
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (keeps(mid)) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

#define CK(expr) HIP_TRY(expr, _e == hipErrorOutOfMemory ? MFX_E_NOMEM : MFX_E_DEVICE, #expr ": ")

// The scene images of c->host in HBM, with the context's device current (ctx_setup at creation;
// mfx_set_camera when the images are built again)
static int scene_upload(mfx_ctx* c) {
    c->image_gen += 1;  // (the camera cuts are the old image's)
    c->stack_size = std::max(1, c->host.stack_entries);
    if (c->stack_size > 96) return fail(MFX_E_INVALID, "mfx_create: BVH too deep for the LDS traversal stack");
    CK(upload(c->d_nodes, c->host.nodes));
    CK(upload(c->d_slots, c->host.slots));
    if (MFX_NODE_F16 && !c->env.node_f32) {  // (MFX_NODE_F32=1: the F16 build on FP32 nodes)
        std::vector<MfxNodeH> nh(c->host.nodes.size());
        for (size_t i = 0; i < nh.size(); ++i) nh[i] = node_to_half(c->host.nodes[i]);
        CK(upload(c->d_nodes_h, nh));
    }
    CK(upload(c->d_slot_ref, c->host.slot_ref));
    CK(upload(c->d_ref_blob, c->host.ref_blob));
    CK(upload(c->d_shade, c->host.shade));
    CK(upload(c->d_albedo, c->host.albedo));
    CK(upload(c->d_light, std::vector<MfxLight>{c->host.light}));
    if (wf_multi_light(c)) CK(upload(c->d_lights, c->host.lights));  // (once per device of a list: every device runs this)
    else c->d_lights.reset();
    CK(upload(c->d_cam, std::vector<MfxCamera>{c->host.camera}));
    CK(upload(c->d_refs, std::vector<const void*>{c->d_slot_ref.get(), c->d_ref_blob.get()}));
    if (!c->host.inst.empty()) CK(upload(c->d_inst, c->host.inst));
    else c->d_inst.reset();
    return MFX_OK;
}

// The tables of a textured context in HBM (ctx_setup, once per device: they outlive an mfx_set_camera
// rebuild). The texels come straight from the caller's arrays (c->tex.src, valid while creation runs).
static int texture_upload(mfx_ctx* c) {
    Textures& t = c->tex;
    if (!t.host.on) return MFX_OK;
    if (!t.src) return fail(MFX_E_STATE, "mfx_create_textured: no texture source");
    CK(upload(t.d_uvrec, t.host.uvrec));
    CK(upload(t.d_ptex, t.host.ptex));
    CK(upload(t.d_desc, t.host.desc));
    CK(t.d_texels.alloc((size_t)std::max<int64_t>(1, t.host.ntexels)));
    for (size_t k = 0; k < t.host.desc.size(); ++k) {
        const MfxTexDesc& d = t.host.desc[k];
        CK(hipMemcpy(t.d_texels.get() + d.base, t.src[k].rgba, (size_t)d.width * d.height * 4, hipMemcpyHostToDevice));
    }
    return MFX_OK;
}

// Occupancy-derived launch shapes of the scene in c->host (its stack bound, node and slot counts,
// instances), and the buffers sized by them; with the context's device current
static int scene_shapes(mfx_ctx* c) {
    const CreateEnv& env = c->env;
    const bool inst = !c->host.inst.empty();
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, c->device));
    int bpc = 0;
    // the megakernel's register budget: 4 waves per SIMD unless the stack is deep (its spills)
    c->mega_waves = c->stack_size <= 36 ? 4 : 1;
    if (env.mega_waves) c->mega_waves = *env.mega_waves == 4 ? 4 : 1;
    CK(mfx_trace_occupancy(c->stack_size, &bpc, inst, c->mega_waves));
    bpc = std::max(1, std::min(bpc, 8));
    c->grid = prop.multiProcessorCount * bpc;
    // Traversal stacks, per kernel: the whole bound in LDS unless that costs resident blocks; then
    // the largest LDS share that keeps them, the deeper entries spilled to a global column (the
    // kernels' SPILL instances). Measured: with a deep BVH (C4's bound is 44 entries: k_extend 3 and
    // k_shadow 2 blocks per CU with full stacks) spilling is +14 %; where the full stacks allow
    // k_extend its 4 blocks and k_shadow 3 (C2, flat C5), k_shadow's fourth block with the largest
    // share that keeps it is +2 % (C2, C5) to +4 % (C4) (r02y: 16 entries, the round-1 rule, gained
    // nothing there).
    WfParams& A = c->pool.params;  // the launch shapes go straight into the trace's parameters
    hipError_t qerr = hipSuccess;  // the first occupancy query that failed (its answer counts as no block)
    // resident blocks per CU of k_extend or k_shadow with nlds stack entries per lane in LDS (the rest
    // spilled), and ntop top nodes and nslot slots beside them
    auto blocks = [&](bool shd, int nlds, int ntop = 0, int nslot = 0) {
        const WfLdsShape s{shd, nlds < c->stack_size, c->d_nodes_h != nullptr, nlds, ntop, (int)c->host.inst.size(), nslot,
                           shd && wf_multi_light(c), shd && wf_textured(c)};
        int b = 0;
        const hipError_t e = mfx_wf_kernel_occupancy(s, &b);
        if (e != hipSuccess && qerr == hipSuccess) qerr = e;
        return e == hipSuccess ? b : 0;
    };
    int ebpc = 0, sbpc = 0;
    for (const bool shd : {false, true}) {
        const int full = blocks(shd, c->stack_size);
        int nlds = c->stack_size;
        if (c->stack_size > WF_STACK_LDS) {
            const int b16 = blocks(shd, WF_STACK_LDS);
            const int target = shd ? std::max(full, std::min(env.shadow_target_blocks.value_or(8), b16)) : b16;
            // (blocks only fall as the share grows)
            if (full < target) nlds = largest_keeping(WF_STACK_LDS, c->stack_size - 1, [&](int n) { return blocks(shd, n) >= target; });
            if (c->diag_iter)
                fprintf(stderr, "wavefront: %s blocks/CU: full %d-entry stacks %d, %d in LDS %d; chosen %d in LDS, %d\n",
                        shd ? "k_shadow" : "k_extend", c->stack_size, full, WF_STACK_LDS, b16, nlds, blocks(shd, nlds));
        }
        if (env.stack_lds) nlds = std::max(1, std::min(c->stack_size, *env.stack_lds));
        (shd ? A.stack_lds_shd : A.stack_lds_ext) = nlds;
        (shd ? sbpc : ebpc) = blocks(shd, nlds);
    }
    {  // top BVH nodes in LDS: as many as fit in the LDS the resident blocks leave over
        int cap = std::min((int)c->host.nodes.size(), WF_NTOP_MAX);
        if (env.ntop) cap = std::max(0, std::min(cap, *env.ntop));
        for (const bool shd : {false, true}) {
            const int nlds = shd ? A.stack_lds_shd : A.stack_lds_ext, want = shd ? sbpc : ebpc;
            // (resident blocks do not grow with ntop)
            const int ntop = largest_keeping(0, cap, [&](int n) { return blocks(shd, nlds, n) >= want; });
            (shd ? A.ntop_shd : A.ntop_ext) = ntop;
            // A small scene's whole slot array (80-B test prefixes) in LDS too, when it fits beside the
            // top nodes without costing a resident block: every leaf test then reads LDS (C3: 26 slots)
            // (two-level scenes: none — their kernel instances never read slots from LDS)
            int ns = inst ? 0 : (int)c->host.slots.size();
            if (ns > WF_SLOT_LDS_MAX || (env.slot_lds && *env.slot_lds == 0)) ns = 0;
            if (ns > 0 && blocks(shd, nlds, ntop, ns) < want) ns = 0;
            (shd ? A.nslot_shd : A.nslot_ext) = ns;
        }
        HIP_TRY(qerr, MFX_E_DEVICE, "mfx_wf_kernel_occupancy: ");
        // k_shadow with at most 3 resident blocks per CU (its LDS) runs the instance compiled for 3
        // waves per SIMD: more registers, no spills (C2 / C5 +2 %); with 4 it keeps the 4-wave one
        A.shadow_waves = sbpc <= 3 ? 3 : 4;
        if (env.shadow_waves) A.shadow_waves = *env.shadow_waves == 3 ? 3 : 4;
        if (wf_multi_light(c) || wf_textured(c)) A.shadow_waves = 4;  // the several-light and textured instances are the 4-wave build's only
        if (A.shadow_waves == 3) sbpc = std::min(sbpc, 3);
        if (c->diag_iter)
            fprintf(stderr,
                    "wavefront: stack %d/%d (extend) %d/%d (shadow) in LDS, blocks/CU extend %d shadow %d (%d-wave "
                    "build), top nodes in LDS %d / %d, slots in LDS %d / %d\n",
                    A.stack_lds_ext, c->stack_size, A.stack_lds_shd, c->stack_size, ebpc, sbpc,
                    A.shadow_waves, A.ntop_ext, A.ntop_shd, A.nslot_ext, A.nslot_shd);
    }
    if (env.blocks_per_cu) {  // tuning knob: resident blocks per CU (<= occupancy)
        ebpc = std::min(ebpc, std::max(1, *env.blocks_per_cu));
        sbpc = std::min(sbpc, std::max(1, *env.blocks_per_cu));
    }
    c->wf_ext_grid = prop.multiProcessorCount * std::max(1, std::min(ebpc, 8));
    {  // camera-ray packets (flat scenes)
        if (env.camera_packets.value_or(1) && !inst) {
            int cb = 0;
            // camera cuts (mfx_camera_cuts.h): on unless MFX_CAMERA_CUTS=0, MFX_CAMERA_CUT_CAP entries a tile
            c->cuts.on = env.camera_cuts.value_or(1) != 0;
            c->cuts.cap = std::max(1, std::min(env.camera_cut_cap.value_or(MFX_CUT_CAP_DEFAULT), MFX_CUT_CAP_MAX));
            c->cuts.min_samples = std::max(1, env.camera_cut_min_samples.value_or(MFX_CUT_MIN_SAMPLES));
            c->cuts.cull_min_samples = std::max(1, env.camera_cut_cull_min_samples.value_or(MFX_CUT_CULL_MIN_SAMPLES));
            CK(mfx_cam_occupancy(c->stack_size, &cb, c->cuts.on));
            if (env.cam_blocks) cb = std::min(cb, std::max(1, *env.cam_blocks));
            c->wf_cam_grid = prop.multiProcessorCount * std::max(1, std::min(cb, 8));
        }
    }
    c->wf_shd_grid = prop.multiProcessorCount * std::max(1, std::min(sbpc, 8));
    {  // deep traversal-stack entries of every lane of the larger grid
        const size_t lanes = (size_t)std::max(c->wf_ext_grid, c->wf_shd_grid) * 256;
        const int deep = c->stack_size - std::min(A.stack_lds_ext, A.stack_lds_shd);
        CK(c->d_spill.alloc(lanes * std::max(1, deep)));
        c->spill_deep = std::max(1, deep);
        c->spill_lanes = (int)lanes;
    }
    CK(c->d_vscratch.alloc(6 * (size_t)(c->host.max_depth + 1) * c->grid * 256));
    return MFX_OK;
}

// Device resources of a context whose host scene, device, seed, flags and partition are set:
// stream, events, the scene images in HBM, accumulators, occupancy-derived launch shapes. On
// failure the caller destroys the context, which releases whatever was allocated.
static int ctx_setup(mfx_ctx* c) {
    c->npix = (int64_t)c->host.width * c->host.height;
    const CreateEnv& env = c->env = read_create_env();
    CK(hipSetDevice(c->device));
    CK(c->stream.create());
    CK(c->h_counters.alloc(WF_NCTR * WF_SHARDS));
    CK(c->ev0.create());
    CK(c->ev1.create());
    MFX_TRY(scene_upload(c));
    MFX_TRY(texture_upload(c));
    const size_t npix = (size_t)c->npix, plane = sizeof(double) * npix;
    CK(c->d_accum_own.alloc(3 * npix));
    c->d_accum = c->d_accum_own;
    CK(c->d_film.alloc(3 * npix));
    CK(c->d_frame.alloc(4 * npix));
    CK(c->d_rgba.alloc(4 * npix));
    CK(c->d_work.alloc(8));
    CK(c->d_counters.alloc(WF_NCTR * WF_SHARDS));
    CK(c->d_counters_total.alloc(WF_NCTR * WF_SHARDS));
    CK(hipMemset(c->d_counters_total, 0, kCounterBytes));
    CK(c->pool.ctl.alloc(WF_CTL_ALLOC));
    size_t mfree = 0, mtotal = 0;
    if (hipMemGetInfo(&mfree, &mtotal) == hipSuccess && mfree > 0)
        c->pool.max = std::max<int64_t>(1 << 20, std::min<int64_t>(c->pool.max, (int64_t)(mfree / 4 / pool_slot_bytes(c))));
    // (at most 2^28 slots: k_extend's pending entries keep a slot index in 28 bits)
    c->pool.fail_once = env.pool_fail_once.value_or(0) != 0;
    if (env.pool) c->pool.max = std::max<int64_t>(2048, std::min<int64_t>(1 << 28, *env.pool));
    c->diag_iter = env.diag_iter;
    c->adp.check = env.adaptive_check.value_or(0) != 0;
    if (env.iter_events) c->iter_events = *env.iter_events != 0 || c->diag_iter;
    if (env.queue_from) c->pool.queue_from = MFX_RAY_QUEUE ? std::max(-2, *env.queue_from) : -1;
    if (env.qchunk) c->pool.qchunk = std::max(64, std::min(WF_CHUNK_MAX, *env.qchunk / 64 * 64));
    if (env.ray_queue && *env.ray_queue == 0) c->pool.queue_from = -1;
    if (env.mega_chunk) c->mega_chunk = std::max(1, *env.mega_chunk);
    // MFX_F_IN_FLIGHT: the caller alternates frames over several contexts of this device, so each
    // launch's ramp-down runs beside another frame's launches: larger chunk fetches and whole ones
    // for k_shadow (r05s, C2's 1/8 share over 3 contexts: 4.44 -> 4.37 ms, the 1/4 share 8.78 -> 8.63)
    if (c->flags & MFX_F_IN_FLIGHT) {
        c->wf_chunk = 512;
        c->wf_shd_half = false;
    }
    if (env.shd_half) c->wf_shd_half = *env.shd_half != 0;
    if (env.chunk) c->wf_chunk = std::max(64, std::min(WF_CHUNK_MAX, *env.chunk / 64 * 64));
    CK(hipMemset(c->d_accum, 0, 3 * plane));
    CK(hipMemset(c->d_film, 0, 3 * plane));
    CK(hipMemset(c->d_counters, 0, kCounterBytes));
    return scene_shapes(c);
}
#undef CK

// Two-level or flat for an instanced scene. The flat image (one BVH over the expansion) is the faster
// search (C5: 5,088 vs 4,729 Mrays/s, r02bt) and exactly the same results, so it is taken whenever it
// fits the budget: traversal slots of the expansion x 512 B (slot, shade record, nodes and reference
// leaves) <= MFX_FLATTEN_MAX_BYTES (default 2 GiB; C5 is 93,698 slots, 48 MB) and, on a device,
// <= a sixteenth of its free memory. MFX_F_TWO_LEVEL keeps the instances two-level regardless;
// MFX_F_FLATTEN flattens regardless (both: rejected, MFX_E_INVALID, by the callers).
static bool flatten_instances(const mfx_scene_desc* scene, const mfx_instance* instances, int32_t ninstances,
                              int32_t flags, size_t device_free = 0) {
    if (flags & MFX_F_FLATTEN) return true;
    if (!instances || (flags & MFX_F_TWO_LEVEL)) return false;
    double budget = 2.0 * 1024 * 1024 * 1024;
    if (const char* e = getenv("MFX_FLATTEN_MAX_BYTES")) budget = atof(e);
    if (device_free > 0) budget = std::min(budget, (double)device_free / 16.0);
    double slots = 0.0;
    for (int32_t i = 0; i < ninstances; ++i) {
        const int64_t f = instances[i].first, n = instances[i].count;
        if (f < 0 || n < 0 || f + n > scene->nprims) return false;  // mfx_build_scene reports the bad entry
        for (int64_t k = f; k < f + n; ++k) slots += scene->prims[k].kind == MFX_PRIM_RECT ? 2.0 : 1.0;
    }
    return slots * 512.0 <= budget;
}

// the device reduce of a list that repeats a device: its staging buffer and events
static hipError_t repeated_device_setup(mfx_ctx* c) {
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = c->multi.reduce_stage.alloc(3 * (size_t)c->npix);
    if (e == hipSuccess) e = c->multi.reduce_done.create(hipEventDisableTiming);
    if (e != hipSuccess) return e;
    for (const auto& p : c->multi.peers) {
        Event ev;
        if ((e = hipSetDevice(p->device)) != hipSuccess) return e;
        if ((e = ev.create(hipEventDisableTiming)) != hipSuccess) return e;
        c->multi.peer_done.push_back(std::move(ev));
    }
    return hipSetDevice(c->device);
}

static_assert(WF_MAX_LIGHTS == MFX_MAX_LIGHTS, "the kernels' light index width is the ABI's bound");

// lights (mfx_create_lights): the list that replaces scene->light (null: scene->light, N = 1)
// tex (mfx_create_textured): the prepared textures of a scene with a textured primitive, with the caller's
// arrays they were prepared from (null: no textures)
static int create_impl(const mfx_scene_desc* scene, const mfx_instance* instances, int32_t ninstances,
                       const mfx_options* opt, mfx_ctx** out, const mfx_quad_light* lights = nullptr, int32_t nlights = 0,
                       const MfxTexHost* tex = nullptr, const mfx_texture* textures = nullptr,
                       const mfx_prim_uv* prim_uv = nullptr) {
    if (!scene || !opt || !out) return fail(MFX_E_INVALID, "mfx_create: null argument");
    *out = nullptr;
    // the megakernel and the counting instances of the trace kernels are built without textures
    if (tex && (opt->flags & (MFX_F_MEGAKERNEL | MFX_F_COUNT_STATS)))
        return fail(MFX_E_INVALID, "mfx_create_textured: MFX_F_MEGAKERNEL and MFX_F_COUNT_STATS need an untextured scene");
    std::vector<MfxLight> prepared;  // the lights' one validation: mfx_build_scene takes the result
    if (lights) {  // on the host, before any device is asked for
        std::string lerr;
        if (!mfx_prepare_lights(lights, nlights, prepared, lerr)) return fail(MFX_E_INVALID, "mfx_create_lights: " + lerr);
        // the megakernel and the counting instances of the trace kernels are built for one light
        if (nlights >= 2 && (opt->flags & (MFX_F_MEGAKERNEL | MFX_F_COUNT_STATS)))
            return fail(MFX_E_INVALID, "mfx_create_lights: MFX_F_MEGAKERNEL and MFX_F_COUNT_STATS need a single light");
    }
    if (opt->part_count < 1 || opt->part_index < 0 || opt->part_index >= opt->part_count)
        return fail(MFX_E_INVALID, "mfx_create: bad sample partition");
    if (opt->ndevices < 0 || opt->ndevices > MFX_MAX_DEVICES || (opt->ndevices > 0 && !opt->devices))
        return fail(MFX_E_INVALID, "mfx_create: bad device list");
    if (opt->render_ahead < 0 || opt->render_ahead > MFX_MAX_RENDER_AHEAD)
        return fail(MFX_E_INVALID, "mfx_create: render_ahead out of range");
    if (scene->nmat > WF_MAT_MAX) return fail(MFX_E_INVALID, "mfx_create: more than 65,536 materials");
    if ((opt->flags & MFX_F_FLATTEN) && (opt->flags & MFX_F_TWO_LEVEL))
        return fail(MFX_E_INVALID, "mfx_create: MFX_F_FLATTEN and MFX_F_TWO_LEVEL exclude each other");
    int ndev = 0;
    HIPCHECK(hipGetDeviceCount(&ndev));
    std::vector<int> devlist;
    if (opt->ndevices == 0) devlist.push_back(opt->device);
    else devlist.assign(opt->devices, opt->devices + opt->ndevices);
    for (int d : devlist)
        if (d < 0 || d >= ndev) return fail(MFX_E_DEVICE, "mfx_create: no such HIP device");
    const int G = (int)devlist.size();
    HIPCHECK(hipSetDevice(devlist[0]));
    size_t dev_free = 0, dev_total = 0;
    if (hipMemGetInfo(&dev_free, &dev_total) != hipSuccess) dev_free = 0;
    std::unique_ptr<mfx_ctx> c(new mfx_ctx());  // destroyed on every early return
    c->device = devlist[0];
    std::string err;
    // the traversal BVH is built on the first device unless the caller asks for the host build
    // (the same tree either way: tests/test_gpu_build.py); the other devices get copies
    const bool flatten = flatten_instances(scene, instances, ninstances, opt->flags, dev_free);
    if (!mfx_build_scene(scene, c->host, err, (opt->flags & MFX_F_HOST_BVH) == 0, instances, ninstances, flatten, lights,
                         lights ? &prepared : nullptr)) {
        const bool dev = err.rfind("GPU BVH build", 0) == 0;
        return fail(dev ? MFX_E_DEVICE : MFX_E_INVALID, "mfx_create: " + err);
    }
    {  // the description stays with the context: mfx_set_camera may have to build the images again
        KeptScene& k = c->kept;
        k.prims.assign(scene->prims, scene->prims + scene->nprims);
        k.albedo.assign(scene->albedo, scene->albedo + 3 * (size_t)scene->nmat);
        if (instances) k.instances.assign(instances, instances + ninstances);
        if (lights) k.lights.assign(lights, lights + nlights);
        if (tex) k.prim_uv.assign(prim_uv, prim_uv + scene->nprims);
        k.desc = *scene;
        k.desc.prims = nullptr;
        k.desc.albedo = nullptr;
        k.instanced = instances != nullptr;
        k.flatten = flatten;
        k.gpu_bvh = (opt->flags & MFX_F_HOST_BVH) == 0;
    }
    // Image partition: device g of G traces the film's tile rows of band g of G, every sample of the
    // caller's partition, so every per-pixel operation (the sample-order sum, the film add, the post)
    // runs on one device in the one-device order: images are bit-identical to one device's, and the
    // devices' buffers merge exactly (a pixel is non-zero on its own device only). With
    // MFX_F_ROW_PARTITION the caller's part_index / part_count select tile rows too: device g renders
    // rows part_index + g * part_count of part_count * G (no sample partition).
    const bool rows = (opt->flags & MFX_F_ROW_PARTITION) != 0;
    auto init = [&](mfx_ctx* d, int g) {
        d->device = devlist[g];
        d->seed = opt->seed;
        d->flags = opt->flags;
        d->part_index = rows ? 0 : opt->part_index;
        d->part_count = rows ? 1 : opt->part_count;
        d->band_index = rows ? opt->part_index + g * opt->part_count : g;
        d->band_count = rows ? opt->part_count * G : G;
        d->api_part_count = opt->part_count;
    };
    // textured: every device gets the tables (ctx_setup uploads them from the caller's arrays)
    auto with_textures = [&](mfx_ctx* d) {
        if (!tex) return;
        d->tex.host = *tex;
        d->tex.src = textures;
    };
    init(c.get(), 0);
    with_textures(c.get());
    c->ahead.k = opt->render_ahead;
    c->multi.device_list = opt->ndevices > 0;
    MFX_TRY(ctx_setup(c.get()));
    if (G > 1) {  // peers: one host thread each (HIP context creation and uploads run concurrently)
        std::vector<int> prc(G - 1, MFX_OK);
        std::vector<std::string> perr(G - 1);
        std::vector<std::thread> th;
        for (int g = 1; g < G; ++g) {
            mfx_ctx* p = new mfx_ctx();
            c->multi.peers.emplace_back(p);
            p->host = c->host;
            init(p, g);
            with_textures(p);
            th.emplace_back([p, g, &prc, &perr] {
                prc[g - 1] = ctx_setup(p);
                if (prc[g - 1]) perr[g - 1] = mfx_last_error();  // this thread's message
            });
        }
        for (auto& t : th) t.join();
        for (int g = 1; g < G; ++g)
            if (prc[g - 1]) return fail(prc[g - 1], "device " + std::to_string(devlist[g]) + ": " + perr[g - 1]);
    }
    if (opt->ndevices > 0) {
        // The device reduce. Distinct devices: one RCCL communicator per device, owned by the
        // library (ncclCommInitAll, single process). A list that repeats a device cannot form a
        // communicator: its accumulators are added into the primary's in device order instead.
        const bool distinct = std::set<int>(devlist.begin(), devlist.end()).size() == devlist.size();
        if (distinct) {
            const Rccl* R = rccl();
            if (!R) return fail(MFX_E_DEVICE, "mfx_create: RCCL (librccl.so.1) could not be loaded");
            c->multi.comms.assign(G, nullptr);
            const ncclResult_t r = R->commInitAll(c->multi.comms.data(), G, devlist.data());
            if (r != ncclSuccess) {
                c->multi.comms.clear();
                return fail(MFX_E_DEVICE, std::string("mfx_create: ncclCommInitAll: ") + R->errorString(r));
            }
        } else {
            const hipError_t e = repeated_device_setup(c.get());
            if (e != hipSuccess)
                return fail(MFX_E_DEVICE, std::string("mfx_create: device reduce setup: ") + hipGetErrorString(e));
        }
    }
    for (mfx_ctx* d : devs_of(c.get())) d->tex.src = nullptr;  // the caller's arrays are the caller's again
    *out = c.release();
    return MFX_OK;
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

// ---- mfx_set_camera -------------------------------------------------------------------------------
// What scene_upload and scene_shapes write: a device context's scene images and the launch shapes
// derived from them. A rebuild parks the old ones here; taking them back undoes it.
struct SceneState {
    MfxHostScene host;
    DevBuf<MfxNode> d_nodes;
    DevBuf<MfxSlot> d_slots;
    DevBuf<MfxNodeH> d_nodes_h;
    DevBuf<int32_t> d_slot_ref;
    DevBuf<uint8_t> d_ref_blob;
    DevBuf<MfxShade> d_shade;
    DevBuf<MfxInstance> d_inst;
    DevBuf<double> d_albedo;
    DevBuf<MfxLight> d_light;
    DevBuf<MfxLight> d_lights;
    DevBuf<MfxCamera> d_cam;
    DevBuf<const void*> d_refs;
    DevBuf<int32_t> d_spill;
    DevBuf<double> d_vscratch;
    WfParams params{};
    int stack_size = 1, grid = 0, mega_waves = 1, wf_ext_grid = 0, wf_shd_grid = 0, wf_cam_grid = 0;
    int spill_deep = 0, spill_lanes = 0;
};
static void swap_scene_state(mfx_ctx* c, SceneState& s) {
    std::swap(c->host, s.host);
    std::swap(c->d_nodes, s.d_nodes);
    std::swap(c->d_slots, s.d_slots);
    std::swap(c->d_nodes_h, s.d_nodes_h);
    std::swap(c->d_slot_ref, s.d_slot_ref);
    std::swap(c->d_ref_blob, s.d_ref_blob);
    std::swap(c->d_shade, s.d_shade);
    std::swap(c->d_inst, s.d_inst);
    std::swap(c->d_albedo, s.d_albedo);
    std::swap(c->d_light, s.d_light);
    std::swap(c->d_lights, s.d_lights);
    std::swap(c->d_cam, s.d_cam);
    std::swap(c->d_refs, s.d_refs);
    std::swap(c->d_spill, s.d_spill);
    std::swap(c->d_vscratch, s.d_vscratch);
    std::swap(c->pool.params, s.params);
    std::swap(c->stack_size, s.stack_size);
    std::swap(c->grid, s.grid);
    std::swap(c->mega_waves, s.mega_waves);
    std::swap(c->wf_ext_grid, s.wf_ext_grid);
    std::swap(c->wf_shd_grid, s.wf_shd_grid);
    std::swap(c->wf_cam_grid, s.wf_cam_grid);
    std::swap(c->spill_deep, s.spill_deep);
    std::swap(c->spill_lanes, s.spill_lanes);
}

// Prepare the kept scene again for `cam` and install it on every device of the context, by creation's
// own steps (mfx_build_scene, scene_upload, scene_shapes). On failure every device has its old images back.
static int rebuild_for_camera(mfx_ctx* c, const mfx_pinhole* cam) {
    const KeptScene& k = c->kept;
    mfx_scene_desc d = k.desc;
    d.prims = k.prims.data();
    d.albedo = k.albedo.data();
    d.camera = *cam;
    HIPCHECK(hipSetDevice(c->device));
    MfxHostScene h;
    std::string err;
    if (!mfx_build_scene(&d, h, err, k.gpu_bvh, k.instanced ? k.instances.data() : nullptr, (int)k.instances.size(), k.flatten,
                         k.lights.empty() ? nullptr : k.lights.data(), &c->host.lights)) {  // (validated at creation)
        const bool dev = err.rfind("GPU BVH build", 0) == 0;
        return fail(dev ? MFX_E_DEVICE : MFX_E_INVALID, "mfx_set_camera: " + err);
    }
    const std::vector<mfx_ctx*> ds = devs_of(c);
    std::vector<SceneState> old(ds.size());
    int rc = MFX_OK;
    size_t done = 0;
    for (; done < ds.size() && rc == MFX_OK; ++done) {
        mfx_ctx* dv = ds[done];
        SceneState& o = old[done];
        o.params = dv->pool.params;  // the pool's arrays stay; the launch shapes are written over
        swap_scene_state(dv, o);
        dv->host = h;  // (the shapes start from a fresh context's defaults: SceneState's)
        rc = hipSetDevice(dv->device) == hipSuccess ? MFX_OK : fail(MFX_E_DEVICE, "mfx_set_camera: hipSetDevice failed");
        if (rc == MFX_OK) rc = scene_upload(dv);
        if (rc == MFX_OK) rc = scene_shapes(dv);
    }
    if (rc != MFX_OK) {
        const std::string msg = mfx_last_error();
        (void)hipGetLastError();
        for (size_t g = 0; g < done; ++g) swap_scene_state(ds[g], old[g]);  // the failed images go with `old`
        (void)hipSetDevice(c->device);
        return fail(rc, msg);
    }
    HIPCHECK(hipSetDevice(c->device));
    c->kept.desc.camera = *cam;
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
    std::memcpy(out, &c->host.camera, sizeof(MfxCamera));
    float eps = 0.f, eps_t = 0.f;
    mfx_camera_eps(c->host, c->host.camera.position, &eps, &eps_t);
    out[12] = (double)c->cam_epoch;
    out[13] = (double)c->host.eps;
    out[14] = (double)eps;
    out[15] = (double)c->cam_rebuilds;
    return MFX_OK;
}

int mfx_set_camera(mfx_ctx* c, const mfx_pinhole* cam) {
    if (!c || !cam) return fail(MFX_E_INVALID, "mfx_set_camera: null argument");
    bool finite = true, zero_dir = true;
    for (int a = 0; a < 3; ++a) {
        finite = finite && std::isfinite(cam->position[a]);
        if (cam->derived) finite = finite && std::isfinite(cam->topleft[a]) && std::isfinite(cam->right[a]) && std::isfinite(cam->down[a]);
        else finite = finite && std::isfinite(cam->direction[a]);
        zero_dir = zero_dir && cam->direction[a] == 0.0;
    }
    if (!cam->derived) finite = finite && std::isfinite(cam->fov) && std::isfinite(cam->aspect);
    if (!finite) return fail(MFX_E_INVALID, "mfx_set_camera: a camera field is not finite");
    if (!cam->derived && zero_dir) return fail(MFX_E_INVALID, "mfx_set_camera: direction is zero");
    MfxCamera m;
    mfx_derive_camera(*cam, m);
    for (const double* v : {m.position, m.topleft, m.right, m.down})
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(v[a])) return fail(MFX_E_INVALID, "mfx_set_camera: the derived camera is not finite");
    if (std::memcmp(&m, &c->host.camera, sizeof(m)) == 0) return MFX_OK;  // the current camera: nothing to do
    // held render-ahead frames are the old camera's: the film comes back to d_film under the old camera, and
    // the frames' epoch ends; then everything the context has enqueued, a background batch included, finishes
    MFX_TRY(ahead_break(c));
    MFX_TRY(mfx_sync(c));
    float eps = 0.f, eps_t = 0.f;
    mfx_camera_eps(c->host, m.position, &eps, &eps_t);
    if (eps <= c->host.eps && eps_t <= c->host.eps_templates) {
        // in place: the boxes stay conservative for every ray this camera can start
        for (mfx_ctx* d : devs_of(c)) {
            HIPCHECK(hipSetDevice(d->device));
            HIPCHECK(hipMemcpy(d->d_cam, &m, sizeof(m), hipMemcpyHostToDevice));
            d->host.camera = m;
        }
        HIPCHECK(hipSetDevice(c->device));
        c->kept.desc.camera = *cam;
    } else {
        MFX_TRY(rebuild_for_camera(c, cam));
        c->cam_rebuilds += 1;
    }
    c->cam_epoch += 1;
    c->adp.accum_valid = false;  // a resume must not mix cameras
    c->ahead.dfilm_buf = -1;
    return MFX_OK;
}

const char* mfx_last_error(void) { return g_err.c_str(); }
int mfx_abi_version(void) { return MFX_ABI_VERSION; }

int mfx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mfx_create(const mfx_scene_desc* scene, const mfx_options* opt, mfx_ctx** out) {
    return create_impl(scene, nullptr, 0, opt, out);
}

int mfx_create_instanced(const mfx_scene_desc* scene, const mfx_instance* instances, int32_t ninstances,
                         const mfx_options* opt, mfx_ctx** out) {
    if (!instances || ninstances < 1) return fail(MFX_E_INVALID, "mfx_create_instanced: no instances");
    return create_impl(scene, instances, ninstances, opt, out);
}

int mfx_create_lights(const mfx_scene_desc* scene, const mfx_quad_light* lights, int32_t nlights,
                      const mfx_instance* instances, int32_t ninstances, const mfx_options* opt, mfx_ctx** out) {
    if (!lights || nlights < 1 || nlights > MFX_MAX_LIGHTS)
        return fail(MFX_E_INVALID, "mfx_create_lights: nlights must be 1 .. MFX_MAX_LIGHTS with a light array");
    const bool flat = !instances && ninstances == 0;
    if (!flat && (!instances || ninstances < 1)) return fail(MFX_E_INVALID, "mfx_create_lights: no instances");
    return create_impl(scene, instances, flat ? 0 : ninstances, opt, out, lights, nlights);
}

int mfx_create_textured(const mfx_scene_desc* scene, const mfx_quad_light* lights, int32_t nlights,
                        const mfx_instance* instances, int32_t ninstances, const mfx_texture* textures,
                        int32_t ntextures, const mfx_prim_uv* prim_uv, const mfx_options* opt, mfx_ctx** out) {
    if (!scene || !opt || !out) return fail(MFX_E_INVALID, "mfx_create_textured: null argument");
    const bool flat = !instances && ninstances == 0;
    if (!flat && (!instances || ninstances < 1)) return fail(MFX_E_INVALID, "mfx_create_textured: no instances");
    MfxTexHost tex;  // on the host, before any device is asked for
    std::string err;
    if (!mfx_prepare_textures(scene, flat ? nullptr : instances, flat ? 0 : ninstances, textures, ntextures, prim_uv, tex, err))
        return fail(MFX_E_INVALID, "mfx_create_textured: " + err);
    // no textured primitive: the call without textures, kernel for kernel
    if (!tex.on) return mfx_create_lights(scene, lights, nlights, instances, ninstances, opt, out);
    if (!lights || nlights < 1 || nlights > MFX_MAX_LIGHTS)
        return fail(MFX_E_INVALID, "mfx_create_textured: nlights must be 1 .. MFX_MAX_LIGHTS with a light array");
    return create_impl(scene, instances, flat ? 0 : ninstances, opt, out, lights, nlights, &tex, textures, prim_uv);
}

int mfx_texture_info(mfx_ctx* c, double out[8]) {
    if (!c || !out) return fail(MFX_E_INVALID, "mfx_texture_info: null argument");
    const bool tx = wf_textured(c), ml = wf_multi_light(c);
    const WfParams& A = c->pool.params;
    HIPCHECK(hipSetDevice(c->device));
    const WfLdsShape s{true, A.stack_lds_shd < c->stack_size, c->d_nodes_h != nullptr, A.stack_lds_shd, A.ntop_shd,
                       (int)c->host.inst.size(), A.nslot_shd, ml, tx};
    int sb = 0, rb = 0;
    HIPCHECK(mfx_wf_kernel_occupancy(s, &sb));
    if (A.shadow_waves == 3) sb = std::min(sb, 3);  // (the 3-wave build: scene_shapes)
    HIPCHECK(mfx_wf_resolve_occupancy(ml, &rb, tx));
    const MfxTexHost& h = c->tex.host;
    const double v[8] = {tx ? (double)h.desc.size() : 0.0,
                         tx ? 1.0 : 0.0,
                         tx ? (double)h.ntexels * 4.0 : 0.0,
                         tx ? (double)(h.uvrec.size() * sizeof(double) + h.ptex.size() * sizeof(int32_t)) : 0.0,
                         tx ? (double)WF_TEXEL_BYTES_PER_SLOT(c->host.max_depth + 1) : 0.0,
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
    const WfParams& A = c->pool.params;
    HIPCHECK(hipSetDevice(c->device));
    const WfLdsShape s{true, A.stack_lds_shd < c->stack_size, c->d_nodes_h != nullptr, A.stack_lds_shd, A.ntop_shd,
                       (int)c->host.inst.size(), A.nslot_shd, ml, wf_textured(c)};
    int sb = 0, rb = 0;
    HIPCHECK(mfx_wf_kernel_occupancy(s, &sb));
    if (A.shadow_waves == 3) sb = std::min(sb, 3);  // (the 3-wave build: scene_shapes)
    HIPCHECK(mfx_wf_resolve_occupancy(ml, &rb, wf_textured(c)));
    const double v[8] = {(double)c->host.lights.size(), ml ? 1.0 : 0.0, ml ? (double)(c->host.lights.size() * sizeof(MfxLight)) : 0.0,
                         ml ? (double)WF_LIGHT_BYTES_PER_SLOT(c->host.max_depth + 1) : 0.0, (double)sb, (double)rb, 0.0, 0.0};
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
    instancing_info(c->host, out);
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
    const MfxHostScene& h = c->host;
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
    const WfParams& A = c->pool.params;
    const bool inst = !c->host.inst.empty();
    const bool cuts = cuts_apply(c);
    if (cuts) MFX_TRY(cuts_read_stats(c));
    const CamCuts& K = c->cuts;
    const int64_t tiles = (int64_t)((c->host.width + 7) / 8) * ((c->host.height + 7) / 8);
    const int32_t v[MFX_LAUNCH_INFO_N] = {
        c->stack_size, A.stack_lds_ext, A.stack_lds_shd, A.stack_lds_ext < c->stack_size, A.stack_lds_shd < c->stack_size,
        A.ntop_ext, A.ntop_shd, A.nslot_ext, A.nslot_shd, inst ? std::min<int>((int)c->host.inst.size(), WF_INST_LDS) : 0,
        A.shadow_waves, c->mega_waves, wf_lit_in_hit(c), wf_gray_light(c), !inst && c->wf_cam_grid > 0,
        c->wf_ext_grid, c->wf_shd_grid, inst ? 0 : c->wf_cam_grid, c->spill_deep, c->spill_lanes,
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
    const size_t tiles = (size_t)((c->host.width + 7) / 8) * (size_t)((c->host.height + 7) / 8);
    const size_t bytes = tiles * c->cuts.cap * sizeof(MfxCutEntry);
    *nbytes = (int64_t)bytes;
    if (!out) return MFX_OK;
    if (cap_bytes < (int64_t)bytes) return fail(MFX_E_INVALID, "mfx_camera_cut_table: output too small");
    if (host) {
        std::vector<MfxCutEntry> t(tiles * c->cuts.cap);
        MfxCutStats st;
        mfx_cut::table_host(c->host.nodes.data(), c->host.slots.data(), c->host.camera, c->host.width, c->host.height, c->cuts.cap, t.data(), st);
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
    out[6] = (double)((int64_t)((c->host.width + 7) / 8) * ((c->host.height + 7) / 8));
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
