// mfx_create.cpp — how a context comes to be (include/mafrix_rt.h: mfx_create, mfx_create_instanced,
// mfx_create_lights, mfx_create_textured) and how mfx_set_camera changes its camera. Both prepare the host
// scene (build_host_scene) and put it on a device with the same two functions: scene_upload and scene_shapes
// fill a SceneImages (mfx_ctx.h). Creation fills the context's own; a camera that needs wider boxes gets fresh
// ones on every device of the context, installed only once all of them are complete.
#include <set>
#include <thread>

#include "mfx_ctx.h"
#include "mfx_half.h"

using namespace mfxh;

namespace {
using mfx_half::node_to_half;  // the per-lane kernels' FP16 nodes (mfx_half.h)

template <typename T>
hipError_t upload(DevBuf<T>& d, const std::vector<T>& v) {
    const hipError_t e = d.alloc(std::max<size_t>(1, v.size()));
    if (e != hipSuccess || v.empty()) return e;
    return hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}
}  // namespace

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

// The scene images of s.host in HBM, on the current device (ctx_setup at creation; mfx_set_camera when
// the images are built again). Of the context it reads the environment alone.
static int scene_upload(SceneImages& s, const CreateEnv& env) {
    s.stack_size = std::max(1, s.host.stack_entries);
    if (s.stack_size > 96) return fail(MFX_E_INVALID, "mfx_create: BVH too deep for the LDS traversal stack");
    CK(upload(s.d_nodes, s.host.nodes));
    CK(upload(s.d_slots, s.host.slots));
    if (MFX_NODE_F16 && !env.node_f32) {  // (MFX_NODE_F32=1: the F16 build on FP32 nodes)
        std::vector<MfxNodeH> nh(s.host.nodes.size());
        for (size_t i = 0; i < nh.size(); ++i) nh[i] = node_to_half(s.host.nodes[i]);
        CK(upload(s.d_nodes_h, nh));
    }
    CK(upload(s.d_slot_ref, s.host.slot_ref));
    CK(upload(s.d_ref_blob, s.host.ref_blob));
    CK(upload(s.d_shade, s.host.shade));
    CK(upload(s.d_albedo, s.host.albedo));
    CK(upload(s.d_light, std::vector<MfxLight>{s.host.light}));
    if (s.multi_light()) CK(upload(s.d_lights, s.host.lights));  // (once per device of a list: every device runs this)
    CK(upload(s.d_cam, std::vector<MfxCamera>{s.host.camera, MfxCamera{}}));  // ([1]: room for a lens record, mfx_set_lens)
    CK(upload(s.d_refs, std::vector<const void*>{s.d_slot_ref.get(), s.d_ref_blob.get()}));
    if (!s.host.inst.empty()) CK(upload(s.d_inst, s.host.inst));
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

WfLdsShape mfxh::wf_lds_shape(const SceneImages& im, bool textured, bool shd, int nlds, int ntop, int nslot) {
    const WfLdsShape s{shd, nlds < im.stack_size, im.d_nodes_h != nullptr, nlds, ntop, (int)im.host.inst.size(), nslot,
                       shd && im.multi_light(), shd && textured, false, shd && im.sky_light, false, shd && im.normals};
    return s;
}

// Occupancy-derived launch shapes of the uploaded scene in s (its stack bound, node and slot counts,
// instances), and the buffers sized by them; on `device`, which is current. Of the context it reads its
// environment, whether it is textured and whether its camera cuts are on.
static int scene_shapes(SceneImages& s, int device, const CreateEnv& env, bool textured, bool cuts_on) {
    const bool inst = !s.host.inst.empty();
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, device));
    int bpc = 0;
    // the megakernel's register budget: 4 waves per SIMD unless the stack is deep (its spills)
    s.mega_waves = s.stack_size <= 36 ? 4 : 1;
    if (env.mega_waves) s.mega_waves = *env.mega_waves == 4 ? 4 : 1;
    CK(mfx_trace_occupancy(s.stack_size, &bpc, inst, s.mega_waves));
    bpc = std::max(1, std::min(bpc, 8));
    s.grid = prop.multiProcessorCount * bpc;
    // Traversal stacks, per kernel: the whole bound in LDS unless that costs resident blocks; then
    // the largest LDS share that keeps them, the deeper entries spilled to a global column (the
    // kernels' SPILL instances). Measured: with a deep BVH (C4's bound is 44 entries: k_extend 3 and
    // k_shadow 2 blocks per CU with full stacks) spilling is +14 %; where the full stacks allow
    // k_extend its 4 blocks and k_shadow 3 (C2, flat C5), k_shadow's fourth block with the largest
    // share that keeps it is +2 % (C2, C5) to +4 % (C4) (r02y: 16 entries, the round-1 rule, gained
    // nothing there).
    LaunchShapes& A = s.shapes;
    hipError_t qerr = hipSuccess;  // the first occupancy query that failed (its answer counts as no block)
    // resident blocks per CU of k_extend or k_shadow with nlds stack entries per lane in LDS (the rest
    // spilled), and ntop top nodes and nslot slots beside them
    auto blocks = [&](bool shd, int nlds, int ntop = 0, int nslot = 0) {
        int b = 0;
        const hipError_t e = mfx_wf_kernel_occupancy(wf_lds_shape(s, textured, shd, nlds, ntop, nslot), &b);
        if (e != hipSuccess && qerr == hipSuccess) qerr = e;
        return e == hipSuccess ? b : 0;
    };
    int ebpc = 0, sbpc = 0;
    for (const bool shd : {false, true}) {
        const int full = blocks(shd, s.stack_size);
        int nlds = s.stack_size;
        if (s.stack_size > WF_STACK_LDS) {
            const int b16 = blocks(shd, WF_STACK_LDS);
            const int target = shd ? std::max(full, std::min(env.shadow_target_blocks.value_or(8), b16)) : b16;
            // (blocks only fall as the share grows)
            if (full < target) nlds = largest_keeping(WF_STACK_LDS, s.stack_size - 1, [&](int n) { return blocks(shd, n) >= target; });
            if (env.diag_iter)
                fprintf(stderr, "wavefront: %s blocks/CU: full %d-entry stacks %d, %d in LDS %d; chosen %d in LDS, %d\n",
                        shd ? "k_shadow" : "k_extend", s.stack_size, full, WF_STACK_LDS, b16, nlds, blocks(shd, nlds));
        }
        if (env.stack_lds) nlds = std::max(1, std::min(s.stack_size, *env.stack_lds));
        (shd ? A.stack_lds_shd : A.stack_lds_ext) = nlds;
        (shd ? sbpc : ebpc) = blocks(shd, nlds);
    }
    {  // top BVH nodes in LDS: as many as fit in the LDS the resident blocks leave over
        int cap = std::min((int)s.host.nodes.size(), WF_NTOP_MAX);
        if (env.ntop) cap = std::max(0, std::min(cap, *env.ntop));
        for (const bool shd : {false, true}) {
            const int nlds = shd ? A.stack_lds_shd : A.stack_lds_ext, want = shd ? sbpc : ebpc;
            // (resident blocks do not grow with ntop)
            const int ntop = largest_keeping(0, cap, [&](int n) { return blocks(shd, nlds, n) >= want; });
            (shd ? A.ntop_shd : A.ntop_ext) = ntop;
            // A small scene's whole slot array (80-B test prefixes) in LDS too, when it fits beside the
            // top nodes without costing a resident block: every leaf test then reads LDS (C3: 26 slots)
            // (two-level scenes: none — their kernel instances never read slots from LDS)
            int ns = inst ? 0 : (int)s.host.slots.size();
            if (ns > WF_SLOT_LDS_MAX || (env.slot_lds && *env.slot_lds == 0)) ns = 0;
            if (ns > 0 && blocks(shd, nlds, ntop, ns) < want) ns = 0;
            (shd ? A.nslot_shd : A.nslot_ext) = ns;
        }
        HIP_TRY(qerr, MFX_E_DEVICE, "mfx_wf_kernel_occupancy: ");
        // k_shadow with at most 3 resident blocks per CU (its LDS) runs the instance compiled for 3
        // waves per SIMD: more registers, no spills (C2 / C5 +2 %); with 4 it keeps the 4-wave one
        A.shadow_waves = sbpc <= 3 ? 3 : 4;
        if (env.shadow_waves) A.shadow_waves = *env.shadow_waves == 3 ? 3 : 4;
        if (s.multi_light() || textured || s.normals) A.shadow_waves = 4;  // the several-light, textured and SN instances are the 4-wave build's only
        if (A.shadow_waves == 3) sbpc = std::min(sbpc, 3);
        if (env.diag_iter)
            fprintf(stderr,
                    "wavefront: stack %d/%d (extend) %d/%d (shadow) in LDS, blocks/CU extend %d shadow %d (%d-wave "
                    "build), top nodes in LDS %d / %d, slots in LDS %d / %d\n",
                    A.stack_lds_ext, s.stack_size, A.stack_lds_shd, s.stack_size, ebpc, sbpc,
                    A.shadow_waves, A.ntop_ext, A.ntop_shd, A.nslot_ext, A.nslot_shd);
    }
    if (env.blocks_per_cu) {  // tuning knob: resident blocks per CU (<= occupancy)
        ebpc = std::min(ebpc, std::max(1, *env.blocks_per_cu));
        sbpc = std::min(sbpc, std::max(1, *env.blocks_per_cu));
    }
    s.wf_ext_grid = prop.multiProcessorCount * std::max(1, std::min(ebpc, 8));
    if (env.camera_packets.value_or(1) && !inst) {  // camera-ray packets (flat scenes)
        int cb = 0;
        CK(mfx_cam_occupancy(s.stack_size, &cb, cuts_on));
        if (env.cam_blocks) cb = std::min(cb, std::max(1, *env.cam_blocks));
        s.wf_cam_grid = prop.multiProcessorCount * std::max(1, std::min(cb, 8));
    }
    s.wf_shd_grid = prop.multiProcessorCount * std::max(1, std::min(sbpc, 8));
    {  // deep traversal-stack entries of every lane of the larger grid
        const size_t lanes = (size_t)std::max(s.wf_ext_grid, s.wf_shd_grid) * 256;
        const int deep = s.stack_size - std::min(A.stack_lds_ext, A.stack_lds_shd);
        CK(s.d_spill.alloc(lanes * std::max(1, deep)));
        s.spill_deep = std::max(1, deep);
        s.spill_lanes = (int)lanes;
    }
    CK(s.d_vscratch.alloc(6 * (size_t)(s.host.max_depth + 1) * s.grid * 256));
    return MFX_OK;
}

// Device resources of a context whose host scene, device, seed, flags and partition are set:
// stream, events, the scene images in HBM, accumulators, occupancy-derived launch shapes. On
// failure the caller destroys the context, which releases whatever was allocated.
static int ctx_setup(mfx_ctx* c) {
    c->npix = (int64_t)c->scene.host.width * c->scene.host.height;
    const CreateEnv& env = c->env = read_create_env();
    CK(hipSetDevice(c->device));
    CK(c->stream.create());
    CK(c->h_counters.alloc(WF_NCTR * WF_SHARDS));
    CK(c->ev0.create());
    CK(c->ev1.create());
    MFX_TRY(scene_upload(c->scene, env));
    c->image_gen += 1;
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
    // camera cuts (mfx_camera_cuts.h): on unless MFX_CAMERA_CUTS=0, MFX_CAMERA_CUT_CAP entries a tile (read only
    // where cuts_apply holds: a flat scene whose camera rays run as packets)
    c->cuts.on = env.camera_cuts.value_or(1) != 0;
    c->cuts.cap = std::max(1, std::min(env.camera_cut_cap.value_or(MFX_CUT_CAP_DEFAULT), MFX_CUT_CAP_MAX));
    c->cuts.min_samples = std::max(1, env.camera_cut_min_samples.value_or(MFX_CUT_MIN_SAMPLES));
    c->cuts.cull_min_samples = std::max(1, env.camera_cut_cull_min_samples.value_or(MFX_CUT_CULL_MIN_SAMPLES));
    CK(hipMemset(c->d_accum, 0, 3 * plane));
    CK(hipMemset(c->d_film, 0, 3 * plane));
    CK(hipMemset(c->d_counters, 0, kCounterBytes));
    return scene_shapes(c->scene, c->device, env, wf_textured(c), c->cuts.on);
}

// mfx_set_environment(_sampled) made the sky a light of c's images or took it away (set_sky_light): the light
// and the light table in HBM with their new pdf_n, and the launch shapes of the k_shadow instance that runs now.
// On c's device, which is current; the context's work has finished.
int mfxh::scene_relight(mfx_ctx* c) {
    SceneImages& s = c->scene;
    CK(upload(s.d_light, std::vector<MfxLight>{s.host.light}));
    if (s.multi_light()) CK(upload(s.d_lights, s.host.lights));
    else s.d_lights.reset();
    return scene_shapes(s, c->device, c->env, wf_textured(c), c->cuts.on);
}

int mfxh::scene_reshape(mfx_ctx* c) { return scene_shapes(c->scene, c->device, c->env, wf_textured(c), c->cuts.on); }
#undef CK

// Two-level or flat for an instanced scene. The flat image (one BVH over the expansion) is the faster
// search (C5: 5,088 vs 4,729 Mrays/s, r02bt) and exactly the same results, so it is taken whenever it
// fits the budget: traversal slots of the expansion x 512 B (slot, shade record, nodes and reference
// leaves) <= MFX_FLATTEN_MAX_BYTES (default 2 GiB; C5 is 93,698 slots, 48 MB) and, on a device,
// <= a sixteenth of its free memory. MFX_F_TWO_LEVEL keeps the instances two-level regardless;
// MFX_F_FLATTEN flattens regardless (both: rejected, MFX_E_INVALID, by the callers).
bool mfxh::flatten_instances(const mfx_scene_desc* scene, const mfx_instance* instances, int32_t ninstances,
                             int32_t flags, size_t device_free) {
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

// What a context's host scene is built from, beside the camera: creation's arguments as the caller gave them
// (nothing is copied or read before mfx_build_scene has checked it), or the context's kept copy of them.
struct SceneSource {
    mfx_scene_desc desc;              // (its camera is not read: build_host_scene takes one)
    const mfx_instance* instances;    // null: no instances
    int32_t ninstances;
    const mfx_quad_light* lights;     // mfx_create_lights' list (null: desc.light)
    int32_t nlights;
    bool flatten, gpu_bvh;
};

static SceneSource source_of(const KeptScene& k) {
    SceneSource src{k.desc, k.instanced ? k.instances.data() : nullptr, (int32_t)k.instances.size(),
                    k.lights.empty() ? nullptr : k.lights.data(), (int32_t)k.lights.size(), k.flatten, k.gpu_bvh};
    src.desc.prims = k.prims.data();
    src.desc.albedo = k.albedo.data();
    return src;
}

// The host scene `h` of a context from `src` under `cam`, with the traversal BVH built on the current device
// if src.gpu_bvh. prepared: what mfx_prepare_lights made of src.lights (the lights' one validation, at
// creation; not read without a list). An MFX_* code with who + ": " + what mfx_build_scene refused.
static int build_host_scene(const char* who, const SceneSource& src, const mfx_pinhole& cam,
                            const std::vector<MfxLight>& prepared, MfxHostScene& h) {
    mfx_scene_desc d = src.desc;
    d.camera = cam;
    std::string err;
    if (mfx_build_scene(&d, h, err, src.gpu_bvh, src.instances, src.ninstances, src.flatten, src.lights, &prepared)) return MFX_OK;
    const bool dev = err.rfind("GPU BVH build", 0) == 0;
    return fail(dev ? MFX_E_DEVICE : MFX_E_INVALID, std::string(who) + ": " + err);
}

// what the four creators pass to create_impl
struct CreateArgs {
    const mfx_scene_desc* scene;
    const mfx_instance* instances;      // null: a flat scene
    int32_t ninstances;
    const mfx_options* opt;
    mfx_ctx** out;
    // mfx_create_lights: the list that replaces scene->light (null: scene->light, N = 1)
    const mfx_quad_light* lights = nullptr;
    int32_t nlights = 0;
    // mfx_create_textured: the prepared textures of a scene with a textured primitive, with the caller's
    // arrays they were prepared from (null: no textures)
    const MfxTexHost* tex = nullptr;
    const mfx_texture* textures = nullptr;
    const mfx_prim_uv* prim_uv = nullptr;
};

static int create_impl(const CreateArgs& a) {
    const mfx_scene_desc* scene = a.scene;
    const mfx_options* opt = a.opt;
    if (!scene || !opt || !a.out) return fail(MFX_E_INVALID, "mfx_create: null argument");
    *a.out = nullptr;
    // the megakernel and the counting instances of the trace kernels are built without textures
    if (a.tex && (opt->flags & (MFX_F_MEGAKERNEL | MFX_F_COUNT_STATS)))
        return fail(MFX_E_INVALID, "mfx_create_textured: MFX_F_MEGAKERNEL and MFX_F_COUNT_STATS need an untextured scene");
    std::vector<MfxLight> prepared;  // the lights' one validation: mfx_build_scene takes the result
    if (a.lights) {  // on the host, before any device is asked for
        std::string lerr;
        if (!mfx_prepare_lights(a.lights, a.nlights, prepared, lerr)) return fail(MFX_E_INVALID, "mfx_create_lights: " + lerr);
        // the megakernel and the counting instances of the trace kernels are built for one light
        if (a.nlights >= 2 && (opt->flags & (MFX_F_MEGAKERNEL | MFX_F_COUNT_STATS)))
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
    // the traversal BVH is built on the first device unless the caller asks for the host build
    // (the same tree either way: tests/test_gpu_build.py); the other devices get copies
    const SceneSource src{*scene, a.instances, a.ninstances, a.lights, a.nlights,
                          flatten_instances(scene, a.instances, a.ninstances, opt->flags, dev_free),
                          (opt->flags & MFX_F_HOST_BVH) == 0};
    MFX_TRY(build_host_scene("mfx_create", src, scene->camera, prepared, c->scene.host));
    {  // the description stays with the context: mfx_set_camera may have to build the images again
        KeptScene& k = c->kept;
        k.prims.assign(scene->prims, scene->prims + scene->nprims);
        k.albedo.assign(scene->albedo, scene->albedo + 3 * (size_t)scene->nmat);
        if (src.instances) k.instances.assign(src.instances, src.instances + src.ninstances);
        if (src.lights) k.lights.assign(src.lights, src.lights + src.nlights);
        if (a.tex) k.prim_uv.assign(a.prim_uv, a.prim_uv + scene->nprims);
        k.desc = *scene;
        k.desc.prims = nullptr;
        k.desc.albedo = nullptr;
        k.instanced = src.instances != nullptr;
        k.flatten = src.flatten;
        k.gpu_bvh = src.gpu_bvh;
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
        if (!a.tex) return;
        // textured: every device gets the tables (ctx_setup uploads them from the caller's arrays)
        d->tex.host = *a.tex;
        d->tex.src = a.textures;
    };
    init(c.get(), 0);
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
            p->scene.host = c->scene.host;
            init(p, g);
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
    *a.out = c.release();
    return MFX_OK;
}

// ---- mfx_set_camera, mfx_set_lens ------------------------------------------------------------------
// Prepare the kept scene again for `cam` by creation's own steps: the host scene once, then for every device
// of the context a fresh SceneImages (scene_upload, scene_shapes). They are moved in only when every device
// has its own, so a failure leaves every context as it was: what was built so far goes with `fresh`.
// at (null: the camera's own position): the point the widening is sized for, a corner of the lens box; the images
// are then those of a camera at `at`, and carry `cam` as their camera.
static int rebuild_for_camera(mfx_ctx* c, const char* who, const mfx_pinhole* cam, const double* at) {
    HIPCHECK(hipSetDevice(c->device));
    MfxHostScene h;
    if (at) {
        MfxCamera m;
        mfx_derive_camera(*cam, m);
        mfx_pinhole sized = *cam;
        sized.derived = 1;
        std::copy(at, at + 3, sized.position);
        std::copy(m.topleft, m.topleft + 3, sized.topleft);
        std::copy(m.right, m.right + 3, sized.right);
        std::copy(m.down, m.down + 3, sized.down);
        MFX_TRY(build_host_scene(who, source_of(c->kept), sized, c->scene.host.lights, h));
        h.camera = m;
    } else {
        MFX_TRY(build_host_scene(who, source_of(c->kept), *cam, c->scene.host.lights, h));
    }
    const std::vector<mfx_ctx*> ds = devs_of(c);
    std::vector<SceneImages> fresh(ds.size());  // (the shapes start from a fresh context's defaults)
    int rc = MFX_OK;
    for (size_t g = 0; g < ds.size() && rc == MFX_OK; ++g) {
        const mfx_ctx* dv = ds[g];
        fresh[g].host = h;
        set_sky_light(fresh[g], dv->scene.sky_light);  // (a sampled sky stays a light of the new images)
        fresh[g].normals = dv->scene.normals;          // (and the normals stay: their tables are the device's, not the images')
        rc = hipSetDevice(dv->device) == hipSuccess ? MFX_OK : fail(MFX_E_DEVICE, std::string(who) + ": hipSetDevice failed");
        if (rc == MFX_OK) rc = scene_upload(fresh[g], dv->env);
        if (rc == MFX_OK) rc = scene_shapes(fresh[g], dv->device, dv->env, wf_textured(dv), dv->cuts.on);
    }
    if (rc != MFX_OK) {
        const std::string msg = mfx_last_error();
        (void)hipGetLastError();
        (void)hipSetDevice(c->device);
        return fail(rc, msg);
    }
    for (size_t g = 0; g < ds.size(); ++g) {  // the old images go with `fresh`
        std::swap(ds[g]->scene, fresh[g]);
        ds[g]->image_gen += 1;  // (the camera cuts are the old image's)
    }
    HIPCHECK(hipSetDevice(c->device));
    c->kept.desc.camera = *cam;
    return MFX_OK;
}

// The widening camera m needs over `host`: its position's, or under a lens the largest over the corners of the
// lens box, P0 +- (|U| + |V|) per axis (every lens origin lies inside). at: the point that asks for it.
static void camera_lens_eps(const MfxHostScene& host, const MfxCamera& m, const MfxLensRec* L, float* eps, float* eps_t, double at[3]) {
    std::copy(m.position, m.position + 3, at);
    mfx_camera_eps(host, m.position, eps, eps_t);
    if (!L) return;
    for (int k = 0; k < 8; ++k) {
        double p[3];
        for (int a = 0; a < 3; ++a) {
            const double r = std::fabs(L->U[a]) + std::fabs(L->V[a]);
            p[a] = (k >> a) & 1 ? m.position[a] + r : m.position[a] - r;
        }
        float e = 0.f, et = 0.f;
        mfx_camera_eps(host, p, &e, &et);
        if (e > *eps || (e == *eps && et > *eps_t)) {
            *eps = e, *eps_t = et;
            std::copy(p, p + 3, at);
        }
    }
}

static const char* lens_refusal(int code) {
    switch (code) {
    case MFX_LENS_BAD_APERTURE: return "aperture must be finite and >= 0";
    case MFX_LENS_BAD_FOCUS: return "focus must be finite and > 0";
    case MFX_LENS_BAD_RIGHT: return "the camera's right has no finite non-zero length (lr)";
    case MFX_LENS_BAD_DOWN: return "the camera's down has no finite non-zero length (ld)";
    case MFX_LENS_BAD_FORWARD: return "the camera's right and down span no plane (ln)";
    case MFX_LENS_BAD_DPLANE: return "dplane must be finite and > 0 (the film plane lies ahead of the camera)";
    default: return "s = focus / dplane is not finite";
    }
}

int mfxh::lens_record(const char* who, const mfx_pinhole* cam, const mfx_lens* lens, MfxLensRec& rec) {
    MfxCamera m;
    mfx_derive_camera(*cam, m);
    const int bad = mfx_lens_record(m.position, lens->aperture, lens->focus, rec, nullptr);
    return bad ? fail(MFX_E_INVALID, std::string(who) + ": " + lens_refusal(bad)) : MFX_OK;
}

int mfxh::apply_camera_lens(mfx_ctx* c, const char* who, const mfx_pinhole* cam, const mfx_lens* lens) {
    MfxCamera m;
    mfx_derive_camera(*cam, m);
    Lens nl = c->lens;  // the lens state after the call
    nl.on = lens != nullptr;
    nl.aperture = lens ? lens->aperture : 0.0;
    nl.focus = lens ? lens->focus : 0.0;
    nl.rec = MfxLensRec{};
    if (lens) MFX_TRY(lens_record(who, cam, lens, nl.rec));  // on the host, before a device is touched
    const bool by_lens = std::strcmp(who, "mfx_set_lens") == 0;
    // held render-ahead frames are the old camera's: the film comes back to d_film under the old camera, and
    // the frames' epoch ends; then everything the context has enqueued, a background batch included, finishes
    MFX_TRY(ahead_break(c));
    MFX_TRY(mfx_sync(c));
    const MfxHostScene& host = c->scene.host;
    float eps = 0.f, eps_t = 0.f;
    double at[3];
    camera_lens_eps(host, m, lens ? &nl.rec : nullptr, &eps, &eps_t, at);
    // images built for a lens box go with the lens: the pinhole context again, digest included
    const bool narrow = !lens && c->lens.widened;
    if (!narrow && eps <= host.eps && eps_t <= host.eps_templates) {
        // in place: the boxes stay conservative for every ray this camera can start
        for (mfx_ctx* d : devs_of(c)) {
            HIPCHECK(hipSetDevice(d->device));
            HIPCHECK(hipMemcpy(d->scene.d_cam, &m, sizeof(m), hipMemcpyHostToDevice));
            d->scene.host.camera = m;
        }
        HIPCHECK(hipSetDevice(c->device));
        c->kept.desc.camera = *cam;
    } else {
        MFX_TRY(rebuild_for_camera(c, who, cam, lens ? at : nullptr));
        (by_lens ? nl.rebuilds : c->cam_rebuilds) += 1;
        nl.widened = lens != nullptr;
    }
    if (lens)  // the record behind the camera, where the LENS instances read it (new images have room for it too)
        for (mfx_ctx* d : devs_of(c)) {
            HIPCHECK(hipSetDevice(d->device));
            HIPCHECK(hipMemcpy(d->scene.d_cam.get() + 1, &nl.rec, sizeof(nl.rec), hipMemcpyHostToDevice));
        }
    HIPCHECK(hipSetDevice(c->device));
    nl.eps = lens ? eps : 0.f;
    if (!lens) nl.rebuilds = 0;  // (mfx_lens_info: all 0 without a lens)
    for (mfx_ctx* d : devs_of(c)) d->lens = nl;
    c->cam_epoch += 1;           // the feature buffers are the old camera's
    c->adp.accum_valid = false;  // a resume must not mix cameras
    c->ahead.dfilm_buf = -1;
    return MFX_OK;
}

extern "C" {
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
    if (std::memcmp(&m, &c->scene.host.camera, sizeof(m)) == 0) return MFX_OK;  // the current camera: nothing to do
    // under a lens the call keeps aperture and focus, derives the record again and sizes the widening for the lens box
    const mfx_lens cur{c->lens.aperture, c->lens.focus};
    return apply_camera_lens(c, "mfx_set_camera", cam, c->lens.on ? &cur : nullptr);
}

int mfx_set_lens(mfx_ctx* c, const mfx_lens* lens) {
    if (!c) return fail(MFX_E_INVALID, "mfx_set_lens: null context");
    if (lens && lens->aperture == 0.0) lens = nullptr;  // an aperture of exactly 0 is the pinhole
    if (lens && (c->flags & (MFX_F_MEGAKERNEL | MFX_F_COUNT_STATS)))
        return fail(MFX_E_STATE, "mfx_set_lens: a context created with MFX_F_MEGAKERNEL or MFX_F_COUNT_STATS has no lens instances");
    if (!lens && !c->lens.on) return MFX_OK;  // no lens, none wanted
    if (lens && c->lens.on && std::memcmp(&lens->aperture, &c->lens.aperture, sizeof(double)) == 0 &&
        std::memcmp(&lens->focus, &c->lens.focus, sizeof(double)) == 0)
        return MFX_OK;  // the current lens
    const mfx_pinhole cam = c->kept.desc.camera;
    return apply_camera_lens(c, "mfx_set_lens", &cam, lens);
}

int mfx_create(const mfx_scene_desc* scene, const mfx_options* opt, mfx_ctx** out) {
    return create_impl({scene, nullptr, 0, opt, out});
}

int mfx_create_instanced(const mfx_scene_desc* scene, const mfx_instance* instances, int32_t ninstances,
                         const mfx_options* opt, mfx_ctx** out) {
    if (!instances || ninstances < 1) return fail(MFX_E_INVALID, "mfx_create_instanced: no instances");
    return create_impl({scene, instances, ninstances, opt, out});
}

int mfx_create_lights(const mfx_scene_desc* scene, const mfx_quad_light* lights, int32_t nlights,
                      const mfx_instance* instances, int32_t ninstances, const mfx_options* opt, mfx_ctx** out) {
    if (!lights || nlights < 1 || nlights > MFX_MAX_LIGHTS)
        return fail(MFX_E_INVALID, "mfx_create_lights: nlights must be 1 .. MFX_MAX_LIGHTS with a light array");
    const bool flat = !instances && ninstances == 0;
    if (!flat && (!instances || ninstances < 1)) return fail(MFX_E_INVALID, "mfx_create_lights: no instances");
    return create_impl({scene, instances, flat ? 0 : ninstances, opt, out, lights, nlights});
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
    return create_impl({scene, instances, flat ? 0 : ninstances, opt, out, lights, nlights, &tex, textures, prim_uv});
}
}  // extern "C"
