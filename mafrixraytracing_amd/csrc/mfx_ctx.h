// mfx_ctx.h — the context behind the extern "C" boundary, shared by its translation units
// (mfx_api.cpp, mfx_create.cpp, mfx_trace.cpp, mfx_readback.cpp, mfx_ahead.cpp, mfx_adaptive.cpp,
// mfx_denoise_api.cpp, mfx_query.cpp, mfx_environment.cpp, mfx_normals.cpp). Internal: never included from include/.
// Ownership: a GPU resource is a member (DevBuf, HostBuf, Event, Stream) of the struct of the
// feature that uses it, and nothing is freed by hand. A feature that allocates at its first call is
// a nested struct of mfx_ctx whose ready() says whether it has.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <optional>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "../../include/mafrix_rt.h"
#include "mfx_device.h"
#include "mfx_denoise.h"
#include "mfx_scene.h"
#include "mfx_wavefront.h"

// What crosses the boundary's translation units is hidden: the library's dynamic symbol table
// holds the header's mfx_* functions only.
namespace mfxh __attribute__((visibility("hidden"))) {

// sets the calling thread's mfx_last_error message and returns `code`
int fail(int code, const std::string& msg);

// a HIP call: a failure _e leaves the calling function with `code` (which may read _e) and `what` + HIP's message
#define HIP_TRY(expr, code, what)                                                                 \
    do {                                                                                          \
        const hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) return mfxh::fail(code, std::string(what) + hipGetErrorString(_e)); \
    } while (0)
#define HIPCHECK(expr) HIP_TRY(expr, MFX_E_DEVICE, #expr ": ")
// a call that returns an MFX_* code: a failure leaves the calling function with it
#define MFX_TRY(expr) do { const int _rc = (expr); if (_rc) return _rc; } while (0)

// ---- owners: move-only, empty after a failed alloc / create, released by their destructors ----
template <typename T, bool kHost>
class Buf {  // device memory (hipMalloc / hipFree) or, kHost, page-locked host memory (hipHostMalloc / hipHostFree)
    T* p_ = nullptr;
public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    Buf& operator=(Buf&& o) noexcept { return std::swap(p_, o.p_), *this; }
    ~Buf() { reset(); }
    hipError_t alloc(size_t count) {  // `count` elements
        reset();
        const size_t bytes = count * sizeof(T);
        const hipError_t e = kHost ? hipHostMalloc((void**)&p_, bytes, hipHostMallocDefault) : hipMalloc((void**)&p_, bytes);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    void reset() { if (p_) (void)(kHost ? hipHostFree(p_) : hipFree(p_)), p_ = nullptr; }
    T* get() const { return p_; }
    operator T*() const { return p_; }
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using HostBuf = Buf<T, true>;

class Event {  // hipEventCreate[WithFlags] / hipEventDestroy
    hipEvent_t e_ = nullptr;
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event& operator=(Event&& o) noexcept { return std::swap(e_, o.e_), *this; }
    ~Event() { reset(); }
    hipError_t create(unsigned flags = 0) {  // 0: a timing event (hipEventCreate)
        reset();
        return flags ? hipEventCreateWithFlags(&e_, flags) : hipEventCreate(&e_);
    }
    void reset() { if (e_) (void)hipEventDestroy(std::exchange(e_, nullptr)); }
    hipEvent_t get() const { return e_; }
    operator hipEvent_t() const { return e_; }
};

class Stream {  // hipStreamCreateWithFlags(hipStreamNonBlocking) / hipStreamDestroy
    hipStream_t s_ = nullptr;
public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    Stream& operator=(Stream&& o) noexcept { return std::swap(s_, o.s_), *this; }
    ~Stream() { reset(); }
    hipError_t create() {
        reset();
        const hipError_t e = hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
        if (e != hipSuccess) s_ = nullptr;
        return e;
    }
    void reset() { if (s_) (void)hipStreamDestroy(std::exchange(s_, nullptr)); }
    hipStream_t get() const { return s_; }
    operator hipStream_t() const { return s_; }
};

// bytes of one set of ray counters [WF_SHARDS][WF_NCTR]
constexpr size_t kCounterBytes = WF_NCTR * WF_SHARDS * sizeof(unsigned long long);

// One render-ahead buffer: the RGBA8 frames that the one-sample render calls of global samples
// [base, base + n) return, the film before the first of them and the film after the last.
struct AheadBuf {
    DevBuf<uint8_t> frames;             // [cap][npix][4] (y-major RGBA8)
    DevBuf<double> film_in;             // [3][npix] the film before sample base (as the frames assume)
    DevBuf<double> film_out;            // [3][npix] the film after sample base + n - 1
    DevBuf<unsigned long long> counters;  // the batch's ray counters [WF_SHARDS][WF_NCTR]
    Event t0, t1;                       // around the batch's trace
    Event ready;                        // frames computed
    int64_t base = 0, n = 0;            // samples held (n == 0: empty)
    int64_t expect = 0;                 // the index whose frame a call may take next
    uint64_t epoch = 0;                 // film epoch the frames were computed in
    double count0 = 0.0;                // Film frameCount before sample base
    bool reported = false;              // a call has reported the batch's rays and time
};

// ---- wf_trace's modes (TraceMode: one of them, or none) ----
// k_resolve's frames mode (render-ahead; WfParams film / frames / count0): the samples are
// one-sample render calls added to `film` in order, the ray counters go to `counters` and the trace is
// bracketed by the events e0 / e1 instead of the context's (no per-iteration events), so a batch
// traced in the background leaves the last call's timing records alone.
struct FrameMode {
    double* film;     // the film state: read before the first sample, written after the last
    uint8_t* frames;  // null: the film only
    double count0;    // frameCount before the first sample
    unsigned long long* counters;
    hipEvent_t e0, e1;
};

// mfx_sample's banded resolve (one device): the last generation's k_resolve runs in nbands column bands
// of tiles, and after each band `after(k, tx0, ntx)` enqueues that band's mean and readback, so the
// frame's copy to the host overlaps the rest of the resolve. used: wf_trace ran it (not the megakernel).
struct ResolveSplit {
    int nbands = 0;
    std::function<int(int, int, int)> after;
    bool used = false;
};

// A listed wavefront trace (mfx_sample_adaptive's passes; WfParams tiles / ntiles / mom): the trace
// covers the film tiles `tiles` instead of the device's band, and k_resolve also adds the moments.
struct TileList {
    const int32_t* tiles;  // device: film tile indices, ascending
    int32_t ntiles;
    double* mom;           // device: [2][npix] the luminance moments k_resolve adds to
    int64_t gen_paths;     // paths per generation at most (a multiple of 4096)
    // mfx_sample_adaptive_resume's passes (WfParams tile_n / list_max; null: one sample range for every tile):
    const int32_t* tile_n = nullptr;  // device: [film tiles] the samples every tile has had, its base in this trace
    int32_t list_max = 0;             // a tile takes min(ns, list_max - tile_n[T]) samples
};

using TraceMode = std::variant<std::monostate, FrameMode, ResolveSplit*, TileList>;

constexpr int kStageChunks = 8;  // host_readback's pipelined pieces (at most)

// RCCL is opened when the first multi-device context is created, not linked: a process that
// already holds an RCCL (PyTorch loads its own librccl.so, soname librccl.so.1) gets that same
// instance back from dlopen by soname, so one process never maps two RCCLs; a process that
// never creates a multi-device context never loads it at all.
struct Rccl {
    decltype(&ncclCommInitAll) commInitAll = nullptr;
    decltype(&ncclCommDestroy) commDestroy = nullptr;
    decltype(&ncclReduce) reduce = nullptr;
    decltype(&ncclGroupStart) groupStart = nullptr;
    decltype(&ncclGroupEnd) groupEnd = nullptr;
    decltype(&ncclGetErrorString) errorString = nullptr;
};
const Rccl* rccl();  // null: it could not be loaded

// The wavefront pipeline's path-slot pool and ray queues: a frame's paths run in generations of at
// most `max` paths (mfx_wavefront.h), every iteration one bounce of every live path
struct WfPool {
    WfParams params{};        // what holds from trace to trace: the pool's arrays (wf_ensure_pool)
    DevBuf<char> mem;
    int32_t slots = 0;
    size_t bytes = 0;         // bytes of mem
    bool queues = false;      // the pool holds the ray queues' arrays too (allocated only for a trace that uses them)
    // MFX_RAY_QUEUE: the ray queues, and the first iteration (0-based) whose k_shadow moves the
    // continuing paths to one (-1: every iteration in place; MFX_RAY_QUEUE=0 / MFX_QUEUE_FROM=d)
    WfQueue wq[2]{};
    int queue_from = MFX_RAY_QUEUE ? -2 : -1;  // -2: automatic (queue_auto)
    int queue_auto = 1;  // from the last trace's live paths per iteration (note_live); 1 before any
    // The first wavefront trace's counters are read once for queue_auto, after every device of
    // the call has been enqueued (settle_queue_auto). Render-ahead batches settle it from each
    // batch's counters instead (note_live in ahead_render).
    bool auto_read = false;
    bool auto_pending = false;  // a trace whose counters settle queue_auto has been enqueued
    int32_t qchunk = 128;  // entries per chunk fetch on a ray queue (MFX_QCHUNK; r04j: 128 against 256, C2 8 spp +2 %)
    // Path slots of the wavefront pool, at most. A pool as large as a frame's path count (C2: 133 M
    // slots, 15 GB) runs the frame as one generation: no kernel ends with a partly filled pool
    // (+11 % on C2 over 32 M slots). Capped at 2^28 slots (31 GB of the 288 GB) and at a quarter
    // of the free HBM.
    int64_t max = 1 << 28;
    int64_t cap = 0;  // the generation cap a memory shortage left (0: none; wf_trace)
    bool fail_once = false;  // MFX_POOL_FAIL_ONCE=1 (tests): the first pool allocation is refused by hipMalloc
    DevBuf<unsigned long long> ctl;  // [WF_CTL_ALLOC] queue 0 counts, chunk heads, queue 1 counts
    int queue_start() const { return queue_from == -2 ? queue_auto : queue_from; }
};

// Render-ahead (mfx_ahead.cpp); allocated at the first render call that uses it
struct Ahead {
    int k = 0;                       // mfx_options.render_ahead (0 after a batch that did not fit)
    AheadBuf ab[2];
    int nbuf = 0;                    // buffers allocated (0: none yet; 1: no background batch)
    int cap = 0;                     // samples per buffer
    int cur = -1;                    // the buffer the last render call was served from (-1: none)
    int64_t last_k = -1;             // and its index in that buffer
    uint64_t film_epoch = 1;         // bumped when the film leaves the held frames' sequence
    bool film_in_dfilm = true;       // d_film holds the film (else: ab[cur].film_in + its samples up to last_k)
    // d_film = ab[dfilm_buf].film_in + that batch's first dfilm_n samples (dfilm_buf >= 0): a later
    // ahead_materialize traces only the samples after those (a caller alternating
    // Render and film_mean re-traced 1, 2, ..., K - 1 samples per batch)
    int dfilm_buf = -1;
    int64_t dfilm_n = 0;
    DevBuf<unsigned long long> counters_aux;           // ray counters of a film-only re-trace (not reported)
    Event aux_ev0, aux_ev1;
    bool ready() const { return nbuf != 0; }
    void release() {  // the buffers go; the film bookkeeping stays
        for (AheadBuf& B : ab) B = AheadBuf{};
        counters_aux.reset(), aux_ev0.reset(), aux_ev1.reset();
        nbuf = cap = 0;
        cur = -1;
    }
};

// Adaptive sampling (mfx_sample_adaptive, mfx_sample_adaptive_resume); allocated at mfx_sample_adaptive's first call
struct Adaptive {
    DevBuf<double> mom;           // [2][npix] per-pixel luminance moments S1, S2
    DevBuf<int32_t> tiles[2];     // [tiles] the active tile list of a pass and the next one's
    DevBuf<int32_t> tile_flags;   // [tiles] the check's verdicts (1: the tile goes on)
    DevBuf<int32_t> tile_spp;     // [tiles] sample count of every tile
    DevBuf<int32_t> tile_count;   // [0] tiles that go on, [1] the most samples one of them gets in the next pass (resume)
    Event ev0, ev1;               // around a pass (trace, check) and the mean
    bool check = false;           // MFX_ADAPTIVE_CHECK=1: the host validates every pass's tile list
    bool accum_valid = false;     // the accumulator, mom and tile_spp hold the last mfx_sample_adaptive's result, as
                                  // mfx_sample_adaptive_resume continued it: set when either succeeds, cleared by
                                  // whatever else writes or swaps the accumulator (a trace's parameters,
                                  // mfx_accum_clear, mfx_accum_attach); mfx_denoise_var and the resume read it
    // of that result (meaningful while accum_valid):
    int64_t B = 0;                // next_sample when its mfx_sample_adaptive began: tile T's samples are B .. B + n_T - 1
    int32_t R = 0;                // the budget reserved so far (that call's max_spp, raised by resumes): next_sample == B + R
    int64_t gen_paths = 0;        // paths per generation of its passes (the first pass's: the pool is that call's)
    bool ready() const { return ev1 != nullptr; }  // the last one adaptive_alloc creates
};

// Feature buffers and denoising (mfx_aov, mfx_denoise, mfx_denoise_var); allocated at their first calls
struct Denoise {
    DevBuf<double> feat;          // [MFX_AOV_PLANES][npix] the feature planes (mfx_aov)
    DevBuf<double> feat_out;      // [npix][MFX_AOV_PLANES] staging of mfx_aov's host output
    DevBuf<double> buf[2];        // [3][npix] each: the filter's ping-pong colour buffers
    DevBuf<double> var[2];        // [npix] each: mfx_denoise_var's ping-pong variance planes
    Event ev0, ev1;               // around either call's kernels
    uint64_t feat_epoch = 0;      // the camera epoch (mfx_ctx::cam_epoch) the feature planes were traced in
    bool ready() const { return feat != nullptr; }  // mfx_aov has run
};

// Temporal reuse (mfx_temporal); allocated at its first call. A history buffer holds the merged result
// and the features of the view it belongs to, plane-major, x-major pixels (MFX_TP_* in mfx_denoise.h):
// the kernel gathers from hist[cur] and writes hist[cur ^ 1], then cur flips (no copy).
struct Temporal {
    DevBuf<double> hist[2];             // [MFX_TP_PLANES][npix] each
    DevBuf<double> count_in;            // [npix] staging of MFX_DN_SRC_HOST's counts
    DevBuf<unsigned long long> accepted;  // [1] pixels that took history
    int cur = -1;                       // the buffer that holds the history (-1: none yet)
    MfxCamera cam{};                    // the camera of the history's view
    uint64_t epoch = 0;                 // and its camera epoch
    bool ready() const { return accepted != nullptr; }  // the last one mfx_temporal allocates
};

// The scene description a context keeps from creation on (host memory only: 104 B per primitive, 24 B
// per material, 48 B per instance entry): what mfx_set_camera builds the images from again when the new
// camera needs wider boxes. Primary context only.
struct KeptScene {
    std::vector<mfx_prim> prims;
    std::vector<double> albedo;
    std::vector<mfx_instance> instances;
    std::vector<mfx_quad_light> lights;  // mfx_create_lights' list (empty: desc.light)
    std::vector<mfx_prim_uv> prim_uv;    // mfx_create_textured's maps of a textured context (56 B per primitive; else empty)
    mfx_scene_desc desc{};   // prims / albedo point nowhere: set from the vectors at use
    bool instanced = false;  // created by mfx_create_instanced
    bool flatten = false;    // the choice creation made for an instanced scene
    bool gpu_bvh = false;
};

// Readback to the caller's host memory (mfx_readback.cpp); each allocated by the first call that needs it
struct Readback {
    HostBuf<uint8_t> stage;          // page-locked staging of large readbacks (host_readback)
    size_t stage_bytes = 0;
    Event stage_ev[kStageChunks];    // host_readback: piece i is in `stage`
    Event band_ev[kStageChunks];     // mfx_sample's banded readback: band i's mean is computed
    Stream copy_stream;  // frame copies to the host (overlap the background trace); created at the first
                         // render-ahead or mfx_sample call, so a batch-only context holds one stream (one
                         // of the process's GPU_MAX_HW_QUEUES hardware queues)
};

// The MFX_* variables that shape a context's launches, as the environment held them when the context was
// created (read_create_env, mfx_create.cpp: the one place that reads them; unset: no value). What they mean,
// their clamps and their defaults are where they are used: scene_upload, scene_shapes, ctx_setup and the
// two wf_* rules below. A rebuild under mfx_set_camera uses these values, not the environment's.
struct CreateEnv {
    using Int = std::optional<int>;
    bool node_f32 = false, diag_iter = false, no_gray_light = false, no_lit_in_hit = false;  // set at all
    Int mega_waves, shadow_target_blocks, stack_lds, ntop, slot_lds, shadow_waves, blocks_per_cu, camera_packets, cam_blocks;
    Int camera_cuts, camera_cut_cap, camera_cut_min_samples, camera_cut_cull_min_samples;
    Int pool_fail_once, adaptive_check, iter_events, queue_from, qchunk, ray_queue, mega_chunk, shd_half, chunk;
    std::optional<int64_t> pool;
};

// The camera cuts of one device (mfx_camera_cuts.h): the table k_camera's CUTS instances start their packets
// from, built lazily by cuts_for_trace (mfx_trace.cpp) on the context's stream for the device's current
// camera and node image, and kept until either changes.
struct CamCuts {
    bool on = true;                  // MFX_CAMERA_CUTS=0: off
    int cap = MFX_CUT_CAP_DEFAULT;   // MFX_CAMERA_CUT_CAP
    int min_samples = MFX_CUT_MIN_SAMPLES;  // a trace of fewer samples does not pay a build (MFX_CAMERA_CUT_MIN_SAMPLES)
    // the slot cull triples the build's time, so a table is built with it once its camera has served this many
    // samples, the coming trace's included (MFX_CAMERA_CUT_CULL_MIN_SAMPLES): a camera that stays pays it once
    int cull_min_samples = MFX_CUT_CULL_MIN_SAMPLES;
    int64_t cam_samples = 0;         // samples traced with the table's camera and image (saturating)
    bool culled = false;             // the table was built with the slot cull
    DevBuf<MfxCutEntry> table;       // [tiles_y * tiles_x][cap]
    DevBuf<MfxCutStats> stats;
    size_t entries = 0;              // allocated
    // what the table was built for: mfx_set_camera changes the camera exactly when cam_epoch moves (on
    // every device of a list), and every installed scene_upload takes a new image_gen
    bool valid = false;
    MfxCamera cam{};
    uint64_t image_gen = 0;
    int64_t builds = 0;
    Event e0, e1;                    // around the last build
    MfxCutStats last{};              // the last build's statistics, read back by mfx_launch_info
    bool last_read = false;
    float last_ms = 0.f;
};

// Albedo textures (mfx_create_textured), per device: the tables the textured kernel instances read. They
// depend on the primitives alone, not on the camera, so they are no part of SceneImages: an mfx_set_camera
// rebuild leaves them where they are.
struct Textures {
    MfxTexHost host;                 // descriptors, UV table, texture per world primitive
    DevBuf<double> d_uvrec;
    DevBuf<int32_t> d_ptex;
    DevBuf<MfxTexDesc> d_desc;
    DevBuf<uint32_t> d_texels;       // every texture's texels, one after the other
    const mfx_texture* src = nullptr;  // the caller's textures: set while creation uploads them, null afterwards
    MfxTexTables tables() const { return host.on ? MfxTexTables{d_uvrec, d_ptex, d_desc, d_texels} : MfxTexTables{}; }
};

// The sky (mfx_set_environment; mfx_environment.cpp), per device: the map's texels in HBM. Like the textures it
// is no part of SceneImages: an mfx_set_camera rebuild leaves it where it is.
struct Environment {
    DevBuf<float> d_rgb;             // [size * size][3] linear RGB radiance
    int32_t size = 0;                // 0: no environment
    // the sky as a light (mfx_set_environment_sampled): the sampling table, one entry per texel (null: unsampled)
    DevBuf<MfxSkyEntry> d_tab;
    bool sampled = false;
    bool on() const { return size > 0; }
};

// The thin lens (mfx_set_lens; mfx_lens.cpp), per device: the record the LENS instances read. Like the sky it is no
// part of SceneImages; its only tie to them is the widening (the images' eps covers the lens box's corners).
struct Lens {
    bool on = false;
    double aperture = 0.0, focus = 0.0;
    MfxLensRec rec{};
    float eps = 0.f;         // the widening the lens camera needs (the largest over the lens box's corners)
    int64_t rebuilds = 0;    // image rebuilds mfx_set_lens caused (primary)
    // the images were built for a lens box (by mfx_set_lens, or by mfx_set_camera under a lens): removing the lens
    // builds them again for the camera alone, so the context is the pinhole one again, digest included (primary)
    bool widened = false;
};

// Smooth shading (mfx_set_normals; mfx_normals.cpp), per device: the tables the SN instances read. Like the textures
// they depend on the primitives alone and are no part of SceneImages: an mfx_set_camera rebuild leaves them where
// they are. Whether they are on is SceneImages::normals (the launch shapes depend on it).
struct Normals {
    DevBuf<double> d_rec;      // [world primitives][12] the normal records
    DevBuf<int32_t> d_flag;    // [world primitives] 1: smooth
    int64_t nworld = 0, nsmooth = 0;
    MfxSnTables tables() const { return d_rec ? MfxSnTables{d_rec, d_flag} : MfxSnTables{}; }
};

// What scene_shapes chooses for k_extend (ext) and k_shadow (shd): wf_trace copies it into a trace's WfParams
struct LaunchShapes {
    int stack_lds_ext = 0, stack_lds_shd = 0;  // traversal stack entries per lane in LDS; the rest in d_spill
    int ntop_ext = 0, ntop_shd = 0;            // top BVH nodes in LDS
    int nslot_ext = 0, nslot_shd = 0;          // slots in LDS (all of a small scene's, or 0)
    int shadow_waves = 0;                      // k_shadow instance: 3 or 4 waves per SIMD
};

// Everything a device holds that the host scene determines: the scene's images in HBM (scene_upload) and the
// launch shapes and buffers sized by it (scene_shapes; both mfx_create.cpp). Creation fills the context's own;
// an mfx_set_camera rebuild fills fresh ones for every device and moves them in once all have succeeded, so
// whatever the two functions write belongs here and nowhere else.
struct SceneImages {
    MfxHostScene host;
    DevBuf<MfxNode> d_nodes;
    DevBuf<MfxSlot> d_slots;
    DevBuf<MfxNodeH> d_nodes_h;  // MFX_NODE_F16 builds: the FP16 copy of d_nodes (per-lane kernels)
    DevBuf<int32_t> d_slot_ref;
    DevBuf<uint8_t> d_ref_blob;
    DevBuf<MfxShade> d_shade;
    DevBuf<MfxInstance> d_inst;  // two-level scenes only
    DevBuf<double> d_albedo;     // [nmat][3]
    DevBuf<MfxLight> d_light;    // the light (k_shadow reads it into LDS)
    DevBuf<MfxLight> d_lights;   // several lights: the table k_shadow<ML> gathers from (null with one light)
    DevBuf<MfxCamera> d_cam;     // the camera (k_camera reads it into LDS)
    DevBuf<const void*> d_refs;  // {d_slot_ref, d_ref_blob} (k_shadow reads them into LDS)
    int stack_size = 1;          // the traversal stack bound
    // launch shapes (scene_shapes)
    LaunchShapes shapes;
    int grid = 0;
    int wf_ext_grid = 0, wf_shd_grid = 0;
    int wf_cam_grid = 0;  // > 0: camera rays as packets (k_camera; MFX_CAMERA_PACKETS=0 turns it off)
    int mega_waves = 1;   // megakernel instance: 4 (128-VGPR budget) or 1 (mfx_kernels.hip)
    DevBuf<int32_t> d_spill;     // deep traversal-stack entries [spill_deep][spill_lanes]
    int spill_deep = 0, spill_lanes = 0;
    DevBuf<double> d_vscratch;   // megakernel: per-lane vertex records [max_depth + 1][6][grid * 256]
    // the sky is a light of this context (mfx_set_environment_sampled): the pick is over N + 1, so the lights'
    // pdf_n in `host` is (1 / area) / (N + 1) and one area light runs the several-light instances too. Set and
    // cleared by set_sky_light, which mfx_set_camera's rebuild applies to the images it builds.
    bool sky_light = false;
    // the context has corner normals (mfx_set_normals): the SN twins of k_shadow, which are the 4-wave build's only
    // and keep 16 B of LDS more. Set and cleared by mfx_set_normals, which asks for the launch shapes again;
    // mfx_set_camera's rebuild copies it to the images it builds.
    bool normals = false;
    // several lights (mfx_create_lights, N >= 2; a sampled sky beside N >= 1): the ML instances of k_shadow and
    // k_resolve, the wavefront pipeline for every trace, a light-index plane in the pool
    bool multi_light() const { return host.lights.size() >= 2 || sky_light; }
};

// Makes the sky a light of the images `s` or takes it away again, on the host: pdf_n = (1 / area_n) / (N + on),
// make_light's two divisions (mfx_scene.cpp). The caller uploads the lights and asks for the launch shapes again.
inline void set_sky_light(SceneImages& s, bool on) {
    s.sky_light = on;
    const double np = (double)(s.host.lights.size() + (on ? 1 : 0));
    for (MfxLight& L : s.host.lights) {
        const double inv = 1. / L.area;
        L.pdf = inv / np;
    }
    if (!s.host.lights.empty()) s.host.light.pdf = s.host.lights[0].pdf;
}

// Multi-device (primary context only)
struct Multi {
    bool device_list = false;            // created with a device list (mfx_options.ndevices > 0)
    std::vector<std::unique_ptr<mfx_ctx>> peers;  // devices[1..G) of the device list, same host scene
    std::vector<ncclComm_t> comms;       // [G] one RCCL communicator per device, rank g = device g
    DevBuf<double> merge;                // [3][npix] the devices' films merged (mfx_film_mean), allocated on first use
    bool accum_merged = true;            // the primary's accumulator holds every device's rows (mfx_accum_reduce
                                         // since the last trace or clear)
    DevBuf<double> reduce_stage;         // repeated-device list: a peer's accumulator copied here
    std::vector<Event> peer_done;        // repeated-device list: per peer, its trace has finished
    Event reduce_done;                   // repeated-device list: the primary has read every peer's buffer
    bool any() const { return !peers.empty() || !comms.empty(); }
};

}  // namespace mfxh

// One mfx_ctx = one `Scene` on one or more GPUs (mfx_api.cpp).
struct __attribute__((visibility("hidden"))) mfx_ctx {
    int device = 0;
    mfxh::Stream stream;
    mfxh::SceneImages scene;   // the scene in HBM and the launch shapes it determines
    double* d_accum = nullptr;         // [3][npix] the active accumulator: d_accum_own, or the caller's
                                       // (mfx_accum_attach; never owned)
    mfxh::DevBuf<double> d_accum_own;
    mfxh::DevBuf<double> d_film;       // [3][npix]
    mfxh::DevBuf<double> d_frame;      // [npix][4] staging for x-major outputs
    mfxh::DevBuf<uint8_t> d_rgba;      // [npix][4]
    mfxh::DevBuf<unsigned long long> d_work;
    mfxh::DevBuf<unsigned long long> d_counters;         // [WF_SHARDS][WF_NCTR] the last trace's counters
    mfxh::DevBuf<unsigned long long> d_counters_total;   // [WF_SHARDS][WF_NCTR] running totals (mfx_ray_counts_total)
    mfxh::HostBuf<unsigned long long> h_counters;  // page-locked [WF_SHARDS][WF_NCTR]: a batch's ray counters
    uint64_t seed = 0;
    int flags = 0;
    int part_index = 0, part_count = 1;  // sample partition: global samples part_index mod part_count
    int api_part_count = 1;              // the caller's partition count (mfx_options.part_count)
    // image partition: this device traces the film's 8-pixel tile rows of band band_index of band_count
    // (band_tile_row, mfx_device.h: one of each band_count consecutive tile rows, serpentine)
    // (device g of a G-device list: g of G; an MFX_F_ROW_PARTITION rank composes with it)
    int band_index = 0, band_count = 1;
    int64_t next_sample = 0;
    double frame_count = 0.0;
    uint64_t cam_epoch = 0;    // 0 after create, +1 per mfx_set_camera that changed the camera (primary)
    int64_t cam_rebuilds = 0;  // of which had to build the images again
    uint64_t image_gen = 0;    // +1 per SceneImages installed on this device (a new node image)
    mfxh::CamCuts cuts;
    mfxh::KeptScene kept;      // (primary)
    int64_t npix = 0;
    mfxh::Event ev0, ev1;
    bool ev_valid = false;
    std::vector<mfxh::Event> it_ev;         // per iteration: start, extend|shadow boundary, end
    int it_recorded = 0;                    // iterations of the last trace with events in it_ev
    int it_per_gen = 0;                     // and per generation
    int generations = 0;
    bool mega_last = false;
    bool cam_last = false;  // the last wavefront trace ran its camera rays as packets (k_camera)
    int wf_chunk = 256;  // slots per chunk fetch (a multiple of 64; r04j: 256 against 1024, C2 64 spp +1 %, 8 spp +6 %)
    bool wf_shd_half = true;  // k_shadow takes half chunks in place on frames of at most 2^25 paths (MFX_SHD_HALF)
    int mega_chunk = 0;   // megakernel: paths a wave takes per atomic (0: by the call's size)
    bool rep_valid = false;          // the last call was served from held frames, or was mfx_sample_adaptive
                                     // (several traces): its stats are rep_*
    double rep_counts[16] = {0};
    double rep_timing[8] = {0};      // mfx_trace_timing's stage split (mfx_sample_adaptive: summed over its passes; else 0)
    double rep_ms = 0.0;
    mfxh::CreateEnv env;
    bool diag_iter = false;
    bool iter_events = true;  // per-iteration HIP events around each launch (mfx_trace_timing's stage split)
    // per feature: each owns what it allocates
    mfxh::WfPool pool;
    mfxh::Ahead ahead;
    mfxh::Adaptive adp;
    mfxh::Denoise dn;
    mfxh::Temporal tp;
    mfxh::Readback rb;
    mfxh::Multi multi;
    mfxh::Textures tex;
    mfxh::Environment sky;
    mfxh::Lens lens;
    mfxh::Normals nrm;

    // the RCCL communicators, then the peers, then this device current; the members release themselves
    ~mfx_ctx();
};

namespace mfxh __attribute__((visibility("hidden"))) {

// the devices of a context, primary first
inline std::vector<mfx_ctx*> devs_of(mfx_ctx* c) {
    std::vector<mfx_ctx*> v{c};
    for (const auto& p : c->multi.peers) v.push_back(p.get());
    return v;
}

// tile rows of the film in a device's band (its image partition)
inline int band_rows(const mfx_ctx* d) {
    const int tr = (d->scene.host.height + 7) / 8;
    return band_row_count(d->band_index, d->band_count, tr);
}

// several lights (SceneImages::multi_light)
inline bool wf_multi_light(const mfx_ctx* c) { return c->scene.multi_light(); }

// albedo textures (mfx_create_textured with a textured primitive): the TX instances of k_shadow, k_resolve
// and k_aov, the wavefront pipeline for every trace, a texel-id plane in the pool
inline bool wf_textured(const mfx_ctx* c) { return c->tex.host.on; }

// a sky (mfx_set_environment): the ENV instances of k_extend, k_camera and k_resolve, the wavefront pipeline
// for every trace, a miss-record word per slot in the pool
inline bool wf_env(const mfx_ctx* c) { return c->sky.on(); }
// a sampled sky (mfx_set_environment_sampled): the SKY instances of k_shadow and k_resolve, which are several-light
// instances (wf_multi_light holds), the sampling table, a texel-id plane per vertex in the pool
inline bool wf_sky_sampled(const mfx_ctx* c) { return c->sky.on() && c->sky.sampled; }

// a thin lens (mfx_set_lens): the LENS twin of the k_extend instance that starts the paths (no k_camera, no camera
// cuts) and of k_aov, the wavefront pipeline for every trace
inline bool wf_lens(const mfx_ctx* c) { return c->lens.on; }

// smooth shading (mfx_set_normals): the SN twins of k_shadow and k_aov, the wavefront pipeline for every trace
inline bool wf_normals(const mfx_ctx* c) { return c->scene.normals; }

// bytes of one path slot of the wavefront pool (ray queues included)
inline size_t pool_slot_bytes(const mfx_ctx* c) {
    const int nv = c->scene.host.max_depth + 1;  // vertices per path
    return WF_DOUBLES_PER_SLOT(nv) * 8 + WF_WORDS_PER_SLOT(nv) * 4 + (wf_multi_light(c) ? WF_LIGHT_BYTES_PER_SLOT(nv) : 0) +
           (wf_textured(c) ? WF_TEXEL_BYTES_PER_SLOT(nv) : 0) + (wf_env(c) ? WF_ENV_BYTES_PER_SLOT : 0) +
           (wf_sky_sampled(c) ? WF_SKY_BYTES_PER_SLOT(nv) : 0);
}

// the scene images' device pointers of a kernel parameter struct (WfParams, TraceParams, AovParams, QueryParams)
template <typename P>
void fill_scene_ptrs(const mfx_ctx* c, P& p) {
    const SceneImages& s = c->scene;
    p.nodes = s.d_nodes;
    p.slots = s.d_slots;
    p.slot_ref = s.d_slot_ref;
    p.ref_blob = s.d_ref_blob;
    p.shade = s.d_shade;
    p.inst = s.d_inst;
    p.tslack = s.host.tslack;
}

// a gray light (bitwise equal intensities): k_shadow records a lit vertex's direct term itself
inline bool wf_gray_light(const mfx_ctx* c) {
    const double* I = c->scene.host.light.color;
    return std::memcmp(&I[0], &I[1], sizeof(double)) == 0 && std::memcmp(&I[0], &I[2], sizeof(double)) == 0 &&
           !c->env.no_gray_light && !wf_multi_light(c);  // (several lights: the term depends on the picked one)
}
// in place, a HIT state word carries the path's lit mask (WfParams.lit_in_hit)
inline bool wf_lit_in_hit(const mfx_ctx* c) {
    const MfxHostScene& h = c->scene.host;
    return h.max_depth <= 3 && h.shade.size() <= ((size_t)1 << 25) && !c->env.no_lit_in_hit;
}

// mfx_create.cpp
// The camera `cam` and the lens (null: none) become the context's, on every device: in place when the images' widening
// covers what they need, by building the images again otherwise (a failure leaves everything as it was). who: the
// calling entry point, for messages. Waits for the context's work and invalidates what mfx_set_camera invalidates.
int apply_camera_lens(mfx_ctx* c, const char* who, const mfx_pinhole* cam, const mfx_lens* lens);
// the lens record of `cam` under `lens`, or MFX_E_INVALID with who + ": " + the field that is refused
int lens_record(const char* who, const mfx_pinhole* cam, const mfx_lens* lens, MfxLensRec& rec);
// after set_sky_light on c's images: the lights in HBM again and the launch shapes of the instances that run now
int scene_relight(mfx_ctx* c);
// after mfx_set_normals set or cleared SceneImages::normals: the launch shapes of the k_shadow instance that runs now
int scene_reshape(mfx_ctx* c);
// the LDS shape of k_extend or (shd) k_shadow over the scene images `s` of a context (textured: wf_textured) with
// nlds stack entries per lane in LDS (the rest spilled), and ntop top nodes and nslot slots beside them
WfLdsShape wf_lds_shape(const SceneImages& s, bool textured, bool shd, int nlds, int ntop = 0, int nslot = 0);
bool flatten_instances(const mfx_scene_desc* scene, const mfx_instance* instances, int32_t ninstances, int32_t flags,
                       size_t device_free = 0);

// MFX_OK, or MFX_E_STATE for a call that needs one device and the whole film and sample set
int whole_film_single_device(const mfx_ctx* c, const char* who);

// mfx_trace.cpp
int wf_trace(mfx_ctx* c, int64_t ns, int64_t sample_base, TraceMode mode = {});
bool cuts_apply(const mfx_ctx* c);
int cuts_ensure(mfx_ctx* c, int64_t ns);
int cuts_read_stats(mfx_ctx* c);
int dev_trace_accumulate(mfx_ctx* c, int32_t spp, int64_t sample_base, ResolveSplit* split = nullptr);
int settle_queue_auto(mfx_ctx* c);
void note_live(mfx_ctx* c, const unsigned long long* h);
void sum_counters(const unsigned long long* h, double out[16]);
int add_stage_times(mfx_ctx* c, double out[8]);
int reduce_planes(mfx_ctx* c, double* (*buf)(mfx_ctx*), double* dst, const char* what);
// mfx_readback.cpp
int host_readback(mfx_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st);
// mfx_ahead.cpp
int ahead_materialize(mfx_ctx* c);
int ahead_break(mfx_ctx* c);

}  // namespace mfxh
