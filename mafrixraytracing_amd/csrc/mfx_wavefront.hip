// mfx_wavefront.hip — wavefront path tracing on gfx950: the integrator loop
// (Integrators.fs:107-137, 161-172) as two persistent kernels per iteration over a pool of
// path slots, one bounce of every live path per iteration (mfx_wavefront.h):
//
//   k_extend   bvh.Hit(ray, 1e-6, 99999999.) (Integrators.fs:108) for NEED_EXT slots; in a
//              generation's first iteration every FREE slot j starts path path_base + j
//              (PixelIntegrator.Sample + PinholeCamera.GetRay, Integrators.fs:161-169,
//              Camera.fs:134-139). Writes the hit point and the hit's shade index.
//   k_shadow   one vertex of PathIntegrator.TraceRay for HIT slots: LambertianBrdf.SampleF and
//              NewAreaLight.Sample_Li (Integrators.fs:110-134), recording the vertex's col, then
//              its shadow ray (Integrators.fs:44) traced by a lane of the same wave; unoccluded ->
//              the vertex's direct term l / pdf_li is recorded too (mfx_wavefront.h).
//   k_resolve  after a generation: each finished path's vertices folded back to the camera in the
//              reference's recursion order, (l / pdf_li + TraceRay(next)) * col (Integrators.fs:136),
//              and added to its pixel in sample order (`color <- color + ...`, Integrators.fs:169).
//
// Both trace kernels keep lanes busy: a lane that finishes its ray takes the next pending ray at
// the next step (persistent while-while with dynamic fetch, Aila & Laine 2009). Pending rays come
// from scanning 64-slot windows with the whole wave: only the state words are read (several
// windows per memory round trip, WF_LOOKAHEAD), the slots to work on are compacted (ballot +
// popcount ranks) into a per-wave LDS list, and the per-slot data is loaded by the lane that takes
// the entry. k_shadow shades 64 listed hits at a time with all lanes and hands the shadow rays to
// the traversal in LDS, so a shadow ray never round-trips through HBM. Path state lives in HBM as
// SoA FP64; every arithmetic step is the same FP64 expression as the oracle, in the same order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>
#include <utility>

#include "mfx_device.h"
#include "mfx_trace_common.h"
#include "mfx_wavefront.h"

#ifndef MFX_TRAV_WAVES
#define MFX_TRAV_WAVES 4  // min waves per SIMD requested from the register allocator (128 VGPRs; a few spills)
#endif

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }


#ifndef MFX_SHADOW_ORDER
#define MFX_SHADOW_ORDER 1  // shadow rays' child order: 0 near-first, 1 far-first (by exit distance)
#endif

#ifndef MFX_NODE_LANES_MIN
#define MFX_NODE_LANES_MIN 16  // node-loop early exit: fewer lanes than this still stepping
#endif
#ifndef MFX_NODE_LANES_MIN_SHD
#define MFX_NODE_LANES_MIN_SHD 12  // the same for shadow rays
#endif

#ifndef MFX_MASKED_PUSH
#define MFX_MASKED_PUSH 1  // node_step's pushes as masked stores without branches (0: three branches a step)
#endif

#ifndef MFX_DIAG_STAMPS
#define MFX_DIAG_STAMPS 0  // diagnostic build only: 1 = k_extend phase stamps, 2 = k_shadow, 3 = k_camera
#endif
struct DiagAcc {
    uint64_t fetch, node, leaf, fin, last, scan, shade, lat;  // lat: node loads' issue-to-use cycles (node_step)
    uint32_t outer, node_iters, windows;
};
__device__ __forceinline__ uint64_t stamp() {
    uint64_t t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define DIAG_MARK(acc, field, on)              \
    do {                                       \
        if (on) {                              \
            const uint64_t _t = stamp();       \
            (acc).field += _t - (acc).last;    \
            (acc).last = _t;                   \
        }                                      \
    } while (0)
__device__ __forceinline__ uint64_t lanes_below() { return (1ULL << lane_id()) - 1ULL; }

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// per-block reduction of a per-lane counter, one atomic per block (the counters are sharded too)
template <int NW>
__device__ __forceinline__ void block_add(unsigned long long* dst, uint32_t v, uint32_t* red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if (lane_id() == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < NW; ++w) s += red[w];
        if (s) atomicAdd(dst, s);
    }
}

// ------------------------------------------------------------------------------------------------
// Slot windows: a wave takes chunks of P.chunk slots (its block's shard first, then the others)
// and scans them 64 at a time.
// ------------------------------------------------------------------------------------------------
static_assert(WF_SHARDS == 64, "shard masks are one bit per lane of a wave");

// Shards of a sharded counter set that are still open (counter below its capacity), one bit per
// shard, from one vector load of all 64 counters (lane g reads shard g). Counters only grow, so a
// stale value can only report a closed shard as open: the caller's atomic then fails and it asks
// again. This replaces walking the shards with one returning atomic each, which cost every wave
// up to 64 serialized round trips at the end of each kernel.
__device__ __forceinline__ uint64_t open_shards(const unsigned long long* ctr, int cap) {
    const unsigned long long v = __hip_atomic_load(ctr + lane_id() * WF_HS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __ballot((int64_t)v < (int64_t)cap);
}

// the first open shard at or after `home` (cyclically); `open` must be non-zero
__device__ __forceinline__ int next_open(uint64_t open, int home) {
    const uint64_t r = home ? ((open >> home) | (open << (64 - home))) : open;
    return (home + __builtin_ctzll(r)) & (WF_SHARDS - 1);
}

#ifndef WF_CLOSED_MASK
#define WF_CLOSED_MASK 1  // closed shards are found from one mask word, not from a load of all 64 heads
#endif
struct Scanner {
    int win_next, win_end, shard;
    bool exhausted;
    uint64_t closed_seen;  // WF_CLOSED_MASK: shards this wave found closed itself
    // state words of the next WF_LOOKAHEAD windows of the chunk, loaded in one round of
    // independent loads (b[0] = the current window; -1 past the chunk's end): windows without
    // work are skipped with no further memory round trip. Slots of a taken chunk change only
    // through this wave, so the words stay current.
    int b[WF_LOOKAHEAD];
    int nbuf;
    // Make [win_next, win_end) non-empty; false once every chunk has been taken. A wave takes
    // chunks from its block's home shard while it lasts, then from the next open shard.
    // qcount: a ray queue's per-shard entry counts (MFX_RAY_QUEUE: a queue fills shard g's range from
    // its start); null: whole shards
    // closed: the launch's closed-shard mask (WF_CLOSED_MASK): bit g set by the one fetch that
    // crosses shard g's end (the fetch whose start lands in [cap, cap + chunk)); a wave also skips the
    // shards its own fetches found closed, so an unset bit never makes it retry one
    // LOAD = false (k_camera: every slot of a generation's first iteration is FREE): no state words
    template <bool LOAD = true>
    __device__ __forceinline__ bool window(unsigned long long* heads, int chunk, int shard_size,
                                           const int32_t* __restrict__ state, const unsigned long long* qcount,
                                           unsigned long long* closed) {
        if (win_next < win_end) return true;
        if (exhausted) return false;
        while (true) {
            unsigned long long c = 0;
            if (lane_id() == 0) c = atomicAdd(heads + shard * WF_HS, (unsigned long long)chunk);
            c = __shfl(c, 0);
            const int cap = qcount ? (int)qcount[shard * WF_HS] : shard_size;
            if ((int64_t)c < cap) {
                win_next = shard * shard_size + (int)c;
                win_end = shard * shard_size + min((int)c + chunk, cap);
                if (LOAD) fill(state);
                return true;
            }
#if WF_CLOSED_MASK
            if (lane_id() == 0 && (int64_t)c < (int64_t)cap + chunk) atomicOr(closed, 1ull << shard);
            closed_seen |= 1ull << shard;
            unsigned long long cm = 0;
            if (lane_id() == 0) cm = __hip_atomic_load(closed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            cm = __shfl(cm, 0);
            const uint64_t open = ~(cm | closed_seen);
#else
            const uint64_t open = open_shards(heads, qcount ? (int)qcount[lane_id() * WF_HS] : shard_size);
#endif
            if (open == 0) {
                exhausted = true;
                return false;
            }
            // the next open shard after this one (a per-wave pseudo-random start instead, WF_SPREAD,
            // measured C2 -0.4 %, C4 -1.9 %, r04c)
            shard = next_open(open, shard);
        }
    }
    __device__ __forceinline__ void fill(const int32_t* __restrict__ state) {
#pragma unroll
        for (int k = 0; k < WF_LOOKAHEAD; ++k) {
            const int j = win_next + 64 * k + lane_id();
            b[k] = j < win_end ? state[j] : -1;
        }
        nbuf = WF_LOOKAHEAD;
    }
    // this lane's state word in the current window
    __device__ __forceinline__ int word() const { return b[0]; }
    __device__ __forceinline__ void advance(const int32_t* __restrict__ state) {
        win_next += 64;
#pragma unroll
        for (int k = 0; k + 1 < WF_LOOKAHEAD; ++k) b[k] = b[k + 1];
        b[WF_LOOKAHEAD - 1] = -1;
        if (--nbuf == 0 && win_next < win_end) fill(state);
    }
};

// the lane's stack: all of it in LDS, or the first P.stack_lds entries (the rest in P.spill)
template <bool SPILL>
__device__ __forceinline__ typename std::conditional<SPILL, SpillStack, LdsStack>::type make_stack(int* lds,
                                                                                                  const WfParams& P,
                                                                                                  int nlds) {
    if constexpr (SPILL)
        return SpillStack{lds, P.spill + blockIdx.x * 256 + threadIdx.x, nlds, (int)gridDim.x * 256};
    else
        return LdsStack{lds};
}

// Traversal state of one lane (one ray) across outer-loop iterations
struct Trav {
#ifdef MFX_DIAG_OCCLUSION
    uint32_t n0, l0;  // the lane's node / cluster counts when this ray started
#endif
    DV o, d;
    double tmax64;
    Best B;
    int node, sp;
    int inst;   // two-level scenes: the instance whose template the lane is in (-1: the world)
    int inst_sp;  // and the stack depth at which it entered (entries below belong to the world)
};

__device__ __forceinline__ void trav_begin(Trav& T, const SceneView& S, DV o, DV d, double tmax) {
    T.o = o;
    T.d = d;
    T.tmax64 = tmax;
    T.B = Best{tmax + S.tslack, -1, -1, false};  // B.t is the node tests' limit until the first hit
    T.sp = 0;
    T.node = 0;
    T.inst = -1;
    T.inst_sp = 0;
}

// one node step of the per-lane traversal (BVH4; shadow rays far-first)
template <bool SHADOW, int NF, typename ST>
__device__ __forceinline__ int trav_node_step(const SceneView& S, int node, const RayF& rf, float tlim, const ST& stack,
                                              int& sp, TopNodes tn, uint64_t* lat) {
    return node_step<true, SHADOW && MFX_SHADOW_ORDER == 1, NF, MFX_MASKED_PUSH != 0>(S.nodes, node, rf, tlim, stack, sp, tn, lat);
}

// Internal nodes until this lane reaches a leaf (while-while), then that one reference leaf in
// exact FP64. Returns true when the ray is finished (closest: stack empty; shadow: occluded or
// stack empty).
// INST: a two-level scene; a lane enters and leaves instances inside the node loop (inst_frame).
// SLDS: the scene's slots are read from the kernel's LDS copy (a small flat scene, SceneView::slots_lds).
// NF: the kernel instance's node format (node_step).
template <bool SHADOW, bool STATS, bool INST, bool SLDS, int NF, typename ST>
__device__ __forceinline__ bool trav_step(Trav& T, const SceneView& S, const ST& stack, TopNodes tn, Stats& st,
                                          DiagAcc& dg, bool diag) {
    // the frame of the entry popped at the end of the last round (an instance left or entered)
    RayF rf{};  // (the frame switch's own ray update is superseded below)
    if (INST) T.node = inst_frame(S, T.node, T.inst, T.inst_sp, T.sp, T.o, T.d, rf);
    // the FP32 ray and the node-test limit are recomputed each round (the same values) rather than
    // held through the leaf tests: fewer live registers, fewer spills (+1 to +5 %)
    rf = INST ? frame_ray(S, T.inst, T.o, T.d) : make_rayf(T.o, T.d);
    const float tlim = f_tlim(T.B.t);  // the query's tMax + tslack until the first hit (trav_begin), then the best t
    while (T.node >= 0) {
        if (STATS) st.nodes++;
#ifdef MFX_DIAG_OCCLUSION
        if (STATS && !SHADOW && T.B.found) st.after_nodes++;
#endif
        if (diag && lane_id() == __builtin_amdgcn_readfirstlane(lane_id())) dg.node_iters++;  // once per wave iteration
        T.node = trav_node_step<SHADOW, NF>(S, T.node, rf, tlim, stack, T.sp, tn, diag ? &dg.lat : nullptr);
        if (INST) T.node = inst_frame(S, T.node, T.inst, T.inst_sp, T.sp, T.o, T.d, rf);
        // leave the node loop once few lanes still step: the rest resume next round, after the
        // leaf tests and a refill of the idle lanes
        if (__popcll(__ballot(T.node >= 0)) < (SHADOW ? MFX_NODE_LANES_MIN_SHD : MFX_NODE_LANES_MIN)) break;
    }
    DIAG_MARK(dg, node, diag);
    if (T.node >= 0) return false;
    if (T.node == MFX_TRAV_EXIT) return true;
#ifdef MFX_DIAG_OCCLUSION
    if (STATS && !SHADOW && T.B.found) st.after_leaves++;
#endif
    const int base = (INST && T.inst >= 0) ? load_inst(S, T.inst).slot_base : 0;
    const bool better = leaf_hit<SHADOW, STATS, false, SLDS>(S, ~T.node, T.o, T.d, 1e-6, T.tmax64, T.B, st, base);
    if (better) {
        if (SHADOW) {
            T.B.found = true;
            return true;
        }
    }
    if (T.sp == 0) return true;
    T.node = stack.get(T.sp - 1, stack.deep(T.sp));
    --T.sp;
    return false;
}

// Path index of this generation -> (sample, 8x8 pixel tile, pixel), sample-major and
// tile-coherent. False for the padding indices of edge tiles (no path). A banded
// trace (image partition) numbers only its own tile rows: its k-th tile row is film tile row
// band_index + k * band_count, so pixels, keys and samples are the whole-film trace's. A listed
// trace (LIST: adaptive sampling's active tiles, ascending, P.ntiles > 0 of them) numbers only the
// list's tiles: per_sample = ntiles * 64 and tile k is film tile P.tiles[k] (list_tile_xy,
// mfx_device.h). LIST is a template parameter of the kernels, so the band instances carry none of
// it (as a run-time branch it moved the scratch size of five k_extend / k_shadow instances).
// WF_LIST_TILE_N (mfx_sample_adaptive_resume's passes): every listed tile continues from its own
// count. The trace's sample d of tile T = P.tiles[k] is the tile's sample P.tile_n[T] + d, which is
// what `smp` returns, and the window is padding (no path, like an edge tile's padding pixels: x =
// P.width) when d >= P.list_max - P.tile_n[T], the tile's clipped share of the pass. It has a
// template value of its own for the reason above: mfx_sample_adaptive's instances are the ones they were.
// PP: WfParams, or k_shadow's LDS copy of the fields it needs (PixParams)
#define WF_LIST_NONE 0
#define WF_LIST_TILES 1
#define WF_LIST_TILE_N 2
template <int LIST, typename PP>
__device__ __forceinline__ bool path_pixel(const PP& P, int64_t p, int& x, int& y, int64_t& smp) {
    // p = path_base + s: the 64-bit split of path_base is done once per generation on the host
    // (base_smp, base_q), so only 32-bit divisions remain here (base_q + s < 2^32)
    const unsigned tiles_x = (unsigned)(P.width + 7) >> 3;
    constexpr bool list = LIST != WF_LIST_NONE;
    const unsigned per_sample = (list ? (unsigned)P.ntiles : tiles_x * (unsigned)P.band_rows) * 64;  // < 2^31 (film limit)
    const unsigned qs = (unsigned)P.base_q + (unsigned)(p - P.path_base);
    const unsigned ds = qs / per_sample;
    smp = P.base_smp + ds;
    const unsigned q = qs - ds * per_sample;
    const unsigned tile = q >> 6, within = q & 63;
    unsigned tx, ty;
    if (list) {
        const unsigned T = (unsigned)P.tiles[tile];
        if (!list_tile_xy(T, tiles_x, (unsigned)(P.height + 7) >> 3, tx, ty)) {
            x = P.width;  // outside the film: no path
            y = 0;
            return false;
        }
        if (LIST == WF_LIST_TILE_N) {  // (T is a tile of the film, so tile_n[T] exists)
            const int tn = P.tile_n[T];
            if (smp >= (int64_t)P.list_max - tn) {
                x = P.width;  // past the tile's share of the pass: no path
                y = 0;
                return false;
            }
            smp += tn;
        }
    } else {
        const unsigned tyl = tile / tiles_x;
        ty = (unsigned)band_tile_row(P.band_index, P.band_count, (int)tyl);
        tx = tile - tyl * tiles_x;
    }
    x = (int)(tx * 8 + (within & 7));
    y = (int)(ty * 8 + (within >> 3));
    return x < P.width && y < P.height;
}
// the global sample index of path_pixel's `smp` (a listed trace is whole-film and unpartitioned:
// whole_film_single_device; k_shadow's PixParams keeps a per-tile trace's fields in the partition's words)
template <int LIST, typename PP>
__device__ __forceinline__ int64_t path_gsample(const PP& P, int64_t smp) {
    if (LIST == WF_LIST_TILE_N) return P.sample_base + smp;
    return P.sample_base + P.part_index + smp * P.part_count;
}

#define WF_EXT_PEND 128  // k_extend per-wave pending list: slot indices (sign bit: camera ray)
#define WF_SHD_LIST 128  // k_shadow per-wave shade list entries

__device__ __forceinline__ bool cont0(int vflag) { return (vflag & 1) != 0; }  // k_shadow: the path continues

// Per-wave LDS list of k_shadow's pending shadow rays: ray index, a flag word, the path's slot and
// its next-queue entry (MFX_RAY_QUEUE) and 6 doubles (direction, tmax, the direct term's operands
// cs and solid), each field a 64-entry column (conflict-free).
struct PendShd {
    static constexpr int BYTES = 64 * (4 + 4 + 8 * 6);
    int* slot;  // the shadow ray's origin, the hit point: its index in the ray arrays, or (a path
                // that continues into the next queue, MFX_RAY_QUEUE) its entry there
    int* flag;
    double* v;  // v[f * 64 + entry]
    __device__ __forceinline__ PendShd(uint8_t* base) {
        slot = (int*)base;
        flag = slot + 64;
        v = (double*)(base + 512);
    }
};

// k_shadow derives a path's key from its slot (as k_extend did for the camera ray) at every vertex:
// no key is stored (r02bs: derived at the first vertex, C2 +0.9 to +2.5 %; at every vertex, r03av:
// -0.3 to -1.2 % then, r05m: C2 +0.5 %, Renault +0.7 % once the depth word was gone too)
#ifndef MFX_HEMI_WAVE_FIRST
#define MFX_HEMI_WAVE_FIRST 1  // trials each owner makes alone before the wave shares them (r02bi: 1 vs 2, C3 +0.8 %, C4 +0.6 %, C2 -0.5 %)
#endif

// hemisphere_ball_wave's share of a round with np pending owners, from a table (one scalar load, no
// divide in the round; the quotients through v_rcp_f32 instead cost the round what the even share
// saved): word 0 = b << 24 | M(b), word 1 = M(b + 1), with b = floor(64 / np) and
// M(d) = floor(65536 / d) + 1 the multiplier with floor(n / d) = (n * M(d)) >> 16 for n < 128, d <= 65
// (n * (M d - 65536) <= 127 * 65 < 65536). The 24-bit multiply reads M under b.
struct EvenShareTab {
    uint32_t w[65][2];
};
constexpr EvenShareTab make_even_share() {
    EvenShareTab t{};
    for (uint32_t n = 1; n <= 64; ++n) {
        const uint32_t b = 64 / n;
        t.w[n][0] = (b << 24) | (65536 / b + 1);
        t.w[n][1] = 65536 / (b + 1) + 1;
    }
    return t;
}
__constant__ EvenShareTab even_share_tab = make_even_share();

// GetRandomInUnitSphere(nm) (Material.fs:9-14) for the wave's shading lanes (`own`), the same
// accepted trial, point and draw count as hemisphere_ball. A lane's loop runs until its first
// accepted trial (3.8 trials on average), but the wave runs until its slowest lane's (about 16):
// after a first round in which every owner tries its own first MFX_HEMI_WAVE_FIRST trials, the np
// owners still rejecting share all 64 lanes of every round evenly: with b = floor(64 / np) and
// e = 64 - b * np, the owner of rank r < e gets b + 1 consecutive trials and the others b, on
// consecutive lanes from lane r * b + min(r, e) (a power-of-two share, m = 2^k with np * m <= 64,
// left 12 to 29 of the 64 lanes idle in the middle rounds and took about one round more). Each owner
// takes the lowest accepted trial of its round (all lower ones were rejected before).
// A worker lane draws from the owner's key and draw count (the trial's three draws at their
// counter positions) and decides with hemi_trial, so p is the owner's own computation's bits.
// scratch: 64 ints of the wave's LDS (owner lane ids in rank order).
__device__ __forceinline__ DV hemisphere_ball_wave(bool own, DV nm, uint64_t key, uint32_t& rn, int* scratch) {
    const int lane = lane_id();
    DV p = dv(0, 0, 0);
    bool done = !own;
    const uint32_t base = rn;  // draws used before trial 0
    if (own) {  // round 0: the owner's own first MFX_HEMI_WAVE_FIRST trials
        const float nx = (float)nm.x, ny = (float)nm.y, nz = (float)nm.z;
        uint32_t r = base;
        uint64_t z[3 * MFX_HEMI_WAVE_FIRST];
#pragma unroll
        for (int i = 0; i < 3 * MFX_HEMI_WAVE_FIRST; ++i) z[i] = rng_bits(key, r);
        for (int i = 0; i < MFX_HEMI_WAVE_FIRST; ++i)
            if (hemi_trial(nm, nx, ny, nz, z[3 * i], z[3 * i + 1], z[3 * i + 2], p)) {
                rn = base + 3 * (i + 1);
                done = true;
                break;
            }
    }
    uint32_t next = MFX_HEMI_WAVE_FIRST;  // the owner's next trial index
    while (true) {
        const uint64_t pend = __ballot(!done);
        if (pend == 0) break;
        const int np = __popcll(pend);
        // trials per pending owner (wave-uniform): b + 1 for the first e ranks, b for the rest; 64 in all
        const uint32_t w0 = even_share_tab.w[np][0], w1 = even_share_tab.w[np][1];
        const int b = (int)(w0 >> 24), e = 64 - b * np;
        const int rank = __popcll(pend & lanes_below());
        if (!done) scratch[rank] = lane;
        wave_lds_sync();
        // this lane works for the owner of rank `slot`, on its trial t of the round
        const bool wide = lane < e * (b + 1);
        const uint32_t ln = (uint32_t)(wide ? lane : lane - e);
        const int slot = (int)(__umul24(ln, wide ? w1 : w0) >> 16);
        const int t = (int)ln - __mul24(slot, wide ? b + 1 : b);
        const int owner = scratch[slot];
        wave_lds_sync();
        const uint64_t k = __shfl(key, owner);
        const uint32_t ob = (uint32_t)__shfl((int)base, owner);
        const uint32_t nt = (uint32_t)__shfl((int)next, owner);
        const DV q = dv(__shfl(nm.x, owner), __shfl(nm.y, owner), __shfl(nm.z, owner));
        DV pt = dv(0, 0, 0);
        uint32_t r = ob + 3 * (nt + (uint32_t)t);
        const uint64_t zx = rng_bits(k, r);
        const uint64_t zy = rng_bits(k, r);
        const uint64_t zz = rng_bits(k, r);
        const bool acc = hemi_trial(q, (float)q.x, (float)q.y, (float)q.z, zx, zy, zz, pt);
        const uint64_t A = __ballot(acc);
        // the owner's own share of the round: m trials on the lanes from first_lane
        const int m = b + (rank < e ? 1 : 0);
        const int first_lane = done ? lane : __mul24(rank, b) + min(rank, e);
        const uint64_t seg = done ? 0 : (A >> first_lane) & (~0ULL >> (64 - m));  // 1 <= m <= 64
        const int src = done ? lane : first_lane + (seg ? __builtin_ctzll(seg) : 0);
        const DV ps = dv(__shfl(pt.x, src), __shfl(pt.y, src), __shfl(pt.z, src));
        if (!done) {
            if (seg) {
                p = ps;
                rn = base + 3 * (next + (uint32_t)__builtin_ctzll(seg) + 1);
                done = true;
            } else {
                next += (uint32_t)m;
            }
        }
    }
    return p;
}

// One vertex of PathIntegrator.TraceRay (Integrators.fs:109-134) for the wave's `own` lanes, at the
// hit point hp with normal nm: LambertianBrdf.SampleF (Material.fs:33-36; the rejection sampler
// spread over the wave, hemisphere_ball_wave) gives the next direction wi and its cosine ei;
// NewAreaLight.Sample_Li (Light.fs:42-47,57-59; Rect/Triangle.SamplePoint) the shadow ray's unit
// direction and length, and the operands of the direct term l / pdf_li, l = (unit . n) *
// L(hit, toLight) (Integrators.fs:52, Light.fs:48-56): cs = unit . n and solid = |cos_o| A / dist^2,
// L black unless cos_o < 0 (lightable). Called by the whole wave; scratch: 64 ints of its LDS.
struct VertexSample {
    DV wi, unit;
    double ei, dist, cs, solid;
    bool lightable;
    int light;  // ML: the picked light
    uint32_t texel;  // SKY: the sky vertex's texel (light == nlights)
};
// k_shadow's several-light instances keep these in the LDS block the one light's copy takes otherwise
struct MlPtrs {
    const MfxLight* lights;
    uint8_t* vlt;
    int32_t nlights;
};
static_assert(sizeof(MlPtrs) <= sizeof(MfxLight), "MlPtrs lies in the light's LDS block: k_shadow's footprint stays");
// the SKY instances' table and plane, in the same block after MlPtrs
struct SkyPtrs {
    MlPtrs ml;
    const MfxSkyEntry* tab;
    uint32_t* vsky;
    int32_t size;
};
static_assert(sizeof(SkyPtrs) <= sizeof(MfxLight), "SkyPtrs lies in the light's LDS block: k_shadow's footprint stays");
// LT1: the light (k_shadow's LDS copy).
// ML: several lights (mfx_create_lights). After the hemisphere sample one more draw r picks light
// n = floor(r * N) of the table `lights` (no clamp: r <= 1 - 2^-53, and (1 - 2^-53) * N rounds below N for
// N <= 64); the lane reads that light's fields from global memory (lanes of a wave pick different
// lights; the table is 208 B a light and stays in L1 / L2), and LT is not read.
// SKY (an ML instance; mfx_set_environment_sampled): the pick is over N + 1, always drawn. A lane whose pick is N
// takes four more draws r1, r2, ju, jv, reads entry k = floor(r1 * n) of the sampling table for its texel t and
// entry t for prob, and gets the direction of (t, ju, jv) (mfx_environment.h): unit, cs = unit . n, pdf_v in
// `solid`, lightable iff cs > 0, dist = the extension ray's far bound. It reads no light.
template <bool ML = false, bool SKY = false>
__device__ __forceinline__ VertexSample sample_vertex(const MfxLight& LT1, bool own, DV hp, DV nm, uint64_t key,
                                                      uint32_t& rn, int* scratch, const MfxLight* lights = nullptr,
                                                      int nlights = 1, const MfxSkyEntry* sky_tab = nullptr,
                                                      int sky_size = 0) {
    VertexSample V{};
#if defined(MFX_DIAG_ONE_TRIAL)  // timing experiment only: the first trial, mirrored into the hemisphere
    DV p = dv(rng_next(key, rn) * 2.0 - 1.0, rng_next(key, rn) * 2.0 - 1.0, rng_next(key, rn) * 2.0 - 1.0);
    if (vdot(nm, p) <= 0.) p = vmul(p, -1.0);
#else
    const DV p = hemisphere_ball_wave(own, nm, key, rn, scratch);
#endif
    if (!own) return V;
    V.wi = vnormalize(p);
    V.ei = vdot(nm, V.wi);
    if constexpr (ML) {  // the pick (RandomDirectLightIntegrator, Integrators.fs:62)
        const double r = rng_next(key, rn);
        V.light = (int)floor(r * (double)(SKY ? nlights + 1 : nlights));
    }
    if constexpr (SKY) {
        if (V.light >= nlights) {  // the sky
            const double r1 = rng_next(key, rn);
            const double r2 = rng_next(key, rn);
            const double ju = rng_next(key, rn);
            const double jv = rng_next(key, rn);
            const uint32_t k = mfx_env_sample_entry(r1, (uint32_t)(sky_size * sky_size));
            const MfxSkyEntry ek = sky_tab[k];
            const uint32_t t = r2 < (double)ek.q ? k : ek.alias;
            double u3[3], len2, len;
            mfx_env_sample_dir(t, ju, jv, sky_size, u3, len2, len);
            V.light = nlights;
            V.texel = t;
            V.unit = dv(u3[0], u3[1], u3[2]);
            V.dist = MFX_ENV_FAR;
            V.cs = vdot(V.unit, nm);
            V.solid = mfx_env_sample_pdf(sky_tab[t].prob, sky_size, len2, len, nlights);
            V.lightable = V.cs > 0.0;
            return V;
        }
    }
    const MfxLight& LT = ML ? lights[V.light] : LT1;
    const double sel = rng_next(key, rn);
    const int lt = sel < 0.5 ? 0 : 1;
    const double tu = rng_next(key, rn);
    const double tv = rng_next(key, rn);
    double uu = tu, vv = tv;
    if (tu + tv > 1.) { uu = 1. - tu; vv = 1. - tv; }
    const double sq = sqrt(1. - uu);
    const double s1 = 1. - sq, s2 = vv * sq;
    // both halves from scalar registers, selected per lane (ML: the lane's half of its light, gathered)
    const DV lv0 = ML ? ld3(LT.v0[lt]) : lt ? ld3(LT.v0[1]) : ld3(LT.v0[0]);
    const DV le1 = ML ? ld3(LT.e1[lt]) : lt ? ld3(LT.e1[1]) : ld3(LT.e1[0]);
    const DV le2 = ML ? ld3(LT.e2[lt]) : lt ? ld3(LT.e2[1]) : ld3(LT.e2[0]);
    const DV lp = vadd(vadd(lv0, vmul(le1, s1)), vmul(le2, s2));
    const DV toLight = vsub(lp, hp);
    V.dist = vlen(toLight);
    V.unit = vdiv(toLight, V.dist);
    // NewAreaLight.L (Light.fs:48-56) and the unclamped cosine (Integrators.fs:52)
    const double cos_o = vdot(toLight, ld3(LT.normal));
    const double dist2 = toLight.x * toLight.x + toLight.y * toLight.y + toLight.z * toLight.z;
    V.solid = fabs(cos_o) * LT.area / dist2;
    V.cs = vdot(V.unit, nm);
    V.lightable = cos_o < 0.;
    return V;
}

// ------------------------------------------------------------------------------------------------
// k_extend: closest hit for NEED_EXT slots; in a generation's first iteration FREE slots start paths
// ------------------------------------------------------------------------------------------------
// Q: the instance for the iterations on ray queues (MFX_RAY_QUEUE; P.qcount); the in-place one
// has none of their code
// SK: the scene kind (WF_SK_FLAT, WF_SK_INST: two-level, WF_SK_SLDS: a small flat scene whose whole
// slot array sits in LDS); only a small scene's instances carry the LDS slot reads (r04c: the runtime
// branch in every leaf test cost C2 1.8 % and C4 4 %)
// START: the instance for a generation's first iteration when k_camera does not take its camera
// rays (two-level scenes, MFX_CAMERA_PACKETS=0); only it carries the camera-ray code (GetRay, the
// path key, the camera's fields), so the bounce instances hold fewer live scalar registers
// LIST: a START instance for a listed trace (adaptive sampling: path_pixel's tile list, WF_LIST_TILES; with
// per-tile counts WF_LIST_TILE_N, whose clipped windows the scan takes as padding: P.tile_padding is set)
// NF: the node format (node_step): the instances a flat scene's default path launches (the bounce and
// queue ones, wf_nf) are built for one format each, so their node loop holds one step and none of the
// other's registers; the rest (STATS, START, LIST, the other scene kinds) take either (MFX_NF_ANY)
// ENV: the instances for a sky (mfx_set_environment): a miss stores the texel of the ray's direction and the
// iteration (the vertices before the miss; wave-uniform) in the path slot's word of P.env_rec, through qslot
// on a queue. A template parameter for ML's reason: the instances without hold none of it.
// LENS: the START instances for a thin lens (mfx_set_lens): the camera ray starts on the lens disk and passes
// through the pinhole ray's point of the focus plane (mfx_lens.h); a flat scene's camera rays take these instead of
// k_camera, whose packets rest on one shared origin. Nothing after the ray's start differs.
template <bool STATS, bool SPILL, int SK, bool Q, bool START = false, int LIST = WF_LIST_NONE, int NF = MFX_NF_ANY,
          bool ENV = false, bool LENS = false>
__global__ void __launch_bounds__(256, MFX_TRAV_WAVES) k_extend(WfParams P) {
    static_assert(!LENS || START, "a lens bends camera rays only");
    constexpr bool INST = SK == WF_SK_INST, SLDS = SK == WF_SK_SLDS;
    extern __shared__ int lds_all[];
#if MFX_NODE_F16
    const TopNodes tn{(const float4*)lds_all, P.ntop_ext, P.nodes_h};
#else
    const TopNodes tn{(const float4*)lds_all, P.ntop_ext};
#endif
#if MFX_NODE_F16
    if (NF == MFX_NF_H || (NF == MFX_NF_ANY && P.nodes_h)) load_top_nodes_h((float4*)lds_all, P.nodes_h, P.ntop_ext);
    else
#endif
        load_top_nodes((float4*)lds_all, P.nodes, P.ntop_ext);
    MfxInstance* inst_lds = (MfxInstance*)(lds_all + P.ntop_ext * 32);
    if (INST) load_inst_lds(inst_lds, P.inst, P.ninst_lds);
    int4* slot_lds = (int4*)(inst_lds + (INST ? P.ninst_lds : 0));
    const int nslot = SLDS ? P.nslot_ext : 0;
    if (SLDS) load_slots_lds(slot_lds, P.slots, nslot);
    int* lds = (int*)(slot_lds + 5 * nslot);
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    using Stack = typename std::conditional<SPILL, SpillStack, LdsStack>::type;
    const Stack stack = make_stack<SPILL>(lds + wave * P.stack_lds_ext * 64 + lane, P, P.stack_lds_ext);
    int* pend = lds + 4 * P.stack_lds_ext * 64 + wave * WF_EXT_PEND;
    uint32_t* red = (uint32_t*)(lds + 4 * P.stack_lds_ext * 64 + 4 * WF_EXT_PEND);
    const SceneView S{P.nodes, P.slots, P.slot_ref, P.ref_blob, P.inst, inst_lds, INST ? P.ninst_lds : 0, slot_lds, nslot, nullptr, P.tslack};
    const int shard_size = P.pool / WF_SHARDS;

    Scanner sc{};
    sc.shard = blockIdx.x & (WF_SHARDS - 1);
    int pend_lo = 0, pend_hi = 0;
    bool active = false;
    int se = 0;  // the lane's listed entry: slot (WF_ENTRY_SLOT), lit mask << 28, camera-ray flag (sign)
    Trav T{};
    // rays started by this wave: every listed entry is started, so the wave counts its lists (a
    // wave-uniform sum) instead of each lane its rays (a per-lane counter spilled to scratch, whose
    // increment put a scratch round trip into every refill)
    uint32_t c_listed = 0;
    Stats st{0, 0, 0};
    constexpr bool DG = MFX_DIAG_STAMPS == 1;
    DiagAcc dg{};
    if (DG) dg.last = stamp();
    // An in-place extension ray's entry carries the path's lit-vertex mask (k_shadow wrote it into
    // the NEED_EXT state word) in bits 28..30 when it fits (iterations 1..3: vertices 0..2), so a
    // miss writes its finished state word, mask included, without loading the depth word (r04b:
    // +0.5 % over that load; k_resolve reading the depth words of misses instead, r04g: -0.3 %).
    // The lane keeps the entry itself: no register for the mask or the camera-ray flag.
    const bool lit_in_entry = !Q && P.iter <= 3;
    // the lane takes listed entry e: its camera ray (FREE slot) or the slot's extension ray
    auto start_ray = [&](int e) {
        se = e;
        const int s = e & WF_ENTRY_SLOT;
        const bool fresh = START && e < 0;
        DV o, d;
        if (fresh) {
            // PixelIntegrator.Sample (Integrators.fs:167-169) + GetRay (Camera.fs:134-139)
            int x, y;
            int64_t smp;
            path_pixel<LIST>(P, P.path_base + s, x, y, smp);
            const int64_t pixel = (int64_t)x * P.height + y;  // Color[w,h] x-major
            const int64_t gsample = path_gsample<LIST>(P, smp);
            const uint64_t key = path_key(P.seed, (uint64_t)pixel, (uint64_t)gsample);
            uint32_t rn = 0;
            const double u = ((double)x + rng_next(key, rn)) / (double)P.width;
            const double v = ((double)y + rng_next(key, rn)) / (double)P.height;
            const MfxCamera& CAM = P.cam;
            if constexpr (LENS) {  // the lens draws come from a stream of their own: the path's counter stays at 2
                double lo[3], ldir[3], la, lb;
                const MfxLensRec L = *(const MfxLensRec*)(P.cam_dev + 1);  // wave-uniform: scalar loads
                mfx_lens_ray(CAM.position, L, key, u, v, lo, ldir, la, lb);
                o = dv(lo[0], lo[1], lo[2]);
                d = dv(ldir[0], ldir[1], ldir[2]);
            } else {
                const DV target = vadd(vadd(ld3(CAM.topleft), vmul(ld3(CAM.right), u)), vmul(ld3(CAM.down), v));
                o = ld3(CAM.position);
                d = vnormalize(vsub(target, o));
            }
            // throughput 1, radiance 0, rn 2 and depth max_depth stay implicit (WF_FRESH); the
            // key is derived again by k_shadow
        } else {
            o = dv(P.ox[s], P.oy[s], P.oz[s]);
            d = dv(P.dx[s], P.dy[s], P.dz[s]);
        }
        trav_begin(T, S, o, d, 99999999.);  // Integrators.fs:108
        active = true;
    };
    // the lane's ray is finished: its closest hit (hit point, shade index) or its miss
    auto finish_ray = [&]() {
        const int s = se & WF_ENTRY_SLOT;
        const bool fresh = START && se < 0;
        const int fl = fresh ? WF_FRESH : 0;
        if (T.B.found) {
            const DV hp = vadd(T.o, vmul(T.d, T.B.t));  // Ray.PointAtParameter (Ray.fs:8-9)
            P.ox[s] = hp.x; P.oy[s] = hp.y; P.oz[s] = hp.z;
            // in place (lit_in_hit): the path's lit mask rides in bits 29..31 for k_shadow
            const int lm = (P.lit_in_hit && lit_in_entry && !fresh) ? ((se >> 28) & 7) << 29 : 0;
            P.state[s] = ((T.B.info & MFX_INFO_SHADE_MASK) << WF_SHADE_SHIFT) | WF_HIT | fl | lm;
        } else {  // a later miss finishes the path: its lit mask goes into the state word
            const int lm = fresh || Q ? 0 : (lit_in_entry ? (se >> 28) & 7 : (P.depth[s] >> WF_LIT_SHIFT) & 0xffff);
            P.state[s] = WF_MISS | (lm << WF_SHADE_SHIFT) | fl;
            if constexpr (ENV)  // the path ends in the sky: k_resolve starts its fold there
                P.env_rec[Q ? P.qslot[s] : s] =
                    mfx_env_texel(T.d.x, T.d.y, T.d.z, P.env_size) | ((uint32_t)P.iter << MFX_ENV_NV_SHIFT);
        }
        active = false;
    };

    while (true) {
        // ---- dynamic fetch: idle lanes take pending rays by rank ----
        bool idle = !active;
        uint64_t m = __ballot(idle);
        while (m != 0) {
            if (pend_lo == pend_hi) {
                // list at least 64 slots to trace (or all that are left) from as many windows as it
                // takes; only state words are read here, WF_LOOKAHEAD windows per round trip
                int n = 0;
                while (n < 64 && sc.window(P.ctl + WF_CTL_EXT, P.chunk, shard_size, P.state, Q ? P.qcount : nullptr, P.ctl + WF_CTL_CLOSED_EXT)) {
                    if (DG) dg.windows++;
                    const int j = sc.win_next + lane;
                    const int sj = sc.word();
                    bool take = (sj & WF_STATE_MASK) == WF_NEED_EXT;
                    if (START && sj == WF_FREE && j < P.total) {
                        int x, y;
                        int64_t smp;
                        // edge-tile padding starts no path (none when 8 divides the film size)
                        take = !P.tile_padding || path_pixel<LIST>(P, P.path_base + j, x, y, smp);
                    }
                    const uint64_t tm = __ballot(take);
                    // entry: slot | camera-ray flag << 31, or slot | lit mask << 28 (lit_in_entry)
                    if (take)
                        pend[n + __popcll(tm & lanes_below())] =
                            (START && sj == WF_FREE) ? (j | (int)0x80000000)
                                          : (lit_in_entry ? j | (((unsigned)sj >> WF_SHADE_SHIFT) & 7) << 28 : j);
                    n += __popcll(tm);
                    sc.advance(P.state);
                }
                wave_lds_sync();
                pend_lo = 0;
                pend_hi = n;
                c_listed += (uint32_t)n;
                if (n == 0) break;  // every chunk scanned
            }
            const int avail = pend_hi - pend_lo;
            const int rank = __popcll(m & lanes_below());
            if (idle && rank < avail) {
                start_ray(pend[pend_lo + rank]);
                idle = false;
            }
            const int pm = __popcll(m);
            pend_lo += pm < avail ? pm : avail;
            m = __ballot(idle);
        }
        if (!__any(active)) break;  // every chunk taken and every pending ray traced
        DIAG_MARK(dg, fetch, DG);
        if (DG) dg.outer++;
        bool fin = false;
        if (active) fin = trav_step<false, STATS, INST, SLDS, NF>(T, S, stack, tn, st, dg, DG);
        DIAG_MARK(dg, leaf, DG);
        if (fin) finish_ray();
        DIAG_MARK(dg, fin, DG);
    }
    unsigned long long* cnt = P.counters + WF_NCTR * (blockIdx.x & (WF_SHARDS - 1));
    // a generation's first iteration lists camera rays only (every slot FREE), the others extension
    // rays only; lane 0 carries the wave's count
    const uint32_t c_wave = lane == 0 ? c_listed : 0u;
    block_add<4>(cnt + 0, P.start ? c_wave : 0u, red);
    // extension rays: per iteration where it has a counter (the paths that went on; the host adds
    // them into counter 1)
    block_add<4>(cnt + (P.iter > 0 && P.iter < WF_ITER_CTRS ? WF_CTR_ITER + P.iter : 1), P.start ? 0u : c_wave, red);
    if (DG) block_add<4>(cnt + 15, dg.node_iters, red);
    if (DG && lane == 0) {
        atomicAdd(cnt + 10, (unsigned long long)dg.fetch);
        atomicAdd(cnt + 11, (unsigned long long)dg.node);
        atomicAdd(cnt + 12, (unsigned long long)dg.leaf);
        atomicAdd(cnt + 13, (unsigned long long)dg.fin);
        atomicAdd(cnt + 14, (unsigned long long)dg.outer);
        atomicAdd(cnt + 3, (unsigned long long)dg.lat);  // (counter 3: unused by the shipped kernels)
    }
    if (STATS) {
        block_add<4>(cnt + 4, st.nodes, red);
        block_add<4>(cnt + 5, st.clusters, red);
        block_add<4>(cnt + 6, st.prims, red);
#ifdef MFX_DIAG_OCCLUSION
        block_add<4>(cnt + 13, st.after_nodes, red);
        block_add<4>(cnt + 14, st.after_leaves, red);
#endif
    }
}

// ------------------------------------------------------------------------------------------------
// k_camera: a generation's first iteration, camera rays traced as packets (MFX_CAMERA_PACKETS). A
// 64-slot window is one 8x8 tile of one sample: its 64 camera rays are coherent, so
// the wave traces them together (packet_closest: uniform nodes through scalar loads, one lane per
// ray). Writes what k_extend writes for a camera ray: the hit point and HIT | FRESH | shade index,
// or MISS | FRESH. Flat scenes only (two-level scenes take k_extend).
// ------------------------------------------------------------------------------------------------
#ifndef MFX_CAM_WAVES
// k_camera's register budget: waves per SIMD (a packet walk is one chain of scalar loads per wave).
// Five (96 VGPRs, 56 B of spill) beat four (112 VGPRs, none): 4.30 -> 4.12 ms per C2 launch, Renault
// 6.46 -> 6.19 (interleaved A/B, profiles/r06/r06r_ab_camera_five_waves.txt): the walk waits on its
// loads more than it issues, and the fifth wave fills those waits
#define MFX_CAM_WAVES 5
#endif
// LIST: the instance for a listed trace (adaptive sampling): a window's tile is one scalar load, and with
// per-tile counts (WF_LIST_TILE_N) so is its count; a window past the tile's share has no active lane
// CUTS: the packets start from their tile's cut (WfParams::cuts) instead of the root; the instance without
// holds none of it
// ENV: the instances for a sky: a camera ray's miss stores the texel of its direction in the slot's word of
// P.env_rec (no vertex before it). A tile whose cut is empty still makes no ray and walks nothing, but its lanes
// derive their key, draws and direction for the texel, unless the map is one texel (id 0 whatever the direction).
template <bool STATS, int LIST = WF_LIST_NONE, bool CUTS = false, bool ENV = false>
__global__ void __launch_bounds__(256, MFX_CAM_WAVES) k_camera(WfParams P) {
    extern __shared__ int lds_all[];
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    uint64_t* stm = (uint64_t*)lds_all + wave * P.stack_size;  // per wave: stack masks, then nodes
    int* stk = (int*)((uint64_t*)lds_all + 4 * P.stack_size) + wave * P.stack_size;
    uint32_t* red = (uint32_t*)((int*)((uint64_t*)lds_all + 4 * P.stack_size) + 4 * P.stack_size);
    // the camera in LDS (read per window), not held in scalar registers through the packet walk
    MfxCamera* cam_lds = (MfxCamera*)(red + 16);
    if (threadIdx.x < sizeof(MfxCamera) / 8) ((double*)cam_lds)[threadIdx.x] = ((const double*)P.cam_dev)[threadIdx.x];
    // the reference-leaf arrays too (as k_shadow): `nodes` and `slots` alone stay in scalar registers
    SceneRefs* refs_lds = (SceneRefs*)(cam_lds + 1);
    if (threadIdx.x == 64) *refs_lds = SceneRefs{(const int32_t*)P.refs_dev[0], (const uint8_t*)P.refs_dev[1]};
    __syncthreads();
    const SceneView S{P.nodes, P.slots, nullptr, nullptr, P.inst, nullptr, 0, nullptr, 0, refs_lds};
    const int shard_size = P.pool / WF_SHARDS;
    Scanner sc{};
    sc.shard = blockIdx.x & (WF_SHARDS - 1);
    uint32_t c_primary = 0;
    Stats st{0, 0, 0};
    uint32_t pk_nodes = 0, pk_slots = 0;  // STATS: the wave's own node and slot fetches (every lane counts them)
    uint32_t pk_cuts = 0;                 // and, CUTS, its cut-entry fetches
#if MFX_DIAG_STAMPS == 3
    // the wave's cycles per phase (window scan, camera ray, node steps, leaf tests, result writes) and
    // its node steps and leaf visits (scripts/camera_phases.py); the shipped build has none of it
    uint64_t ph[4] = {0, 0, 0, 0}, t_scan = 0, t_gen = 0, t_out = 0, t_last = stamp();
#define CAM_MARK(acc)                  \
    do {                               \
        const uint64_t _t = stamp();   \
        (acc) += _t - t_last;          \
        t_last = _t;                   \
    } while (0)
#else
#define CAM_MARK(acc) \
    do {              \
    } while (0)
#endif
    // Every slot is FREE in a generation's first iteration (wf_trace zeroes the state words), so the
    // windows are taken without reading them, and a window is one 8x8 tile of one sample: its
    // (sample, tile) come from one wave-uniform path_pixel (scalar arithmetic), the lanes' pixels by
    // offset (the same x, y, sample path_pixel gives each slot; r06: the per-lane 32-bit divisions and
    // state loads were the window scan's 12 % of k_camera's wave time, scripts/latency_roof.py)
    while (sc.window<false>(P.ctl + WF_CTL_EXT, P.chunk, shard_size, P.state, nullptr, P.ctl + WF_CTL_CLOSED_EXT)) {
        const int jw = __builtin_amdgcn_readfirstlane(sc.win_next);
        sc.win_next += 64;
        const int j = jw + lane;
        int x = 0, y = 0;
        int64_t smp = 0;
        path_pixel<LIST>(P, P.path_base + jw, x, y, smp);  // the window's first slot: its tile's corner
        // the tile's row of the cut table (wave-uniform; read only by a window with an active lane)
        const MfxCutEntry* row = nullptr;
        if (CUTS)
            row = P.cuts + (size_t)__builtin_amdgcn_readfirstlane((y >> 3) * ((P.width + 7) >> 3) + (x >> 3)) * (size_t)P.cut_cap;
        x += lane & 7;
        y += lane >> 3;
        // edge-tile padding starts no path
        const bool act = j < P.total && x < P.width && y < P.height;
        if (!__any(act)) continue;
        CAM_MARK(t_scan);
        // A tile whose cut is empty: its widened pyramid misses every box, so every camera ray of the window
        // misses whatever its jitter; the miss needs no key, no draw and no ray (one scalar load decides,
        // the first the walk would issue)
        // (wave-uniform: the packet below finds no lane and returns, and the lanes write their miss)
        const bool seen = !(CUTS && MFX_CUT_EMPTY_SKIP) || row->code != MFX_CUT_END;
        if (act && !seen) c_primary++;
        DV o = dv(0, 0, 0), d = dv(0, 0, 1);
        const bool aim = seen || (ENV && P.env_size > 1);  // (without ENV: seen)
        if (act && aim) {  // PixelIntegrator.Sample (Integrators.fs:167-169) + GetRay (Camera.fs:134-139)
            const int64_t pixel = (int64_t)x * P.height + y;  // Color[w,h] x-major
            const int64_t gsample = path_gsample<LIST>(P, smp);
            const uint64_t key = path_key(P.seed, (uint64_t)pixel, (uint64_t)gsample);
            uint32_t rn = 0;
            const double u = ((double)x + rng_next(key, rn)) / (double)P.width;
            const double v = ((double)y + rng_next(key, rn)) / (double)P.height;
            const MfxCamera& CAM = *cam_lds;
            const DV target = vadd(vadd(ld3(CAM.topleft), vmul(ld3(CAM.right), u)), vmul(ld3(CAM.down), v));
            o = ld3(CAM.position);
            d = vnormalize(vsub(target, o));
            if (!ENV || seen) c_primary++;
        }
        Best B;
#if MFX_DIAG_STAMPS == 3
        CAM_MARK(t_gen);
        packet_closest<STATS, true, CUTS>(S, act && seen, o, d, 99999999., B, stk, stm, st, pk_nodes, pk_slots, ph, row, P.cut_cap, &pk_cuts);
        t_last = stamp();
#else
        packet_closest<STATS, false, CUTS>(S, act && seen, o, d, 99999999., B, stk, stm, st, pk_nodes, pk_slots, nullptr, row, P.cut_cap,
                                           &pk_cuts);  // Integrators.fs:108
#endif
        if (act) {
            if (B.found) {
                const DV hp = vadd(o, vmul(d, B.t));  // Ray.PointAtParameter (Ray.fs:8-9)
                P.ox[j] = hp.x; P.oy[j] = hp.y; P.oz[j] = hp.z;
                P.state[j] = ((B.info & MFX_INFO_SHADE_MASK) << WF_SHADE_SHIFT) | WF_HIT | WF_FRESH;
            } else {
                P.state[j] = WF_MISS | WF_FRESH;
                if constexpr (ENV) P.env_rec[j] = mfx_env_texel(d.x, d.y, d.z, P.env_size);
            }
        }
        CAM_MARK(t_out);
    }
#undef CAM_MARK
    unsigned long long* cnt = P.counters + WF_NCTR * (blockIdx.x & (WF_SHARDS - 1));
    block_add<4>(cnt + 0, c_primary, red);
#if MFX_DIAG_STAMPS == 3
    if (lane == 0) {  // (MFX_DIAG_ITER prints counters 10..17 as "stamps ... outer ... node ... scan shade")
        atomicAdd(cnt + 10, (unsigned long long)t_scan);
        atomicAdd(cnt + 11, (unsigned long long)t_gen);
        atomicAdd(cnt + 12, (unsigned long long)ph[0]);
        atomicAdd(cnt + 13, (unsigned long long)ph[1]);
        atomicAdd(cnt + 14, (unsigned long long)t_out);
        atomicAdd(cnt + 15, (unsigned long long)ph[2]);
        atomicAdd(cnt + 16, (unsigned long long)ph[3]);
    }
#endif
    if (STATS) {
        block_add<4>(cnt + 4, st.nodes, red);
        block_add<4>(cnt + 5, st.clusters, red);
        block_add<4>(cnt + 6, st.prims, red);
        // packet fetches, once per wave (lane 0's count): mfx_ray_counts out[10], out[11]
        block_add<4>(cnt + 10, lane == 0 ? pk_nodes : 0u, red);
        block_add<4>(cnt + 11, lane == 0 ? pk_slots : 0u, red);
#if MFX_DIAG_STAMPS != 3
        // and the cut entries the wave read (32 B each): out[12]; not part of the fetch index above
        if (CUTS) block_add<4>(cnt + 12, lane == 0 ? pk_cuts : 0u, red);
#endif
    }
}

// the fields path_pixel and path_key read, in k_shadow's LDS (after its array pointers): a shading
// vertex derives its path's key from the slot, and these are not held in scalar registers through
// the traversal loop
// (a trace has a band or a tile list, never both: the list pointer takes the band's two words, so the
// block is the size it was and k_shadow's LDS footprint does not move)
struct PixParams {
    int64_t path_base, base_q, base_smp, sample_base;
    uint64_t seed;
    int32_t width, height;
    union {
        struct { int32_t band_index, band_count; };
        const int32_t* tiles;  // ntiles > 0
    };
    // (a per-tile listed trace, WF_LIST_TILE_N, is unpartitioned: its counts and their bound take the
    // partition's words, path_gsample reads neither)
    union {
        struct { int32_t band_rows, part_index; };
        const int32_t* tile_n;
    };
    union {
        int32_t part_count;
        int32_t list_max;
    };
    int32_t ntiles;
};
static_assert(sizeof(PixParams) == 72, "PixParams: k_shadow's LDS layout");
// k_shadow's textured instances keep these in LDS after the scene references
struct TxShd {
    const double* uvrec;
    const int32_t* ptex;
    const MfxTexDesc* desc;
    uint32_t* vtex;
};
// k_shadow's SN twins keep the normal tables in LDS after TxShd's place (after the scene references without TX)
static_assert(sizeof(MfxSnTables) == 16, "SnShd: 16 B of k_shadow's LDS");
// k_shadow's array pointers in its LDS (after the light)
struct ShdPtrs {
    double *ox, *oy, *oz, *dx, *dy, *dz, *vei, *vls;
    WfMat* vmat;
    uint32_t* rn;
    int32_t* depth;
    const MfxShade* shade;
    int32_t* fstate;
    const int32_t* qslot;
    double *nox, *noy, *noz, *ndx, *ndy, *ndz;
    uint32_t* nrn;
    int32_t *ndepth, *nstate, *nslot;
    unsigned long long* ncount;
    unsigned long long *ctl, *counters;
    int32_t* state;
    const unsigned long long* qcount;
};

// ------------------------------------------------------------------------------------------------
// k_shadow: shade HIT slots (listed at scan time), trace the vertex's shadow ray, continue or finish
// ------------------------------------------------------------------------------------------------
// Q: the instance that reads a ray queue (P.qslot) or writes the next one (P.ncount), MFX_RAY_QUEUE
// LIST: the instances for a listed trace (adaptive sampling: path_pixel's tile list, and WF_LIST_TILE_N's counts)
// NF: the node format, as k_extend's
// ML: the instances for several lights (mfx_create_lights, N >= 2): the pick draw and the picked light's
// gather in sample_vertex, the light's index in bits 24..29 of the pending flag word (free: the lit mask
// ends at bit 23), and a lit vertex's index written to P.vlt beside its cs and solid. The table pointer,
// the count and vlt lie in the LDS block the one light's copy takes otherwise (MlPtrs), so the LDS
// footprint, and with it the blocks per CU, are the one-light instance's. A template parameter, not a
// branch on the count: the one-light instances hold none of this (r04c: one run-time branch in the leaf
// test cost 1.8 to 4 %).
// TX: the instances for albedo textures (mfx_create_textured): after the shade record, the lane of a
// textured primitive loads its 64-B UV record and its texture's descriptor, computes the texel id of the
// hit point (mfx_texture.h) and stores it in P.vtex beside the vertex's material, all before the sampler
// runs, so the record is dead by then; an untextured primitive stores MFX_TEXEL_NONE. The table pointers
// lie in 32 B of LDS after the scene references (TxShd). A template parameter for ML's reason.
// SKY: the twins of the ML instances for a sampled sky (mfx_set_environment_sampled): the pick is over N + 1 and
// the lane whose pick is N samples the map (sample_vertex), stores the texel's id in P.vsky at shading time,
// sends its shadow ray to the extension ray's far bound, and records cs and pdf_v where cs and solid go and N
// as the light index. The table, the plane and the map's size lie in the light's LDS block after MlPtrs
// (SkyPtrs), so the LDS footprint is the ML instance's.
// SN: the twins for smooth shading (mfx_set_normals) of every 4-wave instance without counters, in each (ML, TX) state
// and of the SKY twins: after the shade record (and TX's block) the lane of a smooth primitive loads its flag and its
// 96-B normal record and replaces nm by the shading normal of the hit point (mfx_normals.h), before the sampler runs,
// so the record is dead by then. The table pointers lie in 16 B of LDS after TxShd's place. A template parameter for
// ML's reason.
template <bool STATS, bool SPILL, int WAVES, int SK, bool Q, int LIST = WF_LIST_NONE, int NF = MFX_NF_ANY, bool ML = false,
          bool TX = false, bool SKY = false, bool SN = false>
__global__ void __launch_bounds__(256, WAVES) k_shadow(WfParams P) {
    constexpr bool INST = SK == WF_SK_INST, SLDS = SK == WF_SK_SLDS;
    extern __shared__ int lds_all[];
#if MFX_NODE_F16
    const TopNodes tn{(const float4*)lds_all, P.ntop_shd, P.nodes_h};
#else
    const TopNodes tn{(const float4*)lds_all, P.ntop_shd};
#endif
    MfxInstance* inst_lds = (MfxInstance*)(lds_all + P.ntop_shd * 32);
    int4* slot_lds = (int4*)(inst_lds + (INST ? P.ninst_lds : 0));
    const int nslot = SLDS ? P.nslot_shd : 0;
    int* lds = (int*)(slot_lds + 5 * nslot);
    uint8_t* pend_base = (uint8_t*)(lds + 4 * P.stack_lds_shd * 64);
    uint32_t* red = (uint32_t*)(pend_base + 4 * PendShd::BYTES);
    // the light, after the four waves' shade lists (8-B aligned): copied before load_top_nodes' barrier
    MfxLight* light_lds = (MfxLight*)((int*)(red + 16) + 4 * 2 * WF_SHD_LIST);
    if constexpr (ML) {
        if constexpr (SKY) {
            if (threadIdx.x == 3) *(SkyPtrs*)light_lds = SkyPtrs{MlPtrs{P.lights, P.vlt, P.nlights}, P.sky_tab, P.vsky, P.env_size};
        } else {
            if (threadIdx.x == 3) *(MlPtrs*)light_lds = MlPtrs{P.lights, P.vlt, P.nlights};
        }
    } else {
        if (threadIdx.x < sizeof(MfxLight) / 8)
            ((double*)light_lds)[threadIdx.x] = ((const double*)P.light_dev)[threadIdx.x];
    }
    if (threadIdx.x == 0)
        *(ShdPtrs*)(light_lds + 1) = ShdPtrs{P.ox, P.oy, P.oz, P.dx, P.dy, P.dz, P.vei, P.vls, P.vmat, P.rn, P.depth,
                                            P.shade, P.fstate, P.qslot, P.nox, P.noy, P.noz, P.ndx, P.ndy, P.ndz,
                                            P.nrn, P.ndepth, P.nstate, P.nslot, P.ncount, P.ctl, P.counters, P.state,
                                            P.qcount};
    SceneRefs* refs_lds = (SceneRefs*)((PixParams*)((ShdPtrs*)(light_lds + 1) + 1) + 1);
    if (threadIdx.x == 2)  // (from device memory: kernel arguments beside `nodes` would be loaded with it)
        *refs_lds = SceneRefs{(const int32_t*)P.refs_dev[0], (const uint8_t*)P.refs_dev[1]};
    [[maybe_unused]] const TxShd& X = *(const TxShd*)(refs_lds + 1);  // TX: after the scene references
    if constexpr (TX) {
        if (threadIdx.x == 4) *(TxShd*)(refs_lds + 1) = TxShd{P.tx.uvrec, P.tx.ptex, P.tx.desc, P.vtex};
    }
    // SN: after TxShd (TX), or in its place
    [[maybe_unused]] const MfxSnTables& NT = *(const MfxSnTables*)((const char*)(refs_lds + 1) + (TX ? sizeof(TxShd) : 0));
    if constexpr (SN) {
        if (threadIdx.x == 5) *(MfxSnTables*)((char*)(refs_lds + 1) + (TX ? sizeof(TxShd) : 0)) = P.sn;
    }
    if (threadIdx.x == 1) {
        PixParams px;
        px.path_base = P.path_base; px.base_q = P.base_q; px.base_smp = P.base_smp; px.sample_base = P.sample_base;
        px.seed = P.seed; px.width = P.width; px.height = P.height;
        if (LIST) {
            px.tiles = P.tiles;
        } else {
            px.band_index = P.band_index; px.band_count = P.band_count;
        }
        if (LIST == WF_LIST_TILE_N) {
            px.tile_n = P.tile_n; px.list_max = P.list_max;
        } else {
            px.band_rows = P.band_rows; px.part_index = P.part_index; px.part_count = P.part_count;
        }
        px.ntiles = LIST ? P.ntiles : 0;
        *(PixParams*)((ShdPtrs*)(light_lds + 1) + 1) = px;
    }
#if MFX_NODE_F16
    if (NF == MFX_NF_H || (NF == MFX_NF_ANY && P.nodes_h)) load_top_nodes_h((float4*)lds_all, P.nodes_h, P.ntop_shd);
    else
#endif
        load_top_nodes((float4*)lds_all, P.nodes, P.ntop_shd);
    if (INST) load_inst_lds(inst_lds, P.inst, P.ninst_lds);
    if (SLDS) load_slots_lds(slot_lds, P.slots, nslot);
    const MfxLight& LT = *light_lds;
    [[maybe_unused]] const MlPtrs& M = *(const MlPtrs*)light_lds;  // ML: the same block holds these instead
    [[maybe_unused]] const SkyPtrs& K = *(const SkyPtrs*)light_lds;  // SKY: and these after them
    // the pool's and the queues' array pointers, read from LDS where they are used (the shading batch,
    // the records) instead of held in scalar registers through the traversal loop
    const ShdPtrs& C = *(const ShdPtrs*)(light_lds + 1);
    const PixParams& PX = *(const PixParams*)((const ShdPtrs*)(light_lds + 1) + 1);
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    using Stack = typename std::conditional<SPILL, SpillStack, LdsStack>::type;
    const Stack stack = make_stack<SPILL>(lds + wave * P.stack_lds_shd * 64 + lane, P, P.stack_lds_shd);
    const PendShd pd(pend_base + wave * PendShd::BYTES);
    const SceneView S{P.nodes, P.slots, nullptr, nullptr, P.inst, inst_lds, INST ? P.ninst_lds : 0, slot_lds, nslot, refs_lds, P.tslack};
    const int shard_size = P.pool / WF_SHARDS;

    int* shl = (int*)(red + 16) + wave * 2 * WF_SHD_LIST;  // shade list: [0,128) path slots, [128,256) shade indices
    Scanner sc{};
    sc.shard = blockIdx.x & (WF_SHARDS - 1);
    int nshade = 0;      // wave-uniform: hits listed for shading
    int pend_lo = 0, pend_hi = 0;
    bool active = false;
    int s = 0;
    Trav T{};
    double scs = 0.0, ssolid = 0.0;  // the operands of this vertex's direct term a_v (cs, solid; gray light: a_v, -)
    int vflag = 0;  // the lane's vertex: bit 0 the path continues, bit 1 lightable (cos_o < 0),
                    // bits 2..5 its index v, bits 8.. the path's lit mask so far (PD_* below)
    uint32_t c_shadow = 0;
    Stats st{0, 0, 0};
#ifdef MFX_DIAG_OCCLUSION
    uint32_t dg_occ = 0, dg_occ_nodes = 0, dg_occ_leaves = 0;
#endif
    constexpr bool DG = MFX_DIAG_STAMPS == 2;
    DiagAcc dg{};
    if (DG) dg.last = stamp();

    while (true) {
        bool idle = !active;
        uint64_t m = __ballot(idle);
        while (m != 0) {
            if (pend_lo == pend_hi) {
                // list hits from as many windows as it takes (state words only): a camera ray's miss
                // frees its slot (TraceRay returns black, Integrators.fs:137), a later miss finishes
                // its path with the radiance already in the slot
                while (nshade < 64 && sc.window(C.ctl + WF_CTL_SHD, P.chunk_shd, shard_size, C.state, Q ? C.qcount : nullptr, C.ctl + WF_CTL_CLOSED_SHD)) {
                    if (DG) dg.windows++;
                    const int j = sc.win_next + lane;
                    const int sj = sc.word();
                    const int sv = sj & WF_STATE_MASK;
                    const bool hit = (sv & ~WF_FRESH) == WF_HIT;
                    // a pool slot's miss stays as k_extend wrote it: k_resolve takes MISS as finished
                    // (its state word holds the lit vertices) and a camera ray's MISS | FRESH as black
                    if (Q && C.qslot && sv == WF_MISS) {  // a queue entry: its slot finishes (no lit vertex: stays unfinished)
                        const int dw = C.depth[j];
                        if (dw >> WF_LIT_SHIFT) C.fstate[C.qslot[j]] = WF_DONE | ((dw >> WF_LIT_SHIFT) << WF_SHADE_SHIFT);
                    }
                    const uint64_t hm = __ballot(hit);
                    if (hit) {
                        const int r = nshade + __popcll(hm & lanes_below());
                        // sign bit: first vertex; lit_in_hit: the lit mask in bits 28..30 (slots < 2^28)
                        const bool lh = P.lit_in_hit && !(Q && C.qslot);
                        shl[r] = (sv & WF_FRESH) ? (j | (int)0x80000000) : (lh ? j | (int)(((unsigned)sj >> 29) << 28) : j);
                        shl[WF_SHD_LIST + r] = (int)(((unsigned)sj >> WF_SHADE_SHIFT) & (lh ? 0x1ffffffu : 0x0fffffffu));
                    }
                    nshade += __popcll(hm);
                    sc.advance(C.state);
                }
                wave_lds_sync();
                DIAG_MARK(dg, scan, DG);
                if (nshade == 0) break;  // every chunk scanned, every hit shaded, every ray handed out
                // ---- shade up to 64 listed hits with all lanes: one vertex of PathIntegrator.TraceRay
                //      (Integrators.fs:109-136) each; every one yields a shadow ray ----
                const int cnt = nshade < 64 ? nshade : 64;
                const bool own = lane < cnt;
                int j = 0, mat = 0, jr = 0, dw = 0;
                bool first = false;
                DV hp = dv(0, 0, 0), nm = dv(0, 0, 0);
                uint64_t key = 0;
                uint32_t rn = 0;
                if (own) {
                    j = shl[lane] & WF_ENTRY_SLOT;
                    first = shl[lane] < 0;  // draws 2, depth max_depth, no lit vertex: implicit
                    const int slot = shl[WF_SHD_LIST + lane];
                    jr = (Q && C.qslot) ? C.qslot[j] : j;
                    // remaining depth | lit mask << 8: in place with lit_in_hit, the iteration's and
                    // the mask the state word carried; otherwise the depth word
                    dw = first ? P.max_depth
                               : ((P.lit_in_hit && !(Q && C.qslot))
                                      ? (P.max_depth - P.iter) | ((((unsigned)shl[lane] >> 28) & 7) << WF_LIT_SHIFT)
                                      : C.depth[j]);
                    hp = dv(C.ox[j], C.oy[j], C.oz[j]);
                    const MfxShade sh = C.shade[slot];
                    if ((sh.prim_kind & 3) == MFX_KIND_SPHERE) nm = vnormalize(vsub(hp, ld3(sh.n)));  // Sphere.fs:39-43
                    else nm = ld3(sh.n);
                    mat = sh.material;
                    if constexpr (TX) {  // the vertex's texel id (v: this vertex's index, as below)
                        const int prim = sh.prim_kind >> 2;
                        const int tex = X.ptex[prim];
                        uint32_t id = MFX_TEXEL_NONE;
                        if (tex >= 0) {
                            const double* r = X.uvrec + (int64_t)MFX_UV_RECORD_DOUBLES * prim;
                            const double h3[3] = {hp.x, hp.y, hp.z};
                            const double rec[8] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
                            double tu, tv;
                            mfx_tx_uv(rec, h3, tu, tv);
                            id = mfx_tx_texel(X.desc[tex], tu, tv);
                        }
                        X.vtex[(int64_t)(P.max_depth - (dw & 0xff)) * P.vstride + jr] = id;
                    }
                    if constexpr (SN) {  // the shading normal of a smooth primitive (a sphere's flag is 0)
                        const int prim = sh.prim_kind >> 2;
                        if (NT.flag[prim]) {
                            const double* r = NT.rec + (int64_t)MFX_SN_RECORD_DOUBLES * prim;
                            const double rec[12] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11]};
                            const double h3[3] = {hp.x, hp.y, hp.z}, g3[3] = {nm.x, nm.y, nm.z};
                            double s3[3];
                            mfx_sn_shade(rec, h3, g3, s3);
                            nm = dv(s3[0], s3[1], s3[2]);
                        }
                    }
                    // the key k_extend derived for the path's camera ray (same expressions), derived
                    // again at every vertex from the path's slot instead of stored (8 B written at the
                    // first vertex and read at every later one: C2 +0.5 %, r05m)
                    {
                        int x, y;
                        int64_t smp;
                        path_pixel<LIST>(PX, PX.path_base + jr, x, y, smp);
                        const int64_t pixel = (int64_t)x * PX.height + y;
                        key = path_key(PX.seed, (uint64_t)pixel, (uint64_t)path_gsample<LIST>(PX, smp));
                    }
                    rn = first ? 2u : C.rn[j];  // the camera ray drew u, v
                }
                // the depth -1 query's result is discarded (Integrators.fs:109): never traced
                const bool cn = own && (dw & 0xff) - 1 >= 0;
                // MFX_RAY_QUEUE: a continuing path's entry in the next queue, in the range of its
                // source shard (capacity: that shard's size), one atomic per shard in the batch
                int qi = 0;
                if (Q && C.ncount) {
                    const int g = cn ? j / shard_size : 0;
                    uint64_t rem = __ballot(cn);
                    while (rem) {
                        const int gl = __shfl(g, __builtin_ctzll(rem));
                        const uint64_t gm = __ballot(cn && g == gl);
                        unsigned long long base = 0;
                        if (lane == __builtin_ctzll(gm)) base = atomicAdd(C.ncount + gl * WF_HS, (unsigned long long)__popcll(gm));
                        base = __shfl(base, __builtin_ctzll(gm));
                        if (cn && g == gl) qi = gl * shard_size + (int)base + __popcll(gm & lanes_below());
                        rem &= ~gm;
                    }
                }
                wave_lds_sync();  // every owner has read its shl entries: shl[0, 64) is the sampler's scratch
                const VertexSample V = sample_vertex<ML, SKY>(LT, own, hp, nm, key, rn, shl, ML ? M.lights : nullptr, ML ? M.nlights : 1,
                                                              SKY ? K.tab : nullptr, SKY ? K.size : 0);
                if (own) {
                    const DV wi = V.wi, unit = V.unit;
                    const double dist = V.dist, cs = V.cs, solid = V.solid;
                    const bool lightable = V.lightable;
                    const int v = P.max_depth - (dw & 0xff);          // this vertex's index
                    // the operands of col = INVPI * a * ei * TwoPi (Material.fs:36), c_v (k_resolve)
                    C.vei[v * P.vstride + jr] = V.ei;
                    C.vmat[v * P.vstride + jr] = (WfMat)mat;
                    if (Q && cn && C.ncount) {  // the next vertex's ray in the next queue (its depth word and
                                           // state are written after the shadow ray)
                        C.nox[qi] = hp.x; C.noy[qi] = hp.y; C.noz[qi] = hp.z;
                        C.ndx[qi] = wi.x; C.ndy[qi] = wi.y; C.ndz[qi] = wi.z;
                        C.nrn[qi] = rn;
                        C.nslot[qi] = jr;
                    } else if (cn) {  // what the next vertex reads, in place
                        C.rn[j] = rn;
                        C.dx[j] = wi.x; C.dy[j] = wi.y; C.dz[j] = wi.z;
                    }
                    // shadow bvh.Hit(Ray(hit.point, unit), 1e-6, dist - 1e-6) (Integrators.fs:44)
                    pd.slot[lane] = (Q && cn && C.ncount) ? qi : j;
                    pd.flag[lane] = (cn ? 1 : 0) | (lightable ? 2 : 0) | (v << 2) | (dw & ~0xff) | (ML ? V.light << 24 : 0);
                    pd.v[0 * 64 + lane] = unit.x; pd.v[1 * 64 + lane] = unit.y; pd.v[2 * 64 + lane] = unit.z;
                    if constexpr (SKY) {  // a sky vertex: its texel, and the query runs to the far bound itself
                        const bool sv = V.light == M.nlights;
                        if (sv) K.vsky[(int64_t)v * P.vstride + jr] = V.texel;
                        pd.v[3 * 64 + lane] = sv ? MFX_ENV_FAR : dist - 1e-6;
                    } else {
                        pd.v[3 * 64 + lane] = dist - 1e-6;
                    }
                    // a gray light: the direct term itself, (cs * (solid * I)) / pdf_li (Integrators.fs:52,
                    // Light.fs:52-53), the expression k_resolve evaluates per channel otherwise
                    // (ML: never gray; k_resolve has every light's intensity and pdf)
                    pd.v[4 * 64 + lane] = (!ML && P.gray_light) ? (cs * (solid * LT.color[0])) / LT.pdf : cs;
                    pd.v[5 * 64 + lane] = solid;
                    c_shadow++;
                }
                // the unshaded rest of the list moves to its front
                const int rest = nshade - cnt;
                int mv_j = 0, mv_s = 0;
                if (lane < rest) { mv_j = shl[cnt + lane]; mv_s = shl[WF_SHD_LIST + cnt + lane]; }
                wave_lds_sync();
                if (lane < rest) { shl[lane] = mv_j; shl[WF_SHD_LIST + lane] = mv_s; }
                wave_lds_sync();
                nshade = rest;
                pend_lo = 0;
                pend_hi = cnt;
                DIAG_MARK(dg, shade, DG);
                continue;
            }
            const int avail = pend_hi - pend_lo;
            const int rank = __popcll(m & lanes_below());
            if (idle && rank < avail) {
                const int e = pend_lo + rank;
                s = pd.slot[e];
                vflag = pd.flag[e];
                scs = pd.v[4 * 64 + e];
                ssolid = (!ML && P.gray_light) ? 0.0 : pd.v[5 * 64 + e];
                // origin = the hit point k_extend stored (a cache hit: the shading just read it), or
                // its copy in the next queue. That copy (nox..noz, and nslot below) was stored in this
                // kernel by the lane that shaded the hit, which may be another lane of this wave: the
                // read is ordered after that store by the wave_lds_sync() calls that end the shading
                // batch (release / acquire fences at wavefront scope cover global memory as well as
                // LDS), and one wave's vector memory operations reach its L1 in order.
                const bool nq = Q && (vflag & 1) && C.ncount;
                const double* hx = nq ? C.nox : C.ox;
                const double* hy = nq ? C.noy : C.oy;
                const double* hz = nq ? C.noz : C.oz;
                trav_begin(T, S, dv(hx[s], hy[s], hz[s]), dv(pd.v[0 * 64 + e], pd.v[1 * 64 + e], pd.v[2 * 64 + e]),
                           pd.v[3 * 64 + e]);

#ifdef MFX_DIAG_OCCLUSION
                T.n0 = st.nodes;
                T.l0 = st.clusters;
#endif
                idle = false;
                active = true;
            }
            const int pm = __popcll(m);
            pend_lo += pm < avail ? pm : avail;
            m = __ballot(idle);
        }
        if (!__any(active)) break;
        DIAG_MARK(dg, fetch, DG);
        if (DG) dg.outer++;
        bool fin = false;
#ifdef MFX_DIAG_SKIP_SHADOW_TRAV
        if (active) {
            T.B.found = false;
            fin = true;
        }
#else
        if (active) fin = trav_step<true, STATS, INST, SLDS, NF>(T, S, stack, tn, st, dg, DG);
#endif
        DIAG_MARK(dg, leaf, DG);
        if (fin) {
#ifdef MFX_DIAG_OCCLUSION  // STATS build: occluded shadow rays and their node / cluster visits
            if (STATS && T.B.found) {
                dg_occ++;
                dg_occ_nodes += st.nodes - T.n0;
                dg_occ_leaves += st.clusters - T.l0;
            }
#endif
            const int v = (vflag >> 2) & 15;
            int mask = (vflag >> WF_LIT_SHIFT) & 0xffff;
            // MFX_RAY_QUEUE: s is the path's next-queue entry (it continues) or its entry in this
            // iteration's queue; its slot is read back where the slot's records are written
            const bool nq = Q && cont0(vflag) && C.ncount;
            if (!T.B.found && (vflag & 2)) {  // unoccluded: record the operands of its direct term a_v
                const int jr = nq ? C.nslot[s] : ((Q && C.qslot) ? C.qslot[s] : s);
                double* vl = C.vls + (int64_t)(2 * v) * P.vstride + jr;
                vl[0] = scs;
                if (ML || !P.gray_light) vl[P.vstride] = ssolid;
                if constexpr (ML) M.vlt[(int64_t)v * P.vstride + jr] = (uint8_t)((vflag >> 24) & (WF_MAX_LIGHTS - 1));
                mask |= 1 << v;
            }
            const bool cont = (vflag & 1) != 0;
            // continue with the next vertex's remaining depth; or finished: k_resolve folds the
            // recorded vertices (none lit: nothing to add, FREE)
            const int dwn = ((P.max_depth - v - 1) & 0xff) | (mask << WF_LIT_SHIFT);
            // in place, NEED_EXT carries the lit mask for k_extend's pending entries (lit_in_entry)
            const int need = WF_NEED_EXT | (nq ? 0 : mask << WF_SHADE_SHIFT);
            if (nq) {
                C.ndepth[s] = dwn;
                C.nstate[s] = need;
            } else if (Q && (C.ncount || C.qslot)) {  // finished; the pool's slot keeps its final words
                if (mask) C.fstate[C.qslot ? C.qslot[s] : s] = WF_DONE | (mask << WF_SHADE_SHIFT);
            } else {
                if (cont && !P.lit_in_hit) C.depth[s] = dwn;
                C.state[s] = cont ? need : (mask ? WF_DONE | (mask << WF_SHADE_SHIFT) : WF_FREE);
            }
            active = false;
        }
        DIAG_MARK(dg, fin, DG);
    }
    unsigned long long* cnt = C.counters + WF_NCTR * (blockIdx.x & (WF_SHARDS - 1));
    block_add<4>(cnt + 2, c_shadow, red);
    if (DG) block_add<4>(cnt + 15, dg.node_iters, red);
    if (DG && lane == 0) {
        atomicAdd(cnt + 10, (unsigned long long)dg.fetch);
        atomicAdd(cnt + 11, (unsigned long long)dg.node);
        atomicAdd(cnt + 12, (unsigned long long)dg.leaf);
        atomicAdd(cnt + 13, (unsigned long long)dg.fin);
        atomicAdd(cnt + 14, (unsigned long long)dg.outer);
        atomicAdd(cnt + 16, (unsigned long long)dg.scan);
        atomicAdd(cnt + 17, (unsigned long long)dg.shade);
        atomicAdd(cnt + 3, (unsigned long long)dg.lat);
    }
    if (STATS) {
        block_add<4>(cnt + 7, st.nodes, red);
#ifdef MFX_DIAG_OCCLUSION
        block_add<4>(cnt + 10, dg_occ, red);
        block_add<4>(cnt + 11, dg_occ_nodes, red);
        block_add<4>(cnt + 12, dg_occ_leaves, red);
#endif
        block_add<4>(cnt + 8, st.clusters, red);
        block_add<4>(cnt + 9, st.prims, red);
    }
}

#ifndef WF_RES_VERTS
#define WF_RES_VERTS 4  // vertices k_resolve loads in one round (max_depth 3 paths); deeper ones in a loop
#endif
#ifndef WF_RES_MAT_LDS
#define WF_RES_MAT_LDS 256  // materials whose albedo k_resolve keeps in LDS (more: read from global memory)
#endif
#ifndef WF_RES_SAMPLES
#define WF_RES_SAMPLES 1  // samples of a pixel whose path records k_resolve loads together
#endif

// One path's vertex records as loaded by k_resolve: for the first WF_RES_VERTS vertices up to its
// deepest lit one, ei and the material; cs and solid for the lit ones. Loaded in one round of
// independent loads (the state word came in the round before), so a path costs two
// dependent memory round trips instead of one per vertex and field.
struct PathRec {
    int mask;  // lit-vertex mask (0: black path, or not a finished path of this generation)
    double ei[WF_RES_VERTS], cs[WF_RES_VERTS], so[WF_RES_VERTS];
    int mat[WF_RES_VERTS];
    int lt[WF_RES_VERTS];  // ML: a lit vertex's light (P.vlt); the one-light instances never touch it
    uint32_t tx[WF_RES_VERTS];  // TX: the vertex's texel (MFX_TEXEL_NONE: untextured); the untextured instances never touch it
    uint32_t sky[WF_RES_VERTS];  // SKY: a lit vertex's sky texel id (P.vsky; read only where lt is N); the others never touch it
};
// TX: the vertex's texel, gathered through its id (P.vtex); MFX_TEXEL_NONE stands for an untextured vertex
__device__ __forceinline__ uint32_t load_texel(const WfParams& P, int64_t at) {
    const uint32_t id = P.vtex[at];
    return id == MFX_TEXEL_NONE ? MFX_TEXEL_NONE : P.tx.texels[id];
}
// ENV: the records up to vertex etop (a path that ended in the sky folds every vertex before its miss, the
// unlit ones above its deepest lit one too; etop < 0: no vertex); without, up to the deepest lit vertex
template <bool ML, bool TX, bool ENV = false, bool SKY = false>
__device__ __forceinline__ void load_path(const WfParams& P, int64_t j, int mask, PathRec& R, int etop = -1) {
    R.mask = mask;
    if (ENV ? etop < 0 : mask == 0) return;
    const int top = ENV ? etop : 31 - __builtin_clz(mask);
#pragma unroll
    for (int v = 0; v < WF_RES_VERTS; ++v) {
        R.ei[v] = 0.0; R.cs[v] = 0.0; R.so[v] = 0.0; R.mat[v] = 0;
        if constexpr (ML) R.lt[v] = 0;
        if constexpr (TX) R.tx[v] = MFX_TEXEL_NONE;
        if constexpr (SKY) R.sky[v] = 0;
        if (v <= top) {
            R.ei[v] = P.vei[v * P.vstride + j];
            R.mat[v] = P.vmat[v * P.vstride + j];
            if constexpr (TX) R.tx[v] = load_texel(P, v * P.vstride + j);
            if ((mask >> v) & 1) {
                const double* vl = P.vls + (int64_t)(2 * v) * P.vstride + j;
                R.cs[v] = vl[0];  // (a gray light: a_v itself)
                if (ML || !P.gray_light) R.so[v] = vl[P.vstride];
                if constexpr (ML) R.lt[v] = P.vlt[v * P.vstride + j] & (WF_MAX_LIGHTS - 1);  // (the mask keeps the LDS read in bounds)
                // (the id k_shadow stored if this is a sky vertex; masked: the map read stays in bounds whatever the word)
                if constexpr (SKY) R.sky[v] = P.vsky[v * P.vstride + j] & MFX_ENV_ID_MASK;
            }
        }
    }
}
// The path's radiance: its vertices folded from the deepest lit one back to the camera, f starting
// as TraceRay below the deepest lit vertex (Color(), black):
//   c_v = col = TwoPi * (ei * (INVPI * a))            (Material.fs:36, the expression k_shadow had)
//   a_v = (cs * (solid * I)) / pdf_li, 0 if unlit     (Integrators.fs:52, Light.fs:52-53)
//   f  <- (a_v + f) * c_v                             (Integrators.fs:135-136, pdf = 1)
// ML (several lights): the lit vertex's light lt selects I and pdf_n from the kernel's LDS table
// lt_lds[light][4] = I[0..2], pdf_n; the same expression, one rounding per operation. Never gray.
// TX (albedo textures): the albedo is the material's times the vertex's texel, a[c] = al[c] * (byte_c / 255.0)
// (mfx_texture.h); a texel whose three bytes are 255, MFX_TEXEL_NONE among them, leaves it as it is, which
// is what the product gives (byte / 255.0 is exactly 1.0).
// SKY (a sampled sky): a lit vertex whose light is N, the sky, takes the radiance of texel `sky` of the map and
// pdf_v from `so`: a_v = ((cs * E[c]) * INVPI) / pdf_v.
template <bool ML, bool TX, bool SKY = false>
__device__ __forceinline__ void fold_vertex(const WfParams& P, bool lit, double ei, int mat, double cs, double so,
                                            const double* alb_lds, double& fx, double& fy, double& fz,
                                            const double* lt_lds, int lt, uint32_t texel, uint32_t sky = 0) {
    [[maybe_unused]] const MfxLight& LT = P.light;
    const double* al = mat < WF_RES_MAT_LDS ? alb_lds + 3 * mat : P.albedo + 3 * mat;
    double a0 = al[0], a1 = al[1], a2 = al[2];
    if constexpr (TX) {
        if ((texel & 0xffffffu) != 0xffffffu) {
            a0 = mfx_tx_albedo(a0, texel, 0);
            a1 = mfx_tx_albedo(a1, texel, 1);
            a2 = mfx_tx_albedo(a2, texel, 2);
        }
    }
    const double cx = TWOPI * (ei * (INVPI * a0));
    const double cy = TWOPI * (ei * (INVPI * a1));
    const double cz = TWOPI * (ei * (INVPI * a2));
    double ax = 0.0, ay = 0.0, az = 0.0;
    if constexpr (ML) {
        if (SKY && lit && lt == P.nlights) {
            const uint32_t n = (uint32_t)P.env_size * (uint32_t)P.env_size;
            const float* e = P.env_rgb + 3 * (size_t)(sky < n ? sky : 0);
            ax = ((cs * (double)e[0]) * INVPI) / so;
            ay = ((cs * (double)e[1]) * INVPI) / so;
            az = ((cs * (double)e[2]) * INVPI) / so;
        } else if (lit) {
            const double* L = lt_lds + 4 * lt;
            ax = (cs * (so * L[0])) / L[3];
            ay = (cs * (so * L[1])) / L[3];
            az = (cs * (so * L[2])) / L[3];
        }
    } else if (lit && P.gray_light) {  // cs holds a_v, recorded by k_shadow with the same expression
        ax = ay = az = cs;
    } else if (lit) {
        ax = (cs * (so * LT.color[0])) / LT.pdf;
        ay = (cs * (so * LT.color[1])) / LT.pdf;
        az = (cs * (so * LT.color[2])) / LT.pdf;
    }
    fx = (ax + fx) * cx;
    fy = (ay + fy) * cy;
    fz = (az + fz) * cz;
}
template <bool ML, bool TX, bool ENV = false, bool SKY = false>
__device__ __forceinline__ void fold_path(const WfParams& P, int64_t j, const PathRec& R, const double* alb_lds,
                                          double& fx, double& fy, double& fz, const double* lt_lds, int etop = -1) {
    const int top = ENV ? etop : 31 - __builtin_clz(R.mask);  // (ENV: f comes in as the sky's radiance, or black)
    // vertices deeper than the batched records (max_depth >= WF_RES_VERTS), read here
    for (int v = top; v >= WF_RES_VERTS; --v) {
        const bool lit = (R.mask >> v) & 1;
        const double* vl = P.vls + (int64_t)(2 * v) * P.vstride + j;
        uint32_t texel = MFX_TEXEL_NONE;
        if constexpr (TX) texel = load_texel(P, v * P.vstride + j);
        fold_vertex<ML, TX, SKY>(P, lit, P.vei[v * P.vstride + j], P.vmat[v * P.vstride + j], lit ? vl[0] : 0.0,
                                 lit ? vl[P.vstride] : 0.0, alb_lds, fx, fy, fz, lt_lds,
                                 (ML && lit) ? P.vlt[v * P.vstride + j] & (WF_MAX_LIGHTS - 1) : 0, texel,
                                 (SKY && lit) ? P.vsky[v * P.vstride + j] & MFX_ENV_ID_MASK : 0);
    }
    // the batched ones, indices known at compile time (the records stay in registers)
#pragma unroll
    for (int v = WF_RES_VERTS - 1; v >= 0; --v)
        if (v <= top)
            fold_vertex<ML, TX, SKY>(P, (R.mask >> v) & 1, R.ei[v], R.mat[v], R.cs[v], R.so[v], alb_lds, fx, fy, fz, lt_lds,
                                     ML ? R.lt[v] : 0, TX ? R.tx[v] : MFX_TEXEL_NONE, SKY ? R.sky[v] : 0);
}

// ------------------------------------------------------------------------------------------------
// k_resolve: after a generation, every pixel adds its finished paths' radiance in sample order
// (PixelIntegrator.Sample: color <- color + TraceRay(...), Integrators.fs:169). A path's radiance
// is its recorded vertices folded from the deepest lit one back to the camera: TraceRay returns
// (l / pdf_li + TraceRay(next)) * col / pdf (Integrators.fs:135-136; pdf = 1, so the division is
// exact), black below the last lit vertex, and l = 0 at an occluded or unlit one. One thread per
// tile-ordered pixel position q; for a fixed sample, consecutive q are consecutive slots, so the
// loads are coalesced. No atomics: one thread owns each pixel, generations are stream-ordered.
// The records of WF_RES_SAMPLES samples are loaded together (state words, which carry a finished
// path's lit mask, then vertex records: two rounds of independent loads), then folded and added in
// sample order.
// Render-ahead (P.film, the frames mode): the samples are one-sample render calls. Each adds its
// 1-spp image — 0.0 + its path, what a one-sample call's zeroed accumulator holds, 0.0 for a black
// one — to the film state in sample order (Film.AddSample, Film.fs:18-23: film + frame / 1.0),
// and with P.frames writes that call's RGBA8 frame (PostProcessAndToScreenBuffer of film /
// frameCount, Scene.fs:315-330; frameCount = count0 + the sample's index + 1): the FP64 operations
// film_post_kernel runs per call, in the same order, so every frame is that call's bytes. The film
// state (P.film) carries across a call's generations.
// ------------------------------------------------------------------------------------------------
// FRAMES: the render-ahead instance (P.film); the accumulator instance carries none of its code
// (with it, k_resolve took 99 VGPRs instead of 88, 4 waves per SIMD instead of 5, and twice the time)
// MODE: WF_RES_MOMENTS is the adaptive sampler's instance, of its own for the same reason. It maps a
// listed trace's tiles (P.ntiles > 0) and adds the luminance moments (P.mom): Y = (fx + fy) + fz and
// Y * Y per path, in sample order beside the accumulator (a black path's Y is 0: nothing to add).
#define WF_RES_ACCUM 0
#define WF_RES_FRAMES 1
#define WF_RES_MOMENTS 2
// ML: the instances for several lights: every light's intensity and pdf_n in LDS (2 KB for 64 lights),
// indexed by the light a lit vertex recorded (P.vlt); the one-light instances carry none of it
// TX: the instances for albedo textures: every vertex's texel, gathered through the id k_shadow<TX> stored
// (P.vtex), scales its albedo; the untextured instances carry none of it
// ENV: the instances for a sky: every path of the generation reads its slot's miss record (P.env_rec). A set
// record means the path ended in a miss after nv vertices: its fold starts with the texel's radiance, widened
// exactly, and covers vertices nv - 1 .. 0 (none for a camera ray's miss: the texel itself, the background),
// and the record goes back to MFX_ENV_NONE. Such a path adds to its pixel whatever its lit mask; a path
// that ended by depth alone is as without.
// SKY: the twins of the ML, ENV instances for a sampled sky: a lit vertex whose light index is N takes the
// radiance of the texel k_shadow<SKY> stored (P.vsky) and its pdf_v (fold_vertex). The miss records are as under
// ENV; the launcher runs the ENV twins of k_extend and k_camera for the camera rays alone, so every record is a
// camera ray's (nv = 0), and one with nv >= 1 is not honoured: cleared, the path as without.
template <int MODE, bool ML = false, bool TX = false, bool ENV = false, bool SKY = false>
__global__ void __launch_bounds__(256) k_resolve(WfParams P) {
    constexpr bool FRAMES = MODE == WF_RES_FRAMES, MOM = MODE == WF_RES_MOMENTS;
    __shared__ double alb[3 * WF_RES_MAT_LDS];
    const int nm = P.nmat < WF_RES_MAT_LDS ? P.nmat : WF_RES_MAT_LDS;
    for (int i = threadIdx.x; i < 3 * nm; i += blockDim.x) alb[i] = P.albedo[i];
    const double* lt_lds = nullptr;
    if constexpr (ML) {
        __shared__ double ltab[4 * WF_MAX_LIGHTS];
        const int nl = P.nlights < WF_MAX_LIGHTS ? P.nlights : WF_MAX_LIGHTS;
        for (int i = threadIdx.x; i < 4 * WF_MAX_LIGHTS; i += blockDim.x) {
            const int n = i >> 2, f = i & 3;
            // (entries past the table: pdf 1, intensity 0; never indexed by a well-formed record)
            ltab[i] = n < nl ? (f < 3 ? P.lights[n].color[f] : P.lights[n].pdf) : (f < 3 ? 0.0 : 1.0);
        }
        lt_lds = ltab;
    }
    __syncthreads();
    const int tiles_x = (P.width + 7) >> 3;
    const bool list = MOM && P.ntiles > 0;
    const int64_t per_sample = list ? (int64_t)P.ntiles * 64 : (int64_t)tiles_x * P.band_rows * 64;
    int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (!list && P.res_ntx > 0) {  // a band of tile columns (mfx_sample's banded resolve): thread -> its tile's q
        const int64_t tl = q >> 6;
        if (tl >= (int64_t)P.res_ntx * P.band_rows) return;
        q = ((tl / P.res_ntx) * tiles_x + P.res_tx0 + tl % P.res_ntx) * 64 + (q & 63);
    }
    if (q >= per_sample) return;
    const int64_t tile = q >> 6;
    const int within = (int)(q & 63);
    int x, y;
    if (list) {  // the trace's tile -> the film's (an index outside the film touches no pixel)
        unsigned tx, ty;
        if (!list_tile_xy((unsigned)P.tiles[tile], (unsigned)tiles_x, (unsigned)(P.height + 7) >> 3, tx, ty)) return;
        x = (int)tx * 8 + (within & 7);
        y = (int)ty * 8 + (within >> 3);
    } else {
        x = (int)(tile % tiles_x) * 8 + (within & 7);
        y = band_tile_row(P.band_index, P.band_count, (int)(tile / tiles_x)) * 8 + (within >> 3);  // the band's film row
    }
    if (x >= P.width || y >= P.height) return;
    const int64_t npix = (int64_t)P.width * P.height;
    const int64_t pixel = (int64_t)x * P.height + y;
    const int64_t end = P.path_base + P.total;
    double* acc = FRAMES ? P.film : P.accum;
    double ax = acc[pixel], ay = acc[npix + pixel], az = acc[2 * npix + pixel];
    double s1 = 0.0, s2 = 0.0;
    if (MOM) {
        s1 = P.mom[pixel];
        s2 = P.mom[npix + pixel];
    }
    constexpr int U = WF_RES_SAMPLES;
    for (int64_t smp0 = P.path_base / per_sample; smp0 * per_sample < end; smp0 += U) {
        int64_t jv[U];
        bool in[U];
        int sw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t p = (smp0 + u) * per_sample + q;
            in[u] = p >= P.path_base && p < end;
            jv[u] = in[u] ? p - P.path_base : 0;
            sw[u] = in[u] ? P.state[jv[u]] : 0;
        }
        int mask[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            mask[u] = ((sw[u] & WF_STATE_MASK) == WF_DONE || (sw[u] & WF_STATE_MASK) == WF_MISS)
                          ? ((unsigned)sw[u] >> WF_SHADE_SHIFT) & 0xffff : 0;
        }
        [[maybe_unused]] uint32_t ew[U];  // ENV: the paths' miss records
        [[maybe_unused]] int etop[U];     // and their deepest vertex to fold (-1: none)
        if constexpr (ENV) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                ew[u] = in[u] ? P.env_rec[jv[u]] : MFX_ENV_NONE;
                if constexpr (SKY) {
                    if (ew[u] != MFX_ENV_NONE && (ew[u] >> MFX_ENV_NV_SHIFT) != 0) {
                        P.env_rec[jv[u]] = MFX_ENV_NONE;
                        ew[u] = MFX_ENV_NONE;
                    }
                }
                etop[u] = ew[u] != MFX_ENV_NONE ? (int)(ew[u] >> MFX_ENV_NV_SHIFT) - 1
                                                : (mask[u] ? 31 - __builtin_clz(mask[u]) : -1);
            }
        }
        PathRec R[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if constexpr (ENV) load_path<ML, TX, true, SKY>(P, jv[u], mask[u], R[u], etop[u]);
            else load_path<ML, TX>(P, jv[u], mask[u], R[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!in[u]) continue;
            double fx = 0.0, fy = 0.0, fz = 0.0;
            if constexpr (ENV) {
                if (ew[u] != MFX_ENV_NONE) {
                    const float* e = P.env_rgb + 3 * (size_t)(ew[u] & MFX_ENV_ID_MASK);
                    fx = (double)e[0];
                    fy = (double)e[1];
                    fz = (double)e[2];
                    P.env_rec[jv[u]] = MFX_ENV_NONE;
                }
                if (etop[u] >= 0) fold_path<ML, TX, true, SKY>(P, jv[u], R[u], alb, fx, fy, fz, lt_lds, etop[u]);
            } else if (R[u].mask) {
                fold_path<ML, TX>(P, jv[u], R[u], alb, fx, fy, fz, lt_lds);
            }
            if (FRAMES) {
                ax = ax + (0.0 + fx) / 1.0;
                ay = ay + (0.0 + fy) / 1.0;
                az = az + (0.0 + fz) / 1.0;
                if (P.frames) {
                    const double cnt = P.count0 + (double)(smp0 + u + 1);
                    uint8_t* o = P.frames + (smp0 + u) * npix * 4 + ((int64_t)y * P.width + x) * 4;
                    o[0] = post_byte(ax / cnt);
                    o[1] = post_byte(ay / cnt);
                    o[2] = post_byte(az / cnt);
                    o[3] = 255;
                }
            } else if (R[u].mask || (ENV && ew[u] != MFX_ENV_NONE)) {  // a path with no lit vertex adds nothing (ENV: unless it ended in the sky)
                ax += fx;
                ay += fy;
                az += fz;
                if (MOM) {
                    const double yl = (fx + fy) + fz;
                    s1 += yl;
                    s2 += yl * yl;
                }
            }
        }
    }
    acc[pixel] = ax;
    acc[npix + pixel] = ay;
    acc[2 * npix + pixel] = az;
    if (MOM) {
        P.mom[pixel] = s1;
        P.mom[npix + pixel] = s2;
    }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
// top nodes, instances, slots, stacks, pending-ray lists, block reduction scratch (64 B) and, for
// k_shadow, the shade lists
static size_t wf_lds_bytes(const WfLdsShape& s) {
    const size_t stacks = (size_t)s.ntop * sizeof(MfxNode) + (size_t)std::min(s.ninst, WF_INST_LDS) * sizeof(MfxInstance) +
                          (size_t)s.nslot * 80 + (size_t)4 * s.stack_lds * 64 * sizeof(int);
    return s.shadow ? stacks + 4 * PendShd::BYTES + 64 + 4 * 2 * WF_SHD_LIST * sizeof(int) + sizeof(MfxLight) + sizeof(ShdPtrs) +
                          sizeof(PixParams) + sizeof(SceneRefs) + (s.tx ? sizeof(TxShd) : 0) + (s.sn ? sizeof(MfxSnTables) : 0)
                    : stacks + 4 * WF_EXT_PEND * sizeof(int) + 64;
}

// An instance of a trace kernel: the kernels' template parameters as run-time values. k_extend takes
// every field but waves, k_shadow every field but start, k_camera stats and list; a key holds the
// fields its kernel does not take at the values the *_built rules below name.
struct WfKey {
    bool stats, spill;
    int sk;  // WF_SK_*
    bool queue, start;
    int list;   // WF_LIST_*
    int nf;     // MFX_NF_*
    int waves;  // k_shadow's build: 3 or 4 waves per SIMD
    bool ml;    // k_shadow's several-light instance (WfParams::lights)
    bool tx;    // k_shadow's textured instance (WfParams::vtex)
};
// a key's number, and the key of a number: the one place a field passes between run time and compile time
constexpr int WF_KEYS = 2 * 2 * 2 * 2 * 3 * 2 * 2 * 3 * 3 * 2;
static constexpr int key_index(const WfKey& k) {
    return ((((((((k.tx * 2 + k.ml) * 2 + k.stats) * 2 + k.spill) * 3 + k.sk) * 2 + k.queue) * 2 + k.start) * 3 + k.list) * 3 + k.nf) * 2 +
           (k.waves - 3);
}
static constexpr WfKey key_at(int i) {
    WfKey k{};
    k.waves = 3 + i % 2, i /= 2;
    k.nf = i % 3, i /= 3;
    k.list = i % 3, i /= 3;
    k.start = i % 2, i /= 2;
    k.queue = i % 2, i /= 2;
    k.sk = i % 3, i /= 3;
    k.spill = i % 2, i /= 2;
    k.stats = i % 2, i /= 2;
    k.ml = i % 2, i /= 2;
    k.tx = i;
    return k;
}

// The rules a key is derived by, each in its one function.
// the scene kind (k_extend / k_shadow SK)
static int scene_kind(bool inst, int nslot) { return inst ? WF_SK_INST : (nslot > 0 ? WF_SK_SLDS : WF_SK_FLAT); }
// the list kind of a trace: none, the adaptive sampler's tile list, or one with per-tile counts
// (mfx_sample_adaptive_resume)
static int list_kind(int ntiles, const int32_t* tile_n) {
    return ntiles > 0 ? (tile_n ? WF_LIST_TILE_N : WF_LIST_TILES) : WF_LIST_NONE;
}
// Which instances are built per node format (k_extend / k_shadow NF): a flat scene's in-place and queue
// instances without STATS, START or LIST, so neither format's loop holds the other's registers; every
// other instance takes either format (MFX_NF_ANY)
static constexpr bool wf_nf_fixed(const WfKey& k) { return k.sk == WF_SK_FLAT && !k.stats && !k.start && !k.list; }
// the node format a context runs: FP16 nodes when it has them (WfParams::nodes_h), FP32 under MFX_NODE_F32
static bool wf_fp16(const WfParams& P) {
#if MFX_NODE_F16
    return P.nodes_h != nullptr;
#else
    return false;
#endif
}
// k_shadow's build: compiled for 3 waves per SIMD (up to 168 VGPRs) when its LDS allows no more blocks anyway
static int shadow_build(int shadow_waves) { return shadow_waves == 3 ? 3 : 4; }

// The instances the code object holds: a key outside these rules names no kernel.
static constexpr bool nf_built(const WfKey& k) {
    return wf_nf_fixed(k) ? k.nf == MFX_NF_F32 || (MFX_NODE_F16 && k.nf == MFX_NF_H) : k.nf == MFX_NF_ANY;
}
// (a queue's entries are never FREE slots; only the iteration that starts paths maps them through a list)
// (several lights, ml: k_shadow alone reads a light, and its ML instances are the 4-wave build without
// the traversal counters: contexts with several lights refuse MFX_F_COUNT_STATS and take the 4-wave build)
// (albedo textures, tx: as ml, k_shadow alone computes a texel id, in the 4-wave build without counters, and
// in both ml states: textured contexts refuse MFX_F_COUNT_STATS too)
static constexpr bool extend_built(const WfKey& k) {
    return !k.ml && !k.tx && k.waves == 4 && nf_built(k) && (k.queue ? !k.start && !k.list : k.start || !k.list);
}
static constexpr bool shadow_built(const WfKey& k) {
    return !k.start && nf_built(k) && ((!k.ml && !k.tx) || (!k.stats && k.waves == 4));
}
static constexpr bool camera_built(const WfKey& k) {
    return !k.ml && !k.tx && !k.spill && k.sk == WF_SK_FLAT && !k.queue && k.start && k.nf == MFX_NF_ANY && k.waves == 4;
}
// (a sky, ENV: k_extend and k_camera record a miss; every instance without the traversal counters has its ENV
// twin, and contexts created with MFX_F_COUNT_STATS refuse mfx_set_environment. Not a key field: the twin is
// chosen beside the key, as k_camera's CUTS twin is. k_shadow has none: shadow rays ignore the sky.)
static constexpr bool extend_env_built(const WfKey& k) { return extend_built(k) && !k.stats; }
static constexpr bool camera_env_built(const WfKey& k) { return camera_built(k) && !k.stats; }
// (a sampled sky, SKY: k_shadow's twin of every several-light instance, textured or not; beside the key as ENV is.
// k_extend and k_camera have none: their ENV twins run the camera rays, their plain instances the bounces.)
static constexpr bool shadow_sky_built(const WfKey& k) { return shadow_built(k) && k.ml; }
// (smooth shading, SN: k_shadow's twin of every 4-wave instance without the traversal counters, in each ml and tx
// state, and of every SKY twin; beside the key as SKY is. Contexts created with MFX_F_COUNT_STATS refuse
// mfx_set_normals, and a context with normals takes the 4-wave build. No other kernel of this file reads a normal.)
static constexpr bool shadow_sn_built(const WfKey& k) { return shadow_built(k) && !k.stats && k.waves == 4; }
static constexpr bool shadow_sky_sn_built(const WfKey& k) { return shadow_sky_built(k) && shadow_sn_built(k); }
// (a thin lens, LENS: k_extend's twin of every path-starting instance without the traversal counters, and of its ENV
// twin; beside the key as ENV is. Contexts created with MFX_F_COUNT_STATS refuse mfx_set_lens. k_camera has none: a
// lens context's camera rays run k_extend; k_shadow and k_resolve never see where a camera ray came from.)
static constexpr bool extend_lens_built(const WfKey& k) { return extend_env_built(k) && k.start; }
static constexpr int built_count(bool (*built)(const WfKey&)) {
    int n = 0;
    for (int i = 0; i < WF_KEYS; ++i) n += built(key_at(i));
    return n;
}
static_assert(built_count(extend_built) == (MFX_NODE_F16 ? 64 : 60) &&
                  built_count(shadow_built) == (MFX_NODE_F16 ? 152 + 3 * 40 : 144 + 3 * 36) && built_count(camera_built) == 6,
              "a new instance is a decision: every one is a kernel to compile, and an occupancy to ask about "
              "(k_shadow: 152 / 144 one-light instances, plus the several-light ones, ML: every spill, scene kind, "
              "queue and list of the 4-wave build without counters, 36, and the FP16 format of the 4 flat unlisted ones; "
              "the textured ones, TX, are as many again in each ML state)");
static_assert(built_count(extend_env_built) == (MFX_NODE_F16 ? 34 : 30) && built_count(camera_env_built) == 3,
              "the sky's instances, ENV: the twin of every k_extend instance without counters, 34 / 30, and of every "
              "k_camera instance without counters in both CUTS states, 2 * 3; k_resolve's twelve have a twin each");
static_assert(built_count(shadow_sky_built) == (MFX_NODE_F16 ? 2 * 40 : 2 * 36),
              "the sampled sky's instances, SKY: the twin of every several-light k_shadow instance, untextured and "
              "textured, 2 * 40 / 2 * 36; k_resolve's six ML, ENV instances have a twin each");
static_assert(built_count(shadow_sn_built) == (MFX_NODE_F16 ? 4 * 40 : 4 * 36) &&
                  built_count(shadow_sky_sn_built) == (MFX_NODE_F16 ? 2 * 40 : 2 * 36),
              "smooth shading's instances, SN: the twin of every 4-wave k_shadow instance without counters, 40 / 36 in each "
              "of the four (ML, TX) states, and of every SKY twin, 2 * 40 / 2 * 36");
static_assert(built_count(extend_lens_built) == 18,
              "the lens's instances, LENS: the twin of every START k_extend instance without counters (both spill states, "
              "three scene kinds, three list kinds), 18, and of the ENV twin of each, 18 more");

enum { WF_K_EXTEND, WF_K_SHADOW, WF_K_CAMERA, WF_K_CAMERA_CUTS, WF_K_EXTEND_ENV, WF_K_CAMERA_ENV, WF_K_CAMERA_CUTS_ENV, WF_K_SHADOW_SKY, WF_K_EXTEND_LENS,
       WF_K_EXTEND_LENS_ENV, WF_K_SHADOW_SN, WF_K_SHADOW_SKY_SN };
template <int KERNEL, int I>
static const void* instance_at() {
    constexpr WfKey k = key_at(I);
    if constexpr (KERNEL == WF_K_EXTEND && extend_built(k))
        return (const void*)k_extend<k.stats, k.spill, k.sk, k.queue, k.start, k.list, k.nf>;
    else if constexpr (KERNEL == WF_K_SHADOW && shadow_built(k))
        return (const void*)k_shadow<k.stats, k.spill, k.waves, k.sk, k.queue, k.list, k.nf, k.ml, k.tx>;
    else if constexpr (KERNEL == WF_K_CAMERA && camera_built(k))
        return (const void*)k_camera<k.stats, k.list>;
    else if constexpr (KERNEL == WF_K_CAMERA_CUTS && camera_built(k))  // every k_camera instance has its CUTS twin
        return (const void*)k_camera<k.stats, k.list, true>;
    else if constexpr (KERNEL == WF_K_EXTEND_ENV && extend_env_built(k))
        return (const void*)k_extend<k.stats, k.spill, k.sk, k.queue, k.start, k.list, k.nf, true>;
    else if constexpr (KERNEL == WF_K_CAMERA_ENV && camera_env_built(k))
        return (const void*)k_camera<k.stats, k.list, false, true>;
    else if constexpr (KERNEL == WF_K_CAMERA_CUTS_ENV && camera_env_built(k))
        return (const void*)k_camera<k.stats, k.list, true, true>;
    else if constexpr (KERNEL == WF_K_SHADOW_SKY && shadow_sky_built(k))
        return (const void*)k_shadow<k.stats, k.spill, k.waves, k.sk, k.queue, k.list, k.nf, k.ml, k.tx, true>;
    else if constexpr (KERNEL == WF_K_EXTEND_LENS && extend_lens_built(k))
        return (const void*)k_extend<k.stats, k.spill, k.sk, k.queue, k.start, k.list, k.nf, false, true>;
    else if constexpr (KERNEL == WF_K_EXTEND_LENS_ENV && extend_lens_built(k))
        return (const void*)k_extend<k.stats, k.spill, k.sk, k.queue, k.start, k.list, k.nf, true, true>;
    else if constexpr (KERNEL == WF_K_SHADOW_SN && shadow_sn_built(k))
        return (const void*)k_shadow<k.stats, k.spill, k.waves, k.sk, k.queue, k.list, k.nf, k.ml, k.tx, false, true>;
    else if constexpr (KERNEL == WF_K_SHADOW_SKY_SN && shadow_sky_sn_built(k))
        return (const void*)k_shadow<k.stats, k.spill, k.waves, k.sk, k.queue, k.list, k.nf, k.ml, k.tx, true, true>;
    else
        return nullptr;
}
template <int KERNEL, size_t... I>
static const void* instance(const WfKey& k, std::index_sequence<I...>) {
    static const void* const table[WF_KEYS] = {instance_at<KERNEL, (int)I>()...};
    return table[key_index(k)];
}
// a key's kernel (null: not built); env: its ENV twin; lens: the LENS twin of either (START keys only)
static const void* extend_kernel(const WfKey& k, bool env = false, bool lens = false) {
    if (lens)
        return env ? instance<WF_K_EXTEND_LENS_ENV>(k, std::make_index_sequence<WF_KEYS>{})
                   : instance<WF_K_EXTEND_LENS>(k, std::make_index_sequence<WF_KEYS>{});
    return env ? instance<WF_K_EXTEND_ENV>(k, std::make_index_sequence<WF_KEYS>{})
               : instance<WF_K_EXTEND>(k, std::make_index_sequence<WF_KEYS>{});
}
// (sky: the SKY twin of a several-light key; sn: the SN twin of either)
static const void* shadow_kernel(const WfKey& k, bool sky = false, bool sn = false) {
    if (sn)
        return sky ? instance<WF_K_SHADOW_SKY_SN>(k, std::make_index_sequence<WF_KEYS>{})
                   : instance<WF_K_SHADOW_SN>(k, std::make_index_sequence<WF_KEYS>{});
    return sky ? instance<WF_K_SHADOW_SKY>(k, std::make_index_sequence<WF_KEYS>{})
               : instance<WF_K_SHADOW>(k, std::make_index_sequence<WF_KEYS>{});
}
// (cuts: the twin that starts from the cut table, WfParams::cuts set; not a key field, k_camera alone has it)
static const void* camera_kernel(const WfKey& k, bool cuts, bool env = false) {
    if (env)
        return cuts ? instance<WF_K_CAMERA_CUTS_ENV>(k, std::make_index_sequence<WF_KEYS>{})
                    : instance<WF_K_CAMERA_ENV>(k, std::make_index_sequence<WF_KEYS>{});
    return cuts ? instance<WF_K_CAMERA_CUTS>(k, std::make_index_sequence<WF_KEYS>{})
                : instance<WF_K_CAMERA>(k, std::make_index_sequence<WF_KEYS>{});
}

// the key of k_extend or k_shadow holding shape s
static WfKey shape_key(const WfLdsShape& s, bool stats, bool queue, bool start, int list, int waves) {
    WfKey k{stats, s.spill, scene_kind(s.ninst > 0, s.nslot), queue, start, list, MFX_NF_ANY, waves, s.shadow && s.ml, s.shadow && s.tx};
    if (wf_nf_fixed(k)) k.nf = s.fp16 ? MFX_NF_H : MFX_NF_F32;
    return k;
}
static WfKey camera_key(bool stats, int list) { return {stats, false, WF_SK_FLAT, false, true, list, MFX_NF_ANY, 4, false, false}; }

// The query asks the instance a launch of the shape runs, with two deliberate differences: the 4-wave
// k_shadow whatever the context's build (scene_shapes chooses the 3-wave build from the answer), and, for
// the scene kinds without per-format instances, k_extend's START instance instead of the bounce one (a
// superset of the bounce instance's code).
hipError_t mfx_wf_kernel_occupancy(const WfLdsShape& s, int* blocks_per_cu) {
    // (a lens: the START instance whatever the scene kind, its LENS twin: the kernel that starts the context's paths)
    const bool start = !s.shadow && (s.lens || !wf_nf_fixed(shape_key(s, false, false, false, WF_LIST_NONE, 4)));
    const WfKey k = shape_key(s, false, false, start, WF_LIST_NONE, 4);
    const size_t lds = wf_lds_bytes(s);
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
        blocks_per_cu, s.shadow ? shadow_kernel(k, s.sky, s.sn) : extend_kernel(k, s.env, s.lens), 256, lds);
    // (the API counts finer LDS granules than the hardware allocates: measured, k_shadow at 53,952 B per
    // block runs 2 blocks per CU where it says 3, a 10 % loss)
    *blocks_per_cu = std::min(*blocks_per_cu, mfx_lds_blocks(lds));
    return e;
}

static size_t cam_lds_bytes(int stack_size) {
    return (size_t)4 * stack_size * (sizeof(int) + sizeof(uint64_t)) + 64 + sizeof(MfxCamera) + sizeof(SceneRefs);
}

hipError_t mfx_cam_occupancy(int stack_size, int* blocks_per_cu, bool cuts) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, camera_kernel(camera_key(false, WF_LIST_NONE), cuts), 256,
                                                        cam_lds_bytes(stack_size));
}

// a launch's error is left to the hipGetLastError that follows the iteration's launches
static void launch(const void* kernel, int grid, size_t lds, hipStream_t st, const WfParams& P) {
    void* args[] = {const_cast<WfParams*>(&P)};
    (void)hipLaunchKernel(kernel, dim3(grid), dim3(256), args, lds, st);
}

// what each trace kernel of this trace keeps in LDS (each its own share of the traversal stack; the rest spills)
static WfLdsShape lds_shape(const WfParams& P, bool shadow) {
    const int stack_lds = shadow ? P.stack_lds_shd : P.stack_lds_ext;
    return {shadow, stack_lds < P.stack_size, wf_fp16(P), stack_lds, shadow ? P.ntop_shd : P.ntop_ext,
            P.inst ? P.ninst_lds : 0, shadow ? P.nslot_shd : P.nslot_ext, shadow && P.lights != nullptr,
            shadow && P.vtex != nullptr, !shadow && P.env_rec != nullptr, shadow && P.sky_tab != nullptr, false,
            shadow && P.sn.rec != nullptr};
}

static hipError_t launch_iteration(const WfParams& P, int ext_grid, int shd_grid, bool stats, hipStream_t st,
                                   hipEvent_t* ev, bool lens) {
    const int list = list_kind(P.ntiles, P.tile_n);
    // a sky: the ENV twins of k_camera and k_extend; a sampled one: for the camera rays alone (the iteration that
    // starts the generation's paths holds nothing else), the plain instances for the bounces
    const bool env = P.env_rec != nullptr && (P.sky_tab == nullptr || P.start);
    if (!P.inst && P.start && P.cam_grid > 0 && !lens) {  // camera rays as packets (a lens: one origin per ray, k_extend)
        const void* cam = camera_kernel(camera_key(stats, list), P.cuts != nullptr, env);
        if (!cam) return hipErrorInvalidValue;  // (a sky with counters: refused by mfx_set_environment)
        launch(cam, P.cam_grid, cam_lds_bytes(P.stack_size), st, P);
    } else {
        WfLdsShape s = lds_shape(P, false);
        s.env = env;
        const bool queue = P.qcount != nullptr, start = !queue && P.start;
        // a lens: the LENS twin starts the paths (the bounces run the plain instances)
        const void* ext = extend_kernel(shape_key(s, stats, queue, start, start ? list : WF_LIST_NONE, 4), env, start && lens);
        if (!ext) return hipErrorInvalidValue;  // (a lens with counters: refused by mfx_set_lens)
        launch(ext, ext_grid, wf_lds_bytes(s), st, P);
    }
    if (ev) {  // between the two kernels (per-stage timing); null: not recorded
        const hipError_t e = hipEventRecord(ev[0], st);
        if (e != hipSuccess) return e;
    }
    const WfLdsShape s = lds_shape(P, true);
    const bool queue = P.qslot || P.ncount;
    const void* shd = shadow_kernel(shape_key(s, stats, queue, false, list, shadow_build(P.shadow_waves)), s.sky, s.sn);
    if (!shd) return hipErrorInvalidValue;  // (several lights, textures or normals with counters or the 3-wave build: refused by their entry points)
    launch(shd, shd_grid, wf_lds_bytes(s), st, P);
    return hipSuccess;
}

hipError_t mfx_wf_iteration(const WfParams& P, int ext_grid, int shd_grid, bool stats, hipStream_t st,
                            hipEvent_t* ev, bool lens) {
    // several lights: the table, its count and the index plane go together (k_shadow<ML> writes vlt)
    // (a sampled sky is the light after them: one area light will do, 63 at most)
    if (P.lights && (!P.vlt || P.nlights < (P.sky_tab ? 1 : 2) || P.nlights > WF_MAX_LIGHTS - (P.sky_tab ? 1 : 0) || P.gray_light || stats))
        return hipErrorInvalidValue;
    // a sampled sky: the table and the id plane go together, with the sky's map and the lights' table
    if ((P.sky_tab != nullptr) != (P.vsky != nullptr) || (P.sky_tab && (!P.env_rec || !P.lights))) return hipErrorInvalidValue;
    // albedo textures: the id plane and the tables go together (k_shadow<TX> reads the tables and writes vtex)
    if (P.vtex && (!P.tx.uvrec || !P.tx.ptex || !P.tx.desc || !P.tx.texels || stats)) return hipErrorInvalidValue;
    // smooth shading: the records and the flags go together (k_shadow<SN> reads both)
    if ((P.sn.rec != nullptr) != (P.sn.flag != nullptr) || (P.sn.rec && stats)) return hipErrorInvalidValue;
    // a sky: the record plane and the map go together (k_extend<ENV> / k_camera<ENV> write env_rec)
    if (P.env_rec && (!P.env_rgb || P.env_size < 1 || P.env_size > MFX_ENV_SIZE_MAX || stats)) return hipErrorInvalidValue;
    // a lens: no counters, no cut table (its camera rays share no origin)
    if (lens && (stats || P.cuts || !P.cam_dev)) return hipErrorInvalidValue;
    // the chunk heads and, beside them (WF_CTL_Q0 / WF_CTL_Q1), the next queue's shard counts
    unsigned long long* z = P.ctl;
    size_t nz = WF_NCTL;
    if (P.ncount) {
        nz += WF_SHARDS * WF_HS;
        if (P.ncount < P.ctl) z = P.ncount;
    }
    hipError_t e = hipMemsetAsync(z, 0, nz * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    e = launch_iteration(P, ext_grid, shd_grid, stats, st, ev, lens);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

// k_resolve's instance of a mode: several lights (ML), albedo textures (TX) and a sky (ENV) each have one
template <int MODE, bool ENV>
static const void* resolve_kernel_env(bool ml, bool tx) {
    return ml ? (tx ? (const void*)k_resolve<MODE, true, true, ENV> : (const void*)k_resolve<MODE, true, false, ENV>)
              : (tx ? (const void*)k_resolve<MODE, false, true, ENV> : (const void*)k_resolve<MODE, false, false, ENV>);
}
template <int MODE>
static const void* resolve_kernel(bool ml, bool tx, bool env, bool sky = false) {
    if (sky)  // the SKY twin of the ML, ENV instance
        return ml && env ? (tx ? (const void*)k_resolve<MODE, true, true, true, true> : (const void*)k_resolve<MODE, true, false, true, true>)
                         : nullptr;
    return env ? resolve_kernel_env<MODE, true>(ml, tx) : resolve_kernel_env<MODE, false>(ml, tx);
}
static hipError_t launch_resolve(const void* kernel, int64_t threads, hipStream_t st, const WfParams& P) {
    void* args[] = {const_cast<WfParams*>(&P)};
    const hipError_t e = hipLaunchKernel(kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), args, 0, st);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t mfx_wf_resolve(const WfParams& P, hipStream_t st) {
    const bool ml = P.lights != nullptr;  // several lights: the ML instance of each mode
    const bool tx = P.vtex != nullptr;    // albedo textures: the TX instance
    const bool sky = P.sky_tab != nullptr;  // a sampled sky: the SKY instance
    if (ml && (!P.vlt || P.nlights < (sky ? 1 : 2) || P.nlights > WF_MAX_LIGHTS - (sky ? 1 : 0) || P.gray_light)) return hipErrorInvalidValue;
    if (tx && !P.tx.texels) return hipErrorInvalidValue;
    if (sky && (!ml || !P.vsky || !P.env_rec)) return hipErrorInvalidValue;
    const bool env = P.env_rec != nullptr;  // a sky: the ENV instance
    if (env && (!P.env_rgb || P.env_size < 1 || P.env_size > MFX_ENV_SIZE_MAX)) return hipErrorInvalidValue;
    if (P.mom || P.ntiles > 0) {  // the adaptive sampler's passes: the moments instance (a listed trace runs no other)
        if (!P.mom || P.film || P.res_ntx > 0) return hipErrorInvalidValue;
        const int64_t n = P.ntiles > 0 ? (int64_t)P.ntiles * 64 : (int64_t)((P.width + 7) >> 3) * P.band_rows * 64;
        return launch_resolve(resolve_kernel<WF_RES_MOMENTS>(ml, tx, env, sky), n, st, P);
    }
    const int64_t per_sample = (int64_t)(P.res_ntx > 0 ? P.res_ntx : (P.width + 7) >> 3) * P.band_rows * 64;
    return launch_resolve(P.film ? resolve_kernel<WF_RES_FRAMES>(ml, tx, env, sky) : resolve_kernel<WF_RES_ACCUM>(ml, tx, env, sky), per_sample, st, P);
}

hipError_t mfx_wf_resolve_occupancy(bool ml, int* blocks_per_cu, bool tx, bool env, bool sky) {
    const void* k = resolve_kernel<WF_RES_ACCUM>(ml, tx, env, sky);
    if (!k) return hipErrorInvalidValue;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k, 256, 0);
}

// ------------------------------------------------------------------------------------------------
// Adaptive sampling: the tile check after a pass (the rule: include/mafrix_rt.h, mfx_sample_adaptive)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// One wave per active tile, a lane per pixel of the tile: v_p = max(0, S2 - S1 * S1 / n) / (n (n - 1))
// and S1 / n from the lane's moments, E and M summed over the wave, m counted from the valid lanes'
// ballot; E m <= rel^2 (|M| + abs_floor m)^2 is the test. True: the tile has converged after ni
// samples (wave-uniform; m: its valid pixels, 0 for an index outside the film).
__device__ __forceinline__ bool tile_converged(const TileCheckParams& C, int T, int ni, int& m) {
    const int lane = lane_id();
    const unsigned tiles_x = (unsigned)(C.width + 7) >> 3, tiles_y = (unsigned)(C.height + 7) >> 3;
    unsigned tx, ty;
    const bool in_film = list_tile_xy((unsigned)T, tiles_x, tiles_y, tx, ty);
    const int x = (int)tx * 8 + (lane & 7), y = (int)ty * 8 + (lane >> 3);
    const bool valid = in_film && x < C.width && y < C.height;
    const double n = (double)ni;
    double v = 0.0, mean = 0.0;
    if (valid) {
        const int64_t npix = (int64_t)C.width * C.height;
        const int64_t pixel = (int64_t)x * C.height + y;
        const double s1 = C.mom[pixel], s2 = C.mom[npix + pixel];
        const double d = s2 - s1 * s1 / n;
        v = (d > 0.0 ? d : 0.0) / (n * (n - 1.0));
        mean = s1 / n;
    }
    const double E = wave_sum(v), M = wave_sum(mean);
    m = __popcll(__ballot(valid));
    const double md = (double)m;
    const double t = fabs(M) + C.abs_floor * md;
    return E * md <= C.rel2 * (t * t);
}

// mfx_sample_adaptive's check: every listed tile has had C.n samples. A tile that stops (converged, or
// at max_spp) gets its count; flags[k] tells k_tile_compact which entries go on.
__global__ void __launch_bounds__(256) k_tile_check(TileCheckParams C) {
    const int k = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (k >= C.ntiles) return;
    const int T = C.tiles[k];  // wave-uniform: one scalar load
    int m;
    const bool conv = tile_converged(C, T, C.n, m);
    if (lane_id() == 0) {
        const bool stop = m == 0 || C.n >= C.max_spp || conv;
        if (stop && m > 0) C.tile_spp[T] = C.n;  // (m > 0: T is a tile of the film)
        C.flags[k] = stop ? 0 : 1;
    }
}

// mfx_sample_adaptive_resume's check: every listed tile T has its own count. The pass before it gave
// the tile min(C.pass_spp, max_spp - tile_spp[T]) samples (pass_spp 0: the entry check, no pass), so
// n is tile_spp[T] plus that. Every checked tile gets its new count, stopping or not: the next pass
// reads it as the tile's base (WfParams::tile_n), and k_tile_compact takes from it the largest share of
// that pass.
__global__ void __launch_bounds__(256) k_tile_check_n(TileCheckParams C) {
    const int k = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (k >= C.ntiles) return;
    const int T = C.tiles[k];
    const unsigned nt = (((unsigned)C.width + 7) >> 3) * (((unsigned)C.height + 7) >> 3);
    if ((unsigned)T >= nt) {  // not a tile of the film: no count to read
        if (lane_id() == 0) C.flags[k] = 0;
        return;
    }
    const int n0 = C.tile_spp[T];
    const int left = C.max_spp - n0;
    const int n = n0 + (left < C.pass_spp ? (left > 0 ? left : 0) : C.pass_spp);
    int m;
    const bool conv = tile_converged(C, T, n, m);
    if (lane_id() == 0) {
        const bool stop = n >= C.max_spp || conv;
        C.tile_spp[T] = n;
        C.flags[k] = stop ? 0 : 1;
    }
}

// The tiles that go on, in list order (ascending: the camera packets and the resolve's coalescing rely
// on tile-row coherence). One block; each wave owns a contiguous run of whole 64-entry rounds, counts
// its flags by ballot, and after the waves' counts are known writes its survivors at their ranks.
// per_tile (mfx_sample_adaptive_resume): next_count[1] gets the largest number of samples a survivor
// takes in the next pass, min(step_spp, max_spp - tile_spp[T]), by which the host sizes that pass (here,
// over the list it walks anyway: one atomic per tile on that word cost 0.23 ms per C2 pass, 88 per us).
#define WF_COMPACT_WAVES 16
__global__ void __launch_bounds__(64 * WF_COMPACT_WAVES) k_tile_compact(TileCheckParams C) {
    __shared__ int wcount[WF_COMPACT_WAVES];
    __shared__ int wshare[WF_COMPACT_WAVES];
    int share = 0;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int per = ((C.ntiles + WF_COMPACT_WAVES - 1) / WF_COMPACT_WAVES + 63) / 64 * 64;
    const int lo = min(wave * per, C.ntiles), hi = min(lo + per, C.ntiles);
    int cnt = 0;
    for (int i = lo; i < hi; i += 64) cnt += __popcll(__ballot(i + lane < hi && C.flags[i + lane] != 0));
    if (lane == 0) wcount[wave] = cnt;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wcount[w];
    for (int i = lo; i < hi; i += 64) {
        const bool f = i + lane < hi && C.flags[i + lane] != 0;
        const uint64_t b = __ballot(f);
        if (f) {
            const int T = C.tiles[i + lane];
            C.next[base + __popcll(b & lanes_below())] = T;
            if (C.per_tile) share = max(share, min(C.step_spp, C.max_spp - C.tile_spp[T]));
        }
        base += __popcll(b);
    }
    if (C.per_tile) {
        for (int off = 32; off > 0; off >>= 1) share = max(share, __shfl_xor(share, off));
        if (lane == 0) wshare[wave] = share;
        __syncthreads();
        if (threadIdx.x == 64 * WF_COMPACT_WAVES - 1) {
            for (int w = 0; w < WF_COMPACT_WAVES; ++w) share = max(share, wshare[w]);
            C.next_count[1] = share;
        }
    }
    if (threadIdx.x == 64 * WF_COMPACT_WAVES - 1) *C.next_count = base;  // the last wave ends at the total
}

hipError_t mfx_wf_tile_check(const TileCheckParams& C, hipStream_t st) {
    if (C.per_tile) {
        if (C.ntiles <= 0 || C.pass_spp < 0 || C.step_spp < 1 || C.max_spp < 2) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_tile_check_n, dim3((unsigned)((C.ntiles + 3) / 4)), dim3(256), 0, st, C);
        hipLaunchKernelGGL(k_tile_compact, dim3(1), dim3(64 * WF_COMPACT_WAVES), 0, st, C);
        return hipGetLastError();
    }
    if (C.ntiles <= 0 || C.n < 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tile_check, dim3((unsigned)((C.ntiles + 3) / 4)), dim3(256), 0, st, C);
    hipLaunchKernelGGL(k_tile_compact, dim3(1), dim3(64 * WF_COMPACT_WAVES), 0, st, C);
    return hipGetLastError();
}
