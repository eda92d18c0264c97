// mfx_readback.cpp — frames to the caller's host memory: the staged readback, mfx_sample (banded
// on one device), mfx_accum_read_mean and mfx_film_mean.
//
// Device -> caller's (pageable) host memory. A pageable destination is slow for large copies
// (mfx_sample's 66 MB FP64 frame at 1080p: ~10 ms, r03b), so a large readback goes to a page-locked
// staging buffer by DMA, in pieces, and from there to the caller's buffer by host threads, each
// copying its slice of every piece as soon as that piece has landed: the copy trails the DMA by one
// piece. r06a (scripts/readback_probe.py): the DMA alone moves 66 MB in 1.17 ms, one thread copies
// it on in 2.07 ms; 4 pieces copied by threads spawned per piece took 2.56 ms with the mean kernel.
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <chrono>
#include <thread>

#include "mfx_ctx.h"

using namespace mfxh;

// the page-locked staging buffer, at least `bytes` (false: none could be allocated)
static bool ensure_stage(mfx_ctx* c, size_t bytes) {
    Readback& rb = c->rb;
    if (bytes > rb.stage_bytes) {
        rb.stage_bytes = 0;
        if (rb.stage.alloc(bytes) == hipSuccess) rb.stage_bytes = bytes;
        else (void)hipGetLastError();
    }
    return rb.stage != nullptr;
}

static double host_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// MFX_SAMPLE_TIMING=1 (diagnostics): the host's clock at each piece's arrival and copy, on stderr
static bool sample_timing() {
    static const bool on = getenv("MFX_SAMPLE_TIMING") && atoi(getenv("MFX_SAMPLE_TIMING")) != 0;
    return on;
}

// NUMA node of the page holding `p` (-1: unknown), by get_mempolicy(MPOL_F_NODE | MPOL_F_ADDR)
static int page_node(const void* p) {
    int node = -1;
    if (syscall(SYS_get_mempolicy, &node, nullptr, 0UL, p, 3UL) != 0) return -1;
    return node;
}
// the device's NUMA node from sysfs (-1: unknown)
static int device_node(int device) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof(bus), device) != hipSuccess) return -1;
    for (char* q = bus; *q; ++q) *q = (char)tolower(*q);
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
    FILE* f = fopen(path.c_str(), "r");
    if (!f) return -1;
    int n = -1;
    if (fscanf(f, "%d", &n) != 1) n = -1;
    fclose(f);
    return n;
}

// Pieces [off[i], off[i] + len[i]) of the staging buffer, each complete once stage_ev[i] has fired,
// copied to dst at the same offsets by nt host threads (MFX_READBACK_THREADS; thread t takes slice t
// of every piece, in piece order). Returns when every piece is in dst.
// rgb: the staging buffer holds interleaved RGB (24 B a pixel; off / len in its bytes, whole pixels)
// and dst RGBA (32 B a pixel): each pixel is widened with alpha 1.0 as it is copied (mfx_sample)
static int copy_staged(mfx_ctx* c, void* dst, const size_t* off, const size_t* len, int npiece, bool rgb = false) {
    int nt = 8;
    if (const char* e = getenv("MFX_READBACK_THREADS")) nt = std::max(1, std::min(32, atoi(e)));
    const bool tm = sample_timing();
    const uint8_t* stage = c->rb.stage;
    double t_ready[kStageChunks] = {0}, t_copied[kStageChunks] = {0};
    const double t0 = tm ? host_ms() : 0.0;
    auto work = [&](int t) -> hipError_t {
        for (int i = 0; i < npiece; ++i) {
            const hipError_t e = hipEventSynchronize(c->rb.stage_ev[i]);
            if (e != hipSuccess) return e;
            if (tm && t == 0) t_ready[i] = host_ms();
            if (rgb) {
                const size_t npx = len[i] / 24, p0 = off[i] / 24;
                const size_t part = (npx / nt + 63) & ~(size_t)63;  // whole pixels, 64 at a time
                if (part * t >= npx) continue;
                const double* src = (const double*)stage + 3 * (p0 + part * t);
                double* out = (double*)dst + 4 * (p0 + part * t);
                const size_t n = std::min(part, npx - part * t);
                for (size_t k = 0; k < n; ++k) {
                    out[4 * k] = src[3 * k];
                    out[4 * k + 1] = src[3 * k + 1];
                    out[4 * k + 2] = src[3 * k + 2];
                    out[4 * k + 3] = 1.0;
                }
                if (tm && t == 0) t_copied[i] = host_ms();
                continue;
            }
            const size_t part = (len[i] / nt + 4095) & ~(size_t)4095;
            if (part * t >= len[i]) continue;
            const size_t o = off[i] + part * t;
            std::memcpy((uint8_t*)dst + o, stage + o, std::min(part, len[i] - part * t));
            if (tm && t == 0) t_copied[i] = host_ms();
        }
        return hipSuccess;
    };
    std::vector<hipError_t> err(nt, hipSuccess);
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back([&, t] { err[t] = work(t); });
    err[0] = work(0);
    for (auto& t : th) t.join();
    if (tm) {
        fprintf(stderr, "copy_staged: %d pieces, from the call's wait (ms): ready/copied", npiece);
        for (int i = 0; i < npiece; ++i) fprintf(stderr, " %.3f/%.3f", t_ready[i] - t0, t_copied[i] - t0);
        fprintf(stderr, "; joined %.3f; nodes: staging %d..%d, frame %d..%d, device %d, this cpu %d\n", host_ms() - t0,
                page_node(stage), page_node(stage + off[npiece - 1] + len[npiece - 1] - 1), page_node(dst),
                page_node((uint8_t*)dst + (off[npiece - 1] + len[npiece - 1]) / (rgb ? 24 : 1) * (rgb ? 32 : 1) - 1), device_node(c->device), sched_getcpu());
    }
    for (hipError_t e : err)
        if (e != hipSuccess) return fail(MFX_E_DEVICE, std::string("readback: ") + hipGetErrorString(e));
    return MFX_OK;
}

static int stage_events(mfx_ctx* c) {
    for (int i = 0; i < kStageChunks; ++i) {
        if (!c->rb.stage_ev[i]) HIPCHECK(c->rb.stage_ev[i].create(hipEventDisableTiming));
        if (!c->rb.band_ev[i]) HIPCHECK(c->rb.band_ev[i].create(hipEventDisableTiming));
    }
    return MFX_OK;
}

// stream-ordered after what `st` has enqueued, complete on return; a small readback (or with no
// staging memory) is a plain copy
int mfxh::host_readback(mfx_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st) {
    const size_t kLarge = 16u << 20;
    if (bytes < kLarge || !ensure_stage(c, bytes)) {
        HIPCHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
        return MFX_OK;
    }
    int npiece = kStageChunks;  // MFX_READBACK_PIECES: A/B knob
    if (const char* e = getenv("MFX_READBACK_PIECES")) npiece = std::max(1, std::min(kStageChunks, atoi(e)));
    MFX_TRY(stage_events(c));
    const size_t piece = (bytes / npiece + 4095) & ~(size_t)4095;
    size_t off[kStageChunks], len[kStageChunks];
    int used = 0;
    for (int i = 0; i < npiece && piece * i < bytes; ++i, ++used) {
        off[i] = piece * i;
        len[i] = std::min(piece, bytes - off[i]);
        HIPCHECK(hipMemcpyAsync(c->rb.stage + off[i], (const uint8_t*)src + off[i], len[i], hipMemcpyDeviceToHost, st));
        HIPCHECK(hipEventRecord(c->rb.stage_ev[i], st));
    }
    return copy_staged(c, dst, off, len, used);
}

// mfx_sample on one device: the trace with its last resolve in column bands of tiles (ResolveSplit),
// each band's mean enqueued right behind its resolve and its readback on the copy stream, so the
// frame's DMA and the host copy overlap the rest of the resolve. A band of tile columns is a contiguous
// range of the x-major frame (pixel = x * h + y). The bits are the unbanded path's: a pixel's sum is
// its own thread's, and the mean is the same division. MFX_SAMPLE_BANDS=0: the unbanded path.
// Returns 1 (nothing done) when the call is not for it (a device list, no staging memory).
static int sample_banded(mfx_ctx* c, int32_t spp, double* frame) {
    // 4 bands, one copy stream: in the bench process's state (r06i, scripts/sample_in_bench_probe.py)
    // 4 x 1 took 32.8-33.0 ms per C2 call, 8 x 1 33.0-33.2, 8 bands over two copy streams 33.7-33.9 and
    // the unbanded path 33.7 (a lone process: 8 x 1 32.1, unbanded 32.7, r06b)
    int nb = 4;
    if (const char* e = getenv("MFX_SAMPLE_BANDS")) nb = std::min(kStageChunks, atoi(e));
    const int W = c->scene.host.width, H = c->scene.host.height;
    nb = std::min(nb, (W + 7) / 8);
    // the means staged as interleaved RGB (MFX_SAMPLE_RGBA=1: the whole RGBA frame, A/B knob): the
    // host writes alpha while it copies, so the DMA carries 49.8 MB of C2's 66 MB frame
    const bool rgb = !(getenv("MFX_SAMPLE_RGBA") && atoi(getenv("MFX_SAMPLE_RGBA")) != 0);
    const size_t pxb = (rgb ? 3 : 4) * sizeof(double);
    const size_t bytes = pxb * (size_t)c->npix;
    if (nb < 1 || c->multi.any() || !ensure_stage(c, bytes)) return 1;
    Readback& rb = c->rb;
    HIPCHECK(hipSetDevice(c->device));
    MFX_TRY(stage_events(c));
    if (!rb.copy_stream) HIPCHECK(rb.copy_stream.create());  // one stream, created at the first Sample call
    // MFX_SAMPLE_ZEROCOPY=1 (A/B knob): each band's mean kernel runs on a copy stream and writes the
    // frame straight into the page-locked staging buffer across the fabric (no DMA)
    const bool zc = getenv("MFX_SAMPLE_ZEROCOPY") && atoi(getenv("MFX_SAMPLE_ZEROCOPY")) != 0;
    void* stage_dev = nullptr;  // the staging buffer's device address (zero-copy)
    if (zc) HIPCHECK(hipHostGetDevicePointer(&stage_dev, rb.stage, 0));
    size_t off[kStageChunks] = {0}, len[kStageChunks] = {0};
    ResolveSplit S;
    S.nbands = nb;
    S.after = [&](int k, int tx0, int ntx) -> int {
        const int64_t p0 = (int64_t)tx0 * 8 * H, p1 = (int64_t)std::min(W, (tx0 + ntx) * 8) * H;
        off[k] = (size_t)p0 * pxb;
        len[k] = (size_t)(p1 - p0) * pxb;
        hipStream_t cs = rb.copy_stream;
        auto mean = [&](double* out, hipStream_t st) {
            return rgb ? mfx_launch_mean_rgb(c->d_accum, c->npix, (double)spp, out, st, p0, p1)
                       : mfx_launch_mean(c->d_accum, c->npix, (double)spp, out, st, p0, p1);
        };
        if (zc) {
            HIPCHECK(hipEventRecord(rb.band_ev[k], c->stream));
            HIPCHECK(hipStreamWaitEvent(cs, rb.band_ev[k], 0));
            HIPCHECK(mean((double*)stage_dev, cs));
        } else {
            HIPCHECK(mean(c->d_frame, c->stream));
            HIPCHECK(hipEventRecord(rb.band_ev[k], c->stream));
            HIPCHECK(hipStreamWaitEvent(cs, rb.band_ev[k], 0));
            if (len[k]) HIPCHECK(hipMemcpyAsync(rb.stage + off[k], (const uint8_t*)c->d_frame.get() + off[k], len[k],
                                                hipMemcpyDeviceToHost, cs));
        }
        HIPCHECK(hipEventRecord(rb.stage_ev[k], cs));
        return MFX_OK;
    };
    c->rep_valid = false;
    c->multi.accum_merged = false;
    const double t0 = sample_timing() ? host_ms() : 0.0;
    MFX_TRY(dev_trace_accumulate(c, spp, c->next_sample, &S));
    MFX_TRY(settle_queue_auto(c));
    c->next_sample += spp;
    if (!S.used) {  // (one sample per pixel: the megakernel ran, no banded resolve)
        MFX_TRY(mfx_accum_read_mean(c, (double)spp, frame));
        return mfx_sync(c);
    }
    if (sample_timing()) fprintf(stderr, "sample_banded: enqueued in %.3f ms\n", host_ms() - t0);
    MFX_TRY(copy_staged(c, frame, off, len, nb, rgb));
    const int rc = mfx_sync(c);
    if (sample_timing()) fprintf(stderr, "sample_banded: call %.3f ms\n", host_ms() - t0);
    return rc;
}

extern "C" {
int mfx_accum_read_mean(mfx_ctx* c, double count, double* frame) {
    if (!c || !frame) return fail(MFX_E_INVALID, "null argument");
    if (!(count > 0.0)) return fail(MFX_E_INVALID, "mfx_accum_read_mean: count must be > 0");
    // a device list whose last trace (a render call's included) has not been merged: merge it first,
    // so the mean covers every device's rows; a merged accumulator is not merged twice
    if (!c->multi.accum_merged && c->multi.any()) MFX_TRY(mfx_accum_reduce(c));
    HIPCHECK(hipSetDevice(c->device));
    // texture[i,j] <- color / float n (Integrators.fs:171): divided by the count itself
    HIPCHECK(mfx_launch_mean(c->d_accum, c->npix, count, c->d_frame, c->stream));
    return host_readback(c, frame, c->d_frame, 4 * sizeof(double) * (size_t)c->npix, c->stream);
}

int mfx_sample(mfx_ctx* c, int32_t spp, double* frame) {
    if (!c || !frame) return fail(MFX_E_INVALID, "null argument");
    if (c->api_part_count != 1)
        return fail(MFX_E_STATE, "mfx_sample needs the whole film and sample set (part_count == 1); "
                                 "partitioned contexts compose with mfx_trace_accumulate + a reduce");
    if (spp < 1) return fail(MFX_E_INVALID, "spp must be >= 1");
    MFX_TRY(ahead_break(c));  // it moves the sample sequence past held frames
    MFX_TRY(mfx_accum_clear(c));
    const int rc = sample_banded(c, spp, frame);
    if (rc != 1) return rc;
    MFX_TRY(mfx_trace_accumulate(c, spp, c->next_sample));
    c->next_sample += spp;
    MFX_TRY(mfx_accum_reduce(c));  // a device list: its bands merged into the primary's accumulator
    MFX_TRY(mfx_accum_read_mean(c, (double)spp, frame));
    return mfx_sync(c);
}

int mfx_film_mean(mfx_ctx* c, double* frame) {
    if (!c || !frame) return fail(MFX_E_INVALID, "null argument");
    HIPCHECK(hipSetDevice(c->device));
    MFX_TRY(ahead_materialize(c));
    const double* film = c->d_film;
    if (c->multi.any()) {  // a device list: the devices' bands of the film, merged
        if (!c->multi.merge) HIPCHECK(c->multi.merge.alloc(3 * (size_t)c->npix));
        MFX_TRY(reduce_planes(c, [](mfx_ctx* d) -> double* { return d->d_film; }, c->multi.merge, "mfx_film_mean"));
        film = c->multi.merge;
    }
    HIPCHECK(mfx_launch_film_mean(film, c->npix, c->frame_count, c->d_frame, c->stream));
    return host_readback(c, frame, c->d_frame, 4 * sizeof(double) * (size_t)c->npix, c->stream);
}
}  // extern "C"
