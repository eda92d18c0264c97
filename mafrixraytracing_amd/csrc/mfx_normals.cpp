// mfx_normals.cpp — smooth shading on the host (include/mafrix_rt.h, mfx_set_normals): what is refused, the
// normal table of the world primitives and its copy to every device, what a change invalidates,
// mfx_normal_info, and the two host-only calls that expose the code the setter and the kernels run
// (mfx_normal_table, mfx_shading_normal; the rule itself: mfx_normals.h).
#include "mfx_ctx.h"

using namespace mfxh;

static_assert(sizeof(mfx_prim_normals) == 80, "the ABI's normals struct");

// one template primitive's normals: the first offender, or true
static bool check_prim_normals(const mfx_prim& p, const mfx_prim_normals& m, int64_t i, std::string& err) {
    if (!m.smooth) return true;
    const std::string who = "primitive " + std::to_string(i);
    if (p.kind == MFX_PRIM_SPHERE) {
        err = who + " is a smooth sphere (a sphere has its own normal)";
        return false;
    }
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(m.n[k][a])) {
                err = who + " normal of corner " + std::to_string(k) + " is not finite";
                return false;
            }
    return true;
}

// The tables of the world primitives of the kept scene `k` under pn: the expansion in entry order
// (mfx_instance), every world primitive with the normals of the template it came from.
static bool world_tables(const KeptScene& k, const mfx_prim_normals* pn, std::vector<double>& rec, std::vector<int32_t>& flag,
                         int64_t& nsmooth, std::string& err) {
    std::vector<mfx_prim> world;
    std::vector<int64_t> from;
    const mfx_prim* wp = k.prims.data();
    int64_t nw = (int64_t)k.prims.size();
    if (k.instanced) {
        if (!mfx_expand(k.prims.data(), (int64_t)k.prims.size(), k.instances.data(), (int)k.instances.size(), world, err)) return false;
        for (const mfx_instance& e : k.instances)
            for (int64_t i = 0; i < e.count; ++i) from.push_back(e.first + i);
        wp = world.data();
        nw = (int64_t)world.size();
    }
    rec.assign((size_t)nw * MFX_SN_RECORD_DOUBLES, 0.0);
    flag.assign((size_t)nw, 0);
    nsmooth = 0;
    for (int64_t w = 0; w < nw; ++w) {
        const mfx_prim_normals& m = pn[k.instanced ? from[(size_t)w] : w];
        if (!m.smooth) continue;
        flag[(size_t)w] = 1;
        mfx_sn_record(wp[w].p[0], wp[w].p[1], wp[w].p[2], m.n, &rec[(size_t)w * MFX_SN_RECORD_DOUBLES]);
        nsmooth += 1;
    }
    return true;
}

extern "C" {
int mfx_set_normals(mfx_ctx* c, const mfx_prim_normals* pn, int64_t nprims) {
    if (!c) return fail(MFX_E_INVALID, "mfx_set_normals: null context");
    if (pn && (c->flags & (MFX_F_MEGAKERNEL | MFX_F_COUNT_STATS)))
        return fail(MFX_E_STATE, "mfx_set_normals: a context created with MFX_F_MEGAKERNEL or MFX_F_COUNT_STATS has no normals instances");
    if (!pn && !wf_normals(c)) return MFX_OK;  // none before, none now: nothing to do
    std::vector<double> rec;
    std::vector<int32_t> flag;
    int64_t nsmooth = 0;
    if (pn) {  // on the host, before a device is touched
        const KeptScene& k = c->kept;
        if (nprims != (int64_t)k.prims.size())
            return fail(MFX_E_INVALID, "mfx_set_normals: nprims " + std::to_string(nprims) + " differs from the context's " +
                                           std::to_string(k.prims.size()) + " template primitives");
        std::string err;
        for (int64_t i = 0; i < nprims; ++i)
            if (!check_prim_normals(k.prims[(size_t)i], pn[i], i, err)) return fail(MFX_E_INVALID, "mfx_set_normals: " + err);
        if (!world_tables(k, pn, rec, flag, nsmooth, err)) return fail(MFX_E_INVALID, "mfx_set_normals: " + err);
    }
    // held render-ahead frames are the old normals': the film comes back to d_film under them, and the frames'
    // epoch ends; then everything the context has enqueued, a background batch included, finishes
    MFX_TRY(ahead_break(c));
    MFX_TRY(mfx_sync(c));
    const std::vector<mfx_ctx*> ds = devs_of(c);
    std::vector<Normals> fresh(ds.size());  // every device's tables first: a failure leaves every context as it was
    if (pn)
        for (size_t g = 0; g < ds.size(); ++g) {
            Normals& n = fresh[g];
            hipError_t e = hipSetDevice(ds[g]->device);
            if (e == hipSuccess) e = n.d_rec.alloc(std::max<size_t>(1, rec.size()));
            if (e == hipSuccess) e = n.d_flag.alloc(std::max<size_t>(1, flag.size()));
            if (e == hipSuccess) e = hipMemcpy(n.d_rec, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(n.d_flag, flag.data(), flag.size() * sizeof(int32_t), hipMemcpyHostToDevice);
            n.nworld = (int64_t)flag.size();
            n.nsmooth = nsmooth;
            if (e != hipSuccess) {
                (void)hipGetLastError();
                fresh.clear();  // (on the devices they were allocated on: hipFree takes any device's pointer)
                (void)hipSetDevice(c->device);
                return fail(e == hipErrorOutOfMemory ? MFX_E_NOMEM : MFX_E_DEVICE, std::string("mfx_set_normals: ") + hipGetErrorString(e));
            }
        }
    for (size_t g = 0; g < ds.size(); ++g) {
        mfx_ctx* d = ds[g];
        HIPCHECK(hipSetDevice(d->device));
        const bool was = wf_normals(d);
        d->nrm = std::move(fresh[g]);
        d->scene.normals = pn != nullptr;
        if (was != wf_normals(d)) MFX_TRY(scene_reshape(d));  // the SN twins' LDS and build: the launch shapes again
    }
    HIPCHECK(hipSetDevice(c->device));
    c->cam_epoch += 1;           // the feature buffers are the old normals'
    c->adp.accum_valid = false;  // a resume must not mix normals
    c->ahead.dfilm_buf = -1;
    return MFX_OK;
}

int mfx_normal_info(mfx_ctx* c, double out[8]) {
    if (!c || !out) return fail(MFX_E_INVALID, "mfx_normal_info: null argument");
    std::fill(out, out + 8, 0.0);
    if (!wf_normals(c)) return MFX_OK;
    const LaunchShapes& A = c->scene.shapes;
    int sb = 0, ab = 0;
    HIPCHECK(hipSetDevice(c->device));
    HIPCHECK(mfx_wf_kernel_occupancy(wf_lds_shape(c->scene, wf_textured(c), true, A.stack_lds_shd, A.ntop_shd, A.nslot_shd), &sb));
    HIPCHECK(mfx_aov_occupancy(!c->scene.host.inst.empty(), wf_textured(c), wf_lens(c), c->scene.stack_size, &ab, true));
    out[0] = (double)c->nrm.nsmooth;
    out[1] = 1.0;
    out[2] = (double)c->nrm.nworld * (double)(MFX_SN_RECORD_DOUBLES * sizeof(double) + sizeof(int32_t));
    out[4] = (double)sb;
    out[5] = (double)ab;
    return MFX_OK;
}

int mfx_normal_table(const mfx_prim* prims, int64_t nprims, const mfx_prim_normals* pn, double* out) {
    if (!prims || !pn || !out || nprims < 0) return fail(MFX_E_INVALID, "mfx_normal_table: null argument");
    for (int64_t i = 0; i < nprims; ++i) {
        double* r = out + i * MFX_SN_RECORD_DOUBLES;
        if (!pn[i].smooth || prims[i].kind == MFX_PRIM_SPHERE) std::fill(r, r + MFX_SN_RECORD_DOUBLES, 0.0);
        else mfx_sn_record(prims[i].p[0], prims[i].p[1], prims[i].p[2], pn[i].n, r);
    }
    return MFX_OK;
}

int mfx_shading_normal(int64_t n, const double* rec, const double* ng, const double* hp, double* out) {
    if (n < 0 || (n > 0 && (!rec || !ng || !hp || !out))) return fail(MFX_E_INVALID, "mfx_shading_normal: null argument");
    for (int64_t k = 0; k < n; ++k) mfx_sn_shade(rec + MFX_SN_RECORD_DOUBLES * k, hp + 3 * k, ng + 3 * k, out + 3 * k);
    return MFX_OK;
}
}  // extern "C"
