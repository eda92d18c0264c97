// mfx_query.cpp — ray queries against a context's scene, its reference leaves, the host-only
// leaf build and the two device self-tests.
#include "mfx_ctx.h"

using namespace mfxh;

#define QCHECK(what, expr) HIP_TRY(expr, MFX_E_DEVICE, what)

template <typename T>
static hipError_t to_device(DevBuf<T>& d, const T* src, size_t count) {
    const hipError_t e = d.alloc(count);
    return e != hipSuccess ? e : hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice);
}

static int run_query(mfx_ctx* c, int64_t n, const double* rays, double tmin, double tmax, const double* tmax_arr,
                     double* t_out, int32_t* prim_out, double* normal_out, int32_t* occ_out, bool shadow) {
    if (!c || !rays || n < 0) return fail(MFX_E_INVALID, "bad query arguments");
    if (n == 0) return MFX_OK;
    HIPCHECK(hipSetDevice(c->device));
    DevBuf<double> d_rays, d_tmax, d_t, d_n;
    DevBuf<int32_t> d_p, d_o;
    QCHECK("query: ", to_device(d_rays, rays, 6 * (size_t)n));
    if (shadow) {
        QCHECK("query: ", to_device(d_tmax, tmax_arr, (size_t)n));
        QCHECK("query: ", d_o.alloc((size_t)n));
    } else {
        QCHECK("query: ", d_t.alloc((size_t)n));
        QCHECK("query: ", d_p.alloc((size_t)n));
        QCHECK("query: ", d_n.alloc(3 * (size_t)n));
    }
    QueryParams Q;
    std::memset(&Q, 0, sizeof(Q));
    fill_scene_ptrs(c, Q);
    Q.rays = d_rays;
    Q.tmax_per_ray = d_tmax;
    Q.t_out = d_t;
    Q.prim_out = d_p;
    Q.normal_out = d_n;
    Q.occ_out = d_o;
    Q.n = n;
    Q.tmin = tmin;
    Q.tmax = tmax;
    Q.stack_size = c->scene.stack_size;
    QCHECK("query: ", mfx_launch_query(Q, shadow, c->stream));
    QCHECK("query: ", hipStreamSynchronize(c->stream));
    if (shadow) {
        QCHECK("query: ", hipMemcpy(occ_out, d_o, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
        return MFX_OK;
    }
    QCHECK("query: ", hipMemcpy(t_out, d_t, sizeof(double) * n, hipMemcpyDeviceToHost));
    QCHECK("query: ", hipMemcpy(prim_out, d_p, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    if (normal_out) QCHECK("query: ", hipMemcpy(normal_out, d_n, sizeof(double) * 3 * n, hipMemcpyDeviceToHost));
    return MFX_OK;
}

extern "C" {
int mfx_closest_hit(mfx_ctx* c, int64_t n, const double* rays, double tmin, double tmax, double* t_out,
                    int32_t* prim_out, double* normal_out) {
    if (!t_out || !prim_out) return fail(MFX_E_INVALID, "null output");
    return run_query(c, n, rays, tmin, tmax, nullptr, t_out, prim_out, normal_out, nullptr, false);
}

int mfx_any_hit(mfx_ctx* c, int64_t n, const double* rays, double tmin, const double* tmax, int32_t* occluded_out) {
    if (!tmax || !occluded_out) return fail(MFX_E_INVALID, "null argument");
    return run_query(c, n, rays, tmin, 0.0, tmax, nullptr, nullptr, nullptr, occluded_out, true);
}

int mfx_ref_leaves(mfx_ctx* c, int32_t* indices_out, int32_t* leaf_first_out, int32_t* leaf_count_out,
                   int32_t* nleaves_out) {
    if (!c || !indices_out || !leaf_first_out || !leaf_count_out || !nleaves_out)
        return fail(MFX_E_INVALID, "null argument");
    std::copy(c->scene.host.ref_indices.begin(), c->scene.host.ref_indices.end(), indices_out);
    std::copy(c->scene.host.leaf_first.begin(), c->scene.host.leaf_first.end(), leaf_first_out);
    std::copy(c->scene.host.leaf_count.begin(), c->scene.host.leaf_count.end(), leaf_count_out);
    *nleaves_out = (int32_t)c->scene.host.leaf_first.size();
    return MFX_OK;
}

int mfx_build_leaves(const mfx_scene_desc* scene, int32_t* indices_out, int32_t* leaf_first_out,
                     int32_t* leaf_count_out, int32_t* nleaves_out, int32_t info_out[4]) {
    MfxHostScene s;
    std::string err;
    if (!mfx_build_scene(scene, s, err)) return fail(MFX_E_INVALID, "mfx_build_leaves: " + err);
    if (indices_out) std::copy(s.ref_indices.begin(), s.ref_indices.end(), indices_out);
    if (leaf_first_out) std::copy(s.leaf_first.begin(), s.leaf_first.end(), leaf_first_out);
    if (leaf_count_out) std::copy(s.leaf_count.begin(), s.leaf_count.end(), leaf_count_out);
    if (nleaves_out) *nleaves_out = (int32_t)s.leaf_first.size();
    if (info_out) {
        info_out[0] = s.nclusters;
        info_out[1] = (int32_t)s.nodes.size();
        info_out[2] = s.stack_entries;
        info_out[3] = (int32_t)s.slots.size();
    }
    return MFX_OK;
}

int mfx_fp64_selftest(int32_t device, int64_t n, const double* a, const double* b, double* div_out, double* sqrt_out) {
    if (n <= 0 || !a || !b || !div_out || !sqrt_out) return fail(MFX_E_INVALID, "bad selftest arguments");
    HIPCHECK(hipSetDevice(device));
    const char* who = "fp64 selftest: ";
    const size_t count = (size_t)n;
    DevBuf<double> da, db, dd, ds;
    QCHECK(who, to_device(da, a, count));
    QCHECK(who, to_device(db, b, count));
    QCHECK(who, dd.alloc(count));
    QCHECK(who, ds.alloc(count));
    QCHECK(who, mfx_launch_fp64_selftest(da, db, n, dd, ds, nullptr));
    QCHECK(who, hipDeviceSynchronize());
    QCHECK(who, hipMemcpy(div_out, dd, sizeof(double) * count, hipMemcpyDeviceToHost));
    QCHECK(who, hipMemcpy(sqrt_out, ds, sizeof(double) * count, hipMemcpyDeviceToHost));
    return MFX_OK;
}

int mfx_aabb_selftest(int32_t device, int64_t n, const double* rec, int32_t* out) {
    if (n <= 0 || !rec || !out) return fail(MFX_E_INVALID, "bad selftest arguments");
    HIPCHECK(hipSetDevice(device));
    const char* who = "aabb selftest: ";
    DevBuf<double> dr;
    DevBuf<int32_t> dout;
    QCHECK(who, to_device(dr, rec, 24 * (size_t)n));
    QCHECK(who, dout.alloc(3 * (size_t)n));
    QCHECK(who, mfx_launch_aabb_selftest(dr, n, dout, nullptr));
    QCHECK(who, hipDeviceSynchronize());
    QCHECK(who, hipMemcpy(out, dout, sizeof(int32_t) * 3 * n, hipMemcpyDeviceToHost));
    return MFX_OK;
}
}  // extern "C"
