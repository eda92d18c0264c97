// mfx_scene.cpp — host-side preparation of a scene for the gfx950 kernels.
//
// 1. Primitive records in FP64, with exactly the reference constructors' arithmetic
//    (Triangle: Trangle.fs:107-119, Rect: Rect.fs:11-20, Sphere: Sphere.fs:9-16).
// 2. The reference's heap BVH (BvhNode.fs:24-61) is built only for its LEAF GROUPING: which
//    2-3 primitives share a leaf decides the shadow-ray result when every primitive of a leaf
//    is hit beyond tMax (Triangle.Hit ignores tMax, Trangle.fs:148; the leaf minBy, :76-80).
//    Its median split sorts with F#'s Array.sortInPlaceBy = .NET 6 introsort, restated here so
//    ties fall the same way.
// 3. A binned-SAH BVH2 over the individual primitives, collapsed to a BVH4, is what the GPU
//    traverses, in FP32 with conservatively widened boxes. Every primitive slot carries its reference leaf and position,
//    so the reference's leaf semantics are applied exactly per candidate hit.
//
// The builders of 2 and 3 are in mfx_scene_bvh.cpp. This file assembles the images from them, in
// the stages mfx_build_scene runs one after the other.
#include "mfx_scene.h"

#include <chrono>
#include <cstdlib>
#include <cstring>

#include "mfx_build.h"
#include "mfx_scene_bvh.h"

using namespace mfx_bvh;

namespace {

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

const char* const TOO_LARGE = "scene too large for the traversal image";

// ---- an instanced scene stands for its expansion (mfx_instance); translated entries that share a
//      template range are traced two-level through one template BVH -------------------------------
struct Use {
    int64_t wbase, count;  // its world primitives
    double off[3];
    int tmpl;
};
struct InstancePlan {
    std::vector<mfx_prim> world;                         // the expansion
    std::vector<Use> uses;                               // the entries traced through a template BVH
    std::vector<std::pair<int64_t, int64_t>> templates;  // (first, count) in the template array
};

bool plan_instances(const mfx_scene_desc* d0, const mfx_instance* instances, int ninstances, bool flatten,
                    InstancePlan& plan, std::string& err) {
    if (!d0) {
        err = "null scene";
        return false;
    }
    if (!mfx_expand(d0->prims, d0->nprims, instances, ninstances, plan.world, err)) return false;
    std::vector<int> uses_of_range(ninstances, 0);
    for (int k = 0; k < ninstances; ++k)
        for (int q = 0; q < ninstances; ++q)
            if (!(instances[q].flags & MFX_INSTANCE_VERBATIM) && instances[q].first == instances[k].first &&
                instances[q].count == instances[k].count)
                ++uses_of_range[k];
    int64_t wb = 0;
    for (int k = 0; k < ninstances; ++k) {
        const mfx_instance& e = instances[k];
        if (!flatten && !(e.flags & MFX_INSTANCE_VERBATIM) && e.count > 0 && uses_of_range[k] >= 2) {
            int tm = 0;
            while (tm < (int)plan.templates.size() && plan.templates[tm] != std::make_pair(e.first, e.count)) ++tm;
            if (tm == (int)plan.templates.size()) plan.templates.emplace_back(e.first, e.count);
            plan.uses.push_back(Use{wb, e.count, {e.offset[0], e.offset[1], e.offset[2]}, tm});
        }
        wb += e.count;
    }
    if ((int)plan.uses.size() > MFX_INST_MAX) {
        err = "too many instances";
        return false;
    }
    return true;
}

bool all_finite(const double* v, int k) {
    for (int i = 0; i < k; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// The light and the create-time camera hold no NaN or inf (mfx_set_camera's rule for a later camera:
// direction, fov and aspect count without `derived`, topleft, right and down with it). The primitives'
// values are checked where their records are made (make_prim_records), before this.
bool validate_light_camera(const mfx_scene_desc& d, std::string& err) {
    for (int k = 0; k < 4; ++k)
        if (!all_finite(d.light.p[k], 3)) {
            err = "light corner " + std::to_string(k) + " is not finite";
            return false;
        }
    const mfx_pinhole& c = d.camera;
    const char* bad = !all_finite(d.light.normal, 3)      ? "light normal"
                      : !all_finite(d.light.intensity, 3) ? "light intensity"
                      : !all_finite(c.position, 3)        ? "camera position"
                      : c.derived ? (!all_finite(c.topleft, 3) ? "camera topleft"
                                     : !all_finite(c.right, 3) ? "camera right"
                                     : !all_finite(c.down, 3)  ? "camera down"
                                                               : nullptr)
                                  : (!all_finite(c.direction, 3) ? "camera direction"
                                     : !std::isfinite(c.fov)     ? "camera fov"
                                     : !std::isfinite(c.aspect)  ? "camera aspect"
                                                                 : nullptr);
    if (bad) err = std::string(bad) + " is not finite";
    return !bad;
}

// The largest R + T (Extent, below; a template frame: R + |off| + T) the FP32 builders hold: 2^126.
// A plane is round_up(x + eps) with |x| <= R and eps = (float)ldexp(R + T, -19), so at most
// (R + T)(1 + 2^-18) in magnitude; a centroid's sum lo + hi and a centroid box's extent hi - lo are at
// most twice that plus a rounding, below 2^127 (1 + 2^-16) < FLT_MAX: every one finite.
const double EXTENT_MAX = 0x1p126;
const char* const TOO_FAR = "scene extent too large: R + T (the coordinates' magnitude plus a ray's length) must not exceed 2^126";

bool validate_desc(const mfx_scene_desc* d, std::string& err) {
    if (!d || !d->prims || d->nprims < 1) {
        err = "scene has no primitives (Bvh.Build on an empty array throws, BvhNode.fs:26)";
        return false;
    }
    if (d->nprims > (1 << 28)) {
        err = "too many primitives";
        return false;
    }
    if (d->width < 1 || d->height < 1 || d->nmat < 1 || !d->albedo) {
        err = "invalid film size or empty material table";
        return false;
    }
    // one sample of the film is ceil(w/8) * ceil(h/8) 8x8 tiles of path slots, indexed in 32-bit
    // arithmetic by the kernels (path_pixel, k_resolve): reject films whose count reaches 2^31
    if ((int64_t)((d->width + 7) / 8) * ((d->height + 7) / 8) * 64 >= ((int64_t)1 << 31)) {
        err = "film too large: padded paths per sample must stay below 2^31";
        return false;
    }
    // PathIntegrator(bvh, maxDepth, light) with maxDepth < 0 still traces the camera ray and
    // returns black (Integrators.fs:108-109); the reference only ever passes 3 (Scene.fs:304)
    if (d->max_depth < 0) {
        err = "max_depth must be >= 0";
        return false;
    }
    // a path's vertices are recorded for the exact fold (mfx_wavefront.h): at most 16 of them
    if (d->max_depth >= 16) {
        err = "max_depth must be <= 15 (the reference uses 3, Scene.fs:304)";
        return false;
    }
    return true;
}

// ---- primitives: FP64 bounds + slot records, in primitive order --------------------------------
struct PrimRecords {
    const mfx_prim* prims = nullptr;
    std::vector<Box> pb;
    std::vector<int32_t> slot_of, nslot_of;  // a primitive's slots: pslots[slot_of[p] .. + nslot_of[p])
    std::vector<MfxSlot> pslots;
    std::vector<MfxShade> pshade;
};

void add_shade(PrimRecords& r, const mfx_scene_desc& d, D3 n, int mat, int prim, int kind) {
    MfxShade sh{};
    put(sh.n, n);
    sh.material = mat;
    std::memcpy(sh.albedo, d.albedo + 3 * (size_t)mat, sizeof(sh.albedo));
    sh.prim_kind = (prim << 2) | kind;
    r.pshade.push_back(sh);
}
void add_tri(PrimRecords& r, const mfx_scene_desc& d, D3 v0, D3 v1, D3 v2, int mat, int prim, int kind) {
    MfxSlot t{};
    D3 e1 = sub(v1, v0), e2 = sub(v2, v0);
    put(t.a, v0);
    put(t.b, e1);
    put(t.c, e2);
    r.pslots.push_back(t);
    D3 a = cross(e1, e2);
    double al = len(a);
    add_shade(r, d, D3{a.x / al, a.y / al, a.z / al}, mat, prim, kind);  // Trangle.fs:110-111
}

bool make_prim_records(const mfx_scene_desc& d, PrimRecords& r, std::string& err) {
    const int n = (int)d.nprims;
    r.prims = d.prims;
    r.pb.resize(n);
    r.slot_of.resize(n);
    r.nslot_of.resize(n);
    for (int i = 0; i < n; ++i) {
        const mfx_prim& p = d.prims[i];
        if (p.material < 0 || p.material >= d.nmat) {
            err = "primitive " + std::to_string(i) + " has material index out of range";
            return false;
        }
        // what the kind reads must be finite (a triangle's p[3] is not read, nor a sphere's p[1][1] on):
        // per primitive the material, then the kind, then its values in order
        const int nv = p.kind == MFX_PRIM_TRIANGLE ? 3 : p.kind == MFX_PRIM_RECT ? 4 : p.kind == MFX_PRIM_SPHERE ? 1 : 0;
        for (int v = 0; v < nv; ++v)
            if (!all_finite(p.p[v], 3)) {
                err = "primitive " + std::to_string(i) + (p.kind == MFX_PRIM_SPHERE ? ": centre" : ": corner " + std::to_string(v)) +
                      " is not finite";
                return false;
            }
        if (p.kind == MFX_PRIM_SPHERE && !std::isfinite(p.p[1][0])) {
            err = "primitive " + std::to_string(i) + ": radius is not finite";
            return false;
        }
        r.slot_of[i] = (int)r.pslots.size();
        if (p.kind == MFX_PRIM_TRIANGLE) {
            D3 v0 = d3(p.p[0]), v1 = d3(p.p[1]), v2 = d3(p.p[2]);
            r.pb[i] = tri_box(v0, v1, v2);
            add_tri(r, d, v0, v1, v2, p.material, i, MFX_KIND_TRI);
        } else if (p.kind == MFX_PRIM_RECT) {
            D3 v0 = d3(p.p[0]), v1 = d3(p.p[1]), v2 = d3(p.p[2]), v3 = d3(p.p[3]);
            r.pb[i] = join(tri_box(v0, v1, v2), tri_box(v0, v2, v3));  // Rect.fs:18
            add_tri(r, d, v0, v1, v2, p.material, i, MFX_KIND_RECT);
            add_tri(r, d, v0, v2, v3, p.material, i, MFX_KIND_RECT);
        } else if (p.kind == MFX_PRIM_SPHERE) {
            D3 c = d3(p.p[0]);
            double rad = p.p[1][0];
            D3 v{rad, rad, rad};
            r.pb[i] = box2(sub(c, v), add(c, v));  // Sphere.fs:14-15
            MfxSlot t{};
            put(t.a, c);
            t.b[0] = rad;
            r.pslots.push_back(t);
            add_shade(r, d, c, p.material, i, MFX_KIND_SPHERE);  // the shade record of a sphere carries its centre
        } else {
            err = "primitive " + std::to_string(i) + " has an unknown kind";
            return false;
        }
        r.nslot_of[i] = (int)r.pslots.size() - r.slot_of[i];
    }
    return true;
}

// ---- reference leaf grouping: s.ref_indices / leaf_first / leaf_count and tslack, the leaf headers
//      and where each primitive sits in them -------------------------------------------------------
struct RefGrouping {
    std::vector<MfxLeaf> leaves;
    std::vector<int32_t> ref_leaf_of, pos_of;  // per primitive: its reference leaf, its position in it
    std::vector<int32_t> ref16;                // per leaf: 16-byte offset of its record in ref_blob
};

bool group_reference_leaves(const PrimRecords& r, MfxHostScene& s, RefGrouping& g, std::string& err) {
    const std::vector<Box>& pb = r.pb;
    const int n = (int)pb.size();
    s.ref_indices.resize(n);
    for (int i = 0; i < n; ++i) s.ref_indices[i] = i;
    s.leaf_first.clear();
    s.leaf_count.clear();
    {
        const auto t0 = Clock::now();
        RefBvh rb{pb, s.ref_indices, std::vector<double>(n), std::vector<int32_t>(n)};
        Box root = rb.bound(0, n);
        rb.subdivide(0, n, root, s.leaf_first, s.leaf_count, 3);  // up to 8 host threads
        s.ms_ref_bvh = ms_since(t0);
    }
    const int nc = (int)s.leaf_first.size();
    g.leaves.resize(nc);
    for (int c = 0; c < nc; ++c) {
        MfxLeaf& lf = g.leaves[c];
        Box b = pb[s.ref_indices[s.leaf_first[c]]];
        for (int k = 1; k < s.leaf_count[c]; ++k) b = join(b, pb[s.ref_indices[s.leaf_first[c] + k]]);
        put(lf.lo, b.lo);
        put(lf.hi, b.hi);
        lf.first = s.leaf_first[c];
        lf.count = s.leaf_count[c];
        lf.pad = 0;
        lf.kinds = 0;
        for (int k = 0; k < lf.count; ++k) lf.kinds |= r.prims[s.ref_indices[lf.first + k]].kind << (2 * k);
    }
    // tslack (mfx_scene.h): the largest diagonal of a reference leaf none of whose primitives' boxes
    // is the leaf's own (4e-6 more: directions are unit to 1e-6, Sphere.fs:23)
    s.tslack = 0.0;
    for (int c = 0; c < nc; ++c) {
        if (s.leaf_count[c] < 2) continue;
        const MfxLeaf& lf = g.leaves[c];
        bool own = false;
        for (int k = 0; k < lf.count; ++k) {
            const Box& q = pb[s.ref_indices[lf.first + k]];
            own = own || (q.lo.x == lf.lo[0] && q.lo.y == lf.lo[1] && q.lo.z == lf.lo[2] && q.hi.x == lf.hi[0] &&
                          q.hi.y == lf.hi[1] && q.hi.z == lf.hi[2]);
        }
        if (own) continue;
        const double diag = len(D3{lf.hi[0] - lf.lo[0], lf.hi[1] - lf.lo[1], lf.hi[2] - lf.lo[2]});
        if (diag > s.tslack) s.tslack = diag;
    }
    s.tslack *= 1.0 + 4e-6;

    g.ref_leaf_of.resize(n);
    g.pos_of.resize(n);
    g.ref16.resize(nc);
    size_t off = 0;
    for (int c = 0; c < nc; ++c) {
        g.ref16[c] = (int32_t)(off / 16);
        off += sizeof(MfxLeaf);
        for (int k = 0; k < g.leaves[c].count; ++k) {
            const int p = s.ref_indices[g.leaves[c].first + k];
            g.ref_leaf_of[p] = c;
            g.pos_of[p] = k;
            off += sizeof(MfxSlot) * r.nslot_of[p];
        }
    }
    if (off / 16 >= (size_t)0x7fffffff) {
        err = "reference-leaf image too large";
        return false;
    }
    return true;
}

// Slot j of primitive p as every image holds it: its record with its reference leaf's box and `first`
// copied in. The caller sets `info`.
MfxSlot finished_slot(const PrimRecords& r, const RefGrouping& g, int p, int j) {
    const MfxLeaf& rl = g.leaves[g.ref_leaf_of[p]];
    MfxSlot sl = r.pslots[r.slot_of[p] + j];
    std::memcpy(sl.lo, rl.lo, sizeof(sl.lo));
    std::memcpy(sl.hi, rl.hi, sizeof(sl.hi));
    sl.first = rl.first;
    return sl;
}
// the info word of a traversal slot whose shade record is shade[shade]
int32_t slot_info(const PrimRecords& r, const RefGrouping& g, int p, int j, int32_t shade) {
    return shade | (g.pos_of[p] << MFX_INFO_POS_SHIFT) | (r.prims[p].kind << MFX_INFO_KIND_SHIFT) |
           (j == 1 ? MFX_INFO_RECT2 : 0);
}

}  // namespace

// ---- camera (Camera.fs:96-133): the one copy of the constructor (mfx_create, mfx_set_camera,
//      mfx_pinhole_derive) ---------------------------------------------------------------------------
void mfx_derive_camera(const mfx_pinhole& c, MfxCamera& cam) {
    D3 fwd = normalize(d3(c.direction));
    D3 up0 = normalize(D3{0, 1, 0});
    D3 hori0 = cross(fwd, normalize(up0));
    D3 vert0 = cross(hori0, fwd);
    double hori = std::tan(0.5 * c.fov * 3.141592653589793 / 360.);
    double vert = hori / c.aspect;
    D3 up = scale(vert0, vert), right = scale(hori0, hori);
    D3 pos = d3(c.position);
    D3 tl = add(sub(add(pos, scale(fwd, 0.5)), scale(right, 0.5)), scale(up, 0.5));
    put(cam.position, pos);
    put(cam.topleft, tl);
    put(cam.right, right);
    put(cam.down, D3{-up.x, -up.y, -up.z});
    if (c.derived) {  // an existing PinholeCamera's fields, taken as they are
        put(cam.topleft, d3(c.topleft));
        put(cam.right, d3(c.right));
        put(cam.down, d3(c.down));
    }
}

namespace {

// ---- camera and light (Light.fs:31-40) ----------------------------------------------------------
// one light of nlights: pdf = (1 / area) / nlights, two divisions (the second by 1.0 is exact)
void make_light(const mfx_quad_light& L, int nlights, MfxLight& out) {
    D3 q[4] = {d3(L.p[0]), d3(L.p[1]), d3(L.p[2]), d3(L.p[3])};
    D3 tv[2][3] = {{q[0], q[1], q[2]}, {q[0], q[2], q[3]}};
    double area = 0;
    for (int t = 0; t < 2; ++t) {
        D3 e1 = sub(tv[t][1], tv[t][0]), e2 = sub(tv[t][2], tv[t][0]);
        put(out.v0[t], tv[t][0]);
        put(out.e1[t], e1);
        put(out.e2[t], e2);
        double al = len(cross(e1, e2));
        double ta = al * 0.5;  // Trangle.fs:114
        area = (t == 0) ? ta : area + ta;
    }
    out.area = area;
    const double inv = 1. / area;
    out.pdf = inv / (double)nlights;
    put(out.normal, d3(L.normal));
    put(out.color, d3(L.intensity));
}

void set_camera_light(const mfx_scene_desc& d, MfxHostScene& s) {
    mfx_derive_camera(d.camera, s.camera);
    make_light(d.light, 1, s.light);
    s.lights.assign(1, s.light);
}

// ---- what the conservative widening of the boxes is sized by: R bounds the magnitude of every
//      coordinate (primitives, camera, light), T the length of a ray; eps = (R + T) * 2^-19 --------
struct Extent {
    double R = 0, T = 0;
};
// the camera's share (R is a maximum: the order its terms are taken in does not matter)
Extent extent_with_camera(const MfxHostScene& s, const double* pos) {
    Extent x;
    x.R = s.extent_R0;
    for (int a = 0; a < 3; ++a) x.R = std::max(x.R, std::fabs(pos[a]));
    const D3 lo = d3(s.box_lo), hi = d3(s.box_hi);
    x.T = len(sub(hi, lo)) + len(sub(d3(pos), scale(add(lo, hi), 0.5)));
    return x;
}
// records what does not depend on the camera (the scene box, R of the primitives and the light) in s:
// mfx_set_camera sizes eps for another position from them (mfx_camera_eps)
// (every light's corners: a shadow ray ends on any of them; d.light is lights[0] when there is a list)
Extent scene_extent(const mfx_scene_desc& d, const std::vector<Box>& pb, MfxHostScene& s,
                    const mfx_quad_light* lights = nullptr, int nlights = 0) {
    Box all = pb[0];
    for (size_t i = 1; i < pb.size(); ++i) all = join(all, pb[i]);
    double R0 = 0;
    for (double v : {all.lo.x, all.lo.y, all.lo.z, all.hi.x, all.hi.y, all.hi.z}) R0 = std::max(R0, std::fabs(v));
    for (int k = 0; k < 4; ++k)
        for (int a = 0; a < 3; ++a) R0 = std::max(R0, std::fabs(d.light.p[k][a]));
    for (int n = 1; n < nlights; ++n)
        for (int k = 0; k < 4; ++k)
            for (int a = 0; a < 3; ++a) R0 = std::max(R0, std::fabs(lights[n].p[k][a]));
    s.extent_R0 = R0;
    put(s.box_lo, all.lo);
    put(s.box_hi, all.hi);
    return extent_with_camera(s, d.camera.position);
}

struct SahParams {
    int max_leaf = 4;
    float c_isect = 1.5f;
};
SahParams read_sah_params() {
    SahParams p;
    if (const char* e = getenv("MFX_LEAF_MAX")) p.max_leaf = std::max(1, std::min(4, atoi(e)));
    if (const char* e = getenv("MFX_SAH_CI")) p.c_isect = (float)atof(e);
    return p;
}

// ---- traversal images ----------------------------------------------------------------------------
// the input of a SAH build: per item its conservative FP32 box, its centroid and its slot weight
struct Items {
    std::vector<FBox> cb;
    std::vector<float> cent;
    std::vector<int32_t> w;
    explicit Items(int n) : cb(n), cent(3 * (size_t)n), w(n) {}
    void set_centroids() {
        for (size_t i = 0; i < cb.size(); ++i)
            for (int a = 0; a < 3; ++a) cent[3 * i + a] = 0.5f * (cb[i].lo[a] + cb[i].hi[a]);
    }
};

std::vector<float> pack_boxes(const std::vector<FBox>& cb) {  // [n][6]: lo xyz, hi xyz
    std::vector<float> pbox(6 * cb.size());
    for (size_t i = 0; i < cb.size(); ++i)
        for (int a = 0; a < 3; ++a) {
            pbox[6 * i + a] = cb[i].lo[a];
            pbox[6 * i + 3 + a] = cb[i].hi[a];
        }
    return pbox;
}

// BVH2, BVH4 collapse and layout of the items on the GPU (mfx_build.hip; the host path's bytes)
bool gpu_build_images(const Items& it, const SahParams& sah, const MfxGpuLayoutIn& in, MfxGpuImages& g,
                      std::string& err) {
    const std::vector<float> pbox = pack_boxes(it.cb);
    const hipError_t he = mfx_gpu_build_images(pbox.data(), it.cent.data(), it.w.data(), (int)it.cb.size(),
                                               sah.max_leaf, sah.c_isect, in, g);
    if (he != hipSuccess) {
        err = std::string("GPU BVH build: ") + hipGetErrorString(he);
        return false;
    }
    return true;
}

// a traversal leaf's child code: ns slots from slot s0 on
bool leaf_code(int s0, int ns, int32_t& code, std::string& err) {
    if (ns > MFX_LEAF_SLOTS_MAX || s0 >= MFX_SLOTS_MAX) {
        err = TOO_LARGE;
        return false;
    }
    code = (s0 << 3) | (ns - 1);
    return true;
}

// Collapse4's child references become final: a node index moves by `base`, a leaf l becomes
// ~codes[l] (codes == nullptr: the leaves are coded already)
void patch_leaf_codes(std::vector<MfxNode>& nodes, const int32_t* codes, int base) {
    for (MfxNode& nd : nodes)
        for (int k = 0; k < 4; ++k) {
            if (nd.child[k] == MFX_CHILD_EMPTY) continue;
            if (nd.child[k] >= 0)
                nd.child[k] += base;
            else if (codes)
                nd.child[k] = ~codes[~nd.child[k]];
        }
}

// what the image builders keep beside MfxHostScene
struct ImageState {
    std::vector<int32_t> shade_of;  // shade[] index of each world primitive's first slot
    std::vector<int> roots;         // tree roots in nodes[] before renumbering: the top level first
};

// a world primitive's slots at the end of slots[] (the top level / the flat BVH), shade[] in step
void emit_world_prim(const PrimRecords& r, const RefGrouping& g, int p, MfxHostScene& s, ImageState& im) {
    im.shade_of[p] = (int32_t)s.shade.size();
    for (int j = 0; j < r.nslot_of[p]; ++j) {
        MfxSlot sl = finished_slot(r, g, p, j);
        sl.info = slot_info(r, g, p, j, (int32_t)s.shade.size());
        s.slots.push_back(sl);
        s.slot_ref.push_back(g.ref16[g.ref_leaf_of[p]]);
        s.shade.push_back(r.pshade[r.slot_of[p] + j]);
    }
}

// The BVH4 over world items into s.nodes and its leaves' slots into s.slots. Items [0, nl) are the
// world primitives loose[i] (i itself when loose is null), the others instances: solo leaves that a
// ray enters instead of testing. A flat image is the case without instances.
struct WorldLevel {
    Tree t;
    int root = 0, max_stack = 0;
    std::vector<int> at_leaf;  // per leaf of t: the stack entries when it is reached
};
bool build_world_level(const Items& it, const std::vector<char>* solo, const std::vector<int>* loose, int nl,
                       const PrimRecords& r, const RefGrouping& g, const SahParams& sah, MfxHostScene& s,
                       ImageState& im, WorldLevel& L, std::string& err) {
    Tree& t = L.t;
    build_tree(it.cb, it.cent, it.w, solo, sah.max_leaf, sah.c_isect, t);
    s.nodes.clear();
    L.at_leaf.assign(t.leaves.size(), 0);
    Collapse4 c4{t.nodes2, s.nodes};
    c4.leaf_stack = &L.at_leaf;
    L.root = c4.run(t.root2, 0, 0, &t.rootbox);  // always an internal node (a lone leaf gets a parent)
    std::vector<int32_t> code(t.leaves.size());
    for (int l : dfs_leaves(s.nodes, L.root)) {
        const int b = t.leaves[l].first, e = t.leaves[l].second;
        if (e - b == 1 && t.ids[b] >= nl) {
            code[l] = MFX_INST_FLAG | (t.ids[b] - nl);
            continue;
        }
        const int s0 = (int)s.slots.size();
        for (int k = b; k < e; ++k) emit_world_prim(r, g, loose ? (*loose)[t.ids[k]] : t.ids[k], s, im);
        if (!leaf_code(s0, (int)s.slots.size() - s0, code[l], err)) return false;
    }
    patch_leaf_codes(s.nodes, code.data(), 0);
    s.ntleaves = (int32_t)t.leaves.size();
    s.top_slots = (int32_t)s.slots.size();
    s.bvh_depth = c4.max_depth;
    L.max_stack = c4.max_stack;
    im.roots.push_back(L.root);
    return true;
}

// the items of a flat build: every world primitive
Items world_items(const PrimRecords& r, float eps) {
    const int n = (int)r.pb.size();
    Items it(n);
    for (int i = 0; i < n; ++i) {
        it.cb[i] = fbox_of(r.pb[i], eps);
        it.w[i] = r.nslot_of[i];
    }
    it.set_centroids();
    return it;
}

// flat: one SAH BVH2 over the primitives, collapsed to a BVH4
bool build_flat_host(const PrimRecords& r, const RefGrouping& g, const SahParams& sah, MfxHostScene& s,
                     ImageState& im, std::string& err) {
    const Items it = world_items(r, s.eps);
    WorldLevel L;
    if (!build_world_level(it, nullptr, nullptr, (int)r.pb.size(), r, g, sah, s, im, L, err)) return false;
    s.bvh_levels = L.t.levels;
    s.nodes2 = (int32_t)L.t.nodes2.size();
    s.stack_entries = std::max(1, L.max_stack);
    return true;
}

// flat, the whole image on the GPU: BVH2, BVH4 collapse, renumbering, slots in depth-first order
bool build_flat_gpu(const PrimRecords& r, const RefGrouping& g, const SahParams& sah, MfxHostScene& s,
                    ImageState& im, std::string& err) {
    const Items it = world_items(r, s.eps);
    const int n = (int)r.pb.size();
    std::vector<MfxSlot> ps(r.pslots.size());
    std::vector<int32_t> so(n + 1), r16(n);
    for (int p = 0; p < n; ++p) {
        so[p] = r.slot_of[p];
        r16[p] = g.ref16[g.ref_leaf_of[p]];
        for (int j = 0; j < r.nslot_of[p]; ++j) {
            MfxSlot sl = finished_slot(r, g, p, j);
            sl.info = slot_info(r, g, p, j, 0);
            ps[r.slot_of[p] + j] = sl;
        }
    }
    so[n] = (int32_t)r.pslots.size();
    if (r.pslots.size() >= (size_t)MFX_SLOTS_MAX) {
        err = TOO_LARGE;
        return false;
    }
    MfxGpuImages gi;
    const MfxGpuLayoutIn in{ps.data(), r.pshade.data(), so.data(), r16.data(), (int32_t)r.pslots.size(), MFX_TOP_NODES};
    if (!gpu_build_images(it, sah, in, gi, err)) return false;
    s.nodes.swap(gi.nodes);
    s.slots.swap(gi.slots);
    s.slots.resize(r.pslots.size());
    s.slot_ref.swap(gi.slot_ref);
    s.shade.swap(gi.shade);
    im.shade_of.swap(gi.shade_of);
    s.bvh_levels = gi.levels;
    s.nodes2 = gi.nodes2;
    s.bvh_depth = gi.max_depth;
    s.stack_entries = std::max(1, gi.max_stack);
    s.ntleaves = gi.nleaves;
    s.top_slots = (int32_t)s.slots.size();
    s.images_gpu = true;
    im.roots.push_back(0);  // already numbered: renumber_top_nodes is the identity
    return true;
}

// A template BVH over template primitives (local coordinates), node indices moved by `base`. Its leaf
// codes count slots from the start of an instance's own run of world slots: first_slot[i] is template
// primitive i's first slot in such a run (the template's depth-first leaf order).
struct TemplateBvh {
    std::vector<MfxNode> nodes;
    std::vector<int32_t> first_slot;
    int root = 0, nslots = 0, nleaves = 0, max_stack = 0, max_depth = 0, levels = 0, nodes2 = 0;
};
bool template_bvh_host(const Items& it, const SahParams& sah, int base, TemplateBvh& b, std::string& err) {
    Tree bt;
    build_tree(it.cb, it.cent, it.w, nullptr, sah.max_leaf, sah.c_isect, bt);
    Collapse4 c4{bt.nodes2, b.nodes};
    const int root = c4.run(bt.root2, 0, 0, &bt.rootbox);
    b.first_slot.resize(it.w.size());
    std::vector<int32_t> code(bt.leaves.size());
    int local = 0;
    for (int l : dfs_leaves(b.nodes, root)) {
        const int s0 = local;
        for (int k = bt.leaves[l].first; k < bt.leaves[l].second; ++k) {
            const int i = bt.ids[k];
            b.first_slot[i] = local;
            local += it.w[i];
        }
        if (!leaf_code(s0, local - s0, code[l], err)) return false;
    }
    patch_leaf_codes(b.nodes, code.data(), base);
    b.root = base + root;
    b.nslots = local;
    b.nleaves = (int)bt.leaves.size();
    b.max_stack = c4.max_stack;
    b.max_depth = c4.max_depth;
    b.levels = bt.levels;
    b.nodes2 = (int)bt.nodes2.size();
    return true;
}
// BVH2, collapse and layout on the GPU, nodes in preorder (as Collapse4 emits them): the root first
bool template_bvh_gpu(const Items& it, const SahParams& sah, int base, TemplateBvh& b, std::string& err) {
    const int tn = (int)it.w.size();
    std::vector<int32_t> so(tn + 1), r16(tn, 0);
    for (int i = 0; i <= tn; ++i) so[i] = i == 0 ? 0 : so[i - 1] + it.w[i - 1];
    std::vector<MfxSlot> ps(so[tn]);
    std::vector<MfxShade> psh(so[tn]);
    MfxGpuImages gi;
    if (!gpu_build_images(it, sah, MfxGpuLayoutIn{ps.data(), psh.data(), so.data(), r16.data(), so[tn], 0}, gi, err))
        return false;
    b.nodes.swap(gi.nodes);
    patch_leaf_codes(b.nodes, nullptr, base);
    b.root = base;
    b.first_slot.swap(gi.shade_of);
    b.nslots = so[tn];
    b.nleaves = gi.nleaves;
    b.max_stack = gi.max_stack;
    b.max_depth = gi.max_depth;
    b.levels = gi.levels;
    b.nodes2 = gi.nodes2;
    return true;
}

// Per instance its own run of world slots (exact world geometry and reference-leaf data, as a flat
// image holds them) in its template's slot order; shade[] stays in slots[] order.
bool emit_instance_runs(const std::vector<Use>& uses, const std::vector<TemplateBvh>& tbs, const PrimRecords& r,
                        const RefGrouping& g, MfxHostScene& s, ImageState& im, std::string& err) {
    for (const Use& u : uses) {
        const TemplateBvh& tb = tbs[u.tmpl];
        MfxInstance I{};
        std::memcpy(I.off, u.off, sizeof(I.off));
        I.root = tb.root;
        I.slot_base = (int32_t)s.slots.size();
        if ((int64_t)I.slot_base + tb.nslots >= MFX_SLOTS_MAX) {
            err = TOO_LARGE;
            return false;
        }
        s.slots.resize(s.slots.size() + tb.nslots);
        s.slot_ref.resize(s.slot_ref.size() + tb.nslots);
        s.shade.resize(s.shade.size() + tb.nslots);
        for (int64_t i = 0; i < u.count; ++i) {
            const int p = (int)(u.wbase + i);
            const int at = I.slot_base + tb.first_slot[i];
            im.shade_of[p] = at;
            for (int j = 0; j < r.nslot_of[p]; ++j) {
                MfxSlot sl = finished_slot(r, g, p, j);
                sl.info = slot_info(r, g, p, j, at + j);
                s.slots[at + j] = sl;
                s.slot_ref[at + j] = g.ref16[g.ref_leaf_of[p]];
                s.shade[at + j] = r.pshade[r.slot_of[p] + j];
            }
        }
        s.inst.push_back(I);
    }
    return true;
}

// two levels: a top-level BVH over the loose primitives and the instances, one template BVH per
// distinct template range (tprims: the template array, local coordinates)
bool build_two_level(const mfx_prim* tprims, const InstancePlan& plan, const Extent& ext, bool gpu_bvh,
                     const PrimRecords& r, const RefGrouping& g, const SahParams& sah, MfxHostScene& s,
                     ImageState& im, std::string& err) {
    const std::vector<Use>& uses = plan.uses;
    const int n = (int)r.pb.size(), K = (int)uses.size();
    std::vector<int> use_of(n, -1);
    for (int k = 0; k < K; ++k)
        for (int64_t i = 0; i < uses[k].count; ++i) use_of[uses[k].wbase + i] = k;
    double offmax = 0;
    for (const Use& u : uses)
        for (int a = 0; a < 3; ++a) offmax = std::max(offmax, std::fabs(u.off[a]));
    // template frame: coordinates and ray origins up to R + |off| in magnitude (mfx_build_scene refuses
    // this before any BVH work; the check stays beside the eps it guards)
    if (!(ext.R + offmax + ext.T <= EXTENT_MAX)) {
        err = TOO_FAR;
        return false;
    }
    const float eps_t = (float)std::ldexp(ext.R + offmax + ext.T, -19);
    s.inst_offmax = offmax;
    s.eps_templates = eps_t;
    // top level: loose primitives (items 0 .. nl-1), then the instances (solo leaves)
    std::vector<int> loose;
    for (int i = 0; i < n; ++i)
        if (use_of[i] < 0) loose.push_back(i);
    const int nl = (int)loose.size(), ni = nl + K;
    Items top(ni);
    std::vector<char> solo(ni, 0);
    for (int i = 0; i < nl; ++i) {
        top.cb[i] = fbox_of(r.pb[loose[i]], s.eps);
        top.w[i] = r.nslot_of[loose[i]];
    }
    for (int k = 0; k < K; ++k) {
        FBox f = FBox::empty();
        for (int64_t i = 0; i < uses[k].count; ++i) f.grow(fbox_of(r.pb[uses[k].wbase + i], s.eps));
        top.cb[nl + k] = f;
        top.w[nl + k] = 8;  // ~ a few node steps and leaves: only steers the top-level SAH
        solo[nl + k] = 1;
    }
    top.set_centroids();
    WorldLevel L;
    if (!build_world_level(top, &solo, &loose, nl, r, g, sah, s, im, L, err)) return false;
    s.tlas_nodes = (int32_t)s.nodes.size();

    std::vector<TemplateBvh> tbs(plan.templates.size());
    int blas_depth = 0;
    for (size_t tm = 0; tm < tbs.size(); ++tm) {
        const int64_t tf = plan.templates[tm].first;
        const int tn = (int)plan.templates[tm].second;
        Items it(tn);
        for (int i = 0; i < tn; ++i) {
            const mfx_prim& p = tprims[tf + i];
            it.cb[i] = fbox_of(prim_box(p), eps_t);
            it.w[i] = p.kind == MFX_PRIM_RECT ? 2 : 1;
        }
        it.set_centroids();
        TemplateBvh& b = tbs[tm];
        const int base = (int)s.nodes.size();
        if (!(gpu_bvh ? template_bvh_gpu(it, sah, base, b, err) : template_bvh_host(it, sah, base, b, err)))
            return false;
        s.nodes.insert(s.nodes.end(), b.nodes.begin(), b.nodes.end());
        im.roots.push_back(b.root);
        s.bvh_levels = std::max(s.bvh_levels, b.levels);
        s.nodes2 += b.nodes2;
        s.ntleaves += b.nleaves;
        s.blas_nodes += (int32_t)b.nodes.size();
        s.blas_slots += b.nslots;
        blas_depth = std::max(blas_depth, b.max_depth);
        std::vector<MfxNode>().swap(b.nodes);
    }
    s.ntemplates = (int32_t)tbs.size();
    if (!emit_instance_runs(uses, tbs, r, g, s, im, err)) return false;
    // the top level's entries when an instance is reached, then the template's own
    int bound = L.max_stack;
    for (size_t l = 0; l < L.t.leaves.size(); ++l) {
        const int b = L.t.leaves[l].first;
        if (L.t.leaves[l].second - b == 1 && L.t.ids[b] >= nl)
            bound = std::max(bound, L.at_leaf[l] + tbs[uses[L.t.ids[b] - nl].tmpl].max_stack);
    }
    s.stack_entries = std::max(1, bound);
    s.bvh_depth += blas_depth;
    return true;
}

// The first MFX_TOP_NODES nodes breadth-first from the root(s) — the top level, then the template
// BVHs' top levels —, then the rest in their order (mfx_layout.h)
void renumber_top_nodes(std::vector<MfxNode>& nodes, const std::vector<int>& roots, std::vector<MfxInstance>& inst) {
    const int nn = (int)nodes.size();
    std::vector<int> bfs{roots[0]};
    size_t h = 0, next_root = 1;
    while ((int)bfs.size() < MFX_TOP_NODES) {
        if (h == bfs.size()) {
            if (next_root == roots.size()) break;
            bfs.push_back(roots[next_root++]);
            continue;
        }
        for (int k = 0; k < 4 && (int)bfs.size() < MFX_TOP_NODES; ++k)
            if (nodes[bfs[h]].child[k] >= 0) bfs.push_back(nodes[bfs[h]].child[k]);
        ++h;
    }
    std::vector<int> idx(nn, -1);
    int next = 0;
    for (int v : bfs) idx[v] = next++;
    for (int v = 0; v < nn; ++v)
        if (idx[v] < 0) idx[v] = next++;
    std::vector<MfxNode> renum(nn);
    for (int v = 0; v < nn; ++v) {
        MfxNode nd = nodes[v];
        for (int k = 0; k < 4; ++k)
            if (nd.child[k] >= 0) nd.child[k] = idx[nd.child[k]];
        renum[idx[v]] = nd;
    }
    nodes.swap(renum);
    for (MfxInstance& I : inst) I.root = idx[I.root];
}

// reference leaves (heap order): FP64 box header + slot copies
void write_ref_blob(const PrimRecords& r, const RefGrouping& g, const ImageState& im, MfxHostScene& s) {
    s.ref_blob.clear();
    for (const MfxLeaf& lf : g.leaves) {
        const uint8_t* hp = (const uint8_t*)&lf;
        s.ref_blob.insert(s.ref_blob.end(), hp, hp + sizeof(MfxLeaf));
        for (int k = 0; k < lf.count; ++k) {
            const int p = s.ref_indices[lf.first + k];
            for (int j = 0; j < r.nslot_of[p]; ++j) {
                MfxSlot sl = finished_slot(r, g, p, j);
                sl.info = (im.shade_of[p] + j) | (k << MFX_INFO_POS_SHIFT);
                const uint8_t* sp = (const uint8_t*)&sl;
                s.ref_blob.insert(s.ref_blob.end(), sp, sp + sizeof(MfxSlot));
            }
        }
    }
    s.ref_blob.resize(s.ref_blob.size() + 3 * sizeof(MfxSlot), 0);
}

}  // namespace

bool mfx_expand(const mfx_prim* prims, int64_t nprims, const mfx_instance* inst, int ninst,
                std::vector<mfx_prim>& world, std::string& err) {
    world.clear();
    if (!prims || nprims < 1 || !inst || ninst < 1) {
        err = "an instanced scene needs template primitives and at least one instance";
        return false;
    }
    int64_t total = 0;
    for (int k = 0; k < ninst; ++k) {
        const mfx_instance& e = inst[k];
        if (e.first < 0 || e.count < 0 || e.first > nprims || e.count > nprims - e.first) {
            err = "instance " + std::to_string(k) + " names primitives outside the template array";
            return false;
        }
        if (e.flags & ~MFX_INSTANCE_VERBATIM) {
            err = "instance " + std::to_string(k) + " has unknown flags";
            return false;
        }
        total += e.count;
    }
    if (total < 1 || total > (1 << 28)) {
        err = total < 1 ? "the instances expand to no primitive" : "too many primitives";
        return false;
    }
    world.reserve((size_t)total);
    for (int k = 0; k < ninst; ++k) {
        const mfx_instance& e = inst[k];
        for (int64_t i = 0; i < e.count; ++i) {
            mfx_prim p = prims[e.first + i];
            if (!(e.flags & MFX_INSTANCE_VERBATIM)) {
                const int nv = p.kind == MFX_PRIM_SPHERE ? 1 : (p.kind == MFX_PRIM_RECT ? 4 : 3);
                for (int v = 0; v < nv; ++v)
                    for (int a = 0; a < 3; ++a) p.p[v][a] = p.p[v][a] + e.offset[a];
            }
            world.push_back(p);
        }
    }
    return true;
}

void mfx_camera_eps(const MfxHostScene& s, const double* pos, float* eps, float* eps_templates) {
    const Extent ext = extent_with_camera(s, pos);
    *eps = (float)std::ldexp(ext.R + ext.T, -19);
    *eps_templates = s.inst.empty() ? 0.f : (float)std::ldexp(ext.R + s.inst_offmax + ext.T, -19);
}

uint64_t mfx_scene_digest(const MfxHostScene& s) {
    uint64_t x = 1469598103934665603ULL;
    auto mix = [&](const void* p, size_t n) {
        const uint8_t* b = (const uint8_t*)p;
        for (size_t i = 0; i < n; ++i) x = (x ^ b[i]) * 1099511628211ULL;
    };
    mix(s.nodes.data(), s.nodes.size() * sizeof(MfxNode));
    mix(s.slots.data(), s.slots.size() * sizeof(MfxSlot));
    mix(s.slot_ref.data(), s.slot_ref.size() * sizeof(int32_t));
    mix(s.ref_blob.data(), s.ref_blob.size());
    mix(s.shade.data(), s.shade.size() * sizeof(MfxShade));
    mix(s.inst.data(), s.inst.size() * sizeof(MfxInstance));
    // several lights: the table too (one light: the digest it always had)
    if (s.lights.size() >= 2) mix(s.lights.data(), s.lights.size() * sizeof(MfxLight));
    return x;
}

bool mfx_prepare_lights(const mfx_quad_light* lights, int nlights, std::vector<MfxLight>& out, std::string& err) {
    if (!lights || nlights < 1 || nlights > MFX_MAX_LIGHTS) {
        err = "nlights must be 1 .. " + std::to_string(MFX_MAX_LIGHTS) + " with a light array";
        return false;
    }
    out.assign((size_t)nlights, MfxLight{});
    for (int n = 0; n < nlights; ++n) {
        const mfx_quad_light& L = lights[n];
        const std::string who = "light " + std::to_string(n);
        for (int k = 0; k < 4; ++k)
            if (!all_finite(L.p[k], 3)) {
                err = who + " corner " + std::to_string(k) + " is not finite";
                return false;
            }
        const char* bad = !all_finite(L.normal, 3) ? " normal" : !all_finite(L.intensity, 3) ? " intensity" : nullptr;
        if (bad) {
            err = who + bad + " is not finite";
            return false;
        }
        make_light(L, nlights, out[n]);
        // (one light keeps mfx_create's behaviour, whatever its area)
        if (nlights >= 2 && !(out[n].area > 0.0 && std::isfinite(out[n].area) && std::isfinite(out[n].pdf))) {
            err = who + " has no finite positive area (its pdf divides the direct term)";
            return false;
        }
    }
    return true;
}

bool mfx_build_scene(const mfx_scene_desc* d0, MfxHostScene& s, std::string& err, bool gpu_bvh,
                     const mfx_instance* instances, int ninstances, bool flatten, const mfx_quad_light* lights,
                     const std::vector<MfxLight>* prepared) {
    const auto t_start = Clock::now();
    InstancePlan plan;
    const mfx_scene_desc* d = d0;
    mfx_scene_desc dw;
    const int nlights = lights && prepared ? (int)prepared->size() : 0;
    if (lights) {  // the list replaces the description's light: lights[0] stands in its place
        if (!d0 || nlights < 1) {
            err = "null scene or no prepared lights";
            return false;
        }
        dw = *d0;
        dw.light = lights[0];
        d = &dw;
    }
    if (instances) {
        if (!plan_instances(d0, instances, ninstances, flatten, plan, err)) return false;
        if (!lights) dw = *d0;
        dw.prims = plan.world.data();
        dw.nprims = (int64_t)plan.world.size();
        d = &dw;
    }
    if (!validate_desc(d, err)) return false;
    s.width = d->width;
    s.height = d->height;
    s.max_depth = d->max_depth;
    s.albedo.assign(d->albedo, d->albedo + 3 * (size_t)d->nmat);

    PrimRecords rec;
    if (!make_prim_records(*d, rec, err)) return false;
    if (!validate_light_camera(*d, err)) return false;
    const Extent ext = scene_extent(*d, rec.pb, s, lights, nlights);
    double offmax = 0;  // a template frame's coordinates reach R + |off| (build_two_level)
    for (const Use& u : plan.uses)
        for (int a = 0; a < 3; ++a) offmax = std::max(offmax, std::fabs(u.off[a]));
    if (!(ext.R + offmax + ext.T <= EXTENT_MAX)) {  // before either BVH is built
        err = TOO_FAR;
        return false;
    }
    RefGrouping grp;
    if (!group_reference_leaves(rec, s, grp, err)) return false;
    set_camera_light(*d, s);
    if (lights) {
        s.lights = *prepared;
        s.light = s.lights[0];  // (N == 1: set_camera_light's own bits, (1 / area) / 1.0)
    }
    s.eps = (float)std::ldexp(ext.R + ext.T, -19);
    s.inst_offmax = 0.0;
    s.eps_templates = 0.f;
    const SahParams sah = read_sah_params();

    const auto t_bvh = Clock::now();
    s.bvh_gpu = gpu_bvh;
    s.images_gpu = false;
    s.bvh_levels = s.nodes2 = 0;
    s.tlas_nodes = s.blas_nodes = s.blas_slots = s.ntemplates = s.top_slots = 0;
    s.slots.clear();
    s.slot_ref.clear();
    s.shade.clear();
    s.inst.clear();
    ImageState im;
    im.shade_of.assign(rec.pb.size(), -1);
    const bool built = !plan.uses.empty() ? build_two_level(d0->prims, plan, ext, gpu_bvh, rec, grp, sah, s, im, err)
                       : gpu_bvh          ? build_flat_gpu(rec, grp, sah, s, im, err)
                                          : build_flat_host(rec, grp, sah, s, im, err);
    if (!built) return false;
    s.ms_bvh = ms_since(t_bvh);
    if (s.shade.size() > MFX_INFO_SHADE_MASK) {
        err = TOO_LARGE;
        return false;
    }
    s.slots.resize(s.slots.size() + MFX_LEAF_SLOTS_MAX, MfxSlot{});  // speculative slot loads stay in bounds

    renumber_top_nodes(s.nodes, im.roots, s.inst);
    write_ref_blob(rec, grp, im, s);
    s.nclusters = (int32_t)grp.leaves.size();
    s.world_slots = (int32_t)rec.pslots.size();
    s.ms_total = ms_since(t_start);
    return true;
}
