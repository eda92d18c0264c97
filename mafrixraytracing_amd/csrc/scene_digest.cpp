// scene_digest.cpp — prints digests of host-built scenes (mfx_build_scene with gpu_bvh = false), one
// line per case, then the error text of each bad description. Host only: tests/test_scene_digest.py
// compares the lines with tests/golden/scene_digests.json, which pins the bytes of the host image on
// a machine without a GPU (tests/test_gpu_build.py pins the GPU-built image to the host-built one).
// Scenes come from an integer hash, so the inputs are the same bits under every standard library.
// The camera is left out: it goes through std::tan, which another libm may round differently.
// After those: half_dir (mfx_half.h) against a search over the table of all finite halves, the FP16 node
// image of every scene above (digest, and how many planes are +-inf, subnormal or not rounded outward),
// and soup_600 scaled and moved past and below the binary16 range.
#include <algorithm>
#include <cfloat>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "mfx_build.h"
#include "mfx_half.h"
#include "mfx_scene.h"

// the host build never reaches the GPU entry point
hipError_t mfx_gpu_build_images(const float*, const float*, const int32_t*, int, int, float, const MfxGpuLayoutIn&,
                                MfxGpuImages&) {
    return hipErrorNotSupported;
}

namespace {

struct Rng {  // splitmix64
    uint64_t x;
    uint64_t next() {
        uint64_t z = (x += 0x9e3779b97f4a7c15ULL);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        return z ^ (z >> 31);
    }
    double unit() { return (double)(next() >> 11) * 0x1p-53; }  // [0, 1)
    double in(double lo, double hi) { return lo + (hi - lo) * unit(); }
};

uint64_t fnv(uint64_t x, const void* p, size_t n) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; ++i) x = (x ^ b[i]) * 1099511628211ULL;
    return x;
}
const uint64_t FNV0 = 1469598103934665603ULL;

const double ALBEDO[9] = {0.75, 0.25, 0.25, 0.25, 0.75, 0.25, 0.5, 0.5, 0.5};

mfx_scene_desc desc_of(const std::vector<mfx_prim>& prims) {
    mfx_scene_desc d;
    std::memset(&d, 0, sizeof(d));
    d.prims = prims.data();
    d.nprims = (int64_t)prims.size();
    d.albedo = ALBEDO;
    d.nmat = 3;
    d.width = 32;
    d.height = 18;
    d.max_depth = 3;
    const double q[4][3] = {{-0.5, 2.5, -0.5}, {0.5, 2.5, -0.5}, {0.5, 2.5, 0.5}, {-0.5, 2.5, 0.5}};
    std::memcpy(d.light.p, q, sizeof(q));
    d.light.normal[1] = -1.0;
    d.light.intensity[0] = 17.0;
    d.light.intensity[1] = 12.0;
    d.light.intensity[2] = 4.0;
    d.camera.position[2] = 4.5;
    d.camera.direction[2] = -1.0;
    d.camera.fov = 90.0;
    d.camera.aspect = 16.0 / 9.0;
    return d;
}

void pt(double* dst, double x, double y, double z) {
    dst[0] = x;
    dst[1] = y;
    dst[2] = z;
}

mfx_prim tri(Rng& r, int material, bool grid = false) {
    mfx_prim p;
    std::memset(&p, 0, sizeof(p));
    p.kind = MFX_PRIM_TRIANGLE;
    p.material = material;
    if (grid) {  // every vertex on a 1/4 grid, two legs along different axes: many coincident centroids
        for (int a = 0; a < 3; ++a) p.p[0][a] = (double)((int64_t)(r.next() % 9) - 4) / 4.0;
        const int a1 = (int)(r.next() % 3), a2 = (a1 + 1 + (int)(r.next() % 2)) % 3;
        std::memcpy(p.p[1], p.p[0], sizeof(p.p[0]));
        std::memcpy(p.p[2], p.p[0], sizeof(p.p[0]));
        p.p[1][a1] += (r.next() & 1) ? 0.25 : -0.25;
        p.p[2][a2] += (r.next() & 1) ? 0.25 : -0.25;
        return p;
    }
    for (int a = 0; a < 3; ++a) p.p[0][a] = r.in(-1.0, 1.0);
    for (int k = 1; k < 3; ++k)
        for (int a = 0; a < 3; ++a) p.p[k][a] = p.p[0][a] + r.in(-0.05, 0.05);
    return p;
}

mfx_prim rect(Rng& r, int material) {
    mfx_prim p;
    std::memset(&p, 0, sizeof(p));
    p.kind = MFX_PRIM_RECT;
    p.material = material;
    const double x = r.in(-1.0, 1.0), y = r.in(-1.0, 1.0), z = r.in(-1.0, 1.0);
    const double u = r.in(0.02, 0.1), v = r.in(0.02, 0.1), t = r.in(-0.03, 0.03);
    pt(p.p[0], x, y, z);
    pt(p.p[1], x + u, y, z + t);
    pt(p.p[2], x + u, y + v, z + t);
    pt(p.p[3], x, y + v, z);
    return p;
}

mfx_prim sphere(Rng& r, int material) {
    mfx_prim p;
    std::memset(&p, 0, sizeof(p));
    p.kind = MFX_PRIM_SPHERE;
    p.material = material;
    pt(p.p[0], r.in(-1.0, 1.0), r.in(-1.0, 1.0), r.in(-1.0, 1.0));
    p.p[1][0] = r.in(0.01, 0.08);
    return p;
}

mfx_prim any_kind(Rng& r, int i) {
    return i % 3 == 0 ? tri(r, i % 3) : (i % 3 == 1 ? rect(r, (i / 3) % 3) : sphere(r, (i / 7) % 3));
}

// triangles, rects and spheres cycling; the last fifth exact duplicates of the first; every tenth flat in y
std::vector<mfx_prim> soup(int n, uint64_t seed) {
    Rng r{seed};
    std::vector<mfx_prim> v(n);
    for (int i = 0; i < n; ++i) {
        v[i] = any_kind(r, i);
        if (i % 10 == 9 && v[i].kind != MFX_PRIM_SPHERE) {
            if (v[i].kind == MFX_PRIM_RECT)  // its height goes to z, so that no triangle degenerates
                for (int k = 2; k < 4; ++k) v[i].p[k][2] += v[i].p[k][1] - v[i].p[0][1];
            for (int k = 1; k < 4; ++k) v[i].p[k][1] = v[i].p[0][1];
        }
    }
    const int nd = n / 5;
    for (int i = 0; i < nd; ++i) v[n - nd + i] = v[i];
    return v;
}

mfx_instance entry(int64_t first, int64_t count, double x, double y, double z, int32_t flags = 0) {
    mfx_instance e;
    std::memset(&e, 0, sizeof(e));
    e.first = first;
    e.count = count;
    pt(e.offset, x, y, z);
    e.flags = flags;
    return e;
}

// templates: [0, 40) triangles, [40, 70) rects and spheres, [70, 90) mixed, [90, 100) triangles
std::vector<mfx_prim> template_prims() {
    Rng r{0x7e3a1e5ULL};
    std::vector<mfx_prim> v;
    for (int i = 0; i < 40; ++i) v.push_back(tri(r, i % 3));
    for (int i = 0; i < 30; ++i) v.push_back(i % 2 ? rect(r, i % 3) : sphere(r, (i / 2) % 3));
    for (int i = 0; i < 20; ++i) v.push_back(any_kind(r, i));
    for (int i = 0; i < 10; ++i) v.push_back(tri(r, 2));
    return v;
}
// two template ranges used three times each, one range used once (stays loose), one verbatim entry
std::vector<mfx_instance> two_level_entries() {
    return {entry(0, 40, 0.0, 0.0, 0.0),      entry(40, 30, 2.5, 0.125, -1.0), entry(70, 20, -0.3, 1.7, 0.2),
            entry(0, 40, -3.0, 0.5, 0.75),    entry(40, 30, 0.0, -2.25, 0.1),  entry(90, 10, 9.0, 9.0, 9.0, MFX_INSTANCE_VERBATIM),
            entry(0, 40, 1.1, 2.2, -3.3),     entry(40, 30, -2.5, -0.125, 1.0)};
}

// ---- the FP16 node image (mfx_half.h): its rounding against a table, its bytes, its planes ----------
double half_value(uint16_t h) {  // finite halves only
    const int e = (h >> 10) & 31, m = h & 1023;
    const double v = e == 0 ? std::ldexp((double)m, -24) : std::ldexp((double)(1024 + m), e - 25);
    return (h & 0x8000) ? -v : v;
}

// half_dir by search: the table of the 31,744 finite non-negative halves in ascending order is indexed by
// their bits; away from zero the least entry >= |x| (none: inf), towards zero the greatest entry <= |x|
uint16_t half_dir_by_search(const std::vector<double>& table, float x, bool up) {
    if (std::isinf(x)) return x > 0 ? 0x7c00 : 0xfc00;
    const bool neg = x < 0;
    const double ax = std::fabs((double)x);
    int i;
    if (up != neg) {
        i = (int)(std::lower_bound(table.begin(), table.end(), ax) - table.begin());  // 31744 == 0x7c00: inf
    } else {
        i = (int)(std::upper_bound(table.begin(), table.end(), ax) - table.begin()) - 1;
    }
    return (uint16_t)(i | (neg ? 0x8000 : 0));
}

float float_of_bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, sizeof(f));
    return f;
}

// every half and its two FP32 neighbours, 2,000,000 FP32 bit patterns and a few extremes, both signs,
// both directions
void print_half_selfcheck() {
    std::vector<double> table(0x7c00);
    for (int h = 0; h < 0x7c00; ++h) table[h] = half_value((uint16_t)h);
    int64_t checks = 0, wrong = 0;
    const auto check = [&](float x) {
        if (std::isnan(x)) return;
        for (const float v : {x, -x})
            for (const bool up : {false, true}) {
                ++checks;
                if (mfx_half::half_dir(v, up) != half_dir_by_search(table, v, up)) ++wrong;
            }
    };
    for (int h = 0; h < 0x7c00; ++h) {
        const float f = (float)table[h];
        check(f);
        check(std::nextafter(f, -FLT_MAX));
        check(std::nextafter(f, FLT_MAX));
    }
    Rng r{16};
    for (int i = 0; i < 2000000; ++i) check(float_of_bits((uint32_t)r.next()));
    for (const float x : {65504.f, 65519.996f, 65520.f, 65536.f, 1e30f, FLT_MAX, FLT_MIN, 1.401298464e-45f, 0x1p-24f,
                          0x1p-25f, 0x1p-14f, HUGE_VALF})
        check(x);
    std::printf("half_dir selfcheck checks=%" PRId64 " wrong=%" PRId64 "\n", checks, wrong);
}

struct HalfImage {
    uint64_t digest = FNV0;
    int planes = 0, inf = 0, subnormal = 0, not_outward = 0;  // over the planes of non-empty children
};
HalfImage half_image(const std::vector<MfxNode>& nodes) {
    HalfImage r;
    for (const MfxNode& n : nodes) {
        const MfxNodeH h = mfx_half::node_to_half(n);
        r.digest = fnv(r.digest, &h, sizeof(h));
        const float* lo32[3] = {n.lox, n.loy, n.loz};
        const float* hi32[3] = {n.hix, n.hiy, n.hiz};
        const uint16_t* lo16[3] = {h.lox, h.loy, h.loz};
        const uint16_t* hi16[3] = {h.hix, h.hiy, h.hiz};
        for (int k = 0; k < 4; ++k) {
            if (n.child[k] == MFX_CHILD_EMPTY) continue;
            for (int a = 0; a < 3; ++a)
                for (int side = 0; side < 2; ++side) {
                    const uint16_t b = side ? hi16[a][k] : lo16[a][k];
                    const double f = side ? hi32[a][k] : lo32[a][k];
                    ++r.planes;
                    if ((b & 0x7fff) == 0x7c00) {
                        ++r.inf;
                        if ((b == 0x7c00) != (side == 1)) ++r.not_outward;  // -inf below, +inf above
                        continue;
                    }
                    if ((b & 0x7c00) == 0 && (b & 0x3ff) != 0) ++r.subnormal;
                    if (side ? half_value(b) < f : half_value(b) > f) ++r.not_outward;
                }
        }
    }
    return r;
}

std::vector<std::pair<std::string, HalfImage>> g_half;  // of every scene print_case built, in order

void print_case(const char* name, const mfx_scene_desc& d, const mfx_instance* inst = nullptr, int ninst = 0,
                bool flatten = false) {
    MfxHostScene s;
    std::string err;
    if (!mfx_build_scene(&d, s, err, false, inst, ninst, flatten)) {
        std::printf("%s FAILED: %s\n", name, err.c_str());
        return;
    }
    g_half.emplace_back(name, half_image(s.nodes));
    uint64_t ref = FNV0;
    ref = fnv(ref, s.ref_indices.data(), s.ref_indices.size() * sizeof(int32_t));
    ref = fnv(ref, s.leaf_first.data(), s.leaf_first.size() * sizeof(int32_t));
    ref = fnv(ref, s.leaf_count.data(), s.leaf_count.size() * sizeof(int32_t));
    const uint64_t light = fnv(FNV0, &s.light, sizeof(s.light));
    std::printf("%s image=%016" PRIx64 " ref=%016" PRIx64 " light=%016" PRIx64
                " nclusters=%d ntleaves=%d world_slots=%d tlas_nodes=%d blas_nodes=%d blas_slots=%d ntemplates=%d"
                " top_slots=%d bvh_depth=%d stack_entries=%d bvh_levels=%d nodes2=%d nodes=%zu slots=%zu inst=%zu"
                " eps=%a tslack=%a\n",
                name, mfx_scene_digest(s), ref, light, s.nclusters, s.ntleaves, s.world_slots, s.tlas_nodes,
                s.blas_nodes, s.blas_slots, s.ntemplates, s.top_slots, s.bvh_depth, s.stack_entries, s.bvh_levels,
                s.nodes2, s.nodes.size(), s.slots.size(), s.inst.size(), (double)s.eps, s.tslack);
}

void print_err(const char* name, const mfx_scene_desc& d, const mfx_instance* inst = nullptr, int ninst = 0) {
    MfxHostScene s;
    std::string err;
    const bool ok = mfx_build_scene(&d, s, err, false, inst, ninst, false);
    std::printf("err %s: %s\n", name, ok ? "(accepted)" : err.c_str());
}

// x*s + off on every point, sphere centre, light corner and the camera's position; radii times s
void similar(std::vector<mfx_prim>& v, mfx_scene_desc& d, double s, const double* off) {
    for (mfx_prim& p : v) {
        const int nv = p.kind == MFX_PRIM_SPHERE ? 1 : 4;
        for (int k = 0; k < nv; ++k)
            for (int a = 0; a < 3; ++a) p.p[k][a] = p.p[k][a] * s + off[a];
        if (p.kind == MFX_PRIM_SPHERE) p.p[1][0] *= s;
    }
    for (int a = 0; a < 3; ++a) {
        for (int k = 0; k < 4; ++k) d.light.p[k][a] = d.light.p[k][a] * s + off[a];
        d.camera.position[a] = d.camera.position[a] * s + off[a];
    }
}

// soup_600 past and below the half range: the host image, its FP16 node image and that image's planes
void print_range(double s, double ox, double oy, double oz) {
    std::vector<mfx_prim> v = soup(600, 600);
    mfx_scene_desc d = desc_of(v);
    const double off[3] = {ox, oy, oz};
    similar(v, d, s, off);
    MfxHostScene h;
    std::string err;
    if (!mfx_build_scene(&d, h, err)) {
        std::printf("range soup_600 s=%a off=(%a,%a,%a) FAILED: %s\n", s, ox, oy, oz, err.c_str());
        return;
    }
    const HalfImage hi = half_image(h.nodes);
    std::printf("range soup_600 s=%a off=(%a,%a,%a) image=%016" PRIx64 " nodes2=%d nodes=%zu eps=%a half=%016" PRIx64
                " planes=%d inf=%d (%.3f) subnormal=%d (%.3f) not_outward=%d\n",
                s, ox, oy, oz, mfx_scene_digest(h), h.nodes2, h.nodes.size(), (double)h.eps, hi.digest, hi.planes, hi.inf,
                (double)hi.inf / hi.planes, hi.subnormal, (double)hi.subnormal / hi.planes, hi.not_outward);
}

}  // namespace

int main() {
    {
        Rng r{1};
        const std::vector<mfx_prim> one{tri(r, 0)};
        print_case("one_tri", desc_of(one));
        const std::vector<mfx_prim> two{tri(r, 1), sphere(r, 2)};
        print_case("tri_sphere", desc_of(two));
    }
    {
        const std::vector<mfx_prim> v = soup(600, 600);
        print_case("soup_600", desc_of(v));
    }
    {
        Rng r{5000};
        std::vector<mfx_prim> v;
        for (int i = 0; i < 5000; ++i) v.push_back(tri(r, i % 3, true));
        print_case("grid_5000", desc_of(v));
    }
    const std::vector<mfx_prim> tp = template_prims();
    const std::vector<mfx_instance> two = two_level_entries();
    {
        print_case("two_level", desc_of(tp), two.data(), (int)two.size());
        const std::vector<mfx_instance> only{entry(0, 40, 0.0, 0.0, 0.0), entry(40, 60, 0.5, 0.0, 0.0),
                                             entry(40, 60, -1.5, 2.0, 0.25), entry(0, 40, 0.0, 3.0, 0.0),
                                             entry(0, 40, 4.0, 0.0, -2.0)};
        print_case("inst_only", desc_of(tp), only.data(), (int)only.size());
        print_case("flattened", desc_of(tp), two.data(), (int)two.size(), true);
    }

    // ---- bad descriptions: the message of each, and which of several comes first ----------------
    Rng r{77};
    const std::vector<mfx_prim> good{tri(r, 0), rect(r, 1), sphere(r, 2)};
    {
        mfx_scene_desc d = desc_of(good);
        d.prims = nullptr;
        print_err("null_prims", d);
    }
    {
        std::vector<mfx_prim> v = good;
        v[1].material = 3;
        print_err("material_range", desc_of(v));
        v = good;
        v[2].kind = 3;
        print_err("unknown_kind", desc_of(v));
    }
    {
        mfx_scene_desc d = desc_of(good);
        d.max_depth = -1;
        print_err("max_depth_neg", d);
        d.max_depth = 16;
        print_err("max_depth_16", d);
        d = desc_of(good);
        d.width = 0;
        print_err("width_0", d);
        d = desc_of(good);
        d.width = 65536;  // 8192 x 4096 tiles of 64 paths = 2^31
        d.height = 32768;
        print_err("film_2_31", d);
    }
    {
        const mfx_scene_desc d = desc_of(good);
        const mfx_instance outside[2] = {entry(0, 3, 0, 0, 0), entry(2, 2, 1, 0, 0)};
        print_err("instance_range", d, outside, 2);
        const mfx_instance flags[2] = {entry(0, 3, 0, 0, 0), entry(0, 3, 1, 0, 0, 2)};
        print_err("instance_flags", d, flags, 2);
        const mfx_instance nothing[2] = {entry(0, 0, 0, 0, 0), entry(3, 0, 1, 0, 0)};
        print_err("instances_empty", d, nothing, 2);
    }
    {
        // several errors at once: an unknown kind, a bad material, a zero width and max_depth 16
        std::vector<mfx_prim> v = good;
        v[0].kind = 7;
        v[1].material = -1;
        mfx_scene_desc d = desc_of(v);
        d.width = 0;
        d.max_depth = 16;
        print_err("several", d);
        d.width = 32;
        print_err("several_depth_then_prims", d);
        const mfx_instance bad[2] = {entry(0, 3, 0, 0, 0, 4), entry(5, 1, 0, 0, 0)};
        print_err("several_instanced", d, bad, 2);
    }

    // ---- values no builder can hold: NaN, inf and extents past 2^126 (mfx_scene.cpp EXTENT_MAX) ------
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    {
        std::vector<mfx_prim> v = good;
        v[1].p[2][1] = nan;
        print_err("nan_coordinate", desc_of(v));
        v = good;
        v[2].p[1][0] = inf;
        print_err("inf_radius", desc_of(v));
        v = good;
        v[0].p[3][0] = nan;  // a triangle reads three corners
        v[2].p[1][1] = nan;  // a sphere reads its centre and p[1][0]
        print_err("nan_unused_values", desc_of(v));
        mfx_scene_desc d = desc_of(good);
        d.light.p[2][1] = nan;
        print_err("nan_light_corner", d);
        d = desc_of(good);
        d.light.intensity[1] = inf;
        print_err("inf_light_intensity", d);
        d = desc_of(good);
        d.camera.position[0] = -inf;
        print_err("inf_camera_position", d);
        d = desc_of(good);
        d.camera.fov = nan;
        print_err("nan_camera_fov", d);
        d.camera.derived = 1;  // fov is not read then
        print_err("nan_camera_fov_derived", d);
    }
    {
        // one thin triangle 2a long and the camera c from its box's middle: R = max(a, c), T = 2a + c
        // exactly (the height's square is below an ulp of 4a^2)
        std::vector<mfx_prim> v{good[0]};
        const double a = 0x1p124;
        pt(v[0].p[0], -a, 0.0, 0.0);
        pt(v[0].p[1], a, 0.0, 0.0);
        pt(v[0].p[2], 0.0, 1.0, 0.0);
        mfx_scene_desc d = desc_of(v);
        pt(d.camera.position, 0.0, 0.5, 0x1p124);
        print_err("extent_2_126", d);
        print_case("extent_2_126", d);
        pt(d.camera.position, 0.0, 0.5, 0x1p124 + 0x1p75);
        print_err("extent_past_2_126", d);
        // two uses of one template 2^75 apart: R + T = 2^126 - 2^74, and the template frame adds |off|
        const mfx_instance apart[2] = {entry(0, 1, 0.0, 0.0, 0.0), entry(0, 1, 0.0, 0.0, 0x1p75)};
        pt(d.camera.position, 0.0, 0.5, 0x1p124);
        print_err("extent_past_2_126_by_instance_offset", d, apart, 2);
    }
    {
        // which comes first: primitives in order, per primitive the material, the kind, then its values;
        // the light and the camera after every primitive, the extent last
        std::vector<mfx_prim> v = good;
        v[0].p[0][0] = nan;
        v[1].material = 3;
        print_err("nan_then_material", desc_of(v));
        v = good;
        v[1].material = 3;
        v[1].p[0][0] = nan;
        v[2].p[1][0] = nan;
        print_err("material_and_nan_in_one", desc_of(v));
        v = good;
        v[2].p[0][2] = inf;
        mfx_scene_desc d = desc_of(v);
        d.light.normal[0] = nan;
        d.camera.aspect = nan;
        d.max_depth = 16;
        print_err("depth_then_nan", d);
        d.max_depth = 3;
        print_err("prim_then_light_then_camera", d);
        d.prims = good.data();
        print_err("light_then_camera", d);
        const mfx_instance moved[2] = {entry(0, 3, 0, 0, 0), entry(0, 3, 1, nan, 0)};
        print_err("nan_instance_offset", desc_of(good), moved, 2);
    }

    // ---- the FP16 node image: half_dir against a table, then every scene above ------------------------
    print_half_selfcheck();
    for (const auto& h : g_half)
        std::printf("half %s digest=%016" PRIx64 " planes=%d inf=%d subnormal=%d not_outward=%d\n", h.first.c_str(),
                    h.second.digest, h.second.planes, h.second.inf, h.second.subnormal, h.second.not_outward);
    print_range(1.0, 0.0, 0.0, 0.0);
    print_range(1.0, 1e5, 0.0, -7e4);
    print_range(1.0, 65504.0, 65504.0, -65504.0);
    print_range(1e5, 0.0, 0.0, 0.0);
    print_range(1e-4, 0.0, 0.0, 0.0);
    print_range(1.0, 1e7, 0.0, 0.0);
    print_range(3e19, 0.0, 0.0, 0.0);
    print_range(1e30, 0.0, 0.0, 0.0);
    return 0;
}
