// cut_check.cpp — checks the camera cuts (mfx_camera_cuts.h) of host-built scenes against brute force.
// Host only: tests/test_camera_cuts.py runs it (and `make cut_check_san` builds it under ASan + UBSan).
//   cut_check [prims.bin]        the checks below, on a soup of 600 random primitives and, if given, on
//                                the primitives of a file (raw mfx_prim records: the spot scene's)
//   cut_check prims.bin W H      the distribution of cut lengths at capacity MFX_CUT_CAP_MAX on a W x H
//                                film with the first camera (how MFX_CUT_CAP_DEFAULT was chosen)
// For every scene, camera, film (40 x 24, 17 x 9) and capacity: every tile's cut by the host twin; for every
// pixel 16 jitters, the four pixel corners among them: the ray by k_camera's FP64 expressions, the BVH4
// walked with the packet walk's FP32 slab test and no distance limit; every leaf reached must be covered by
// an entry of its tile's cut (itself or an ancestor), and that entry's lb must not exceed the ray's FP32
// entry distance to the entry's box. With the slot cull a leaf entry may hold a part of its leaf's slots, or
// be dropped: a reached leaf under no internal entry has every slot put to the host's restatement of the exact
// test (tri_hit64 / sphere_hit64, the ray's FP64 origin and direction, tMin 1e-6, tMax 99999999), and every
// slot it accepts must lie in the kept range of a leaf entry of the tile's row: none may be lost. Besides the
// soup and the mesh, scenes made against the cull for each film: triangles and rects with an edge through a
// tile's corner ray, along a tile's side (its own and the widened one), edge-on to a ray of the tile (the
// divisor changes sign across it; the camera lies on their plane), with a vertex at the camera, and nearly so.
// Exit status 1 on any failure.
#include <algorithm>
#include <cfloat>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mfx_build.h"
#include "mfx_camera_cuts.h"
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

const double ALBEDO[9] = {0.75, 0.25, 0.25, 0.25, 0.75, 0.25, 0.5, 0.5, 0.5};

mfx_pinhole pinhole(double px, double py, double pz, double dx, double dy, double dz, double fov) {
    mfx_pinhole c;
    std::memset(&c, 0, sizeof(c));
    c.position[0] = px; c.position[1] = py; c.position[2] = pz;
    c.direction[0] = dx; c.direction[1] = dy; c.direction[2] = dz;
    c.fov = fov;
    c.aspect = 16.0 / 9.0;
    return c;
}

mfx_scene_desc desc_of(const std::vector<mfx_prim>& prims, const mfx_pinhole& cam) {
    mfx_scene_desc d;
    std::memset(&d, 0, sizeof(d));
    d.prims = prims.data();
    d.nprims = (int64_t)prims.size();
    d.albedo = ALBEDO;
    d.nmat = 3;
    d.width = 40;
    d.height = 24;
    d.max_depth = 3;
    const double q[4][3] = {{-0.5, 2.5, -0.5}, {0.5, 2.5, -0.5}, {0.5, 2.5, 0.5}, {-0.5, 2.5, 0.5}};
    std::memcpy(d.light.p, q, sizeof(q));
    d.light.normal[1] = -1.0;
    d.light.intensity[0] = d.light.intensity[1] = d.light.intensity[2] = 3.0;
    d.camera = cam;
    return d;
}

// triangles, rects and spheres cycling in [-1, 1]^3
std::vector<mfx_prim> soup(int n, uint64_t seed) {
    Rng r{seed};
    std::vector<mfx_prim> v(n);
    for (int i = 0; i < n; ++i) {
        mfx_prim& p = v[i];
        std::memset(&p, 0, sizeof(p));
        p.material = i % 3;
        const double x = r.in(-1.0, 1.0), y = r.in(-1.0, 1.0), z = r.in(-1.0, 1.0);
        if (i % 3 == 0) {
            p.kind = MFX_PRIM_TRIANGLE;
            const double c[3] = {x, y, z};
            for (int k = 0; k < 3; ++k)
                for (int a = 0; a < 3; ++a) p.p[k][a] = c[a] + (k ? r.in(-0.05, 0.05) : 0.0);
        } else if (i % 3 == 1) {
            p.kind = MFX_PRIM_RECT;
            const double u = r.in(0.02, 0.1), w = r.in(0.02, 0.1), t = r.in(-0.03, 0.03);
            const double q[4][3] = {{x, y, z}, {x + u, y, z + t}, {x + u, y + w, z + t}, {x, y + w, z}};
            std::memcpy(p.p, q, sizeof(q));
        } else {
            p.kind = MFX_PRIM_SPHERE;
            p.p[0][0] = x; p.p[0][1] = y; p.p[0][2] = z;
            p.p[1][0] = r.in(0.01, 0.08);
        }
    }
    return v;
}

// Primitives placed against the slot cull for the camera `def` on a W x H film: per chosen tile, with P(px, py,
// r) the point at r times the unnormalised direction through film point (px, py) (these points lie in planes
// parallel to the film, so a segment between two of one r maps to a segment of the film),
//  - a triangle with an edge through the tile's corner ray, and one with an edge through the widened corner's;
//  - triangles with an edge along the tile's left side, along the widened left side and along its top side;
//  - a rect with a side along the tile's right side;
//  - edge-on triangles: their plane holds the camera position and the ray through the tile's middle (the
//    divisor changes sign across the tile), exactly and lifted off that plane by 1e-12, 1e-9 and 1e-5;
//  - triangles with a vertex at the camera position, and 1e-9 from it.
// 60 random soup primitives give the BVH some depth.
std::vector<mfx_prim> adversarial(const mfx_pinhole& def, int W, int H) {
    MfxCamera cam;
    mfx_derive_camera(def, cam);
    std::vector<mfx_prim> v = soup(60, 61);
    const auto P = [&](double px, double py, double r, double* out) {
        const mfx_cut::V3 c = mfx_cut::film_dir(cam, px, py, W, H);
        out[0] = cam.position[0] + r * c.x; out[1] = cam.position[1] + r * c.y; out[2] = cam.position[2] + r * c.z;
    };
    const auto tri = [&](const double* a, const double* b, const double* c) {
        mfx_prim p;
        std::memset(&p, 0, sizeof(p));
        p.kind = MFX_PRIM_TRIANGLE;
        p.material = (int)(v.size() % 3);
        std::memcpy(p.p[0], a, 24); std::memcpy(p.p[1], b, 24); std::memcpy(p.p[2], c, 24);
        v.push_back(p);
    };
    const int tiles_x = (W + 7) / 8, tiles_y = (H + 7) / 8;
    const int picks[3][2] = {{0, 0}, {tiles_x / 2, tiles_y / 2}, {tiles_x - 1, tiles_y - 1}};  // the last one is padded
    for (const auto& pk : picks) {
        const double x0 = pk[0] * 8, y0 = pk[1] * 8, x1 = std::min<double>(x0 + 8, W), y1 = std::min<double>(y0 + 8, H);
        const double xm = 0.5 * (x0 + x1), ym = 0.5 * (y0 + y1);
        double a[3], b[3], c[3], d[3];
        for (const double w : {0.0, 1.0}) {  // the tile's own corner, the widened one
            P(x0 - w - 3, y0 - w - 2, 2.0, a); P(x0 - w + 3, y0 - w + 2, 2.0, b); P(x0 - w - 6, y0 - w + 7, 2.0, c);
            tri(a, b, c);
            tri(b, a, c);  // and facing the other way
        }
        for (const double w : {0.0, 1.0}) {  // along the left side, away from the tile and over it
            P(x0 - w, y0 - 5, 2.5, a); P(x0 - w, y1 + 5, 2.5, b);
            P(x0 - w - 9, ym, 2.5, c); tri(a, b, c);
            P(x0 - w + 9, ym, 2.5, c); tri(a, b, c);
        }
        P(x0 - 4, y0, 3.0, a); P(x1 + 4, y0, 3.0, b); P(xm, y0 - 7, 3.0, c); tri(a, b, c);  // along the top side
        {  // a rect beside the tile, one side along the tile's right side
            mfx_prim p;
            std::memset(&p, 0, sizeof(p));
            p.kind = MFX_PRIM_RECT;
            P(x1, y0, 2.2, a); P(x1 + 6, y0, 2.2, b); P(x1 + 6, y1, 2.2, c); P(x1, y1, 2.2, d);
            std::memcpy(p.p[0], a, 24); std::memcpy(p.p[1], b, 24); std::memcpy(p.p[2], c, 24); std::memcpy(p.p[3], d, 24);
            v.push_back(p);
        }
        for (const double lift : {0.0, 1e-12, 1e-9, 1e-5}) {  // edge-on: the plane through the camera and the middle ray
            P(xm, ym, 1.5, a); P(xm, ym, 3.0, b); P(xm + 4, ym + 1, 2.0, c);
            c[1] += lift;
            tri(a, b, c);
        }
        for (const double off : {0.0, 1e-9}) {  // a vertex at the camera
            a[0] = cam.position[0] + off; a[1] = cam.position[1]; a[2] = cam.position[2];
            P(x0 - 2, y0 - 2, 2.0, b); P(x1 + 2, ym, 2.0, c);
            tri(a, b, c);
        }
    }
    return v;
}

bool load_prims(const char* path, std::vector<mfx_prim>& v) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (bytes <= 0 || bytes % (long)sizeof(mfx_prim) != 0) {
        std::fclose(f);
        return false;
    }
    v.resize((size_t)bytes / sizeof(mfx_prim));
    const size_t got = std::fread(v.data(), sizeof(mfx_prim), v.size(), f);
    std::fclose(f);
    return got == v.size();
}

// make_rayf (mfx_trace_common.h) on the host
struct RayF {
    float ix, iy, iz, oix, oiy, oiz;
};
RayF make_rayf(const double* o, const double* d) {
    float dx = (float)d[0], dy = (float)d[1], dz = (float)d[2];
    const float tiny = 1e-20f;
    if (std::fabs(dx) < tiny) dx = std::copysign(tiny, dx);
    if (std::fabs(dy) < tiny) dy = std::copysign(tiny, dy);
    if (std::fabs(dz) < tiny) dz = std::copysign(tiny, dz);
    RayF r;
    r.ix = 1.0f / dx; r.iy = 1.0f / dy; r.iz = 1.0f / dz;
    r.oix = (float)o[0] * r.ix; r.oiy = (float)o[1] * r.iy; r.oiz = (float)o[2] * r.iz;
    return r;
}
// the packet node step's test of child k (the general form; the octant form gives the same bits), no
// distance limit: true with the entry distance n when the ray's FP32 test hits the box
bool slab(const MfxNode& nd, int k, const RayF& r, float& n) {
    const float a0 = std::fmaf(nd.lox[k], r.ix, -r.oix), a1 = std::fmaf(nd.hix[k], r.ix, -r.oix);
    const float b0 = std::fmaf(nd.loy[k], r.iy, -r.oiy), b1 = std::fmaf(nd.hiy[k], r.iy, -r.oiy);
    const float c0 = std::fmaf(nd.loz[k], r.iz, -r.oiz), c1 = std::fmaf(nd.hiz[k], r.iz, -r.oiz);
    n = std::fmax(std::fmax(std::fmin(a0, a1), std::fmin(b0, b1)), std::fmax(std::fmin(c0, c1), 0.0f));
    const float f = std::fmin(std::fmin(std::fmax(a0, a1), std::fmax(b0, b1)), std::fmin(std::fmax(c0, c1), FLT_MAX));
    return n <= f;
}

struct Totals {
    long long rays = 0, leaves = 0, uncovered = 0, lb_above = 0, tiles = 0, root = 0, empty = 0, multi = 0;
    long long accepted = 0, lost = 0, slots_seen = 0, slots_culled = 0, dropped = 0, narrowed = 0;
};

// the entry of an internal node or the root; for a leaf's child word, the leaf entry that holds a part of
// its slots (leaves are disjoint runs of slots, so at most one does)
int find_entry(const MfxCutEntry* row, int cap, int code) {
    for (int i = 0; i < cap && row[i].code != MFX_CUT_END; ++i) {
        if (row[i].code == code) return i;
        if (code < 0 && row[i].code < 0) {
            const int lc = ~code, ec = ~row[i].code;
            if ((ec >> 3) >= (lc >> 3) && (ec >> 3) + (ec & 7) <= (lc >> 3) + (lc & 7)) return i;
        }
    }
    return -1;
}

// tri_hit64 / sphere_hit64 (mfx_trace_common.h) on the host: the same operations in the same order
struct D3 {
    double x, y, z;
};
D3 d3(const double* p) { return {p[0], p[1], p[2]}; }
D3 vsub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
double vdot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
D3 vcross(D3 a, D3 v) { return {a.y * v.z - a.z * v.y, a.z * v.x - a.x * v.z, a.x * v.y - a.y * v.x}; }
bool tri_hit64(const MfxSlot& s, D3 o, D3 d, double tMin) {
    const D3 e1 = d3(s.b), e2 = d3(s.c);
    const D3 s1 = vcross(d, e2);
    const double divisor = vdot(s1, e1);
    if (std::fabs(divisor) < 1e-6) return false;
    const double inv = 1. / divisor;
    const D3 dd = vsub(o, d3(s.a));
    const double b1 = vdot(dd, s1) * inv;
    if (b1 < 0. || b1 > 1.) return false;
    const D3 s2 = vcross(dd, e1);
    const double b2 = vdot(d, s2) * inv;
    if (b2 < 0. || (b1 + b2) >= 1.) return false;
    const double t = vdot(e2, s2) * inv;
    return t > tMin;
}
bool sphere_hit64(const MfxSlot& s, D3 o, D3 d, double tMin, double tMax) {
    const D3 oc = vsub(o, d3(s.a));
    const double a = 1.;
    const double b = 2.0 * vdot(oc, d);
    const double c = vdot(oc, oc) - s.b[0] * s.b[0];
    const double disc = b * b - 4.0 * a * c;
    if (disc > 0) {
        const double rd = std::sqrt(disc);
        const double q = (b < 0.) ? -0.5 * (b - rd) : -0.5 * (b + rd);
        const double t0 = q, t1 = c / q;
        const double tmn = t0 < t1 ? t0 : t1, tmx = t0 > t1 ? t0 : t1;
        if (tmn >= tMin && tmn < tMax) return true;
        if (tmx > tMin && tmx < tMax) return true;
    }
    return false;
}

// a reached leaf under no internal entry: every slot the exact test accepts lies in the kept range of the
// leaf's entry (cov, -1: the entry was dropped)
void check_leaf_slots(const std::vector<MfxSlot>& slots, int child, const double* o, const double* d, const MfxCutEntry* row,
                      int cov, Totals& t) {
    const int lc = ~child, s0 = lc >> 3, n = (lc & 7) + 1;
    int k0 = 0, k1 = 0;  // the kept range, as slot indices
    if (cov >= 0) {
        const int ec = ~row[cov].code;
        k0 = ec >> 3;
        k1 = k0 + (ec & 7) + 1;
    }
    for (int k = 0; k < n; ++k) {
        const MfxSlot& sl = slots[s0 + k];
        const int kind = (sl.info >> MFX_INFO_KIND_SHIFT) & 3;
        const bool hit = kind == MFX_KIND_SPHERE ? sphere_hit64(sl, d3(o), d3(d), 1e-6, 99999999.) : tri_hit64(sl, d3(o), d3(d), 1e-6);
        if (!hit) continue;
        ++t.accepted;
        if (s0 + k < k0 || s0 + k >= k1) ++t.lost;
    }
}

// one ray against its tile's row
void check_ray(const std::vector<MfxNode>& nodes, const std::vector<MfxSlot>& slots, const RayF& r, const double* o,
               const double* d, const MfxCutEntry* row, int cap, Totals& t) {
    struct Item {
        int node, cov;
    };
    std::vector<Item> stack{{0, find_entry(row, cap, 0)}};
    while (!stack.empty()) {
        const Item it = stack.back();
        stack.pop_back();
        const MfxNode& nd = nodes[it.node];
        for (int k = 0; k < 4; ++k) {
            if (nd.child[k] == MFX_CHILD_EMPTY) continue;
            float n = 0.f;
            if (!slab(nd, k, r, n)) continue;
            int cov = it.cov;
            const bool above = cov < 0;  // no internal entry above this child
            if (cov < 0) {
                cov = find_entry(row, cap, nd.child[k]);
                if (cov >= 0 && !(row[cov].lb <= n)) ++t.lb_above;
            }
            if (nd.child[k] >= 0) {
                stack.push_back({nd.child[k], cov});
            } else {
                ++t.leaves;
                // a leaf of its own: covered by what its entry keeps (a dropped entry keeps nothing); without
                // the slot cull an entry is never dropped, and a missing one is a reached leaf not covered
                if (above) check_leaf_slots(slots, nd.child[k], o, d, row, cov, t);
                if (cov < 0 && !MFX_CUT_SLOT_CULL) ++t.uncovered;
            }
        }
    }
}

void check_case(const char* scene, const char* camname, const MfxHostScene& s, const MfxCamera& cam, int W, int H, int cap,
                Totals& all, double* root_share = nullptr) {
    const int tiles_x = (W + 7) / 8, tiles_y = (H + 7) / 8;
    std::vector<MfxCutEntry> table((size_t)tiles_x * tiles_y * cap);
    MfxCutStats st;
    mfx_cut::table_host(s.nodes.data(), s.slots.data(), cam, W, H, cap, table.data(), st);
    Totals t;
    t.slots_seen = (long long)st.slots_seen; t.slots_culled = (long long)st.slots_culled;
    t.dropped = (long long)st.leaves_dropped; t.narrowed = (long long)st.leaves_narrowed;
    t.tiles = (long long)tiles_x * tiles_y;
    t.root = (long long)st.root_tiles;
    t.empty = (long long)st.empty_tiles;
    for (int n = 2; n <= MFX_CUT_CAP_MAX; ++n) t.multi += (long long)st.hist[n];
    Rng jr{(uint64_t)(W * 131 + H * 7 + cap)};
    const double one = 1.0 - 0x1p-53;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const MfxCutEntry* row = table.data() + (size_t)((y / 8) * tiles_x + x / 8) * cap;
            for (int j = 0; j < 16; ++j) {
                const double ju = j < 4 ? ((j & 1) ? one : 0.0) : jr.unit(), jv = j < 4 ? ((j & 2) ? one : 0.0) : jr.unit();
                // GetRay (Camera.fs:134-139) as k_camera evaluates it
                const double u = ((double)x + ju) / (double)W, v = ((double)y + jv) / (double)H;
                double o[3], d[3];
                for (int a = 0; a < 3; ++a) {
                    o[a] = cam.position[a];
                    d[a] = ((cam.topleft[a] + cam.right[a] * u) + cam.down[a] * v) - o[a];
                }
                const double l = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                if (l != 0.0)
                    for (int a = 0; a < 3; ++a) d[a] = d[a] / l;
                ++t.rays;
                check_ray(s.nodes, s.slots, make_rayf(o, d), o, d, row, cap, t);
            }
        }
    std::printf("%s %s %dx%d cap=%d: tiles=%lld root=%lld empty=%lld multi=%lld mean_len=%.3f max_len=%llu rays=%lld leaves=%lld"
                " uncovered=%lld lb_above=%lld accepted=%lld lost=%lld slots_seen=%lld slots_culled=%lld dropped=%lld narrowed=%lld\n",
                scene, camname, W, H, cap, t.tiles, t.root, t.empty, t.multi, (double)st.len_sum / (double)t.tiles, st.len_max,
                t.rays, t.leaves, t.uncovered, t.lb_above, t.accepted, t.lost, t.slots_seen, t.slots_culled, t.dropped, t.narrowed);
    if (root_share) *root_share = (double)t.root / (double)t.tiles;
    all.rays += t.rays; all.leaves += t.leaves; all.uncovered += t.uncovered; all.lb_above += t.lb_above;
    all.tiles += t.tiles; all.root += t.root; all.empty += t.empty; all.multi += t.multi;
    all.accepted += t.accepted; all.lost += t.lost; all.slots_seen += t.slots_seen; all.slots_culled += t.slots_culled;
    all.dropped += t.dropped; all.narrowed += t.narrowed;
}

bool build(const std::vector<mfx_prim>& prims, const mfx_pinhole& cam, MfxHostScene& s) {
    const mfx_scene_desc d = desc_of(prims, cam);
    std::string err;
    if (!mfx_build_scene(&d, s, err)) {
        std::printf("build FAILED: %s\n", err.c_str());
        return false;
    }
    return true;
}

struct NamedCam {
    const char* name;
    mfx_pinhole cam;
};

// the scene's cameras: the default one, then five around the scene box's centre c and half diagonal R
std::vector<NamedCam> cameras(const mfx_pinhole& def, const MfxHostScene& s) {
    double c[3], R = 0.0;
    for (int a = 0; a < 3; ++a) {
        c[a] = 0.5 * (s.box_lo[a] + s.box_hi[a]);
        R = std::max(R, 0.5 * (s.box_hi[a] - s.box_lo[a]));
    }
    const double* p = def.position;
    const double* d = def.direction;
    const double dl = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    return {{"default", def},
            {"inside", pinhole(c[0], c[1], c[2], d[0], d[1], d[2], 90.0)},
            {"away", pinhole(p[0], p[1], p[2], -d[0], -d[1], -d[2], 90.0)},
            {"axis", pinhole(c[0], c[1], c[2] + 3.0 * R, 0.0, 0.0, -1.0, 90.0)},
            {"far_0.6deg", pinhole(c[0] - 200.0 * R * d[0] / dl, c[1] - 200.0 * R * d[1] / dl, c[2] - 200.0 * R * d[2] / dl, d[0],
                                   d[1], d[2], 0.6)},
            {"fov120", pinhole(p[0], p[1], p[2], d[0], d[1], d[2], 120.0)}};
}

int check_scene(const char* name, const std::vector<mfx_prim>& prims, const mfx_pinhole& def, bool cap_root_share, Totals& all) {
    MfxHostScene s;
    if (!build(prims, def, s)) return 1;
    int bad = 0;
    for (const NamedCam& nc : cameras(def, s)) {
        MfxCamera cam;
        mfx_derive_camera(nc.cam, cam);
        const int films[2][2] = {{40, 24}, {17, 9}};
        for (const auto& f : films)
            for (const int cap : {MFX_CUT_CAP_DEFAULT, 1, 2, MFX_CUT_CAP_MAX}) {
                double share = 0.0;
                check_case(name, nc.name, s, cam, f[0], f[1], cap, all, &share);
                if (cap_root_share && cap == MFX_CUT_CAP_DEFAULT && std::strcmp(nc.name, "default") == 0) {
                    std::printf("%s default %dx%d: {root} share %.4f (cap 0.05)\n", name, f[0], f[1], share);
                    if (share > 0.05) {
                        std::printf("FAIL: {root} share above 5 %%\n");
                        ++bad;
                    }
                }
            }
    }
    return bad;
}

int distribution(const std::vector<mfx_prim>& prims, const mfx_pinhole& def, int W, int H) {
    MfxHostScene s;
    if (!build(prims, def, s)) return 1;
    MfxCamera cam;
    mfx_derive_camera(def, cam);
    const int tiles = ((W + 7) / 8) * ((H + 7) / 8);
    for (const int cap : {MFX_CUT_CAP_MAX, MFX_CUT_CAP_DEFAULT}) {
        std::vector<MfxCutEntry> table((size_t)tiles * cap);
        MfxCutStats st;
        mfx_cut::table_host(s.nodes.data(), s.slots.data(), cam, W, H, cap, table.data(), st);
        long long internal = 0, entries = 0;
        for (const MfxCutEntry& e : table)
            if (e.code != MFX_CUT_END) {
                ++entries;
                internal += e.code >= 0;
            }
        std::printf("%dx%d cap=%d nodes=%zu tiles=%d mean=%.3f max=%llu root=%llu empty=%llu internal_entries=%.4f hist:", W, H, cap,
                    s.nodes.size(), tiles, (double)st.len_sum / tiles, st.len_max, st.root_tiles, st.empty_tiles,
                    entries ? (double)internal / (double)entries : 0.0);
        for (int n = 0; n <= cap; ++n) std::printf(" %d:%llu", n, st.hist[n]);
        std::printf("\n");
        // the slot cull: (tile, leaf-entry slot) pairs the cuts took in, the share their entries no longer hold
        std::printf("%dx%d cap=%d slot_cull=%d leaf_entry_slots=%llu culled=%llu culled_share=%.4f entries_dropped=%llu"
                    " entries_narrowed=%llu\n",
                    W, H, cap, MFX_CUT_SLOT_CULL, st.slots_seen, st.slots_culled,
                    st.slots_seen ? (double)st.slots_culled / (double)st.slots_seen : 0.0, st.leaves_dropped, st.leaves_narrowed);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    // the spot scene's camera (scenes/spot.xml) for a primitive file, the digest tool's for the soup
    const mfx_pinhole spot_cam = pinhole(2.4, 1.3, -3.4, -2.4, -1.2, 3.4, 90.0);
    const mfx_pinhole soup_cam = pinhole(0.0, 0.0, 4.5, 0.0, 0.0, -1.0, 90.0);
    std::vector<mfx_prim> mesh;
    if (argc > 1 && !load_prims(argv[1], mesh)) {
        std::printf("cannot read %s\n", argv[1]);
        return 2;
    }
    if (argc == 4) return distribution(mesh, spot_cam, std::atoi(argv[2]), std::atoi(argv[3]));
    if (argc == 11) {  // ... W H px py pz dx dy dz fov: another scene's camera
        double v[7];
        for (int i = 0; i < 7; ++i) v[i] = std::atof(argv[4 + i]);
        return distribution(mesh, pinhole(v[0], v[1], v[2], v[3], v[4], v[5], v[6]), std::atoi(argv[2]), std::atoi(argv[3]));
    }
    Totals all;
    int bad = check_scene("soup_600", soup(600, 600), soup_cam, false, all);
    bad += check_scene("adv_40x24", adversarial(soup_cam, 40, 24), soup_cam, false, all);
    bad += check_scene("adv_17x9", adversarial(soup_cam, 17, 9), soup_cam, false, all);
    if (!mesh.empty()) bad += check_scene("mesh", mesh, spot_cam, true, all);
    std::printf("total: rays=%lld leaves=%lld uncovered=%lld lb_above=%lld tiles=%lld root=%lld empty=%lld multi=%lld accepted=%lld"
                " lost=%lld slots_seen=%lld slots_culled=%lld dropped=%lld narrowed=%lld\n",
                all.rays, all.leaves, all.uncovered, all.lb_above, all.tiles, all.root, all.empty, all.multi, all.accepted, all.lost,
                all.slots_seen, all.slots_culled, all.dropped, all.narrowed);
    if (all.uncovered || all.lb_above) {
        std::printf("FAIL: a reached leaf is not covered, or an entry's lb is above a ray's entry distance\n");
        ++bad;
    }
    if (all.lost) {
        std::printf("FAIL: a slot the exact test accepts lies outside its tile's kept ranges\n");
        ++bad;
    }
    if (all.accepted == 0 || (MFX_CUT_SLOT_CULL && (all.slots_culled == 0 || all.dropped == 0 || all.narrowed == 0))) {
        std::printf("FAIL: vacuous (no slot accepted, or the slot cull culled, dropped or narrowed nothing)\n");
        ++bad;
    }
    if (all.empty == 0 || all.multi == 0 || all.leaves == 0) {
        std::printf("FAIL: vacuous (no empty cut, no cut of more than one entry, or no leaf reached)\n");
        ++bad;
    }
    return bad ? 1 : 0;
}
