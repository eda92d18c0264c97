// mfx_camera_cuts.h — the per-tile BVH cut k_camera's packets start from ("Camera cuts").
// One routine, host- and device-callable: mfx_build.hip runs it one thread per film tile, the host twin
// (mfx_cut::table_host) serves the CPU checker (cut_check.cpp) and the byte comparison of the two tables.
// FP64 throughout, one rounding per operation (-ffp-contract=off), so both give the same bytes.
//
// A tile's cut is a list of at most `cap` entries, each a node of the BVH4 the packet walk walks (an
// internal node or a leaf code) with the FP32 box its parent stores for it and `lb`, a lower bound on the
// distance at which a camera ray of the tile can enter that box. Coverage: every leaf a ray of the tile
// can reach with the walk's FP32 slab test is in the cut, itself or under an entry.
//
// The tile's rays start at the camera position and pass through the tile's rectangle of the film plane.
// The rectangle widened by one pixel on every side gives four corner directions; each pair of adjacent
// corners spans a side plane through the position. With the inward unit normal n of a side plane, a box
// is outside it when its farthest corner along n is: sum_a max(n_a (lo_a - p_a), n_a (hi_a - p_a)) < -m.
// Every ray direction of the tile is a convex combination of the four corner directions of the tile's own
// (unwidened) rectangle, so it suffices that those four lie strictly inside all four planes: `gap` is the
// least n . c / |c| over them, and a tile whose gap is below MFX_CUT_MIN_GAP (a field of view too narrow
// for a pixel to matter, a degenerate or non-finite normal, an opening of 180 degrees or more) takes the
// trivial cut {root}. The margin m = 2^-17 (max |box coordinate| + max |position coordinate|) covers the
// FP32 walk: its ray is the FP64 ray with origin and direction rounded to FP32 (a point of it is within
// 2^-21 of that magnitude of the FP64 ray's), and its slab test accepts a box the ray misses by the
// rounding of plane * (1/d) - o * (1/d), 2^-22 of the same magnitude along each axis; m is eight times
// their sum, measured along n (|n|_1 <= sqrt 3). The FP64 evaluation's own error is 2^-50 of it.
//
// The slot cull (MFX_CUT_SLOT_CULL): a leaf entry of a finished cut keeps only the slots a ray of the tile
// can hit. The exact test of a triangle slot (tri_hit64: v0, e1, e2; o is the camera position for every
// camera ray) is, with dd = o - v0 and the four vectors
//     ND = e2 x e1,  N1 = e2 x dd,  N2 = dd x e1,  N0 = ND - N1 - N2,
// divisor = d . ND, b1 = d . N1 / divisor, b2 = d . N2 / divisor, 1 - b1 - b2 = d . N0 / divisor. N1, N2 and
// N0 are the normals of the triangle's three edge planes through the camera position (e2 x dd = (v2 - o) x
// (v0 - o), and so on), ND is the face normal. The test rejects when b1 < 0, b2 < 0 or b1 + b2 >= 1: when
// one of the three numerators and the divisor have opposite signs. So the slot is culled when, for one sign
// s and one edge k, all four corner directions c of the widened tile have
//     s (c . ND) > mu E^2 |c|   and   s (c . N_k) < -mu (Q + E) E |c|,
// E = max |coordinate of e1, e2|, Q = max |coordinate of dd|, mu = 2^-32 (MFX_CUT_SLOT_MARGIN): the tile
// sees one face of the triangle and lies outside one edge plane. Both inequalities are linear in c, and a
// ray direction d of the tile is a combination sum l_i c_i with l_i >= 0 and sum l_i |c_i| >= |d| = 1 (the
// FP64 rounding of k_camera's direction, 2^-50, is far inside the one-pixel widening, MFX_CUT_MIN_GAP), so
// s (d . ND) > mu E^2 and s (d . N_k) < -mu (Q + E) E for every ray. The edge plane alone does not do: a ray
// behind which the triangle lies has all three numerators on the divisor's side and is rejected by t > tMin
// only, which a camera on the triangle's plane leaves to rounding; hence the condition on ND (a triangle
// that turns its face within the tile is kept).
// The test's rounding: its numerators are sums of six products of magnitude at most 6 Q E, the divisor's of
// 6 E^2, each with an absolute error below 40 eps (2^-47) of that bound, dd's own rounding included; the
// evaluation here (the same products, c in place of d) errs as much, relative to |c|. So the computed
// numerator and divisor keep their signs with a factor 2^14 to spare, and b1 (b2) comes out negative: inv =
// 1 / divisor and the product keep the sign, and |b| >= mu / 6 is far from underflow (scales at which (Q + E) E
// or E^2 times mu is below 2^-900 are not culled). For k = 0 the test compares b1 + b2, both products with
// the same inv, against 1: fl(b1) + fl(b2) >= 1 holds when the numerators' sum exceeds the divisor by more
// than 4 eps |divisor| + eps (|numerator 1| + |numerator 2|) <= 36 eps (Q + E) E, and the exact excess is
// |d . N0| > mu (Q + E) E. The |divisor| < 1e-6 reject only adds misses. Spheres are never culled; a rect's
// two slots go together (leaf_hit pairs them by position).
// A leaf entry whose slots are all culled is dropped (before the capacity is counted, so the expansion may
// open another entry); otherwise its code is narrowed to the smallest run of whole primitives that holds
// every kept slot (a culled middle stays). The box and lb stay the leaf's. A culled slot's test is false
// for every ray of the tile, so it is no candidate: the walk loses none.
#ifndef MFX_CAMERA_CUTS_H
#define MFX_CAMERA_CUTS_H

#include <math.h>
#include <stdint.h>

#include "mfx_layout.h"

#if defined(__HIPCC__)
#define MFX_CUT_HD __host__ __device__ inline
#else
#define MFX_CUT_HD inline
#endif

#define MFX_CUT_CAP_MAX 16     // entries of a tile's row, at most (MFX_CAMERA_CUT_CAP is clamped to it)
#define MFX_CUT_CAP_DEFAULT 8  // the cut-length distribution it was chosen from
#define MFX_CUT_END (-0x7fffffff - 1)  // code of a row's unused entries (no node or leaf code: MFX_CHILD_EMPTY)
#define MFX_CUT_MIN_GAP 0x1p-16
#define MFX_CUT_MARGIN 0x1p-17
#ifndef MFX_CUT_SLOT_CULL
#define MFX_CUT_SLOT_CULL 1  // 0 (A/B builds): leaf entries keep every slot
#endif
#define MFX_CUT_SLOT_MARGIN 0x1p-32
// a trace of fewer samples walks from the root: the build is not worth it
#define MFX_CUT_MIN_SAMPLES 32
// the samples a camera has to serve before its table is built with the slot cull (the
// cull adds 0.81 ms to C2's build and saves 0.0075 ms per sample more: 108 samples)
#define MFX_CUT_CULL_MIN_SAMPLES 128

// 32 B: one scalar load. code == 0 is the root (it has no box: lo / hi are -FLT_MAX / FLT_MAX, unread).
struct alignas(32) MfxCutEntry {
    int32_t code;  // >= 0 an internal node, < 0 a leaf code as a node's child word holds it, or MFX_CUT_END
    float lb;
    float lo[3], hi[3];
};

struct MfxCutStats {  // summed over a table's tiles by its build
    unsigned long long len_sum, len_max, root_tiles, empty_tiles, hist[MFX_CUT_CAP_MAX + 1];
    // the slot cull, over the leaf entries the cuts took in: their slots, those culled, entries dropped
    // whole, entries narrowed
    unsigned long long slots_seen, slots_culled, leaves_dropped, leaves_narrowed;
};

namespace mfx_cut {

struct V3 {
    double x, y, z;
};
MFX_CUT_HD V3 v3(const double* p) { return {p[0], p[1], p[2]}; }
MFX_CUT_HD V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
MFX_CUT_HD V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
MFX_CUT_HD V3 mul(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
MFX_CUT_HD double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
MFX_CUT_HD V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
MFX_CUT_HD double max2(double a, double b) { return a > b ? a : b; }
MFX_CUT_HD double abs1(double a) { return a < 0.0 ? -a : a; }
MFX_CUT_HD bool finite1(double a) { return a - a == 0.0; }

// the direction through film point (px / W, py / H), by k_camera's expressions (Camera.fs:134-139), unnormalised
MFX_CUT_HD V3 film_dir(const MfxCamera& cam, double px, double py, int W, int H) {
    const double u = px / (double)W, v = py / (double)H;
    const V3 target = add(add(v3(cam.topleft), mul(v3(cam.right), u)), mul(v3(cam.down), v));
    return sub(target, v3(cam.position));
}

struct Pyramid {
    V3 n[4];  // inward unit normals of the four side planes
    V3 c[4];  // the widened rectangle's corner directions and their lengths (the slot cull)
    double cl[4];
    V3 pos;
    double mpos;  // max |position coordinate|
    bool ok;      // false: the tile takes the trivial cut
};

MFX_CUT_HD Pyramid pyramid_of(const MfxCamera& cam, int W, int H, int tx, int ty) {
    Pyramid P;
    P.pos = v3(cam.position);
    P.mpos = max2(abs1(P.pos.x), max2(abs1(P.pos.y), abs1(P.pos.z)));
    P.ok = true;
    const int x0 = tx * 8, y0 = ty * 8;
    const int x1 = x0 + 8 < W ? x0 + 8 : W, y1 = y0 + 8 < H ? y0 + 8 : H;
    // the rectangle widened by one pixel: corners [row][column]
    const V3 c00 = film_dir(cam, x0 - 1, y0 - 1, W, H), c01 = film_dir(cam, x1 + 1, y0 - 1, W, H);
    const V3 c10 = film_dir(cam, x0 - 1, y1 + 1, W, H), c11 = film_dir(cam, x1 + 1, y1 + 1, W, H);
    const V3 mid = add(add(c00, c01), add(c10, c11));
    P.c[0] = c00; P.c[1] = c01; P.c[2] = c10; P.c[3] = c11;
    for (int i = 0; i < 4; ++i) P.cl[i] = sqrt(dot(P.c[i], P.c[i]));
    const V3 raw[4] = {cross(c00, c10), cross(c01, c11), cross(c00, c01), cross(c10, c11)};  // left, right, top, bottom
    for (int k = 0; k < 4; ++k) {
        V3 n = raw[k];
        const double l2 = dot(n, n);
        if (!(l2 > 0.0) || !finite1(l2)) {
            P.ok = false;
            n = V3{0.0, 0.0, 0.0};
        } else {
            const double l = sqrt(l2);
            n = mul(n, (dot(n, mid) < 0.0 ? -1.0 : 1.0) / l);
        }
        P.n[k] = n;
    }
    // the tile's own corner directions lie inside every plane by MFX_CUT_MIN_GAP (sine of the angle)
    const V3 in[4] = {film_dir(cam, x0, y0, W, H), film_dir(cam, x1, y0, W, H), film_dir(cam, x0, y1, W, H),
                      film_dir(cam, x1, y1, W, H)};
    for (int i = 0; i < 4; ++i) {
        const double l2 = dot(in[i], in[i]);
        if (!(l2 > 0.0) || !finite1(l2)) {
            P.ok = false;
            continue;
        }
        const double l = sqrt(l2);
        for (int k = 0; k < 4; ++k)
            if (!(dot(P.n[k], in[i]) / l >= MFX_CUT_MIN_GAP)) P.ok = false;
    }
    return P;
}

// max |coordinate| of a box
MFX_CUT_HD double box_mag(const float* lo, const float* hi) {
    double m = 0.0;
    for (int a = 0; a < 3; ++a) m = max2(m, max2(abs1((double)lo[a]), abs1((double)hi[a])));
    return m;
}

// the box lies wholly on the outer side of one of the pyramid's planes
MFX_CUT_HD bool outside(const Pyramid& P, const float* lo, const float* hi) {
    const double m = MFX_CUT_MARGIN * (box_mag(lo, hi) + P.mpos);
    if (!finite1(m)) return false;
    const double p[3] = {P.pos.x, P.pos.y, P.pos.z};
    for (int k = 0; k < 4; ++k) {
        const double n[3] = {P.n[k].x, P.n[k].y, P.n[k].z};
        double s = 0.0;
        for (int a = 0; a < 3; ++a) s += max2(n[a] * ((double)lo[a] - p[a]), n[a] * ((double)hi[a] - p[a]));
        if (s < -m) return true;
    }
    return false;
}

// An FP32 lower bound on the distance at which a ray from the position enters the box: camera rays have
// unit directions, so the Euclidean distance to the box bounds the entry parameter below; it is taken down
// by 2^-20 of itself (the FP32 direction's length and the test's relative rounding) and by the margin (the
// test's absolute rounding, header comment), then rounded down. 0 inside the box.
MFX_CUT_HD float lower_bound(const Pyramid& P, const float* lo, const float* hi) {
    const double p[3] = {P.pos.x, P.pos.y, P.pos.z};
    double d2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double d = max2(max2((double)lo[a] - p[a], p[a] - (double)hi[a]), 0.0);
        d2 += d * d;
    }
    if (!(d2 > 0.0)) return 0.0f;
    const double dist = sqrt(d2);
    const double lb = dist - (dist * 0x1p-20 + MFX_CUT_MARGIN * (box_mag(lo, hi) + P.mpos));
    if (!(lb > 0.0) || !finite1(lb)) return 0.0f;
    float f = (float)lb;
    if ((double)f > lb) f = nextafterf(f, 0.0f);
    return f;
}

MFX_CUT_HD MfxCutEntry root_entry() {
    return MfxCutEntry{0, 0.0f, {-3.402823466e38f, -3.402823466e38f, -3.402823466e38f},
                       {3.402823466e38f, 3.402823466e38f, 3.402823466e38f}};
}

// no ray of the tile passes the slot's exact triangle test (header comment)
MFX_CUT_HD bool slot_culled(const Pyramid& P, const MfxSlot& s) {
    const V3 e1 = v3(s.b), e2 = v3(s.c), dd = sub(P.pos, v3(s.a));
    const V3 nd = cross(e2, e1), n1 = cross(e2, dd), n2 = cross(dd, e1);
    const double E = max2(max2(max2(abs1(e1.x), abs1(e1.y)), abs1(e1.z)), max2(max2(abs1(e2.x), abs1(e2.y)), abs1(e2.z)));
    const double Q = max2(max2(abs1(dd.x), abs1(dd.y)), abs1(dd.z));
    const double tn = MFX_CUT_SLOT_MARGIN * ((Q + E) * E), td = MFX_CUT_SLOT_MARGIN * (E * E);
    if (!(tn > 0x1p-900) || !(td > 0x1p-900) || !finite1(tn)) return false;
    const double s0 = dot(P.c[0], nd) < 0.0 ? -1.0 : 1.0;
    bool out0 = true, out1 = true, out2 = true;
    for (int i = 0; i < 4; ++i) {
        const double hd = s0 * dot(P.c[i], nd), h1 = s0 * dot(P.c[i], n1), h2 = s0 * dot(P.c[i], n2);
        const double h0 = (hd - h1) - h2;
        if (!(hd > td * P.cl[i])) return false;
        const double m = -(tn * P.cl[i]);
        out0 = out0 && h0 < m;
        out1 = out1 && h1 < m;
        out2 = out2 && h2 < m;
    }
    return out0 || out1 || out2;
}

// A leaf child word with the slots no ray of the tile can hit taken off both ends, whole primitives only;
// MFX_CUT_END when none is left. seen / culled: the leaf's slots and those the entry no longer holds.
MFX_CUT_HD int cull_leaf(const Pyramid& P, const MfxSlot* slots, int child, int& seen, int& culled) {
    const int code = ~child;
    seen = culled = 0;
    if (!MFX_CUT_SLOT_CULL || !slots || (code & MFX_INST_FLAG)) return child;
    const int s0 = code >> 3, n = (code & 7) + 1;
    int first = n, end = 0;
    for (int k = 0; k < n;) {
        const int kind = (slots[s0 + k].info >> MFX_INFO_KIND_SHIFT) & 3;
        const int w = kind == MFX_KIND_RECT && k + 1 < n ? 2 : 1;
        bool gone = kind != MFX_KIND_SPHERE && slot_culled(P, slots[s0 + k]);
        if (kind == MFX_KIND_RECT) gone = gone && w == 2 && slot_culled(P, slots[s0 + k + 1]);
        if (!gone) {
            if (k < first) first = k;
            end = k + w;
        }
        k += w;
    }
    seen = n;
    culled = end == 0 ? n : n - (end - first);
    if (end == 0) return MFX_CUT_END;
    return ~(((s0 + first) << 3) | (end - first - 1));
}

// The cut of film tile (tx, ty) into row[0 .. cap): its entries sorted by lb ascending, the rest of the
// row MFX_CUT_END. Returns the length (0: the pyramid misses every box). Starting from {root}, an internal
// entry is replaced by those of its children that are not outside the pyramid whenever the list still
// fits in cap, until no entry can be; an entry that cannot be replaced stays as it is (it covers its
// subtree), so {root} is what a tile whose first level overflows cap keeps.
// list: the working list, entry i at list[i * stride], at least cap entries (the device build keeps it in
// LDS, one column per thread: a private array would live in scratch memory).
// slots: the scene's slot array for the slot cull (null: none); tally: if not null, the cull's four counts
// of MfxCutStats are added to tally[0 .. 4).
MFX_CUT_HD int tile_cut(const MfxNode* nodes, const MfxSlot* slots, const MfxCamera& cam, int W, int H, int tx, int ty, int cap,
                        MfxCutEntry* row, MfxCutEntry* list, int stride, unsigned* tally = nullptr) {
    cap = cap < 1 ? 1 : (cap > MFX_CUT_CAP_MAX ? MFX_CUT_CAP_MAX : cap);
    int n = 1;
    list[0] = root_entry();
    const Pyramid P = pyramid_of(cam, W, H, tx, ty);
    // per list index, 4 bits: the surviving children of an entry that did not fit when it was last looked
    // at (2 .. 4; 0: not known). It is looked at again only once the list is short enough for them.
    uint64_t need = 0;
    bool changed = P.ok;
    while (changed) {
        changed = false;
        for (int i = 0; i < n;) {
            const int code = list[i * stride].code;
            const int known = (int)((need >> (4 * i)) & 15);
            if (code < 0 || (known && n - 1 + known > cap)) {
                ++i;
                continue;
            }
            const MfxNode& nd = nodes[code];
            int k = 0;
            unsigned keep = 0;
            int ccode[4] = {0, 0, 0, 0}, cseen[4] = {0, 0, 0, 0}, cgone[4] = {0, 0, 0, 0};  // leaf children after the slot cull
            for (int c = 0; c < 4; ++c) {
                if (nd.child[c] == MFX_CHILD_EMPTY) continue;
                const float lo[3] = {nd.lox[c], nd.loy[c], nd.loz[c]}, hi[3] = {nd.hix[c], nd.hiy[c], nd.hiz[c]};
                if (outside(P, lo, hi)) continue;
                ccode[c] = nd.child[c];
                if (nd.child[c] < 0) {
                    ccode[c] = cull_leaf(P, slots, nd.child[c], cseen[c], cgone[c]);
                    if (ccode[c] == MFX_CUT_END) continue;  // (counted when the node is opened, below)
                }
                keep |= 1u << c;
                ++k;
            }
            if (n - 1 + k > cap) {
                need = (need & ~((uint64_t)15 << (4 * i))) | ((uint64_t)k << (4 * i));
                ++i;
                continue;
            }
            --n;  // the last entry moves to i (i == n: dropped, or overwritten below), with what is known of it
            list[i * stride] = list[n * stride];
            need = (need & ~((uint64_t)15 << (4 * i))) | (((need >> (4 * n)) & 15) << (4 * i));
            for (int c = 0; c < 4; ++c) {
                if (tally && cseen[c]) {
                    tally[0] += (unsigned)cseen[c];
                    tally[1] += (unsigned)cgone[c];
                    tally[2] += ccode[c] == MFX_CUT_END;
                    tally[3] += ccode[c] != MFX_CUT_END && ccode[c] != nd.child[c];
                }
                if (!((keep >> c) & 1)) continue;
                MfxCutEntry e;
                e.code = ccode[c];
                e.lo[0] = nd.lox[c]; e.lo[1] = nd.loy[c]; e.lo[2] = nd.loz[c];
                e.hi[0] = nd.hix[c]; e.hi[1] = nd.hiy[c]; e.hi[2] = nd.hiz[c];
                e.lb = lower_bound(P, e.lo, e.hi);
                need &= ~((uint64_t)15 << (4 * n));
                list[n * stride] = e;
                ++n;
            }
            changed = true;  // the entry now at i is looked at next
        }
    }
    for (int i = 1; i < n; ++i) {  // insertion sort by (lb, code): a total order, the same on host and device
        const MfxCutEntry e = list[i * stride];
        int j = i;
        while (j > 0 && (list[(j - 1) * stride].lb > e.lb || (list[(j - 1) * stride].lb == e.lb && list[(j - 1) * stride].code > e.code))) {
            list[j * stride] = list[(j - 1) * stride];
            --j;
        }
        list[j * stride] = e;
    }
    for (int i = 0; i < cap; ++i) row[i] = i < n ? list[i * stride] : MfxCutEntry{MFX_CUT_END, 0.0f, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    return n;
}
// the host's form: the working list on the stack
inline int tile_cut(const MfxNode* nodes, const MfxSlot* slots, const MfxCamera& cam, int W, int H, int tx, int ty, int cap,
                    MfxCutEntry* row, unsigned* tally = nullptr) {
    MfxCutEntry list[MFX_CUT_CAP_MAX];
    return tile_cut(nodes, slots, cam, W, H, tx, ty, cap, row, list, 1, tally);
}

MFX_CUT_HD void count_tile(MfxCutStats& s, int n, const MfxCutEntry* row) {
    s.len_sum += (unsigned long long)n;
    if ((unsigned long long)n > s.len_max) s.len_max = (unsigned long long)n;
    if (n == 1 && row[0].code == 0) s.root_tiles += 1;
    if (n == 0) s.empty_tiles += 1;
    s.hist[n] += 1;
}

// the host twin of the device build (mfx_build.hip, mfx_build_cut_table): rows [ty * tiles_x + tx][cap]
inline void table_host(const MfxNode* nodes, const MfxSlot* slots, const MfxCamera& cam, int W, int H, int cap, MfxCutEntry* table,
                       MfxCutStats& stats) {
    const int tiles_x = (W + 7) / 8, tiles_y = (H + 7) / 8;
    stats = MfxCutStats{};
    for (int ty = 0; ty < tiles_y; ++ty)
        for (int tx = 0; tx < tiles_x; ++tx) {
            MfxCutEntry* row = table + (size_t)(ty * tiles_x + tx) * cap;
            unsigned tally[4] = {0, 0, 0, 0};
            count_tile(stats, tile_cut(nodes, slots, cam, W, H, tx, ty, cap, row, tally), row);
            stats.slots_seen += tally[0];
            stats.slots_culled += tally[1];
            stats.leaves_dropped += tally[2];
            stats.leaves_narrowed += tally[3];
        }
}

}  // namespace mfx_cut

#endif
