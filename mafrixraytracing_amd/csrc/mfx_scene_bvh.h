// mfx_scene_bvh.h — the host builders behind mfx_scene.cpp (internal; bodies in mfx_scene_bvh.cpp):
// FP64 vectors and boxes with the reference's arithmetic, the reference's heap BVH (its leaf grouping),
// the binned-SAH BVH2 and its collapse to the BVH4 the GPU traverses.
#ifndef MFX_SCENE_BVH_H
#define MFX_SCENE_BVH_H

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <utility>
#include <vector>

#include "../../include/mafrix_rt.h"
#include "mfx_layout.h"

namespace mfx_bvh {

struct D3 {
    double x, y, z;
};
inline D3 d3(const double* p) { return {p[0], p[1], p[2]}; }
inline D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline D3 add(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline D3 scale(D3 v, double a) { return {v.x * a, v.y * a, v.z * a}; }
inline D3 cross(D3 a, D3 v) { return {a.y * v.z - a.z * v.y, a.z * v.x - a.x * v.z, a.x * v.y - a.y * v.x}; }
inline double len(D3 v) { return std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z); }
inline D3 normalize(D3 v) {
    double l = len(v);
    if (l == 0.0) return {0, 0, 0};
    return {v.x / l, v.y / l, v.z / l};
}
inline double comp(D3 v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : v.z); }
inline double mn(double a, double b) { return a < b ? a : b; }
inline double mx(double a, double b) { return a > b ? a : b; }
inline void put(double* dst, D3 v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; }

struct Box {
    D3 lo, hi;
};
inline Box box2(D3 p, D3 q) {  // Bound(p1, p2), Aggregate.fs:9-11
    return {{mn(p.x, q.x), mn(p.y, q.y), mn(p.z, q.z)}, {mx(p.x, q.x), mx(p.y, q.y), mx(p.z, q.z)}};
}
inline Box join(Box a, Box b) {  // Bound.Union, Aggregate.fs:58-61
    return box2({mn(a.lo.x, b.lo.x), mn(a.lo.y, b.lo.y), mn(a.lo.z, b.lo.z)},
                {mx(a.hi.x, b.hi.x), mx(a.hi.y, b.hi.y), mx(a.hi.z, b.hi.z)});
}
inline Box join_pt(Box a, D3 p) {
    return box2({mn(a.lo.x, p.x), mn(a.lo.y, p.y), mn(a.lo.z, p.z)}, {mx(a.hi.x, p.x), mx(a.hi.y, p.y), mx(a.hi.z, p.z)});
}
inline Box tri_box(D3 a, D3 b, D3 c) { return join_pt(box2(a, b), c); }  // Trangle.fs:113

// FP64 box of a primitive in its own coordinates (Trangle.fs:113, Rect.fs:18, Sphere.fs:14-15)
Box prim_box(const mfx_prim& p);

// ---- reference heap BVH: leaf grouping only ------------------------------------------------
// Subtrees are independent: each sorts only its own index range (keys / tmp are indexed by the
// range, not from 0), so the two halves of the top splits run on their own host threads and their
// leaves are concatenated left to right — the same leaves, in the same order, as the sequential
// recursion (the introsort of every range is unchanged).
struct RefBvh {
    const std::vector<Box>& pb;
    std::vector<int32_t>& idx;
    std::vector<double> keys;
    std::vector<int32_t> tmp;

    Box bound(int first, int count) const;  // InitNode, BvhNode.fs:32-37
    // Subdivide (BvhNode.fs:42-61), visiting leaves left to right; `par` more levels split onto
    // a second thread (ranges of at least 8,192 primitives)
    void subdivide(int first, int count, Box b, std::vector<int32_t>& lf, std::vector<int32_t>& lc, int par);
};

// ---- binned SAH BVH2 over items, collapsed to a BVH4 ---------------------------------------
struct FBox {
    float lo[3], hi[3];
    void grow(const FBox& b) {
        for (int i = 0; i < 3; ++i) {
            lo[i] = std::min(lo[i], b.lo[i]);
            hi[i] = std::max(hi[i], b.hi[i]);
        }
    }
    float area() const {
        float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        if (dx < 0 || dy < 0 || dz < 0) return 0.f;
        return 2.f * (dx * dy + dx * dz + dy * dz);
    }
    static FBox empty() {
        FBox b;
        for (int i = 0; i < 3; ++i) {
            b.lo[i] = FLT_MAX;
            b.hi[i] = -FLT_MAX;
        }
        return b;
    }
};

inline float round_down(double x) {
    float f = (float)x;
    if ((double)f > x) f = std::nextafter(f, -FLT_MAX);
    return f;
}
inline float round_up(double x) {
    float f = (float)x;
    if ((double)f < x) f = std::nextafter(f, FLT_MAX);
    return f;
}
// the conservative FP32 box: widened by eps, rounded outward
inline FBox fbox_of(const Box& b, float eps) {
    FBox f;
    for (int a = 0; a < 3; ++a) {
        f.lo[a] = round_down(comp(b.lo, a) - (double)eps);
        f.hi[a] = round_up(comp(b.hi, a) + (double)eps);
    }
    return f;
}

struct Node2 {  // binned-SAH BVH2 node (host only; collapsed to MfxNode BVH4 for the device)
    FBox box[2];
    int32_t child[2];
};

// A binned-SAH BVH2 over items (their conservative FP32 boxes, centroids and slot weights), built on
// the host; mfx_build.hip builds the same tree on the GPU. solo (optional): items that must sit alone
// in a leaf (instances).
struct Tree {
    std::vector<Node2> nodes2;
    std::vector<std::pair<int, int>> leaves;  // [b, e) ranges of ids
    std::vector<int32_t> ids;
    int root2 = 0;
    FBox rootbox;
    int levels = 0;
};
void build_tree(const std::vector<FBox>& cb, const std::vector<float>& cent, const std::vector<int32_t>& weight,
                const std::vector<char>* solo, int max_leaf, float c_isect, Tree& t);

// BVH2 -> BVH4: a node adopts the children of its largest-area internal child until it has four
// (Wald et al. 2008 style collapse). Preorder output; records the depth and the stack bound
// (max over nodes of the pushes its ancestors can leave on the stack plus its own).
struct Collapse4 {
    const std::vector<Node2>& n2;
    std::vector<MfxNode>& out;
    int max_depth = 0, max_stack = 0;
    std::vector<int>* leaf_stack = nullptr;  // optional: per leaf, the stack entries when it is reached

    int run(int ref, int depth, int pushed, const FBox* leaf_box = nullptr);
};

// leaves (~child refs) of a BVH4 in depth-first order, children in order
std::vector<int> dfs_leaves(const std::vector<MfxNode>& nodes, int root);

}  // namespace mfx_bvh

#endif
