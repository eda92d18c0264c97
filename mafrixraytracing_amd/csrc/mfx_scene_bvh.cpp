// mfx_scene_bvh.cpp — the host builders of mfx_scene_bvh.h.
#include "mfx_scene_bvh.h"

#include <cstring>
#include <thread>

namespace mfx_bvh {

namespace {

// ---- .NET 6 GenericArraySortHelper<double,int>.IntroSort (tie behaviour of Array.Sort) ------
struct NetSort {
    double* k;
    int32_t* v;
    void swap(int i, int j) {
        std::swap(k[i], k[j]);
        std::swap(v[i], v[j]);
    }
    void swap_if_greater(int i, int j) {
        if (k[i] > k[j]) swap(i, j);
    }
    void insertion(int n) {
        for (int i = 0; i < n - 1; ++i) {
            double t = k[i + 1];
            int32_t tv = v[i + 1];
            int j = i;
            for (; j >= 0 && t < k[j]; --j) {
                k[j + 1] = k[j];
                v[j + 1] = v[j];
            }
            k[j + 1] = t;
            v[j + 1] = tv;
        }
    }
    void down_heap(int i, int n) {
        double d = k[i - 1];
        int32_t dv = v[i - 1];
        while (i <= n >> 1) {
            int c = 2 * i;
            if (c < n && k[c - 1] < k[c]) ++c;
            if (!(d < k[c - 1])) break;
            k[i - 1] = k[c - 1];
            v[i - 1] = v[c - 1];
            i = c;
        }
        k[i - 1] = d;
        v[i - 1] = dv;
    }
    void heap(int n) {
        for (int i = n >> 1; i >= 1; --i) down_heap(i, n);
        for (int i = n; i > 1; --i) {
            swap(0, i - 1);
            down_heap(1, i - 1);
        }
    }
    int partition(int n) {
        const int hi = n - 1, mid = hi >> 1;
        swap_if_greater(0, mid);
        swap_if_greater(0, hi);
        swap_if_greater(mid, hi);
        const double pivot = k[mid];
        swap(mid, hi - 1);
        int l = 0, r = hi - 1;
        while (l < r) {
            while (pivot > k[++l]) {
            }
            while (pivot < k[--r]) {
            }
            if (l >= r) break;
            swap(l, r);
        }
        if (l != hi - 1) swap(l, hi - 1);
        return l;
    }
    static void intro(double* kk, int32_t* vv, int n, int depth) {
        while (n > 1) {
            NetSort s{kk, vv};
            if (n <= 16) {
                if (n == 2) {
                    s.swap_if_greater(0, 1);
                } else if (n == 3) {
                    s.swap_if_greater(0, 1);
                    s.swap_if_greater(0, 2);
                    s.swap_if_greater(1, 2);
                } else {
                    s.insertion(n);
                }
                return;
            }
            if (depth == 0) {
                s.heap(n);
                return;
            }
            --depth;
            int p = s.partition(n);
            intro(kk + p + 1, vv + p + 1, n - p - 1, depth);
            n = p;
        }
    }
    static void sort(double* kk, int32_t* vv, int n) {
        if (n < 2) return;
        int lg = 0;
        for (unsigned x = (unsigned)n; x >>= 1;) ++lg;
        intro(kk, vv, n, 2 * (lg + 1));
    }
};

}  // namespace

Box RefBvh::bound(int first, int count) const {
    Box b = pb[idx[first]];
    for (int k = 1; k < count; ++k) b = join(b, pb[idx[first + k]]);
    return b;
}

void RefBvh::subdivide(int first, int count, Box b, std::vector<int32_t>& lf, std::vector<int32_t>& lc, int par) {
    if (count <= 3) {
        lf.push_back(first);
        lc.push_back(count);
        return;
    }
    D3 d = sub(b.hi, b.lo);  // MaximumExtent, Aggregate.fs:29-36
    int axis = (d.x > d.y && d.x > d.z) ? 0 : (d.y > d.z ? 1 : 2);
    double* kk = keys.data() + first;
    int32_t* tt = tmp.data() + first;
    for (int k = 0; k < count; ++k) {
        int p = idx[first + k];
        const Box& q = pb[p];
        D3 c = add(q.lo, scale(sub(q.hi, q.lo), 0.5));
        kk[k] = comp(c, axis);
        tt[k] = p;
    }
    NetSort::sort(kk, tt, count);
    std::memcpy(&idx[first], tt, sizeof(int32_t) * count);
    int left = count / 2;
    Box bl = bound(first, left), br = bound(first + left, count - left);
    if (par > 0 && count >= 8192) {
        std::vector<int32_t> lf2, lc2;
        std::thread t([&] { subdivide(first + left, count - left, br, lf2, lc2, par - 1); });
        subdivide(first, left, bl, lf, lc, par - 1);
        t.join();
        lf.insert(lf.end(), lf2.begin(), lf2.end());
        lc.insert(lc.end(), lc2.begin(), lc2.end());
    } else {
        subdivide(first, left, bl, lf, lc, 0);
        subdivide(first + left, count - left, br, lf, lc, 0);
    }
}

namespace {

struct SahBuilder {
    std::vector<FBox> cb;       // item boxes (conservative FP32)
    std::vector<float> cent;    // centroids [3*n]
    std::vector<float> weight;  // intersection cost of an item (slots it tests)
    std::vector<int32_t> ids;   // permutation being partitioned
    std::vector<char> solo;     // optional: items that must sit alone in a leaf (instances)
    std::vector<std::pair<int, int>> leaves;  // [b, e) ranges of ids, in creation order
    std::vector<Node2>& nodes;
    int max_depth = 0;
    int max_leaf = 4;
    float c_isect = 1.5f;  // cost of one primitive slot test relative to one node step
    static constexpr int NB = 32;

    explicit SahBuilder(std::vector<Node2>& n) : nodes(n) {}

    int make_leaf(int b, int e, FBox& out) {
        out = FBox::empty();
        for (int i = b; i < e; ++i) out.grow(cb[ids[i]]);
        leaves.emplace_back(b, e);
        return ~(int)(leaves.size() - 1);
    }

    // returns child reference (>= 0 node, < 0 ~leaf); fills `out` with the subtree box
    int build(int b, int e, int depth, FBox& out) {
        max_depth = std::max(max_depth, depth);
        const int n = e - b;
        if (n == 1) return make_leaf(b, e, out);
        FBox cbox = FBox::empty(), box = FBox::empty();
        float wsum = 0.f;
        bool any_solo = false;
        for (int i = b; i < e; ++i) {
            if (!solo.empty() && solo[ids[i]]) any_solo = true;
            FBox p;
            for (int a = 0; a < 3; ++a) p.lo[a] = p.hi[a] = cent[3 * ids[i] + a];
            cbox.grow(p);
            box.grow(cb[ids[i]]);
            wsum += weight[ids[i]];
        }
        int best_axis = -1, best_split = 0;
        float best_cost = FLT_MAX;
        for (int a = 0; a < 3; ++a) {
            float ext = cbox.hi[a] - cbox.lo[a];
            if (!(ext > 0.f)) continue;
            FBox bb[NB];
            float wb[NB] = {0};
            int cnt[NB] = {0};
            for (int k = 0; k < NB; ++k) bb[k] = FBox::empty();
            // the cast never sees a NaN: mfx_build_scene refuses non-finite coordinates and extents past
            // 2^126, so centroids and ext are finite, ext > 0 here, and the quotient lies in [0, 1]
            for (int i = b; i < e; ++i) {
                int k = (int)((cent[3 * ids[i] + a] - cbox.lo[a]) / ext * NB);
                k = std::min(NB - 1, std::max(0, k));
                cnt[k]++;
                wb[k] += weight[ids[i]];
                bb[k].grow(cb[ids[i]]);
            }
            float ra[NB], rw[NB];
            int rc[NB];
            FBox acc = FBox::empty();
            int c = 0;
            float w = 0.f;
            for (int k = NB - 1; k > 0; --k) {
                acc.grow(bb[k]);
                c += cnt[k];
                w += wb[k];
                ra[k] = acc.area();
                rc[k] = c;
                rw[k] = w;
            }
            acc = FBox::empty();
            c = 0;
            w = 0.f;
            for (int k = 0; k < NB - 1; ++k) {
                acc.grow(bb[k]);
                c += cnt[k];
                w += wb[k];
                if (c == 0 || rc[k + 1] == 0) continue;
                float cost = acc.area() * w + ra[k + 1] * rw[k + 1];
                if (cost < best_cost) {
                    best_cost = cost;
                    best_axis = a;
                    best_split = k;
                }
            }
        }
        // SAH: leaf if testing everything here is no dearer than one more node step plus the split
        const float area = box.area();
        if (n <= max_leaf && !any_solo && (best_axis < 0 || c_isect * wsum * area <= area + c_isect * best_cost))
            return make_leaf(b, e, out);
        int mid;
        if (best_axis < 0) {
            mid = (b + e) / 2;  // all centroids coincide: split by position
        } else {
            const float lo = cbox.lo[best_axis], ext = cbox.hi[best_axis] - cbox.lo[best_axis];
            // stable: the GPU build (mfx_build.hip) partitions the same way, so both builds agree
            auto it = std::stable_partition(ids.begin() + b, ids.begin() + e, [&](int id) {
                int k = (int)((cent[3 * id + best_axis] - lo) / ext * NB);
                k = std::min(NB - 1, std::max(0, k));
                return k <= best_split;
            });
            mid = (int)(it - ids.begin());
            if (mid == b || mid == e) mid = (b + e) / 2;
        }
        int self = (int)nodes.size();
        nodes.push_back(Node2{});
        FBox lb, rb;
        int l = build(b, mid, depth + 1, lb);
        int r = build(mid, e, depth + 1, rb);
        Node2& nd = nodes[self];
        nd.box[0] = lb;
        nd.box[1] = rb;
        nd.child[0] = l;
        nd.child[1] = r;
        out = lb;
        out.grow(rb);
        return self;
    }
};

}  // namespace

int Collapse4::run(int ref, int depth, int pushed, const FBox* leaf_box) {
    if (ref < 0 && depth > 0) {
        if (leaf_stack) (*leaf_stack)[~ref] = pushed;
        return ref;
    }
    max_depth = std::max(max_depth, depth);
    int ch[4];
    FBox bx[4];
    int nc = 2;
    if (ref < 0) {  // the whole scene is one leaf: a root node with one child
        nc = 1;
        ch[0] = ref;
        bx[0] = *leaf_box;
    } else {
        for (int k = 0; k < 2; ++k) {
            ch[k] = n2[ref].child[k];
            bx[k] = n2[ref].box[k];
        }
    }
    while (nc > 1 && nc < 4) {
        int best = -1;
        float ba = -1.f;
        for (int k = 0; k < nc; ++k)
            if (ch[k] >= 0 && bx[k].area() > ba) {
                ba = bx[k].area();
                best = k;
            }
        if (best < 0) break;
        const Node2& m = n2[ch[best]];
        for (int k = nc; k > best + 1; --k) {  // children of `best` replace it in place
            ch[k] = ch[k - 1];
            bx[k] = bx[k - 1];
        }
        ch[best] = m.child[0];
        bx[best] = m.box[0];
        ch[best + 1] = m.child[1];
        bx[best + 1] = m.box[1];
        ++nc;
    }
    max_stack = std::max(max_stack, pushed + nc - 1);  // node_step writes stack[pushed .. pushed + nc - 2]
    const int self = (int)out.size();
    out.push_back(MfxNode{});
    int ref4[4];
    for (int k = 0; k < nc; ++k) ref4[k] = run(ch[k], depth + 1, pushed + nc - 1);
    MfxNode& nd = out[self];
    for (int k = 0; k < 4; ++k) {
        const bool v = k < nc;
        nd.lox[k] = v ? bx[k].lo[0] : FLT_MAX;
        nd.hix[k] = v ? bx[k].hi[0] : FLT_MAX;
        nd.loy[k] = v ? bx[k].lo[1] : FLT_MAX;
        nd.hiy[k] = v ? bx[k].hi[1] : FLT_MAX;
        nd.loz[k] = v ? bx[k].lo[2] : FLT_MAX;
        nd.hiz[k] = v ? bx[k].hi[2] : FLT_MAX;
        nd.child[k] = v ? ref4[k] : MFX_CHILD_EMPTY;
        nd.pad[k] = 0;
    }
    return self;
}

Box prim_box(const mfx_prim& p) {
    if (p.kind == MFX_PRIM_SPHERE) {
        const double r = p.p[1][0];
        const D3 c = d3(p.p[0]), v{r, r, r};
        return box2(sub(c, v), add(c, v));
    }
    const Box b = tri_box(d3(p.p[0]), d3(p.p[1]), d3(p.p[2]));
    return p.kind == MFX_PRIM_RECT ? join(b, tri_box(d3(p.p[0]), d3(p.p[2]), d3(p.p[3]))) : b;
}

void build_tree(const std::vector<FBox>& cb, const std::vector<float>& cent, const std::vector<int32_t>& weight,
                const std::vector<char>* solo, int max_leaf, float c_isect, Tree& t) {
    const int n = (int)cb.size();
    t.nodes2.clear();
    SahBuilder sb(t.nodes2);
    sb.max_leaf = max_leaf;
    sb.c_isect = c_isect;
    sb.cb = cb;
    sb.cent = cent;
    sb.weight.resize(n);
    sb.ids.resize(n);
    for (int i = 0; i < n; ++i) {
        sb.weight[i] = (float)weight[i];
        sb.ids[i] = i;
    }
    if (solo) sb.solo = *solo;
    t.root2 = sb.build(0, n, 0, t.rootbox);
    t.levels = sb.max_depth + 1;
    t.leaves = sb.leaves;
    t.ids = sb.ids;
}

// leaves (~child refs) of a BVH4 in depth-first order, children in order
std::vector<int> dfs_leaves(const std::vector<MfxNode>& nodes, int root) {
    std::vector<int> order, st{root};
    while (!st.empty()) {
        const int ref = st.back();
        st.pop_back();
        if (ref < 0) {
            order.push_back(~ref);
        } else {
            for (int k = 3; k >= 0; --k)
                if (nodes[ref].child[k] != MFX_CHILD_EMPTY) st.push_back(nodes[ref].child[k]);
        }
    }
    return order;
}

}  // namespace mfx_bvh
