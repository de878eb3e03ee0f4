/*
 * ppg_scene_build.h — the pure stage of ppg_set_scene: everything between the caller's ppg_scene (with the side lists of the ppg_set_*
 * calls) and the host tables the device reads.  buildScene() validates the scene and fills a HostScene; it makes no HIP call and knows no
 * context, so a refused scene has touched nothing (ppg_hip.hip uploads and commits a HostScene in one place), and
 * tests/scene_build_check.hip runs it without a device.
 */
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ppg_device.h"

namespace {

// ------------------------------------------------------------------------------------------------
// BVH2 construction (binned SAH), stands in for Scene::initialize → ShapeKDTree::build
// ------------------------------------------------------------------------------------------------
struct BvhBuilder {
    const float *pos; const uint32_t *idx;
    std::vector<uint32_t> order;
    std::vector<float> bmin, bmax, cent;  // per tri
    std::vector<BvhNode> nodes;
    float pad;
    int maxLeaf = 4;  // triangles per leaf (the BVH4 child code holds up to 8)

    struct Box { float lo[3], hi[3]; };
    static Box empty() { Box b; for (int a = 0; a < 3; ++a) { b.lo[a] = INFINITY; b.hi[a] = -INFINITY; } return b; }
    static void grow(Box &b, const float *lo, const float *hi) { for (int a = 0; a < 3; ++a) { b.lo[a] = std::min(b.lo[a], lo[a]); b.hi[a] = std::max(b.hi[a], hi[a]); } }
    static float area(const Box &b) { float d[3] = {b.hi[0] - b.lo[0], b.hi[1] - b.lo[1], b.hi[2] - b.lo[2]}; if (d[0] < 0) return 0; return 2 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0]); }

    Box boundsOf(int first, int count) const {
        Box b = empty();
        for (int i = first; i < first + count; ++i) grow(b, &bmin[3 * order[i]], &bmax[3 * order[i]]);
        return b;
    }

    // ---- the binary tree: one triangle per leaf; which subtrees become leaves of up to maxLeaf triangles is decided by collapse() ----
    struct N2 {
        float lo[3], hi[3];  // unpadded
        int parent, c0, c1;  // c0 < 0: a leaf
        int tri;             // leaf: its triangle
        int first, count;    // range in `order` (layout())
    };
    std::vector<N2> t2;
    static float areaN(const N2 &n) { const float d[3] = {n.hi[0] - n.lo[0], n.hi[1] - n.lo[1], n.hi[2] - n.lo[2]}; return 2 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0]); }
    static float areaU(const N2 &p, const N2 &q) {
        float d[3];
        for (int a = 0; a < 3; ++a) d[a] = std::max(p.hi[a], q.hi[a]) - std::min(p.lo[a], q.lo[a]);
        return 2 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0]);
    }
    // Ranges of up to SWEEP triangles: the exact SAH — all 3 (count - 1) object partitions along the sorted centroids; above: 16 bins per axis
    // (the sweep matters in the lower levels, where a bin holds a handful of triangles; higher up the bins see the same planes.  On KITCHEN
    // thresholds of 0 / 64 / 256 trace 10.8 / 10.0 - 10.6 / 10.7 node steps per ray after the re-optimisation: profiles/bvh_quality.json)
    static constexpr int SWEEP = 64;
    std::vector<uint32_t> swCur, swBest;
    std::vector<float> swArea;
    int sweepSplit(int first, int count) {
        swCur.resize((size_t)count); swBest.resize((size_t)count); swArea.resize((size_t)count);
        float bestCost = INFINITY; int bestI = -1;
        for (int a = 0; a < 3; ++a) {
            std::copy(order.begin() + first, order.begin() + first + count, swCur.begin());
            std::sort(swCur.begin(), swCur.end(), [&](uint32_t x, uint32_t y) { const float cx = cent[3 * x + a], cy = cent[3 * y + a]; return cx < cy || (cx == cy && x < y); });
            Box acc = empty();
            for (int i = count - 1; i >= 1; --i) { grow(acc, &bmin[3 * swCur[i]], &bmax[3 * swCur[i]]); swArea[i] = area(acc); }
            acc = empty();
            bool better = false;
            for (int i = 1; i < count; ++i) {
                grow(acc, &bmin[3 * swCur[i - 1]], &bmax[3 * swCur[i - 1]]);
                const float cost = area(acc) * i + swArea[i] * (count - i);
                if (cost < bestCost) { bestCost = cost; bestI = i; better = true; }
            }
            if (better) swBest.swap(swCur);
        }
        if (bestI < 0) return first + count / 2;  // (areas not finite)
        std::copy(swBest.begin(), swBest.end(), order.begin() + first);
        return first + bestI;
    }
    int binnedSplit(int first, int count, const Box &cb) {
        int bestAxis = -1, bestSplit = -1; float bestCost = INFINITY;
        const int NB = 16;
        for (int a = 0; a < 3; ++a) {
            float ext = cb.hi[a] - cb.lo[a];
            if (!(ext > 0)) continue;
            Box bb[NB]; int bc[NB];
            for (int k = 0; k < NB; ++k) { bb[k] = empty(); bc[k] = 0; }
            for (int i = first; i < first + count; ++i) {
                int k = std::min(NB - 1, (int)((cent[3 * order[i] + a] - cb.lo[a]) / ext * NB));
                grow(bb[k], &bmin[3 * order[i]], &bmax[3 * order[i]]); bc[k]++;
            }
            float la[NB]; int lc[NB]; Box acc = empty(); int c = 0;
            for (int k = 0; k < NB; ++k) { if (bc[k]) grow(acc, bb[k].lo, bb[k].hi); c += bc[k]; la[k] = area(acc); lc[k] = c; }
            acc = empty(); c = 0;
            for (int k = NB - 1; k > 0; --k) {
                if (bc[k]) grow(acc, bb[k].lo, bb[k].hi); c += bc[k];
                if (lc[k - 1] == 0 || c == 0) continue;
                float cost = la[k - 1] * lc[k - 1] + area(acc) * c;
                if (cost < bestCost) { bestCost = cost; bestAxis = a; bestSplit = k; }
            }
        }
        if (bestAxis < 0) return first + count / 2;
        float ext = cb.hi[bestAxis] - cb.lo[bestAxis], lo = cb.lo[bestAxis];
        auto it = std::partition(order.begin() + first, order.begin() + first + count, [&](uint32_t t) {
            int k = std::min(NB - 1, (int)((cent[3 * t + bestAxis] - lo) / ext * NB));
            return k < bestSplit;
        });
        int mid = (int)(it - order.begin());
        if (mid == first || mid == first + count) mid = first + count / 2;
        return mid;
    }
    int build2(int first, int count, int parent) {
        const int me = (int)t2.size();
        t2.emplace_back();
        {
            N2 &n = t2[(size_t)me];
            const Box b = boundsOf(first, count);
            for (int a = 0; a < 3; ++a) { n.lo[a] = b.lo[a]; n.hi[a] = b.hi[a]; }
            n.parent = parent; n.c0 = n.c1 = -1; n.tri = (int)order[first]; n.first = first; n.count = count;
        }
        if (count == 1) return me;
        Box cb = empty();
        for (int i = first; i < first + count; ++i) grow(cb, &cent[3 * order[i]], &cent[3 * order[i]]);
        int mid;
        if (!(cb.hi[0] > cb.lo[0]) && !(cb.hi[1] > cb.lo[1]) && !(cb.hi[2] > cb.lo[2])) mid = first + count / 2;  // coincident centroids: median
        else mid = count <= SWEEP ? sweepSplit(first, count) : binnedSplit(first, count, cb);
        const int l = build2(first, mid - first, me), r = build2(mid, first + count - mid, me);
        t2[(size_t)me].c0 = l; t2[(size_t)me].c1 = r;
        return me;
    }

    // ---- insertion-based re-optimisation of the binary tree (Bittner, Hapala, Havran: Fast insertion-based optimization of bounding volume
    // hierarchies, CGF 2013).  A top-down build never revisits a split: a large triangle (a wall, a table top) inflates every box above it.
    // Per batch the interior nodes that promise most (large, with a child much smaller than themselves) are taken out one after the other; the two
    // subtrees below a removed node are put back where a branch-and-bound search finds the least increase of the tree's total surface area.
    // Deterministic: one thread, a fixed number of batches, every tie broken by the node index — the same scene gives the same tree on every
    // rank and in every run. ----
    void refit(int v) {
        for (; v >= 0; v = t2[(size_t)v].parent) {
            N2 &n = t2[(size_t)v];
            const N2 &p = t2[(size_t)n.c0], &q = t2[(size_t)n.c1];
            bool same = true;
            for (int a = 0; a < 3; ++a) {
                const float lo = std::min(p.lo[a], q.lo[a]), hi = std::max(p.hi[a], q.hi[a]);
                same = same && lo == n.lo[a] && hi == n.hi[a];
                n.lo[a] = lo; n.hi[a] = hi;
            }
            if (same) break;
        }
    }
    void replaceChild(int p, int was, int now) { N2 &n = t2[(size_t)p]; if (n.c0 == was) n.c0 = now; else n.c1 = now; t2[(size_t)now].parent = p; }
    typedef std::pair<float, int> QEnt;  // (area the ancestors grow by, node)
    std::vector<QEnt> heap;
    int findTarget(int x) {
        auto later = [](const QEnt &p, const QEnt &q) { return p.first > q.first || (p.first == q.first && p.second > q.second); };
        const float ax = areaN(t2[(size_t)x]);
        float best = INFINITY; int bestNode = -1;
        heap.clear();
        heap.push_back(QEnt(0.0f, 0));
        while (!heap.empty()) {
            std::pop_heap(heap.begin(), heap.end(), later);
            const QEnt e = heap.back();
            heap.pop_back();
            if (e.first + ax >= best && bestNode >= 0) break;
            const N2 &v = t2[(size_t)e.second];
            const float total = e.first + areaU(v, t2[(size_t)x]);
            if (e.second != 0 && (total < best || bestNode < 0)) { best = total; bestNode = e.second; }
            const float below = total - areaN(v);
            if (v.c0 >= 0 && (below + ax < best || bestNode < 0)) {
                heap.push_back(QEnt(below, v.c0)); std::push_heap(heap.begin(), heap.end(), later);
                heap.push_back(QEnt(below, v.c1)); std::push_heap(heap.begin(), heap.end(), later);
            }
        }
        return bestNode;
    }
    void insertAt(int x, int spare) {
        const int b = findTarget(x), bp = t2[(size_t)b].parent;
        replaceChild(bp, b, spare);
        N2 &f = t2[(size_t)spare];
        f.c0 = b; f.c1 = x;
        t2[(size_t)b].parent = spare; t2[(size_t)x].parent = spare;
        for (int a = 0; a < 3; ++a) { f.lo[a] = std::min(t2[(size_t)b].lo[a], t2[(size_t)x].lo[a]); f.hi[a] = std::max(t2[(size_t)b].hi[a], t2[(size_t)x].hi[a]); }
        refit(bp);
    }
    bool movable(int n) const { return n > 0 && t2[(size_t)n].c0 >= 0 && t2[(size_t)n].parent > 0; }
    void reinsert(int n) {
        const int p = t2[(size_t)n].parent, g = t2[(size_t)p].parent;
        const int s = t2[(size_t)p].c0 == n ? t2[(size_t)p].c1 : t2[(size_t)p].c0;
        replaceChild(g, p, s);
        refit(g);
        int l = t2[(size_t)n].c0, r = t2[(size_t)n].c1;
        if (areaN(t2[(size_t)l]) < areaN(t2[(size_t)r])) std::swap(l, r);
        insertAt(l, n);   // the two nodes the removal set free carry the two subtrees back
        insertAt(r, p);
    }
    // Eight batches, each the most promising 1 % of the interior nodes — fixed numbers, never a clock.  profiles/bvh_quality.json: KITCHEN's
    // traced node steps per ray are 10.0 - 10.8 for 4 to 40 batches of 1 - 4 % (14.2 without any) while the build grows from 3.2 to 13 s.
    static constexpr int REOPT_PART = 100, REOPT_BATCHES = 8;
    void reoptimise() {
        if (t2.size() < 16) return;
        std::vector<QEnt> cand;
        for (int batch = 0; batch < REOPT_BATCHES; ++batch) {
            cand.clear();
            for (int v = 1; v < (int)t2.size(); ++v) {
                if (!movable(v)) continue;
                const float a = areaN(t2[(size_t)v]), a0 = areaN(t2[(size_t)t2[(size_t)v].c0]), a1 = areaN(t2[(size_t)t2[(size_t)v].c1]);
                const float tiny = 1e-30f;
                const float prio = a * (a / std::max(std::min(a0, a1), tiny)) * (a / std::max(0.5f * (a0 + a1), tiny));  // M_AREA M_MIN M_SUM of the paper
                if (prio == prio) cand.push_back(QEnt(prio, v));
            }
            const size_t k = std::min(cand.size(), std::max<size_t>(1, t2.size() / (2 * REOPT_PART)));
            auto first = [](const QEnt &p, const QEnt &q) { return p.first > q.first || (p.first == q.first && p.second < q.second); };
            std::partial_sort(cand.begin(), cand.begin() + (long)k, cand.end(), first);
            for (size_t i = 0; i < k; ++i) if (movable(cand[i].second)) reinsert(cand[i].second);
        }
    }

    // leaf order = the tree's depth-first order, so that every subtree's triangles are contiguous (a leaf is a range); `pre` = the nodes
    // parents first
    std::vector<int> pre;
    void layout() {
        std::vector<uint32_t> fresh;
        fresh.reserve(order.size());
        pre.clear(); pre.reserve(t2.size());
        std::vector<int> stack(1, 0);
        while (!stack.empty()) {
            const int v = stack.back();
            stack.pop_back();
            pre.push_back(v);
            N2 &n = t2[(size_t)v];
            if (n.c0 < 0) { n.first = (int)fresh.size(); n.count = 1; fresh.push_back((uint32_t)n.tri); }
            else { stack.push_back(n.c1); stack.push_back(n.c0); }
        }
        for (size_t i = pre.size(); i-- > 0;) {
            N2 &n = t2[(size_t)pre[i]];
            if (n.c0 >= 0) { n.first = t2[(size_t)n.c0].first; n.count = t2[(size_t)n.c0].count + t2[(size_t)n.c1].count; }
        }
        order.swap(fresh);
    }

    // ---- collapse to 4-wide nodes: a dynamic programme over the binary tree, bottom up.  cost[v][k - 1] = the least expected cost of
    // presenting v's triangles as exactly k children of a 4-wide node; for k = 1 the cheaper of ONE LEAF with all its triangles (where they are
    // at most maxLeaf) and a 4-wide node of its own over the best cut of 2..4 descendants.  A child costs its box's area times C_NODE (an
    // interior child: one more node step) or C_LEAF + C_TRI per triangle.  The constants are in node steps of k_trace: a triangle test in
    // the (ray, triangle)-pair compaction costs about a quarter of a node step, a leaf visit (pop, vote) about as much once ----
    static constexpr double C_NODE = 1.0, C_LEAF = 0.25, C_TRI = 0.25;
    struct Cost4 { double k[4]; };
    std::vector<Cost4> cost;
    std::vector<unsigned char> asLeaf;
    double paddedArea(const N2 &n) const {
        const double d[3] = {(double)n.hi[0] - n.lo[0] + 2.0 * pad, (double)n.hi[1] - n.lo[1] + 2.0 * pad, (double)n.hi[2] - n.lo[2] + 2.0 * pad};
        return 2 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0]);
    }
    void collapse() {
        cost.resize(t2.size()); asLeaf.assign(t2.size(), 0);
        for (size_t i = pre.size(); i-- > 0;) {
            const int v = pre[i];
            const N2 &n = t2[(size_t)v];
            const double A = paddedArea(n);
            Cost4 &c = cost[(size_t)v];
            if (n.c0 < 0) { c.k[0] = A * (C_LEAF + C_TRI); c.k[1] = c.k[2] = c.k[3] = INFINITY; asLeaf[(size_t)v] = 1; continue; }
            const Cost4 &l = cost[(size_t)n.c0], &r = cost[(size_t)n.c1];
            double cut = INFINITY;
            for (int k = 2; k <= 4; ++k) {
                double best = INFINITY;
                for (int j = 1; j < k; ++j) best = std::min(best, l.k[j - 1] + r.k[k - j - 1]);
                c.k[k - 1] = best;
                cut = std::min(cut, best);
            }
            const double node = A * C_NODE + cut, leaf = n.count <= maxLeaf ? A * (C_LEAF + C_TRI * n.count) : INFINITY;
            asLeaf[(size_t)v] = leaf <= node;
            c.k[0] = std::min(leaf, node);
        }
    }
    void cut4(int v, int k, int *ch, int &m) const {  // the k descendants of v that cost[v][k - 1] stands for
        if (k == 1) { ch[m++] = v; return; }
        const N2 &n = t2[(size_t)v];
        const Cost4 &l = cost[(size_t)n.c0], &r = cost[(size_t)n.c1];
        int bj = 1;
        for (int j = 2; j < k; ++j) if (l.k[j - 1] + r.k[k - j - 1] < l.k[bj - 1] + r.k[k - bj - 1]) bj = j;
        cut4(n.c0, bj, ch, m);
        cut4(n.c1, k - bj, ch, m);
    }
    int cutOf(int v, int *ch) const {  // the children of the 4-wide node that emit4 makes of v
        int m = 0, bk = 2;
        for (int k = 3; k <= 4; ++k) if (cost[(size_t)v].k[k - 1] < cost[(size_t)v].k[bk - 1]) bk = k;
        cut4(v, bk, ch, m);
        return m;
    }

    // ---- the traversal stack's bound.  The ordered walk (trace_closest4, trace_slice_bvh4) descends into the nearest child of a node and
    // leaves the other children that were hit on its stack: on the way to a node the stack holds at most the sum of (children - 1) over the
    // interior nodes on the path, that node included.  The STACK NEED of a tree is the largest such sum, and the kernels' stacks hold
    // STACK_MAX entries without a range check (ppg_device.h TStack).  The SAH has no such bound: on nested geometry the sweep peels one
    // triangle per level and the collapsed tree is a chain.  Where the need of the tree the collapse would emit exceeds the bound, the
    // offending subtrees are built again with median splits and the tree is laid out and collapsed again.  A subtree is rebuilt as far
    // down the offending path as a balanced one is expected to fit, so that as little of the SAH tree as possible is given up (a scene
    // of a million triangles whose tree needs 51 loses a few subtrees of some dozen triangles, not its top): a balanced subtree of c
    // triangles is ceil(log2 c) binary levels deep, a 4-wide node takes one to three of them on a path and adds at most 3 — 1.5 per level
    // where the collapse pairs the levels, at most 3.  The first rounds expect 1.5 per level; a round that has not reached the bound is
    // followed by one that expects 2, then 3 (the certain figure), which rebuilds higher up; the last resort is medians throughout.
    // A tree within the bound is not touched. ----
    static constexpr int STACK_MAX = 48;
    int stackNeed = 0;  // of the finished tree (run)
    std::vector<int> need4;
    int needOf(int v) {  // v heads a 4-wide node
        int ch[4];
        const int m = cutOf(v, ch);
        int below = 0;
        for (int k = 0; k < m; ++k) if (!asLeaf[(size_t)ch[k]]) below = std::max(below, needOf(ch[k]));
        return need4[(size_t)v] = m - 1 + below;
    }
    int perLevel2 = 3;  // twice the entries per binary level that rebound expects of a balanced subtree
    int balancedNeed(int count) const { int l = 0; while ((1ll << l) < count) ++l; return (perLevel2 * l + 1) / 2; }
    int buildMedian(int first, int count, int parent) {
        const int me = (int)t2.size();
        t2.emplace_back();
        {
            N2 &n = t2[(size_t)me];
            const Box b = boundsOf(first, count);
            for (int a = 0; a < 3; ++a) { n.lo[a] = b.lo[a]; n.hi[a] = b.hi[a]; }
            n.parent = parent; n.c0 = n.c1 = -1; n.tri = (int)order[first]; n.first = first; n.count = count;
        }
        if (count == 1) return me;
        Box cb = empty();
        for (int i = first; i < first + count; ++i) grow(cb, &cent[3 * order[i]], &cent[3 * order[i]]);
        int a = 0;
        for (int k = 1; k < 3; ++k) if (cb.hi[k] - cb.lo[k] > cb.hi[a] - cb.lo[a]) a = k;
        std::sort(order.begin() + first, order.begin() + first + count, [&](uint32_t x, uint32_t y) { const float cx = cent[3 * x + a], cy = cent[3 * y + a]; return cx < cy || (cx == cy && x < y); });
        const int mid = first + count / 2;
        const int l = buildMedian(first, mid - first, me), r = buildMedian(mid, first + count - mid, me);
        t2[(size_t)me].c0 = l; t2[(size_t)me].c1 = r;
        return me;
    }
    void rebuildBalanced(int v) {  // v's triangles are order[first, first + count) (layout)
        const int first = t2[(size_t)v].first, count = t2[(size_t)v].count, p = t2[(size_t)v].parent;
        const int fresh = buildMedian(first, count, p);
        if (p >= 0) { replaceChild(p, v, fresh); return; }
        t2[0] = t2[(size_t)fresh];  // the root stays node 0
        t2[0].parent = -1;
        t2[(size_t)t2[0].c0].parent = 0; t2[(size_t)t2[0].c1].parent = 0;
    }
    // v heads a 4-wide node that `above` entries lie under and whose subtree overruns the bound; a balanced subtree in v's place is expected to fit
    void rebound(int v, int above) {
        int ch[4];
        const int m = cutOf(v, ch), here = above + m - 1;
        bool deeper = true;  // every offending child can be mended below v
        for (int k = 0; k < m; ++k) {
            const int c = ch[k];
            if (!asLeaf[(size_t)c] && here + need4[(size_t)c] > STACK_MAX && here + balancedNeed(t2[(size_t)c].count) > STACK_MAX) deeper = false;
        }
        if (!deeper) { rebuildBalanced(v); return; }
        for (int k = 0; k < m; ++k) if (!asLeaf[(size_t)ch[k]] && here + need4[(size_t)ch[k]] > STACK_MAX) rebound(ch[k], here);
    }
    void boundStack() {
        for (int round = 0; round < 8; ++round) {
            need4.assign(t2.size(), 0);
            if (needOf(0) <= STACK_MAX) return;
            perLevel2 = round < 3 ? 3 : (round < 5 ? 4 : 6);
            if (round < 7) rebound(0, 0);
            else rebuildBalanced(0);  // (the collapse above a mended subtree may change; should that never settle: medians throughout)
            layout();
            collapse();
        }
    }
    // the stack need of the finished nodes
    static int stackNeedOf(const std::vector<Bvh4Node> &nodes4) {
        int need = 0;
        std::vector<std::pair<int, int>> todo(1, {0, 0});
        while (!todo.empty()) {
            const std::pair<int, int> e = todo.back();
            todo.pop_back();
            const Bvh4Node &nd = nodes4[(size_t)e.first];
            int m = 0;
            for (int k = 0; k < 4; ++k) m += nd.child[k] != PPG_BVH4_EMPTY ? 1 : 0;
            const int here = e.second + std::max(0, m - 1);
            need = std::max(need, here);
            for (int k = 0; k < 4; ++k) if (nd.child[k] >= 0 && nd.child[k] != PPG_BVH4_EMPTY) todo.push_back({nd.child[k], here});
        }
        return need;
    }

    std::vector<Bvh4Node> nodes4;
    int emit4(int v) {
        int ch[4];
        const int m = cutOf(v, ch);
        const int me = (int)nodes4.size();
        nodes4.emplace_back();
        Bvh4Node nd;
        for (int k = 0; k < 4; ++k) {
            if (k < m) {
                const N2 &c = t2[(size_t)ch[k]];
                nd.lox[k] = c.lo[0] - pad; nd.loy[k] = c.lo[1] - pad; nd.loz[k] = c.lo[2] - pad;
                nd.hix[k] = c.hi[0] + pad; nd.hiy[k] = c.hi[1] + pad; nd.hiz[k] = c.hi[2] + pad;
                if (asLeaf[(size_t)ch[k]]) nd.child[k] = ~((c.first << 3) | (c.count - 1));
                else nd.child[k] = emit4(ch[k]);
            } else {
                nd.lox[k] = nd.loy[k] = nd.loz[k] = 0; nd.hix[k] = nd.hiy[k] = nd.hiz[k] = 0; nd.child[k] = PPG_BVH4_EMPTY;
            }
            nd.pad[k] = 0;
        }
        nodes4[(size_t)me] = nd;
        return me;
    }
    // the binary node array (BvhNode) with the same leaves
    int emit2(int v) {
        const int me = (int)nodes.size();
        nodes.emplace_back();
        BvhNode nd;
        const int ch[2] = {t2[(size_t)v].c0, t2[(size_t)v].c1};
        int ref[2], cnt[2];
        for (int k = 0; k < 2; ++k) {
            const N2 &c = t2[(size_t)ch[k]];
            if (asLeaf[(size_t)ch[k]]) { ref[k] = c.first; cnt[k] = c.count; }
            else { ref[k] = emit2(ch[k]); cnt[k] = 0; }
            float *lo = k ? nd.lo1 : nd.lo0, *hi = k ? nd.hi1 : nd.hi0;
            for (int a = 0; a < 3; ++a) { lo[a] = c.lo[a] - pad; hi[a] = c.hi[a] + pad; }
        }
        nd.c0 = ref[0]; nd.n0 = cnt[0]; nd.c1 = ref[1]; nd.n1 = cnt[1];
        nodes[(size_t)me] = nd;
        return me;
    }

    // quantise the child boxes of every BVH4 node (Bvh4QNode, ppg_device.h); conservativeness is verified in the device's arithmetic
    std::vector<Bvh4QNode> nodes4q;
    static float scaleOf(unsigned int e) { const uint32_t bits = e << 23; float f; memcpy(&f, &bits, 4); return f; }
    void quantise() {
        nodes4q.resize(nodes4.size());
        for (size_t i = 0; i < nodes4.size(); ++i) {
            const Bvh4Node &nd = nodes4[i];
            Bvh4QNode q{};
            const float *lo[3] = {nd.lox, nd.loy, nd.loz}, *hi[3] = {nd.hix, nd.hiy, nd.hiz};
            float org[3];
            unsigned int ex[3], qlo[3] = {0, 0, 0}, qhi[3] = {0, 0, 0};
            for (int a = 0; a < 3; ++a) {
                float mn = INFINITY, mx = -INFINITY;
                for (int k = 0; k < 4; ++k) if (nd.child[k] != PPG_BVH4_EMPTY) { mn = std::min(mn, lo[a][k]); mx = std::max(mx, hi[a][k]); }
                if (!(mn <= mx)) { mn = 0; mx = 0; }
                org[a] = mn;
                int x = 0;
                (void)std::frexp((double)(mx - mn) / 255.0, &x);  // value = m 2^x, m in [0.5, 1): 2^x >= value
                // exponent range: bvh4_children scales the ray by 2^-e and 1/d (up to 1e30, safe_inv) by 2^e — both stay finite within 64..154
                // (cells of 1e-19 .. 1.3e8 scene units; ppg_set_scene refuses scenes of more than 1e9 units)
                int e = std::max(64, std::min(154, x + 127));
                for (;;) {  // find a cell size for which all four boxes fit into 0..255 conservatively
                    const float s = scaleOf((unsigned int)e);
                    bool ok = true;
                    unsigned int wl = 0, wh = 0;
                    for (int k = 0; k < 4 && ok; ++k) {
                        if (nd.child[k] == PPG_BVH4_EMPTY) { wl |= 255u << (8 * k); continue; }  // inverted box: never entered
                        long ql = (long)std::floor(((double)lo[a][k] - (double)mn) / (double)s), qh = (long)std::ceil(((double)hi[a][k] - (double)mn) / (double)s);
                        ql = std::max(0l, std::min(255l, ql)); qh = std::max(0l, qh);
                        // neither the float decode (trace_closest4_wave) nor the exact plane (bvh4_children) may cut into the box
                        auto below = [&](long qq) { return mn + (float)qq * s <= lo[a][k] && (double)mn + (double)qq * (double)s <= (double)lo[a][k]; };
                        auto above = [&](long qq) { return mn + (float)qq * s >= hi[a][k] && (double)mn + (double)qq * (double)s >= (double)hi[a][k]; };
                        while (ql > 0 && !below(ql)) --ql;
                        while (qh <= 255 && !above(qh)) ++qh;
                        if (qh > 255 || !below(ql)) { ok = false; break; }
                        wl |= (unsigned int)ql << (8 * k); wh |= (unsigned int)qh << (8 * k);
                    }
                    if (ok) { qlo[a] = wl; qhi[a] = wh; break; }
                    if (++e > 154) { e = 154; qlo[a] = 0; qhi[a] = 0xffffffffu; break; }  // (unreachable below 1e9 scene units)
                }
                ex[a] = (unsigned int)e;
            }
            q.ox = org[0]; q.oy = org[1]; q.oz = org[2];
            q.exps = ex[0] | (ex[1] << 8) | (ex[2] << 16);
            q.qlox = qlo[0]; q.qloy = qlo[1]; q.qloz = qlo[2]; q.qhix = qhi[0]; q.qhiy = qhi[1]; q.qhiz = qhi[2];
            for (int k = 0; k < 4; ++k) q.child[k] = nd.child[k];
            nodes4q[i] = q;
        }
    }

    // The TOP CUT of the tree for trace_closest4_wave (a whole wave walking ONE ray): up to 64 subtrees that partition the scene — the root's
    // descendants after opening, level by level and then by surface area, as many interior entries as fit —, each with its box exactly as the
    // traversal would decode it from its parent (float decode of Bvh4QNode) and its child reference.  The wave tests all of them in ONE step,
    // one lane each, instead of descending the first three levels one dependent step at a time.  Two float4 per entry: (lo, ref) (hi, -).
    std::vector<float> topCut;
    void buildTopCut() {
        struct Ent { float lo[3], hi[3]; int ref; };
        auto childrenOfQ = [&](int node, Ent out[4]) {
            const Bvh4QNode &q = nodes4q[(size_t)node];
            const float sx = scaleOf(q.exps & 255u), sy = scaleOf((q.exps >> 8) & 255u), sz = scaleOf((q.exps >> 16) & 255u);
            int m = 0;
            for (int k = 0; k < 4; ++k) {
                if (q.child[k] == PPG_BVH4_EMPTY) continue;
                const int sh = 8 * k;
                Ent e;
                e.lo[0] = q.ox + (float)((q.qlox >> sh) & 255u) * sx; e.lo[1] = q.oy + (float)((q.qloy >> sh) & 255u) * sy; e.lo[2] = q.oz + (float)((q.qloz >> sh) & 255u) * sz;
                e.hi[0] = q.ox + (float)((q.qhix >> sh) & 255u) * sx; e.hi[1] = q.oy + (float)((q.qhiy >> sh) & 255u) * sy; e.hi[2] = q.oz + (float)((q.qhiz >> sh) & 255u) * sz;
                e.ref = q.child[k];
                out[m++] = e;
            }
            return m;
        };
        std::vector<Ent> cut;
        {
            Ent ch[4];
            const int m = nodes4q.empty() ? 0 : childrenOfQ(0, ch);
            for (int k = 0; k < m; ++k) cut.push_back(ch[k]);
        }
        auto areaOf = [](const Ent &e) { const float d[3] = {e.hi[0] - e.lo[0], e.hi[1] - e.lo[1], e.hi[2] - e.lo[2]}; return d[0] * d[1] + d[1] * d[2] + d[2] * d[0]; };
        for (;;) {  // open the interior entry with the largest box while the cut stays within 64 entries
            int pick = -1; float best = -1;
            for (size_t k = 0; k < cut.size(); ++k) if (cut[k].ref >= 0 && areaOf(cut[k]) > best) { best = areaOf(cut[k]); pick = (int)k; }
            if (pick < 0) break;
            Ent ch[4];
            const int m = childrenOfQ(cut[(size_t)pick].ref, ch);
            if (cut.size() - 1 + (size_t)m > 64) break;
            cut.erase(cut.begin() + pick);
            for (int k = 0; k < m; ++k) cut.push_back(ch[k]);
        }
        topCut.assign(8 * cut.size(), 0.0f);
        for (size_t k = 0; k < cut.size(); ++k) {
            float *o = &topCut[8 * k];
            o[0] = cut[k].lo[0]; o[1] = cut[k].lo[1]; o[2] = cut[k].lo[2]; memcpy(o + 3, &cut[k].ref, 4);
            o[4] = cut[k].hi[0]; o[5] = cut[k].hi[1]; o[6] = cut[k].hi[2];
        }
    }

    void run(const float *positions, const uint32_t *indices, uint32_t nTris, float padAbs) {
        runTree(positions, indices, nTris, padAbs);
        buildTopCut();
    }
    void runTree(const float *positions, const uint32_t *indices, uint32_t nTris, float padAbs) {
        pos = positions; idx = indices; pad = padAbs;
        order.resize(nTris); bmin.resize(3 * (size_t)nTris); bmax.resize(3 * (size_t)nTris); cent.resize(3 * (size_t)nTris);
        for (uint32_t t = 0; t < nTris; ++t) {
            order[t] = t;
            for (int a = 0; a < 3; ++a) {
                float v0 = pos[3 * idx[3 * t] + a], v1 = pos[3 * idx[3 * t + 1] + a], v2 = pos[3 * idx[3 * t + 2] + a];
                bmin[3 * t + a] = std::min(v0, std::min(v1, v2)); bmax[3 * t + a] = std::max(v0, std::max(v1, v2));
                cent[3 * t + a] = 0.5f * (bmin[3 * t + a] + bmax[3 * t + a]);
            }
        }
        nodes.clear();
        nodes.reserve(nTris);
        nodes.emplace_back();  // root placeholder, must be an interior node
        if (nTris == 0) {  // spheres only: one node without children
            nodes4.assign(1, Bvh4Node{});
            for (int k = 0; k < 4; ++k) nodes4[0].child[k] = PPG_BVH4_EMPTY;
            quantise();
            return;
        }
        if (nTris <= 4) {  // one node with one leaf
            BvhNode &nd = nodes[0];
            Box bb = boundsOf(0, (int)nTris);
            for (int a = 0; a < 3; ++a) { nd.lo0[a] = bb.lo[a] - pad; nd.hi0[a] = bb.hi[a] + pad; nd.lo1[a] = 0; nd.hi1[a] = 0; }
            nd.c0 = 0; nd.n0 = (int)nTris; nd.c1 = 0; nd.n1 = -1;
            Bvh4Node n4{};
            for (int k = 0; k < 4; ++k) n4.child[k] = PPG_BVH4_EMPTY;
            n4.lox[0] = nd.lo0[0]; n4.loy[0] = nd.lo0[1]; n4.loz[0] = nd.lo0[2]; n4.hix[0] = nd.hi0[0]; n4.hiy[0] = nd.hi0[1]; n4.hiz[0] = nd.hi0[2];
            n4.child[0] = ~((0 << 3) | ((int)nTris - 1));
            nodes4.assign(1, n4);
            quantise();
            return;
        }
        nodes.pop_back();
        t2.clear(); t2.reserve(2 * (size_t)nTris);
        build2(0, (int)nTris, -1);  // nTris > 4 ⇒ the root is interior
        reoptimise();
        layout();
        collapse();
        boundStack();
        nodes4.clear(); nodes4.reserve(t2.size() / 4 + 1);
        emit4(0);
        emit2(0);
        stackNeed = stackNeedOf(nodes4);
        quantise();
    }
};

// TriAccel::load (triaccel.h:62-97), same float operations as the oracle's: the three words of a triangle's record (tri_hit_regs), orig in a2.w
static void triAccelLoad(const float *A, const float *B, const float *C, int orig, float4 out[3]) {
    static const int waldModulo[4] = {1, 2, 0, 1};
    const float b[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]}, c[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
    const float N[3] = {c[1] * b[2] - c[2] * b[1], c[2] * b[0] - c[0] * b[2], c[0] * b[1] - c[1] * b[0]};
    int kk = 0;
    for (int j = 0; j < 3; j++) if (ppg_abs(N[j]) > ppg_abs(N[kk])) kk = j;
    const int u = waldModulo[kk], v = waldModulo[kk + 1];
    const float n_k = N[kk], denom = b[u] * c[v] - b[v] * c[u];
    float n_u = 0, n_v = 0, n_d = 0, a_u = 0, a_v = 0, b_nu = 0, b_nv = 0, c_nu = 0, c_nv = 0;
    if (denom == 0) {
        kk = 3;
    } else {
        n_u = N[u] / n_k; n_v = N[v] / n_k;
        n_d = (A[0] * N[0] + A[1] * N[1] + A[2] * N[2]) / n_k;
        b_nu = b[u] / denom; b_nv = -b[v] / denom;
        a_u = A[u]; a_v = A[v];
        c_nu = c[v] / denom; c_nv = -c[u] / denom;
    }
    out[0] = make_float4(n_u, n_v, n_d, __builtin_bit_cast(float, kk));
    out[1] = make_float4(a_u, a_v, b_nu, b_nv);
    out[2] = make_float4(c_nu, c_nv, 0.0f, __builtin_bit_cast(float, orig));
}

// A box of the scene: Scene::getAABB() and its parts
struct SceneBox { float mn[3], mx[3]; };

// Scene::getAABB() (scene.cpp:386-414): the kd-tree's box expanded by the sensor's box — the pinhole position (perspective.cpp:444-446) or,
// with a thin lens, the aperture disk (-r, -r, 0) .. (r, r, 0) through the camera's world transform (thinlens.cpp:516-520, track.cpp:123-143)
// ... and by every emitter's box (scene.cpp:400-413): the position of a point or spot emitter (getTranslationBounds of its static
// transform); a directional emitter's box is empty
static void deltaBox(SceneBox &b, const std::vector<ppg_delta_emitter> &deltaEmitters) {
    for (const ppg_delta_emitter &e : deltaEmitters) {
        if (e.type == PPG_EMITTER_DIRECTIONAL) continue;
        for (int a = 0; a < 3; ++a) {
            b.mn[a] = ppg_min(b.mn[a], e.position[a]);
            b.mx[a] = ppg_max(b.mx[a], e.position[a]);
        }
    }
}
static SceneBox sceneBox(const float *geomMin, const float *geomMax, const ppg_lens *lens, const float *c2w, const std::vector<ppg_delta_emitter> &deltaEmitters) {
    SceneBox b;
    for (int a = 0; a < 3; ++a) { b.mn[a] = geomMin[a]; b.mx[a] = geomMax[a]; }
    if (!lens) {
        for (int a = 0; a < 3; ++a) {
            float c = c2w[4 * a + 3];
            b.mn[a] = ppg_min(b.mn[a], c);
            b.mx[a] = ppg_max(b.mx[a], c);
        }
    } else {
        const float r = lens->aperture_radius;
        for (int j = 0; j < 8; ++j) {  // AABB::getCorner(j) of the flat box, Transform::operator()(Point)
            const float p[3] = {(j & 1) ? r : -r, (j & 2) ? r : -r, 0.0f};
            float q[4];
            for (int a = 0; a < 4; ++a) q[a] = c2w[4 * a] * p[0] + c2w[4 * a + 1] * p[1] + c2w[4 * a + 2] * p[2] + c2w[4 * a + 3];
            for (int a = 0; a < 3; ++a) {
                const float v = q[3] == 1.0f ? q[a] : q[a] / q[3];
                b.mn[a] = ppg_min(b.mn[a], v);
                b.mx[a] = ppg_max(b.mx[a], v);
            }
        }
    }
    deltaBox(b, deltaEmitters);
    return b;
}

// Constant / EnvironmentMap: bounding sphere of createShape() (constant.cpp:67-78, envmap.cpp:330-355) around Scene::getAABB()
static float4 envBSphere(const float *aabbMin, const float *aabbMax) {
    float c[3], r2 = 0;
    for (int a = 0; a < 3; ++a) { c[a] = (aabbMax[a] + aabbMin[a]) * 0.5f; }
    const float dx = c[0] - aabbMax[0], dy = c[1] - aabbMax[1], dz = c[2] - aabbMax[2];
    r2 = dx * dx + dy * dy + dz * dz;
    return make_float4(c[0], c[1], c[2], ppg_max(PPG_EPSILON, std::sqrt(r2) * 1.5f));
}

// One record of ppg_set_shapes: Mitsuba's own checks (disk.cpp:101-112; cylinder.cpp:99-107 leaves a rotation) and the inverse of its
// affine transform (in double, rounded once).
static bool shapeCheck(const ppg_shape &sh, float *inv, std::string &err) {
    if (sh.type != PPG_SHAPE_DISK && sh.type != PPG_SHAPE_CYLINDER) { err = "unknown type"; return false; }
    const float *m = sh.to_world;
    for (int i = 0; i < 12; ++i) if (!std::isfinite(m[i])) { err = "a value is not finite"; return false; }
    const bool cyl = sh.type == PPG_SHAPE_CYLINDER;
    if (cyl && (!std::isfinite(sh.radius) || !std::isfinite(sh.length))) { err = "a value is not finite"; return false; }
    if (cyl && !(sh.radius > 0)) { err = "cylinder: radius must be > 0"; return false; }
    if (cyl && !(sh.length > 0)) { err = "cylinder: length must be > 0"; return false; }
    double c[3][3], len[3];
    for (int j = 0; j < 3; ++j) {
        for (int a = 0; a < 3; ++a) c[j][a] = m[4 * a + j];
        len[j] = std::sqrt(c[j][0] * c[j][0] + c[j][1] * c[j][1] + c[j][2] * c[j][2]);
    }
    const double det = c[0][0] * (c[1][1] * c[2][2] - c[1][2] * c[2][1]) - c[0][1] * (c[1][0] * c[2][2] - c[1][2] * c[2][0]) +
                       c[0][2] * (c[1][0] * c[2][1] - c[1][1] * c[2][0]);
    if (len[0] == 0 || len[1] == 0 || len[2] == 0 || !(std::abs(det) > 1e-9 * len[0] * len[1] * len[2])) { err = "its transformation is singular"; return false; }
    auto ndot = [&](int i, int j) { return std::abs((c[i][0] * c[j][0] + c[i][1] * c[j][1] + c[i][2] * c[j][2]) / (len[i] * len[j])); };
    if (!cyl) {
        if (ndot(0, 1) > 1e-3) { err = "disk: its transformation contains shear"; return false; }
        if (std::abs(len[0] / len[1] - 1) > 1e-3) { err = "disk: its transformation contains a non-uniform scale"; return false; }
    } else {
        if (ndot(0, 1) > 1e-3 || ndot(0, 2) > 1e-3 || ndot(1, 2) > 1e-3 || std::abs(len[0] / len[1] - 1) > 1e-3 || std::abs(len[0] / len[2] - 1) > 1e-3 ||
            std::abs(len[0] - 1) > 1e-3) {
            err = "cylinder: the linear part of its transformation is not a rotation (the scale belongs in radius and length)"; return false;
        }
    }
    // inverse of [L | t]: [L^-1 | -L^-1 t]; row i of L^-1 = cross products of L's columns / det
    double li[3][3];
    for (int i = 0; i < 3; ++i) {
        const double *a = c[(i + 1) % 3], *b = c[(i + 2) % 3];
        li[i][0] = (a[1] * b[2] - a[2] * b[1]) / det; li[i][1] = (a[2] * b[0] - a[0] * b[2]) / det; li[i][2] = (a[0] * b[1] - a[1] * b[0]) / det;
    }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) inv[4 * i + j] = (float)li[i][j];
        inv[4 * i + 3] = (float)-(li[i][0] * (double)m[3] + li[i][1] * (double)m[7] + li[i][2] * (double)m[11]);
    }
    return true;
}

// What ppg_set_scene builds a scene from: the caller's ppg_scene, the side lists of the ppg_set_* calls, the lens and the tuning switches
struct SceneInputs {
    const ppg_scene *s;
    const std::vector<ppg_material_textures> &materialTextures;
    const std::vector<ppg_microfacet> &microfacet;
    const std::vector<ppg_coating> &coatings;
    const std::vector<ppg_blend> &blends;
    const std::vector<ppg_delta_emitter> &deltaEmitters;
    const std::vector<ppg_shape> &shapes;
    const ppg_lens *lens;  // the thin lens, or nullptr: a pinhole
    float bvhPad;          // PPG_BVH_PAD
    int bvhLeaf;           // PPG_BVH_LEAF
    bool noTopCut;         // PPG_NO_TOPCUT
    const ppg_media *media = nullptr;  // ppg_set_media's list as the context keeps it, or nullptr: none
    const ppg_media_volumes *mediaVolumes = nullptr;  // ppg_set_media_volumes' list as the context keeps it, or nullptr: none
};

// Every table of a scene as the device reads it, on the host; `scene` carries every scalar of the DevScene and no pointer (the upload fills
// those in), the rest is what the context keeps beside it.
struct HostScene {
    std::vector<float4> tris, accel, accelSmall, normals;
    std::vector<float2> uvs;
    std::vector<BvhNode> nodes;
    std::vector<Bvh4QNode> nodes4q;
    std::vector<float4> topCut;
    std::vector<float4> mats, ems, mfd, coat, blend;  // mfd, coat, blend: empty unless a material uses them
    std::vector<std::vector<float4>> texTexels;
    std::vector<DevTex> textures;  // (texels: null)
    std::vector<float4> envTexels;
    std::vector<float> envCdfRows, envCdfCols, envRowWeights;
    std::vector<float> emSel, emArea;
    std::vector<int4> emInfo;
    std::vector<float4> emTris, emNormals;
    std::vector<float4> delta, shapes, spheres;
    std::vector<float4> media;            // PPG_MEDIUM_STRIDE per medium; media and primMedia: empty unless the list binds a medium
    std::vector<unsigned int> primMedia;  // one binding word per primitive: triangles in leaf order, spheres, shapes
    unsigned int cameraMedium = 0;        // 1 + the sensor's medium
    // ppg_set_media_volumes (HetArgs, ppg_device.h): PPG_VOLUME_STRIDE per volume, the grids' data, PPG_HET_STRIDE per medium; all empty
    // unless a bound medium is heterogeneous
    std::vector<float4> volumes, het;
    std::vector<float> volPool;
    std::vector<float> rtrans;
    std::vector<ppg_delta_emitter> deltaEmitters;  // the list the scene's box was built with (ppg_set_lens builds it again)
    DevScene scene{};
    float geomMin[3], geomMax[3];  // the kd-tree's box (m_kdtree->getAABB()): Scene::getAABB() before the sensor's box is added
    float aabbMin[3], aabbMax[3];  // Scene::getAABB()
    bool fullMaterials = false;
    uint32_t nMaterials = 0;
    int ldsNodes = 0, ldsTris = 0;  // scene part cached in LDS by k_trace
    int W = 0, H = 0;
};

// a scene needs materials and at least one primitive; triangle arrays may be absent when it consists of analytic shapes only
static bool sceneComplete(const SceneInputs &in) {
    const ppg_scene *s = in.s;
    return s && s->materials && !(s->n_triangles == 0 && s->n_spheres == 0 && in.shapes.empty()) &&
           !(s->n_triangles > 0 && (!s->positions || !s->indices || !s->tri_material || !s->tri_emitter));
}

// DiscreteDistribution::normalize (pmf.h:101-114) on a cdf of `entries` running sums, the first of them 0: every entry times
// 1 / (the last), the last set to 1.  Returns the normalisation.  (A sum of 0 is the caller's to deal with.)
static float normalizeCdf(float *cdf, size_t entries) {
    const float normalization = 1.0f / cdf[entries - 1];
    for (size_t i = 1; i < entries; ++i) cdf[i] *= normalization;
    cdf[entries - 1] = 1.0f;
    return normalization;
}

// buildScene's stages, one per kind of table, in the order ppg_set_scene has always checked a scene in: of several defects the first one
// met is the one reported.  What a later stage needs of an earlier one is kept here.
struct SceneBuilder {
    const SceneInputs &in;
    HostScene &H;
    std::string &err;
    const ppg_scene *const s;
    BvhBuilder bb;
    std::vector<int> emitterSphere, emitterShape;  // per emitter: the analytic sphere / the disk or cylinder carrying it, or -1
    std::vector<float> shapeInv;                   // the shapes' inverse transformations, row-major 3x4

    int refuse(const std::string &why) { err = why; return PPG_ERR_INVALID; }
    // the bitmap slots of material i
    ppg_material_textures mtOf(uint32_t i) const { return in.materialTextures.empty() ? ppg_material_textures{0u, 0u, 0u, 0u} : in.materialTextures[i]; }
    // A primitive's material and emitter: both indices and the BSDF type.  `who` names a shape; triangles and spheres name neither
    // themselves nor the index.
    int checkReferences(uint32_t material, int32_t emitter, const std::string &who = "") {
        const bool named = !who.empty();
        if (material >= s->n_materials) return refuse(named ? who + "material index out of range" : "index out of range");
        if (emitter >= (int32_t)s->n_emitters) return refuse(named ? who + "emitter index out of range" : "index out of range");
        if (s->materials[material].type < 0 || s->materials[material].type > PPG_BSDF_LAST_HIP) return refuse(who + "unsupported BSDF type");
        return PPG_OK;
    }
    // a per-material side list is empty or has one entry per material
    int checkListLength(const char *name, size_t entries) {
        if (entries == 0 || entries == s->n_materials) return PPG_OK;
        return refuse(std::string(name) + ": the list has " + std::to_string(entries) + " entries, the scene " + std::to_string(s->n_materials) + " materials");
    }
    // visit(label, material) for every analytic primitive, the spheres ("sphere") before the shapes ("shape k"), until one is refused
    template <typename F> int forEachAnalytic(F visit) {
        for (uint32_t k = 0; k < s->n_spheres; ++k) if (int rc = visit(std::string("sphere"), s->spheres[k].material)) return rc;
        for (size_t k = 0; k < in.shapes.size(); ++k) if (int rc = visit("shape " + std::to_string(k), in.shapes[k].material)) return rc;
        return PPG_OK;
    }
    // the triangle's vertices have texture coordinates (a mesh without them: none, or NaN)
    bool hasTexcoords(uint32_t t) const {
        bool has = s->texcoords != nullptr;
        for (int v = 0; has && v < 3; ++v) { const float q = s->texcoords[2 * (size_t)s->indices[3 * (size_t)t + v]]; if (q != q) has = false; }
        return has;
    }
    // an anisotropic BSDF needs UV tangents, which need texture coordinates (trimesh.cpp:686-691); `what`: ": " or ": blend: "
    template <typename F> int checkAnisotropicTexcoords(F anisotropic, const char *what) {
        for (uint32_t t = 0; t < s->n_triangles; ++t)
            if (anisotropic(s->tri_material[t]) && !hasTexcoords(t))
                return refuse("triangle " + std::to_string(t) + ": material " + std::to_string(s->tri_material[t]) + what +
                              "anisotropic microfacet distribution: the mesh is missing texture coordinates! The tangent space cannot be computed");
        return PPG_OK;
    }

    int primitives(), geometry(), materials(), microfacet(), coatings(), blends(), textures(), envmap(), emitterTables(), deltaEmitters(), shapesAndSpheres(),
        media(), mediaVolumes(), cameraAndLds();
};

// The references of every primitive — triangles, spheres, shapes — and who carries which emitter
int SceneBuilder::primitives() {
    for (uint32_t t = 0; t < s->n_triangles; ++t) {
        if (int rc = checkReferences(s->tri_material[t], s->tri_emitter[t])) return rc;
        for (int k = 0; k < 3; ++k) if (s->indices[3 * t + k] >= s->n_vertices) return refuse("vertex index out of range");
    }
    std::vector<int> users(s->n_emitters, 0);  // per emitter: the primitives met so far that carry it (an analytic one shares it with nobody)
    for (uint32_t t = 0; t < s->n_triangles; ++t) if (s->tri_emitter[t] >= 0) users[s->tri_emitter[t]] = 1;
    emitterSphere.assign(s->n_emitters, -1);
    if (s->n_spheres && !s->spheres) return refuse("spheres: n_spheres > 0 but no array");
    for (uint32_t k = 0; k < s->n_spheres; ++k) {
        const ppg_sphere &sp = s->spheres[k];
        if (!(sp.radius > 0)) return refuse("sphere: radius must be > 0");
        if (int rc = checkReferences(sp.material, sp.emitter)) return rc;
        if (sp.emitter >= 0 && users[sp.emitter]++) return refuse("sphere: its emitter is shared with another shape");
        if (sp.emitter >= 0) emitterSphere[sp.emitter] = (int)k;
    }
    emitterShape.assign(s->n_emitters, -1);
    shapeInv.assign(12 * in.shapes.size(), 0.0f);
    for (size_t k = 0; k < in.shapes.size(); ++k) {
        const ppg_shape &sh = in.shapes[k];
        const std::string who = "shape " + std::to_string(k) + ": ";
        std::string why;
        if (!shapeCheck(sh, &shapeInv[12 * k], why)) return refuse(who + why);
        if (int rc = checkReferences(sh.material, sh.emitter, who)) return rc;
        if (sh.emitter >= 0 && users[sh.emitter]++) return refuse(who + "its emitter is shared with another shape");
        if (sh.emitter >= 0) emitterShape[sh.emitter] = (int)k;
    }
    return PPG_OK;
}

// The scene's boxes, the BVH and the triangle records in its leaf order
int SceneBuilder::geometry() {
    // Scene::getAABB(): kd-tree box enlarged by MTS_KD_AABB_EPSILON (gkdtree.h:1213-1220) + sensor position (scene.cpp:386-414)
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t t = 0; t < 3 * (size_t)s->n_triangles; ++t)
        for (int a = 0; a < 3; ++a) { float v = s->positions[3 * s->indices[t] + a]; mn[a] = ppg_min(mn[a], v); mx[a] = ppg_max(mx[a], v); }
    for (uint32_t k = 0; k < s->n_spheres; ++k)  // Sphere::getAABB, sphere.cpp:152-157
        for (int a = 0; a < 3; ++a) { mn[a] = ppg_min(mn[a], s->spheres[k].center[a] - s->spheres[k].radius); mx[a] = ppg_max(mx[a], s->spheres[k].center[a] + s->spheres[k].radius); }
    for (const ppg_shape &sh : in.shapes) {
        const float *m = sh.to_world;
        for (int a = 0; a < 3; ++a) {
            if (sh.type == PPG_SHAPE_DISK) {  // Disk::getAABB, disk.cpp:117-130: the points (+-1, 0, 0), (0, +-1, 0) transformed
                for (int c = 0; c < 2; ++c) for (int sg = 0; sg < 2; ++sg) {
                    const float v = (sg ? -m[4 * a + c] : m[4 * a + c]) + m[4 * a + 3];
                    mn[a] = ppg_min(mn[a], v); mx[a] = ppg_max(mx[a], v);
                }
            } else {  // Cylinder::getAABB, cylinder.cpp:252-273: the two end circles, component-wise
                const float x1 = m[4 * a] * sh.radius, x2 = m[4 * a + 1] * sh.radius;
                const float p0 = m[4 * a + 3], p1 = m[4 * a + 2] * sh.length + m[4 * a + 3];
                const float range = std::sqrt(x1 * x1 + x2 * x2);
                mn[a] = ppg_min(ppg_min(mn[a], p0 - range), p1 - range);
                mx[a] = ppg_max(ppg_max(mx[a], p0 + range), p1 + range);
            }
        }
    }
    const float eps = 1e-3f;
    for (int a = 0; a < 3; ++a) {
        H.geomMin[a] = mn[a] - ((mx[a] - mn[a]) * eps + eps);
        H.geomMax[a] = mx[a] + ((mx[a] - H.geomMin[a]) * eps + eps);
    }
    const SceneBox box = sceneBox(H.geomMin, H.geomMax, in.lens, s->camera.camera_to_world, in.deltaEmitters);
    for (int a = 0; a < 3; ++a) { H.aabbMin[a] = box.mn[a]; H.aabbMax[a] = box.mx[a]; }
    H.deltaEmitters = in.deltaEmitters;
    float ext = 0;
    for (int a = 0; a < 3; ++a) ext = std::max(ext, mx[a] - mn[a]);
    if (!(ext < 1e9f)) return refuse("scene extent of 1e9 units or more (or not finite)");  // BvhBuilder::quantise
    // Box padding: the BVH must return what brute force returns.  A slab test carries a few ulps of error in t, i.e. up to
    // ~4 * 2^-24 * (distance travelled) in position; 2e-6 * (scene extent) leaves an 8x margin.  (1e-4 * extent, the first
    // choice, made the leaf boxes of a finely tessellated model under a 100 m sky dome several triangles thick: 4x slower.)
    const float padRel = in.bvhPad;
    bb.maxLeaf = in.bvhLeaf;
    bb.run(s->positions, s->indices, s->n_triangles, padRel * ext + 1e-30f);
    if (bb.stackNeed > BvhBuilder::STACK_MAX)   // (not reached by medians below 2^16 triangles per offending subtree: BvhBuilder::boundStack)
        return refuse("the scene's BVH needs a traversal stack of " + std::to_string(bb.stackNeed) + " entries, the kernels' holds " + std::to_string(BvhBuilder::STACK_MAX));
    // the triangles' records in leaf order: positions, TriAccel and, where the mesh has them, normals and texture coordinates
    std::vector<float4> &tris = H.tris, &nrm = H.normals, &accel = H.accel;
    tris.assign(3 * (size_t)s->n_triangles, float4{}); accel.assign(3 * (size_t)s->n_triangles, float4{});
    if (s->normals) nrm.resize(tris.size());
    if (s->texcoords) H.uvs.resize(tris.size());
    for (uint32_t k = 0; k < s->n_triangles; ++k) {
        uint32_t t = bb.order[k];
        triAccelLoad(s->positions + 3 * s->indices[3 * t], s->positions + 3 * s->indices[3 * t + 1], s->positions + 3 * s->indices[3 * t + 2], (int)t, &accel[3 * k]);
        for (int v = 0; v < 3; ++v) {
            const float *p = s->positions + 3 * s->indices[3 * t + v];
            float w = v == 0 ? __builtin_bit_cast(float, (int)s->tri_material[t]) : (v == 1 ? __builtin_bit_cast(float, (int)s->tri_emitter[t]) : __builtin_bit_cast(float, (int)t));
            tris[3 * k + v] = make_float4(p[0], p[1], p[2], w);
            if (s->normals) { const float *n = s->normals + 3 * s->indices[3 * t + v]; nrm[3 * k + v] = make_float4(n[0], n[1], n[2], 0); }
            if (s->texcoords) { const float *q = s->texcoords + 2 * (size_t)s->indices[3 * t + v]; H.uvs[3 * (size_t)k + v] = make_float2(q[0], q[1]); }
        }
    }
    {   // small scenes are traced by brute force from LDS: the same records grouped by projection axis (degenerate ones dropped,
        // the rest padded with never-hit records so that n_tris records can always be staged), leaf-order index in record[2].z
        std::vector<float4> &small = H.accelSmall;
        small.assign(accel.size(), make_float4(0, 0, 0, __builtin_bit_cast(float, 3)));
        int n[3] = {0, 0, 0};
        if (s->n_triangles <= 64) {
            size_t w = 0;
            for (int axis = 0; axis < 3; ++axis)
                for (uint32_t k = 0; k < s->n_triangles; ++k)
                    if (__builtin_bit_cast(int, accel[3 * k].w) == axis) {
                        small[3 * w] = accel[3 * k]; small[3 * w + 1] = accel[3 * k + 1]; small[3 * w + 2] = accel[3 * k + 2];
                        small[3 * w + 2].z = __builtin_bit_cast(float, (int)k);
                        ++w; ++n[axis];
                    }
        }
        for (int axis = 0; axis < 3; ++axis) H.scene.small_n[axis] = n[axis];
    }
    H.nodes = std::move(bb.nodes); H.nodes4q = std::move(bb.nodes4q);
    H.topCut.resize(bb.topCut.size() / 4);
    if (!bb.topCut.empty()) memcpy(H.topCut.data(), bb.topCut.data(), bb.topCut.size() * sizeof(float));
    H.scene.n_top = in.noTopCut ? 0 : (int)(bb.topCut.size() / 8);
    H.scene.n_tris = (int)s->n_triangles;
    return PPG_OK;
}

// The material table with the bitmap slots of ppg_set_material_textures: PPG_MAT_STRIDE float4 per BSDF = (reflectance, type) (specular, alpha)
// (eta, flags) (k, fdrInt) (opacity, rtrans slice) (texture words); the lean kernels read only the first.  configure()-time normalisation as in
// the plugins: "none" conductor = (eta 0, k 1) (conductor.cpp:171-173), GGX alpha clamped (microfacet.h:135), plastic's internal diffuse Fresnel
// reflectance (plastic.cpp:191-193).  Also the emitters' radiance and the rough-transmittance slices.
int SceneBuilder::materials() {
    std::vector<float4> &mats = H.mats;
    mats.assign(PPG_MAT_STRIDE * (size_t)s->n_materials, float4{});
    bool hasNull = false;
    if (int rc = checkListLength("material textures", in.materialTextures.size())) return rc;
    for (uint32_t i = 0; i < s->n_materials; ++i) {
        ppg_material m = s->materials[i];
        const ppg_material_textures mt = mtOf(i);
        if (m.type == PPG_BSDF_DIFFUSE && m.flags == PPG_MAT_TWOSIDED) { m.type = PPG_BSDF_TWOSIDED_DIFFUSE; m.flags = 0; }
        if (m.type == PPG_BSDF_TWOSIDED_DIFFUSE) m.flags &= ~PPG_MAT_TWOSIDED;
        if (m.type == PPG_BSDF_MIRROR) for (int c = 0; c < 3; ++c) { m.eta[c] = 0.0f; m.k[c] = 1.0f; }
        if (m.type == PPG_BSDF_ROUGHCONDUCTOR || m.type == PPG_BSDF_ROUGHDIELECTRIC || m.type == PPG_BSDF_ROUGHPLASTIC) m.alpha = ppg_max(m.alpha, 1e-4f);
        if ((m.type == PPG_BSDF_PLASTIC || m.type == PPG_BSDF_DIELECTRIC || m.type == PPG_BSDF_THINDIELECTRIC || m.type == PPG_BSDF_ROUGHDIELECTRIC) && !(m.eta[0] > 0))
            return refuse("plastic / dielectric need eta[0] = intIOR / extIOR > 0");
        float fdrInt = m.type == PPG_BSDF_PLASTIC ? ppg_fresnel_diffuse_reflectance(1 / m.eta[0]) : 0.0f;
        if (m.type == PPG_BSDF_ROUGHPLASTIC) {  // Fdr = 1 - internal diffuse transmittance, the last entry of the slice (roughplastic.cpp:372)
            if (m.rtrans < 0 || (uint32_t)m.rtrans >= s->n_rtrans || !s->rtrans || s->rtrans_samples < 2)
                return refuse("roughplastic: material.rtrans is not a slice of scene.rtrans");
            if (!(m.eta[0] > 0)) return refuse("plastic / dielectric need eta[0] = intIOR / extIOR > 0");
            fdrInt = 1 - s->rtrans[(size_t)m.rtrans * (s->rtrans_samples + 1) + s->rtrans_samples];
        } else m.rtrans = 0;
        {   // roughdiffuse, difftrans and phong: the lobes kernels (ppg_device.h PPG_LOBES)
            const std::string who = "material " + std::to_string(i) + ": ";
            const bool lobe = m.type == PPG_BSDF_ROUGHDIFFUSE || m.type == PPG_BSDF_DIFFTRANS || m.type == PPG_BSDF_PHONG;
            if ((m.flags & PPG_MAT_FAST_APPROX) && m.type != PPG_BSDF_ROUGHDIFFUSE) return refuse(who + "PPG_MAT_FAST_APPROX (useFastApprox) is a flag of roughdiffuse only");
            if (m.type == PPG_BSDF_DIFFTRANS && (m.flags & PPG_MAT_TWOSIDED))
                return refuse(who + "difftrans cannot be two-sided: only BRDFs can be (twosided.cpp:84-88)");
            if (m.type == PPG_BSDF_ROUGHDIFFUSE && !(std::isfinite(m.alpha) && m.alpha >= 0)) return refuse(who + "roughdiffuse: alpha must be finite and not negative");
            if (m.type == PPG_BSDF_PHONG) {
                if (!(std::isfinite(m.alpha) && m.alpha >= 0)) return refuse(who + "phong: exponent must be finite and not negative");
                const float dAvg = m.reflectance[0] * 0.212671f + m.reflectance[1] * 0.715160f + m.reflectance[2] * 0.072169f;
                const float sAvg = m.specular[0] * 0.212671f + m.specular[1] * 0.715160f + m.specular[2] * 0.072169f;
                if (dAvg == 0 && sAvg == 0)
                    return refuse(who + "phong: diffuseReflectance and specularReflectance both have luminance 0 (specularSamplingWeight would be 0 / 0)");
            }
            if (lobe && (mt.specular || mt.alpha))
                return refuse(who + "texture slot " + (mt.specular ? "specular" : "alpha") + ": roughdiffuse, difftrans and phong read no bitmap but `reflectance` and `opacity`");
            if (lobe) H.scene.lobes |= 1;
        }
        {   // the normalmap adapter and the null BSDF: compiled by the top kernel family alone (ppg_device.h PPG_NORMALMAP_NULL)
            const std::string who = "material " + std::to_string(i) + ": ";
            if ((m.flags & PPG_MAT_NORMALMAP) && !(m.texture >> 16))
                return refuse(who + "PPG_MAT_NORMALMAP without a normal map: bits 16..31 of `texture` are 0");
            if (m.type == PPG_BSDF_NULL) {
                if (m.flags & PPG_MAT_TWOSIDED) return refuse(who + "null cannot be two-sided: only BRDFs can be (twosided.cpp:84-88)");
                if (m.flags & PPG_MAT_MASK) return refuse(who + "null: a mask around the null BSDF is not supported");
                if (m.flags) return refuse(who + "null takes no flags");
                if (m.texture) return refuse(who + "null reads no bitmap and takes no bump or normal map: `texture` must be 0");
                if (mt.specular || mt.alpha || mt.opacity)
                    return refuse(who + "texture slot " + (mt.specular ? "specular" : mt.alpha ? "alpha" : "opacity") + ": null reads no bitmap");
            }
            if ((m.flags & PPG_MAT_NORMALMAP) || m.type == PPG_BSDF_NULL) H.scene.lobes |= 2;
        }
        if (m.type > PPG_BSDF_MIRROR || m.flags != 0) H.fullMaterials = true;
        if (m.type == PPG_BSDF_THINDIELECTRIC || m.type == PPG_BSDF_NULL || (m.flags & PPG_MAT_MASK)) hasNull = true;
        mats[PPG_MAT_STRIDE * i + 0] = make_float4(m.reflectance[0], m.reflectance[1], m.reflectance[2], (float)m.type);
        mats[PPG_MAT_STRIDE * i + 1] = make_float4(m.specular[0], m.specular[1], m.specular[2], m.alpha);
        mats[PPG_MAT_STRIDE * i + 2] = make_float4(m.eta[0], m.eta[1], m.eta[2], __builtin_bit_cast(float, m.flags));
        mats[PPG_MAT_STRIDE * i + 3] = make_float4(m.k[0], m.k[1], m.k[2], fdrInt);
        mats[PPG_MAT_STRIDE * i + 4] = make_float4(m.opacity[0], m.opacity[1], m.opacity[2], __builtin_bit_cast(float, m.rtrans));
        {   // bitmap on the diffuse reflectance / bump map around the BSDF
            const uint32_t ta = m.texture & 0xffffu, tb = m.texture >> 16;
            if (ta > s->n_textures || tb > s->n_textures || (m.texture && !s->textures)) return refuse("material.texture: index out of range");
            // (every BSDF type reads `reflectance`: the diffuse reflectance, or the specularReflectance of conductors and dielectrics)
            // bitmaps on specular / alpha / opacity: ppg_set_material_textures
            const std::string who = "material " + std::to_string(i) + ": texture slot ";
            const bool readsSpecular = m.type == PPG_BSDF_PLASTIC || m.type == PPG_BSDF_ROUGHPLASTIC || m.type == PPG_BSDF_DIELECTRIC ||
                                       m.type == PPG_BSDF_THINDIELECTRIC || m.type == PPG_BSDF_ROUGHDIELECTRIC;
            if (mt._reserved) return refuse(who + "_reserved must be 0");
            if ((mt.specular || mt.alpha || mt.opacity) && !s->textures) return refuse(who + "set, but the scene has no textures");
            if (mt.specular > s->n_textures) return refuse(who + "specular: index out of range");
            if (mt.alpha > s->n_textures) return refuse(who + "alpha: index out of range");
            if (mt.opacity > s->n_textures) return refuse(who + "opacity: index out of range");
            if (mt.specular && !readsSpecular) return refuse(who + "specular: only plastic, roughplastic and the dielectrics read `specular`");
            if (mt.alpha && m.type == PPG_BSDF_ROUGHPLASTIC)
                return refuse(who + "alpha: roughplastic's rough-transmittance slice is tabulated for one alpha; a roughness map is not supported");
            if (mt.alpha && m.type != PPG_BSDF_ROUGHCONDUCTOR && m.type != PPG_BSDF_ROUGHDIELECTRIC)
                return refuse(who + "alpha: only roughconductor and roughdielectric read `alpha`");
            if (mt.opacity && !(m.flags & PPG_MAT_MASK)) return refuse(who + "opacity: the material is not masked (PPG_MAT_MASK)");
            if (m.texture || mt.specular || mt.alpha || mt.opacity) H.fullMaterials = true;  // the texture code lives in the FULL kernel variants
            if (mt.opacity || (mt.specular && m.type == PPG_BSDF_THINDIELECTRIC))  // what mat_eval_null reads is a bitmap (ppg_device.h)
                mats[PPG_MAT_STRIDE * i + 2].w = __builtin_bit_cast(float, m.flags | PPG_MATF_NULL_TEXTURED);
            mats[PPG_MAT_STRIDE * i + 5] = make_float4(__builtin_bit_cast(float, m.texture), __builtin_bit_cast(float, mt.specular), __builtin_bit_cast(float, mt.alpha),
                                                       __builtin_bit_cast(float, mt.opacity));
        }
    }
    H.scene.has_null = hasNull ? 1 : 0;
    if (int rc = forEachAnalytic([&](const std::string &label, uint32_t sm) {
            if (s->materials[sm].type == PPG_BSDF_NULL)
                return refuse(label + ": material " + std::to_string(sm) + ": the null BSDF is only supported on triangle meshes (not on spheres, disks or cylinders)");
            if (s->materials[sm].texture)
                return refuse(label + ": textured BSDFs are only supported on triangle meshes" + (label == "sphere" ? " (not on spheres, disks or cylinders)" : ""));
            if (mtOf(sm).specular || mtOf(sm).alpha || mtOf(sm).opacity)
                return refuse(label + ": material " + std::to_string(sm) + ": a texture slot (specular / alpha / opacity) is set; textured BSDFs are only supported on triangle meshes");
            return (int)PPG_OK;
        })) return rc;
    H.ems.assign(std::max<uint32_t>(1, s->n_emitters), float4{});
    for (uint32_t i = 0; i < s->n_emitters; ++i) H.ems[i] = make_float4(s->emitters[i].radiance[0], s->emitters[i].radiance[1], s->emitters[i].radiance[2], 0);
    if (s->n_rtrans && s->rtrans) H.rtrans.assign(s->rtrans, s->rtrans + (size_t)s->n_rtrans * (s->rtrans_samples + 1));
    H.scene.rtrans_n = (int)s->rtrans_samples;
    H.nMaterials = s->n_materials;
    return PPG_OK;
}

// ppg_set_microfacet: the general MicrofacetDistribution of the three rough plug-ins
int SceneBuilder::microfacet() {
    bool anyGeneral = false;
    std::vector<float4> &mfdTab = H.mfd;
    if (int rc = checkListLength("microfacet", in.microfacet.size())) return rc;
    if (!in.microfacet.empty()) {
        mfdTab.assign(s->n_materials, make_float4(0, 0, 0, 0));
        for (uint32_t i = 0; i < s->n_materials; ++i) {
            const ppg_microfacet &g = in.microfacet[i];
            const ppg_material &m = s->materials[i];
            const std::string who = "material " + std::to_string(i) + ": microfacet: ";
            if (g._reserved[0] || g._reserved[1] || g._reserved[2]) return refuse(who + "_reserved must be 0");
            if (!g.general) continue;
            if (m.type != PPG_BSDF_ROUGHCONDUCTOR && m.type != PPG_BSDF_ROUGHDIELECTRIC && m.type != PPG_BSDF_ROUGHPLASTIC)
                return refuse(who + "only roughconductor, roughdielectric and roughplastic have a microfacet distribution");
            if (g.distribution != 0 && g.distribution != 1) return refuse(who + "distribution must be 0 (ggx / beckmann) or 1 (phong)");
            if (!std::isfinite(g.alpha_v)) return refuse(who + "alpha_v is not finite");
            if (g.alpha_v_texture > s->n_textures || (g.alpha_v_texture && !s->textures)) return refuse(who + "alpha_v_texture: index out of range");
            const float alphaU = ppg_max(m.alpha, 1e-4f), alphaV = ppg_max(g.alpha_v, 1e-4f);
            if (m.type == PPG_BSDF_ROUGHPLASTIC && g.alpha_v_texture)
                return refuse(who + "alpha_v_texture: roughplastic's rough-transmittance slice is tabulated for one alpha; a roughness map is not supported");
            if (m.type == PPG_BSDF_ROUGHPLASTIC && alphaU != alphaV)  // roughplastic.cpp:221
                return refuse(who + "roughplastic: the 'roughplastic' plugin currently does not support anisotropic microfacet distributions!");
            const bool alphaTextured = g.alpha_v_texture || mtOf(i).alpha;
            uint32_t bits = PPG_MFDF_GENERAL;
            if (g.distribution == 1) bits |= PPG_MFDF_PHONG | PPG_MFDF_SAMPLE_ALL;  // microfacet.h:141-142
            if (g.sample_all) bits |= PPG_MFDF_SAMPLE_ALL;
            if (alphaU != alphaV || alphaTextured) bits |= PPG_MFDF_ANISO;
            mfdTab[i] = make_float4(alphaV, __builtin_bit_cast(float, bits), __builtin_bit_cast(float, g.alpha_v_texture), 0.0f);
            anyGeneral = true;
        }
    }
    if (!anyGeneral) { mfdTab.clear(); return PPG_OK; }
    if (int rc = forEachAnalytic([&](const std::string &label, uint32_t sm) {
            return __builtin_bit_cast(uint32_t, mfdTab[sm].z) ? refuse(label + ": a textured alphaV is only supported on triangle meshes") : (int)PPG_OK;
        })) return rc;
    if (int rc = checkAnisotropicTexcoords([&](uint32_t m) { return (__builtin_bit_cast(uint32_t, mfdTab[m].y) & PPG_MFDF_ANISO) != 0; }, ": ")) return rc;
    H.fullMaterials = true;  // (the rough types are FULL anyway)
    return PPG_OK;
}

// ppg_set_coatings: the coating / roughcoating adapters
int SceneBuilder::coatings() {
    bool anyCoat = false;
    std::vector<float4> &coatTab = H.coat;
    if (int rc = checkListLength("coatings", in.coatings.size())) return rc;
    if (!in.coatings.empty()) {
        coatTab.assign(PPG_COAT_STRIDE * (size_t)s->n_materials, make_float4(0, 0, 0, 0));
        for (uint32_t i = 0; i < s->n_materials; ++i) {
            const ppg_coating &c = in.coatings[i];
            const ppg_material &m = s->materials[i];
            const std::string who = "material " + std::to_string(i) + ": coating: ";
            if (c._reserved[0] || c._reserved[1] || c._reserved[2]) return refuse(who + "_reserved must be 0");
            if (c.kind == 0) continue;
            if (c.kind != 1 && c.kind != 2) return refuse(who + "kind must be 0 (none), 1 (coating) or 2 (roughcoating)");
            const char *name = c.kind == 1 ? "coating" : "roughcoating";
            if (m.type == PPG_BSDF_ROUGHDIFFUSE || m.type == PPG_BSDF_DIFFTRANS || m.type == PPG_BSDF_PHONG)
                return refuse(who + name + " over roughdiffuse, difftrans or phong is not supported");
            if (m.type == PPG_BSDF_NULL) return refuse(who + name + " over the null BSDF is not supported");
            if (m.type == PPG_BSDF_DIELECTRIC || m.type == PPG_BSDF_THINDIELECTRIC || m.type == PPG_BSDF_ROUGHDIELECTRIC || m.type < 0 || m.type > PPG_BSDF_LAST_HIP)
                return refuse(who + name + " over dielectric, thindielectric or roughdielectric is not supported");
            if (c.kind == 2 && (m.type == PPG_BSDF_MIRROR || m.type == PPG_BSDF_CONDUCTOR || m.type == PPG_BSDF_PLASTIC))
                return refuse(who + "roughcoating over a BSDF with a delta component (conductor, plastic) is not supported");
            bool finite = std::isfinite(c.eta) && std::isfinite(c.thickness);
            for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(c.sigma_a[k]) && std::isfinite(c.specular[k]);
            if (c.kind == 2) finite = finite && std::isfinite(c.alpha);
            if (!finite) return refuse(who + "a value is not finite");
            if (!(c.eta > 0) || c.eta == 1.0f) return refuse(who + "the interior and exterior indices of refraction must be positive and differ (eta > 0, eta != 1)");
            if (c.thickness < 0) return refuse(who + "thickness must not be negative");
            if (c.sigma_a[0] < 0 || c.sigma_a[1] < 0 || c.sigma_a[2] < 0) return refuse(who + "sigma_a must not be negative");
            uint32_t bits = (uint32_t)c.kind;
            int rows = 0;
            if (c.kind == 2) {
                if (c.distribution < 0 || c.distribution > 2) return refuse(who + "distribution must be 0 (beckmann), 1 (ggx) or 2 (phong)");
                if (c.rtrans < 0 || (uint32_t)c.rtrans >= s->n_rtrans || !s->rtrans || s->rtrans_samples < 2) return refuse(who + "rtrans is not a slice of scene.rtrans");
                bits |= (uint32_t)c.distribution << PPG_COATF_TYPE_SHIFT;
                if (c.sample_all || c.distribution == 2) bits |= PPG_COATF_SAMPLE_ALL;  // microfacet.h:141-142
                rows = c.rtrans - (m.type == PPG_BSDF_ROUGHPLASTIC ? m.rtrans : 0);  // from the slice the material record names (Mat::rt)
            }
            // m_specularSamplingWeight (coating.cpp:178-181), once, with the library's own exp: every host gets the same bits
            float sum = 0.0f;
            for (int k = 0; k < 3; ++k) sum += ppg_exp(c.sigma_a[k] * (-2 * c.thickness));
            const float avgAbsorption = sum * (1.0f / 3);
            const float weight = 1.0f / (avgAbsorption + 1.0f);
            coatTab[PPG_COAT_STRIDE * (size_t)i + 0] = make_float4(c.eta, c.thickness, weight, __builtin_bit_cast(float, bits));
            coatTab[PPG_COAT_STRIDE * (size_t)i + 1] = make_float4(c.sigma_a[0], c.sigma_a[1], c.sigma_a[2], c.kind == 2 ? c.alpha : 0.0f);
            coatTab[PPG_COAT_STRIDE * (size_t)i + 2] = make_float4(c.specular[0], c.specular[1], c.specular[2], __builtin_bit_cast(float, rows));
            anyCoat = true;
        }
    }
    if (anyCoat) H.fullMaterials = true;
    else coatTab.clear();
    return PPG_OK;
}

// ppg_set_blends: the blendbsdf / mixturebsdf combinators.  Everything the device code relies on is checked here — every child index,
// and that a child is a plain leaf —, so its loops over the children are bounded and nothing recurses.
int SceneBuilder::blends() {
    bool anyBlend = false;
    std::vector<float4> &blendTab = H.blend;
    const std::vector<float4> &mfdTab = H.mfd;  // (empty without a general entry)
    std::vector<unsigned char> readsBitmap(s->n_materials, 0), anisoChild(s->n_materials, 0);
    if (int rc = checkListLength("blends", in.blends.size())) return rc;
    if (!in.blends.empty()) {
        blendTab.assign(PPG_BLEND_STRIDE * (size_t)s->n_materials, make_float4(0, 0, 0, 0));
        for (uint32_t i = 0; i < s->n_materials; ++i) {
            const ppg_blend &b = in.blends[i];
            const ppg_material &m = s->materials[i];
            const std::string who = "material " + std::to_string(i) + ": blend: ";
            if (b._reserved[0] || b._reserved[1] || b._reserved[2] || b._reserved[3]) return refuse(who + "_reserved must be 0");
            if (b.kind == 0) continue;
            if (b.kind != 1 && b.kind != 2) return refuse(who + "kind must be 0 (none), 1 (blendbsdf) or 2 (mixturebsdf)");
            const char *name = b.kind == 1 ? "blendbsdf" : "mixturebsdf";
            if (b.kind == 1 && b.n != 2) return refuse(who + "blendbsdf takes exactly two nested BSDFs (n = " + std::to_string(b.n) + ")");
            if (b.n < 1 || b.n > PPG_BLEND_MAX)
                return refuse(who + "mixturebsdf takes 1 .. " + std::to_string(PPG_BLEND_MAX) + " nested BSDFs (n = " + std::to_string(b.n) + ")");
            if (m.type != PPG_BSDF_DIFFUSE) return refuse(who + "the blended material's own record must be of type PPG_BSDF_DIFFUSE (it only carries the adapters)");
            if (!in.coatings.empty() && in.coatings[i].kind) return refuse(who + "coating(" + name + ") is not supported");
            if (m.texture & 0xffffu) return refuse(who + "a reflectance bitmap on the blended record itself is not supported (set it on a child)");
            if (mtOf(i).specular || mtOf(i).alpha) return refuse(who + "a specular / alpha texture slot on the blended record itself is not supported (set it on a child)");
            if (!in.microfacet.empty() && in.microfacet[i].general)
                return refuse(who + "a microfacet entry on the blended record itself is not supported (set it on a child)");
            for (uint32_t k = 0; k < b.n; ++k) {
                const uint32_t c = b.child[k];
                const std::string kid = who + "child " + std::to_string(k) + " (material " + std::to_string(c) + ")";
                if (c >= s->n_materials) return refuse(kid + ": index out of range");
                const ppg_material &cm = s->materials[c];
                if (in.blends[c].kind) return refuse(kid + " is itself blended: blends of blends are not supported");
                if (!in.coatings.empty() && in.coatings[c].kind) return refuse(kid + " is coated: coated children are not supported");
                if (cm.type == PPG_BSDF_ROUGHDIFFUSE || cm.type == PPG_BSDF_DIFFTRANS || cm.type == PPG_BSDF_PHONG)
                    return refuse(kid + ": roughdiffuse, difftrans and phong children are not supported");
                if (cm.type == PPG_BSDF_NULL) return refuse(kid + ": a null child is not supported");
                if (cm.type == PPG_BSDF_DIELECTRIC || cm.type == PPG_BSDF_THINDIELECTRIC || cm.type == PPG_BSDF_ROUGHDIELECTRIC || cm.type < 0 || cm.type > PPG_BSDF_LAST_HIP)
                    return refuse(kid + ": dielectric, thindielectric and roughdielectric children are not supported");
                if ((cm.flags & (PPG_MAT_TWOSIDED | PPG_MAT_MASK)) || cm.type == PPG_BSDF_TWOSIDED_DIFFUSE || (cm.texture >> 16))
                    return refuse(kid + " is masked, two-sided or bump-mapped: the adapters go around the blend, on its own record");
                if ((cm.texture & 0xffffu) || mtOf(c).specular || mtOf(c).alpha || (!in.microfacet.empty() && in.microfacet[c].general && in.microfacet[c].alpha_v_texture))
                    readsBitmap[i] = 1;
                if (!mfdTab.empty() && (__builtin_bit_cast(uint32_t, mfdTab[c].y) & PPG_MFDF_ANISO)) anisoChild[i] = 1;
            }
            for (uint32_t k = b.n; k < PPG_BLEND_MAX; ++k)
                if (b.child[k] || b.weight[k] != 0.0f) return refuse(who + "child and weight beyond n must be 0");
            float we[PPG_BLEND_MAX] = {0, 0, 0, 0}, cdf[PPG_BLEND_MAX + 1] = {0, 0, 0, 0, 0};
            uint32_t weightTex = 0;
            if (b.kind == 1) {
                if (!std::isfinite(b.weight[0]) || b.weight[0] < 0) return refuse(who + "weight must be finite and not negative");
                if (b.weight[1] != 0.0f) return refuse(who + "blendbsdf reads weight[0] only; weight[1] must be 0");
                if (b.ensure_energy_conservation) return refuse(who + "ensure_energy_conservation belongs to mixturebsdf; must be 0");
                if (b.weight_texture > s->n_textures || (b.weight_texture && !s->textures)) return refuse(who + "weight_texture: index out of range");
                weightTex = b.weight_texture;
                if (weightTex) readsBitmap[i] = 1;
                const float w = ppg_min(1.0f, ppg_max(0.0f, b.weight[0]));  // blendbsdf.cpp:136-137
                we[0] = 1 - w; we[1] = w;
                cdf[1] = we[0]; cdf[2] = 1.0f;  // (the device chooses by sample.x < weights[0], as the plug-in does: not read)
            } else {
                if (b.weight_texture) return refuse(who + "weight_texture belongs to blendbsdf; must be 0");
                float total = 0.0f;
                for (uint32_t k = 0; k < b.n; ++k) {
                    if (!std::isfinite(b.weight[k]) || b.weight[k] < 0) return refuse(who + "weights must be finite and not negative");
                    we[k] = b.weight[k];
                    total += we[k];  // mixturebsdf.cpp:123-125
                }
                if (!std::isfinite(total)) return refuse(who + "weights must be finite and not negative");
                if (!(total > 0)) return refuse(who + "The weights must sum to a value greater than zero!");
                if (b.ensure_energy_conservation && total > 1) {  // mixturebsdf.cpp:130-141
                    const float scale = 1.0f / total;
                    for (uint32_t k = 0; k < b.n; ++k) we[k] *= scale;
                }
                for (uint32_t k = 0; k < b.n; ++k) cdf[k + 1] = cdf[k] + we[k];  // DiscreteDistribution::append, pmf.h:68-70
                normalizeCdf(cdf, b.n + 1);
            }
            bool smoothAny = false;
            for (uint32_t k = 0; k < b.n; ++k) {
                const int t = s->materials[b.child[k]].type;
                smoothAny = smoothAny || t == PPG_BSDF_DIFFUSE || t == PPG_BSDF_ROUGHCONDUCTOR || t == PPG_BSDF_PLASTIC || t == PPG_BSDF_ROUGHPLASTIC;
            }
            uint32_t bits = (uint32_t)b.kind | (b.n << PPG_BLENDF_N_SHIFT);
            if (readsBitmap[i] || anisoChild[i]) bits |= PPG_BLENDF_TEXTURED;
            if (smoothAny) bits |= PPG_BLENDF_SMOOTH;
            float4 *row = &blendTab[PPG_BLEND_STRIDE * (size_t)i];
            row[0] = make_float4(__builtin_bit_cast(float, b.child[0]), __builtin_bit_cast(float, b.child[1]), __builtin_bit_cast(float, b.child[2]), __builtin_bit_cast(float, b.child[3]));
            row[1] = make_float4(we[0], we[1], we[2], we[3]);
            row[2] = make_float4(cdf[0], cdf[1], cdf[2], cdf[3]);
            row[3] = make_float4(cdf[4], __builtin_bit_cast(float, bits), __builtin_bit_cast(float, weightTex), 0.0f);
            anyBlend = true;
        }
    }
    if (!anyBlend) { blendTab.clear(); return PPG_OK; }
    if (int rc = forEachAnalytic([&](const std::string &label, uint32_t sm) {
            return readsBitmap[sm] ? refuse(label + ": material " + std::to_string(sm) + ": blend: textured BSDFs are only supported on triangle meshes") : (int)PPG_OK;
        })) return rc;
    // an anisotropic child needs UV tangents, as an anisotropic material does
    if (int rc = checkAnisotropicTexcoords([&](uint32_t m) { return anisoChild[m] != 0; }, ": blend: ")) return rc;
    H.fullMaterials = true;
    return PPG_OK;
}

// the bitmaps: texels as (rgb, -) and the table that describes them
int SceneBuilder::textures() {
    if (s->n_textures) {
        if (!s->textures) return refuse("textures: n_textures > 0 but no array");
        std::vector<DevTex> &table = H.textures;
        table.assign(s->n_textures, DevTex{});
        H.texTexels.resize(s->n_textures);
        for (uint32_t i = 0; i < s->n_textures; ++i) {
            const ppg_texture &t = s->textures[i];
            if (!t.rgb || t.width == 0 || t.height == 0 || t.width > 0x7fff || t.height > 0x7fff || t.wrap_u < 0 || t.wrap_u > PPG_WRAP_ONE || t.wrap_v < 0 || t.wrap_v > PPG_WRAP_ONE)
                return refuse("texture: needs pixels, 0 < width, height < 32768 and valid wrap modes");
            const size_t n = (size_t)t.width * t.height;
            std::vector<float4> &px = H.texTexels[i];
            px.resize(n);
            for (size_t k = 0; k < n; ++k) px[k] = make_float4(t.rgb[3 * k], t.rgb[3 * k + 1], t.rgb[3 * k + 2], 0.0f);
            DevTex &d = table[i];
            d.texels = nullptr; d.w = (int)t.width; d.h = (int)t.height; d.su = t.uv_scale[0]; d.sv = t.uv_scale[1]; d.ou = t.uv_offset[0]; d.ov = t.uv_offset[1];
            d.wrap_u = t.wrap_u; d.wrap_v = t.wrap_v; d.nearest = t.nearest != 0; d.pad = 0;
        }
    }
    return PPG_OK;
}

// the image-based environment emitter.  EnvironmentMap::configure (envmap.cpp:255-322): the same float running sums as the oracle's
int SceneBuilder::envmap() {
    if (s->envmap) {
        const ppg_envmap &em = *s->envmap;
        if (s->environment) return refuse("envmap: a scene has one environment emitter (`environment` is set as well)");
        if (!em.rgb || em.width == 0 || em.height == 0 || em.width > 0xFFFF || em.height > 0xFFFF) return refuse("envmap: needs pixels and 0 < width, height < 65536");
        const int w = (int)em.width, h = (int)em.height;
        std::vector<float4> &tex = H.envTexels;
        std::vector<float> &cdfCols = H.envCdfCols, &cdfRows = H.envCdfRows, &rowWeights = H.envRowWeights;
        tex.assign((size_t)w * h, float4{});
        cdfCols.assign((size_t)(w + 1) * h, 0.0f); cdfRows.assign(h + 1, 0.0f); rowWeights.assign(h, 0.0f);
        size_t colPos = 0, rowPos = 0;
        float rowSum = 0.0f;
        cdfRows[rowPos++] = 0;
        for (int y = 0; y < h; ++y) {
            float colSum = 0;
            cdfCols[colPos++] = 0;
            for (int x = 0; x < w; ++x) {
                const float *px = em.rgb + 3 * ((size_t)y * w + x);
                tex[(size_t)y * w + x] = make_float4(px[0], px[1], px[2], 0.0f);
                colSum += px[0] * 0.212671f + px[1] * 0.715160f + px[2] * 0.072169f;
                cdfCols[colPos++] = colSum;
            }
            normalizeCdf(&cdfCols[colPos - (size_t)(w + 1)], (size_t)w + 1);
            float weight, cosUnused;
            ppg_sincos((y + 0.5f) * PPG_PI_F / h, &weight, &cosUnused);
            rowWeights[y] = weight;
            rowSum += colSum * weight;
            cdfRows[rowPos++] = rowSum;
        }
        normalizeCdf(cdfRows.data(), (size_t)h + 1);
        if (!(rowSum > 0) || !std::isfinite(rowSum)) return refuse("envmap: the environment map is completely black or holds nan / inf (envmap.cpp:308-312)");
        DevScene &E = H.scene;
        E.em_w = w; E.em_h = h; E.em_scale = em.scale;
        E.em_norm = 1.0f / (rowSum * (2 * PPG_PI_F / w) * (PPG_PI_F / h));
        E.em_px = 2 * PPG_PI_F / w; E.em_py = PPG_PI_F / h;
        memcpy(E.em_R, em.to_world, sizeof E.em_R);
    }
    return PPG_OK;
}

// luminaire sampling tables: TriMesh::prepareSamplingTable (trimesh.cpp:388-403) per emitter (= the triangles carrying its id, in index
// order) and Scene::configure's emitter pmf (scene.cpp:375-380, samplingWeight = 1); float running sums and
// DiscreteDistribution::normalize() (pmf.h:101-114) exactly as the oracle builds them.  Also the environment emitter's place among them.
int SceneBuilder::emitterTables() {
    const uint32_t ne = s->n_emitters;
    std::vector<std::vector<uint32_t>> emTris(ne);
    for (uint32_t t = 0; t < s->n_triangles; ++t) if (s->tri_emitter[t] >= 0) emTris[s->tri_emitter[t]].push_back(t);
    std::vector<float> &selCdf = H.emSel, &areaCdf = H.emArea;
    std::vector<int4> &info = H.emInfo;
    std::vector<float4> &etris = H.emTris, &enrm = H.emNormals;
    selCdf.assign(1, 0.0f);
    info.assign(std::max<uint32_t>(1, ne), int4{});
    for (uint32_t e = 0; e < ne; ++e) {
        const size_t first = areaCdf.size();
        areaCdf.push_back(0.0f);
        const int firstTri = (int)(etris.size() / 3);
        for (uint32_t t : emTris[e]) {
            const float *p0 = s->positions + 3 * s->indices[3 * t], *p1 = s->positions + 3 * s->indices[3 * t + 1], *p2 = s->positions + 3 * s->indices[3 * t + 2];
            const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
            const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
            const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
            areaCdf.push_back(areaCdf.back() + 0.5f * std::sqrt(cx * cx + cy * cy + cz * cz));  // Triangle::surfaceArea, triangle.cpp:61-67
            for (int v = 0; v < 3; ++v) {
                const float *p = s->positions + 3 * s->indices[3 * t + v];
                etris.push_back(make_float4(p[0], p[1], p[2], 0));
                if (s->normals) { const float *n = s->normals + 3 * s->indices[3 * t + v]; enrm.push_back(make_float4(n[0], n[1], n[2], 0)); }
            }
        }
        float area = 0, inv = -1;
        if (!emTris[e].empty()) {  // (an emitter of area 0 keeps its sums: DiscreteDistribution::normalize does nothing then)
            area = areaCdf.back();
            if (area > 0) normalizeCdf(&areaCdf[first], emTris[e].size() + 1);
            inv = 1.0f / area;
        }
        info[e] = make_int4(firstTri, (int)emTris[e].size(), (int)first, __builtin_bit_cast(int, inv));
        if (emitterSphere[e] >= 0) info[e].y = -(emitterSphere[e] + 1);  // sampled analytically (sphere_sample_direct)
        if (emitterShape[e] >= 0) {  // a disk or a cylinder: (-(shape + 1), 1, -, invSurfaceArea): sampled by shape_sample_direct; on the hit
                                     // side the count of 1 sends it down the generic invSurfaceArea * dist^2 / |dn| density
            const ppg_shape &sh = in.shapes[emitterShape[e]];
            float invArea;
            if (sh.type == PPG_SHAPE_DISK) {  // Disk::configure, disk.cpp:101-115
                const float *m = sh.to_world;
                const float len = std::sqrt(m[0] * m[0] + m[4] * m[4] + m[8] * m[8]);
                invArea = 1.0f / (PPG_PI_F * len * len);
            } else invArea = 1 / (2 * PPG_PI_F * sh.radius * sh.length);  // cylinder.cpp:106
            info[e] = make_int4(-(emitterShape[e] + 1), 1, (int)first, __builtin_bit_cast(int, invArea));
        }
        selCdf.push_back(selCdf.back() + 1.0f);
    }
    for (size_t k = 0; k < in.deltaEmitters.size(); ++k) selCdf.push_back(selCdf.back() + 1.0f);  // delta emitters follow the area emitters
    if (s->environment || s->envmap) selCdf.push_back(selCdf.back() + 1.0f);  // the environment emitter is the last one
    const float selNorm = selCdf.size() > 1 ? normalizeCdf(selCdf.data(), selCdf.size()) : 0.0f;  // (every emitter weighs 1: the sum is > 0)
    if (etris.empty()) etris.push_back(make_float4(0, 0, 0, 0));
    if (areaCdf.empty()) areaCdf.push_back(0.0f);
    DevScene &S = H.scene;
    if (s->environment || s->envmap) {
        if (s->environment) S.env = make_float4(s->environment[0], s->environment[1], s->environment[2], 1.0f);
        else S.env = make_float4(0, 0, 0, 2.0f);  // image based: DevScene::em_*
        S.bsphere = envBSphere(H.aabbMin, H.aabbMax);
        H.fullMaterials = true;  // the environment code lives in the FULL kernel variants
    } else {
        S.env = make_float4(0, 0, 0, 0); S.bsphere = make_float4(0, 0, 0, 0);
    }
    S.n_emitters = (int)ne; S.em_sel_norm = selNorm;
    return PPG_OK;
}

// ppg_set_delta_emitters: the point, spot and directional emitters
int SceneBuilder::deltaEmitters() {
    DevScene &S = H.scene;
    S.n_delta = (int)in.deltaEmitters.size(); S.dir_sphere = make_float4(0, 0, 0, 0);
    if (S.n_delta) {
        std::vector<float4> &tab = H.delta;
        tab.assign(PPG_DELTA_STRIDE * in.deltaEmitters.size(), float4{});
        for (size_t k = 0; k < in.deltaEmitters.size(); ++k) {
            const ppg_delta_emitter &e = in.deltaEmitters[k];
            const float *v = e.type == PPG_EMITTER_DIRECTIONAL ? e.direction : e.position;
            float4 *Q = &tab[PPG_DELTA_STRIDE * k];
            Q[0] = make_float4(e.intensity[0], e.intensity[1], e.intensity[2], __builtin_bit_cast(float, (int)e.type));
            Q[1] = make_float4(v[0], v[1], v[2], e.cutoff_angle);
            Q[2] = Q[3] = make_float4(0, 0, 0, 0);
            if (e.type == PPG_EMITTER_SPOT) {  // SpotEmitter::configure (spot.cpp:89-94)
                Q[2] = make_float4(e.to_local[6], e.to_local[7], e.to_local[8], 1.0f / (e.cutoff_angle - e.beam_width));
                Q[3] = make_float4(std::cos(e.cutoff_angle), std::cos(e.beam_width), 0, 0);
            }
        }
        {   // DirectionalEmitter::createShape (directional.cpp:88-94): AABB::getBSphere (aabb.h) of the kd-tree's box, radius * 1.1
            float c[3];
            for (int a = 0; a < 3; ++a) c[a] = (H.geomMax[a] + H.geomMin[a]) * 0.5f;
            const float dx = c[0] - H.geomMax[0], dy = c[1] - H.geomMax[1], dz = c[2] - H.geomMax[2];
            S.dir_sphere = make_float4(c[0], c[1], c[2], std::sqrt(dx * dx + dy * dy + dz * dz) * 1.1f);
        }
        H.fullMaterials = true;  // the delta-emitter code lives in the FULL kernel variants
    }
    return PPG_OK;
}

// ppg_set_shapes' disks and cylinders and the scene's spheres
int SceneBuilder::shapesAndSpheres() {
    DevScene &S = H.scene;
    S.n_shapes = (int)in.shapes.size(); S.n_spheres = (int)s->n_spheres;
    if (S.n_shapes) {
        std::vector<float4> &tab = H.shapes;
        tab.assign(PPG_SHAPE_STRIDE * in.shapes.size(), float4{});
        for (size_t k = 0; k < in.shapes.size(); ++k) {
            const ppg_shape &sh = in.shapes[k];
            float4 *Q = &tab[PPG_SHAPE_STRIDE * k];
            const float *m = sh.to_world, *iv = &shapeInv[12 * k];
            for (int r = 0; r < 3; ++r) {
                Q[r] = make_float4(m[4 * r], m[4 * r + 1], m[4 * r + 2], m[4 * r + 3]);
                Q[3 + r] = make_float4(iv[4 * r], iv[4 * r + 1], iv[4 * r + 2], iv[4 * r + 3]);
            }
            Q[6] = make_float4(sh.type == PPG_SHAPE_CYLINDER ? sh.radius : 1.0f, sh.type == PPG_SHAPE_CYLINDER ? sh.length : 0.0f, 0.0f, __builtin_bit_cast(float, (int)sh.type));
            Q[7] = make_float4(__builtin_bit_cast(float, (int)sh.material), __builtin_bit_cast(float, sh.emitter), __builtin_bit_cast(float, sh.flip_normals ? 1 : 0), 0.0f);
        }
        H.fullMaterials = true;  // the shape code lives in the FULL kernel variants, on the BVH path
    }
    if (s->n_spheres) {
        std::vector<float4> &sph = H.spheres;
        sph.assign(4 * (size_t)s->n_spheres, float4{});
        for (uint32_t k = 0; k < s->n_spheres; ++k) {
            const ppg_sphere &sp = s->spheres[k];
            sph[4 * k + 0] = make_float4(sp.center[0], sp.center[1], sp.center[2], sp.radius);
            sph[4 * k + 1] = make_float4(sp.to_world[0], sp.to_world[1], sp.to_world[2], __builtin_bit_cast(float, (int)sp.material));
            sph[4 * k + 2] = make_float4(sp.to_world[3], sp.to_world[4], sp.to_world[5], __builtin_bit_cast(float, sp.emitter));
            sph[4 * k + 3] = make_float4(sp.to_world[6], sp.to_world[7], sp.to_world[8], __builtin_bit_cast(float, sp.flip_normals ? 1 : 0));
        }
        H.fullMaterials = true;  // the sphere code lives in the FULL kernel variants, on the BVH path
    }
    return PPG_OK;
}

// ppg_set_media: homogeneous media and who lies in which.  Everything the device code relies on is checked here — every medium index of
// every binding word, every coefficient —, and what HomogeneousMedium's constructor derives is derived here: sigmaT = sigmaA + sigmaS
// (medium.cpp), the default mediumSamplingWeight (homogeneous.cpp:168-184) and `single`'s sampling density (:188-204).
int SceneBuilder::media() {
    DevScene &S = H.scene;
    const ppg_media *L = in.media;
    if (!L || L->n_media == 0) return PPG_OK;
    if (L->_reserved) return refuse("media: a reserved word is not 0");
    if (!L->media) return refuse("media: n_media > 0 but no array");
    if (L->n_media > 65535u) return refuse("media: " + std::to_string(L->n_media) + " media, at most 65535 are supported");
    if (L->tri_media && L->n_tri_media != s->n_triangles)
        return refuse("media: tri_media has " + std::to_string(L->n_tri_media) + " entries, the scene " + std::to_string(s->n_triangles) + " triangles");
    if (L->sphere_media && L->n_sphere_media != s->n_spheres)
        return refuse("media: sphere_media has " + std::to_string(L->n_sphere_media) + " entries, the scene " + std::to_string(s->n_spheres) + " spheres");
    if (L->shape_media && L->n_shape_media != in.shapes.size())
        return refuse("media: shape_media has " + std::to_string(L->n_shape_media) + " entries, the scene " + std::to_string(in.shapes.size()) + " shapes");
    std::vector<float4> tab(PPG_MEDIUM_STRIDE * (size_t)L->n_media);
    for (uint32_t k = 0; k < L->n_media; ++k) {
        const ppg_medium &m = L->media[k];
        const std::string who = "medium " + std::to_string(k) + ": ";
        for (int c = 0; c < 3; ++c) {
            if (!std::isfinite(m.sigma_a[c]) || !std::isfinite(m.sigma_s[c])) return refuse(who + "a coefficient is not finite");
            if (m.sigma_a[c] < 0 || m.sigma_s[c] < 0) return refuse(who + "a coefficient is negative");
        }
        for (int c = 0; c < 4; ++c) if (m._reserved[c]) return refuse(who + "a reserved word is not 0");
        if (m.strategy != PPG_MEDIUM_BALANCE && m.strategy != PPG_MEDIUM_SINGLE && m.strategy != PPG_MEDIUM_MANUAL) return refuse(who + "unknown sampling strategy");
        if (m.phase != PPG_PHASE_ISOTROPIC && m.phase != PPG_PHASE_HG) return refuse(who + "unknown phase function");
        if (m.phase == PPG_PHASE_HG && !(m.g > -1.0f && m.g < 1.0f)) return refuse(who + "hg: g must lie in (-1, 1)");
        if (!(m.sampling_weight == -1.0f || (m.sampling_weight >= 0.0f && m.sampling_weight <= 1.0f))) return refuse(who + "mediumSamplingWeight must lie in [0, 1] (or be -1: derive it)");
        if (m.strategy == PPG_MEDIUM_SINGLE && m.channel > 2) return refuse(who + "single: channel must be 0, 1 or 2 (or negative: the smallest sigmaT)");
        if (m.strategy == PPG_MEDIUM_MANUAL && !(std::isfinite(m.sampling_density) && m.sampling_density > 0)) return refuse(who + "manual: samplingDensity must be finite and > 0");
        float sigmaT[3];
        for (int c = 0; c < 3; ++c) {
            sigmaT[c] = m.sigma_a[c] + m.sigma_s[c];
            if (!std::isfinite(sigmaT[c])) return refuse(who + "a coefficient is not finite");
        }
        float weight = m.sampling_weight;
        if (weight == -1.0f) {  // the highest albedo over the channels that extinguish at all; at least one half if the medium scatters
            for (int c = 0; c < 3; ++c) {
                const float albedo = m.sigma_s[c] / sigmaT[c];
                if (albedo > weight && sigmaT[c] != 0) weight = albedo;
            }
            if (weight > 0) weight = ppg_max(weight, 0.5f);
            // (a medium without extinction keeps -1 in the reference and never samples a distance; 0 says the same)
            if (weight < 0) weight = 0.0f;
        }
        float density = 0.0f;
        if (m.strategy == PPG_MEDIUM_SINGLE) {
            int channel = 0;
            float smallest = INFINITY;
            for (int c = 0; c < 3; ++c) if (sigmaT[c] < smallest) { smallest = sigmaT[c]; channel = c; }
            if (m.channel >= 0) channel = m.channel;
            density = sigmaT[channel];
        } else if (m.strategy == PPG_MEDIUM_MANUAL) {
            density = m.sampling_density;
        }
        float4 *Q = &tab[PPG_MEDIUM_STRIDE * (size_t)k];
        Q[0] = make_float4(m.sigma_s[0], m.sigma_s[1], m.sigma_s[2], weight);
        Q[1] = make_float4(sigmaT[0], sigmaT[1], sigmaT[2], density);
        Q[2] = make_float4(m.phase == PPG_PHASE_HG ? m.g : 0.0f, __builtin_bit_cast(float, (int)m.strategy), __builtin_bit_cast(float, (int)m.phase), 0.0f);
    }
    auto checkWord = [&](uint32_t w, const std::string &who) {
        if ((w & 0xffffu) > L->n_media || (w >> 16) > L->n_media) return refuse("media: " + who + ": medium index out of range");
        return (int)PPG_OK;
    };
    if (L->camera_medium > L->n_media) return refuse("media: camera_medium: medium index out of range");
    bool bound = L->camera_medium != 0;
    const size_t nPrims = (size_t)s->n_triangles + s->n_spheres + in.shapes.size();
    std::vector<unsigned int> words(nPrims, 0u);
    if (L->tri_media)
        for (uint32_t k = 0; k < s->n_triangles; ++k) {  // leaf order, as the kernels number the triangles
            const uint32_t t = bb.order[k], w = L->tri_media[t];
            if (int rc = checkWord(w, "triangle " + std::to_string(t))) return rc;
            words[k] = w; bound = bound || w != 0;
        }
    if (L->sphere_media)
        for (uint32_t k = 0; k < s->n_spheres; ++k) {
            if (int rc = checkWord(L->sphere_media[k], "sphere " + std::to_string(k))) return rc;
            words[s->n_triangles + k] = L->sphere_media[k]; bound = bound || L->sphere_media[k] != 0;
        }
    if (L->shape_media)
        for (size_t k = 0; k < in.shapes.size(); ++k) {
            if (int rc = checkWord(L->shape_media[k], "shape " + std::to_string(k))) return rc;
            words[(size_t)s->n_triangles + s->n_spheres + k] = L->shape_media[k]; bound = bound || L->shape_media[k] != 0;
        }
    if (!bound) return PPG_OK;  // a list that binds nothing renders as no list does
    H.media = std::move(tab); H.primMedia = std::move(words);
    H.cameraMedium = L->camera_medium;
    S.has_null = 1;             // shadow segments and the search for emitters walk their pieces (transmittance per piece) as behind null surfaces
    H.fullMaterials = true;     // the media code lives in the FULL kernel variants
    return PPG_OK;
}

// ppg_set_media_volumes: heterogeneous media (medium/heterogeneous.cpp, Woodcock tracking) over const and grid volumes.  Everything the
// tracking loops rely on is checked here — every index, every texel of a density grid against [0, 1], the expected length of a loop —, and
// what the reference's configure() calls derive is derived here: worldToGrid and the world box (gridvolume.cpp:188-201), maxDensity and
// its inverse (heterogeneous.cpp:239-242).
int SceneBuilder::mediaVolumes() {
    const ppg_media_volumes *L = in.mediaVolumes;
    if (!L || L->n_entries == 0) return PPG_OK;
    const std::string list = "media volumes: ";
    for (int c = 0; c < 4; ++c) if (L->_reserved[c]) return refuse(list + "a reserved word is not 0");
    if (!L->entries || (L->n_volumes && !L->volumes)) return refuse(list + "a count > 0 but no array");
    const ppg_media *M = in.media;
    if (!M || M->n_media == 0) return refuse(list + "no media list (ppg_set_media) to name a medium of");
    struct Derived { float w2g[12]; float mn[3], mx[3]; float diag; size_t offset; };
    std::vector<Derived> derived(L->n_volumes);
    std::vector<float4> vtab(PPG_VOLUME_STRIDE * (size_t)L->n_volumes);
    std::vector<float> pool;
    for (uint32_t k = 0; k < L->n_volumes; ++k) {
        const ppg_volume &v = L->volumes[k];
        const std::string who = list + "volume " + std::to_string(k) + ": ";
        Derived &G = derived[k];
        memset(&G, 0, sizeof G);
        if (v._reserved[0] || v._reserved[1]) return refuse(who + "a reserved word is not 0");
        if (v.kind != PPG_VOLUME_CONST && v.kind != PPG_VOLUME_GRID) return refuse(who + "unknown kind");
        if (v.channels != 1 && v.channels != 3) return refuse(who + "channels must be 1 or 3");
        float4 *Q = &vtab[PPG_VOLUME_STRIDE * (size_t)k];
        for (int i = 0; i < PPG_VOLUME_STRIDE; ++i) Q[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        Q[0].x = __builtin_bit_cast(float, (int)(v.kind | (v.channels << 8)));
        if (v.kind == PPG_VOLUME_CONST) {
            for (int c = 0; c < v.channels; ++c) if (!std::isfinite(v.value[c])) return refuse(who + "a value is not finite");
            Q[4] = v.channels == 1 ? make_float4(v.value[0], v.value[0], v.value[0], 0.0f) : make_float4(v.value[0], v.value[1], v.value[2], 0.0f);
            continue;
        }
        for (int a = 0; a < 3; ++a) if (v.res[a] < 2) return refuse(who + "a res component is below 2");
        if ((double)v.res[0] * v.res[1] * v.res[2] * v.channels > 536870912.0) return refuse(who + "more than 2^29 floats");
        if (!v.data) return refuse(who + "a grid without data");
        double ext[3];
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(v.aabb_min[a]) || !std::isfinite(v.aabb_max[a])) return refuse(who + "the data box is not finite");
            ext[a] = (double)v.aabb_max[a] - (double)v.aabb_min[a];
            if (!(ext[a] > 0)) return refuse(who + "the data box is empty");
        }
        const float *m = v.to_world;
        for (int i = 0; i < 16; ++i) if (!std::isfinite(m[i])) return refuse(who + "to_world is not finite");
        if (m[12] != 0 || m[13] != 0 || m[14] != 0 || m[15] != 1) return refuse(who + "to_world is not affine (its last row must be 0 0 0 1)");
        double c[3][3], len[3];
        for (int j = 0; j < 3; ++j) {
            for (int a = 0; a < 3; ++a) c[j][a] = m[4 * a + j];
            len[j] = std::sqrt(c[j][0] * c[j][0] + c[j][1] * c[j][1] + c[j][2] * c[j][2]);
        }
        const double det = c[0][0] * (c[1][1] * c[2][2] - c[1][2] * c[2][1]) - c[0][1] * (c[1][0] * c[2][2] - c[1][2] * c[2][0]) +
                           c[0][2] * (c[1][0] * c[2][1] - c[1][1] * c[2][0]);
        if (len[0] == 0 || len[1] == 0 || len[2] == 0 || !(std::abs(det) > 1e-9 * len[0] * len[1] * len[2])) return refuse(who + "to_world is singular");
        // worldToGrid = scale((res - 1) / extents) * translate(-min) * to_world^-1; row i of L^-1 = cross products of L's columns / det
        for (int i = 0; i < 3; ++i) {
            const double *a = c[(i + 1) % 3], *b = c[(i + 2) % 3];
            const double li[3] = {(a[1] * b[2] - a[2] * b[1]) / det, (a[2] * b[0] - a[0] * b[2]) / det, (a[0] * b[1] - a[1] * b[0]) / det};
            const double tr = -(li[0] * (double)m[3] + li[1] * (double)m[7] + li[2] * (double)m[11]);
            const double sc = (v.res[i] - 1) / ext[i];
            for (int j = 0; j < 3; ++j) G.w2g[4 * i + j] = (float)(sc * li[j]);
            G.w2g[4 * i + 3] = (float)(sc * (tr - (double)v.aabb_min[i]));
        }
        for (int a = 0; a < 3; ++a) { G.mn[a] = INFINITY; G.mx[a] = -INFINITY; }
        for (int corner = 0; corner < 8; ++corner) {  // m_aabb.expandBy(m_volumeToWorld(m_dataAABB.getCorner(i)))
            const float p[3] = {(corner & 1) ? v.aabb_max[0] : v.aabb_min[0], (corner & 2) ? v.aabb_max[1] : v.aabb_min[1], (corner & 4) ? v.aabb_max[2] : v.aabb_min[2]};
            for (int a = 0; a < 3; ++a) {
                const float w = m[4 * a] * p[0] + m[4 * a + 1] * p[1] + m[4 * a + 2] * p[2] + m[4 * a + 3];
                G.mn[a] = std::min(G.mn[a], w); G.mx[a] = std::max(G.mx[a], w);
            }
        }
        const double dx = (double)G.mx[0] - G.mn[0], dy = (double)G.mx[1] - G.mn[1], dz = (double)G.mx[2] - G.mn[2];
        G.diag = (float)std::sqrt(dx * dx + dy * dy + dz * dz);
        if (!std::isfinite(G.diag)) return refuse(who + "the world box is not finite");
        const size_t count = (size_t)v.res[0] * v.res[1] * v.res[2] * v.channels;
        for (size_t i = 0; i < count; ++i)
            if (!(v.data[i] >= 0.0f && v.data[i] <= 1.0f)) return refuse(who + "texel " + std::to_string(i) + " lies outside [0, 1] or is not finite");
        G.offset = pool.size();
        if (G.offset + count > 1073741824u) return refuse(who + "the grids hold more than 2^30 floats");
        pool.insert(pool.end(), v.data, v.data + count);
        Q[0].y = __builtin_bit_cast(float, (int)v.res[0]); Q[0].z = __builtin_bit_cast(float, (int)v.res[1]); Q[0].w = __builtin_bit_cast(float, (int)v.res[2]);
        for (int i = 0; i < 3; ++i) Q[1 + i] = make_float4(G.w2g[4 * i], G.w2g[4 * i + 1], G.w2g[4 * i + 2], G.w2g[4 * i + 3]);
        Q[4] = make_float4(0.0f, 0.0f, 0.0f, __builtin_bit_cast(float, (int)G.offset));
    }
    std::vector<float4> htab(PPG_HET_STRIDE * (size_t)M->n_media, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    std::vector<char> named(M->n_media, 0);
    for (uint32_t k = 0; k < L->n_entries; ++k) {
        const ppg_medium_volumes &e = L->entries[k];
        const std::string who = list + "entry " + std::to_string(k) + ": ";
        for (int c = 0; c < 4; ++c) if (e._reserved[c]) return refuse(who + "a reserved word is not 0");
        if (e.medium >= M->n_media) return refuse(who + "medium index out of range");
        if (e.density >= L->n_volumes || e.albedo >= L->n_volumes) return refuse(who + "volume index out of range");
        if (named[e.medium]) return refuse(who + "medium " + std::to_string(e.medium) + " is named twice");
        named[e.medium] = 1;
        const ppg_volume &dv = L->volumes[e.density], &av = L->volumes[e.albedo];
        if (dv.channels != 1) return refuse(who + "the density volume must have 1 channel");
        if (av.channels != 3) return refuse(who + "the albedo volume must have 3 channels");
        if (!(std::isfinite(e.scale) && e.scale > 0)) return refuse(who + "scale must be finite and > 0");
        if (dv.kind == PPG_VOLUME_CONST && !(std::isfinite(dv.value[0]) && dv.value[0] > 0)) return refuse(who + "a const density must be finite and > 0");
        if (av.kind == PPG_VOLUME_CONST)
            for (int c = 0; c < 3; ++c) if (!(av.value[c] >= 0.0f && av.value[c] <= 1.0f)) return refuse(who + "the albedo lies outside [0, 1] or is not finite");
        const ppg_medium &md = M->media[e.medium];
        bool plain = md.strategy == 0 && md.sampling_density == 0.0f && (md.sampling_weight == 0.0f || md.sampling_weight == -1.0f) && (md.channel == 0 || md.channel == -1);
        for (int c = 0; c < 3; ++c) plain = plain && md.sigma_a[c] == 0.0f && md.sigma_s[c] == 0.0f;
        if (!plain) return refuse(who + "medium " + std::to_string(e.medium) + " states coefficients or a sampling strategy: a heterogeneous medium takes its density and albedo from volumes");
        // m_maxDensity = m_scale * m_density->getMaximumFloatValue(): 1 for a grid, the value for a const volume
        const float maxDensity = e.scale * (dv.kind == PPG_VOLUME_GRID ? 1.0f : dv.value[0]);
        const float invMaxDensity = 1.0f / maxDensity;
        if (!(std::isfinite(maxDensity) && maxDensity > 0 && std::isfinite(invMaxDensity) && invMaxDensity > 0)) return refuse(who + "scale times the maximum density is not finite and positive");
        if (dv.kind == PPG_VOLUME_GRID && !((double)maxDensity * derived[e.density].diag <= (double)PPG_HETMEDIUM_MAX_MEAN_STEPS))
            return refuse(who + "the grid is too long to track: scale times the diagonal of its world box is " + std::to_string((double)maxDensity * derived[e.density].diag) +
                          " majorant free paths, at most " + std::to_string((int)PPG_HETMEDIUM_MAX_MEAN_STEPS) + " are supported");
        float4 *Hr = &htab[PPG_HET_STRIDE * (size_t)e.medium];
        Hr[0] = make_float4(__builtin_bit_cast(float, (int)(e.density + 1u)), __builtin_bit_cast(float, (int)e.albedo), e.scale, invMaxDensity);
        if (dv.kind == PPG_VOLUME_GRID) {
            const Derived &G = derived[e.density];
            Hr[1] = make_float4(G.mn[0], G.mn[1], G.mn[2], maxDensity); Hr[2] = make_float4(G.mx[0], G.mx[1], G.mx[2], 0.0f);
        } else {  // AABB's default: invalid
            Hr[1] = make_float4(INFINITY, INFINITY, INFINITY, maxDensity); Hr[2] = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.0f);
        }
    }
    // which media are bound: the hetmedia kernels are needed when one of them is heterogeneous
    bool bound = false;
    auto side = [&](unsigned int med) { if (med && named[med - 1]) bound = true; };
    side(H.cameraMedium);
    for (unsigned int w : H.primMedia) { side(w & 0xffffu); side(w >> 16); }
    if (!bound) return PPG_OK;  // (nothing of the list is reachable: the scene renders as without it)
    if (pool.empty()) pool.push_back(0.0f);
    H.volumes = std::move(vtab); H.volPool = std::move(pool); H.het = std::move(htab);
    return PPG_OK;
}

// the sensor, the film size and how much of the scene k_trace caches in LDS
int SceneBuilder::cameraAndLds() {
    DevScene &S = H.scene;
    memcpy(S.cam.s2c, s->camera.sample_to_camera, 64); memcpy(S.cam.c2w, s->camera.camera_to_world, 64);
    S.cam.near_clip = s->camera.near_clip; S.cam.far_clip = s->camera.far_clip;
    S.cam.width = s->camera.width; S.cam.height = s->camera.height;
    S.cam.inv_w = 1.0f / (float)s->camera.width; S.cam.inv_h = 1.0f / (float)s->camera.height;
    S.cam.lens = in.lens ? 1 : 0; S.cam.aperture = in.lens ? in.lens->aperture_radius : 0.0f; S.cam.focus = in.lens ? in.lens->focus_distance : 0.0f;
    H.W = s->camera.width; H.H = s->camera.height;
    {   // LDS budget of k_trace: 32 KB keeps 5 workgroups per CU resident
        const size_t budget = 32 * 1024;
        H.ldsNodes = (int)std::min<size_t>(H.nodes.size(), budget / 64);
        size_t left = budget - (size_t)H.ldsNodes * 64;
        H.ldsTris = ((size_t)s->n_triangles * 48 <= left) ? (int)s->n_triangles : 0;
    }
    return PPG_OK;
}

// Validate the scene and build every host table of it.  PPG_OK, or PPG_ERR_INVALID with `err` saying why; H is complete only after PPG_OK.
static int buildScene(const SceneInputs &in, HostScene &H, std::string &err) {
    if (!sceneComplete(in)) { err = "incomplete scene"; return PPG_ERR_INVALID; }
    H = HostScene{};
    SceneBuilder b{in, H, err, in.s, {}, {}, {}, {}};
    for (auto stage : {&SceneBuilder::primitives, &SceneBuilder::geometry, &SceneBuilder::materials, &SceneBuilder::microfacet, &SceneBuilder::coatings,
                       &SceneBuilder::blends, &SceneBuilder::textures, &SceneBuilder::envmap, &SceneBuilder::emitterTables, &SceneBuilder::deltaEmitters,
                       &SceneBuilder::shapesAndSpheres, &SceneBuilder::media, &SceneBuilder::mediaVolumes, &SceneBuilder::cameraAndLds})
        if (int rc = (b.*stage)()) return rc;
    return PPG_OK;
}

}  // namespace
