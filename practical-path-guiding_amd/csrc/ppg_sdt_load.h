// ppg_sdt_load.h — the import of a dumped SD-tree (ppg_load_sdtree, include/ppg.h "Loading a dumped SD-tree"): the bytes of an .sdt file,
// the context's cubified tree box and the spatial filter in; a host description of the whole sampling SD-tree, or a refusal that names the
// file offset and the leaf, out.  No device, no context: every index a kernel will follow is checked here, before a byte is uploaded, and
// tests/sdt_load_check.cpp checks this header on the host alone, case by case.  The rules are in DESIGN.md §3 ("Loading a dumped SD-tree").
//
// The file (dumpSDTreeFile of ppg_hip.hip = GP:1191-1208 + DTreeWrapper::dump GP:699-711; read by visualizer/src/main.cpp:142-176):
//   float[16]  camera matrix (ignored: the tree lives in world space)
//   per leaf of statistical weight > 0, depth first, child 0 before child 1:
//     float p[3], size[3], mean;  uint64 statisticalWeight, numNodes;  numNodes x 4 x { float sum; uint16 child }
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace ppg_sdt {

// values of include/ppg.h, include/ppg_testhooks.h, include/ppg_detmath.h and ppg_kernels.h this header needs (ppg_hip.hip asserts that they agree)
constexpr int kOk = 0, kErrInvalid = -1, kErrNoMem = -5;  // PPG_OK, PPG_ERR_INVALID, PPG_ERR_NOMEM
constexpr int kSpatialFilterBox = 2;                      // SF_BOX
constexpr uint32_t kStreeMaxDepth = 94;                   // PPG_STREE_MAX_DEPTH
constexpr float kPi = 3.14159265358979323846f;            // PPG_PI_F
constexpr int kDTreeMaxDepth = 20;                        // the newMaxDepth of every DTree::reset (GP:1111); the root is at depth 1
constexpr uint64_t kDTreeMaxNodes = 65536;                // children are uint16
constexpr size_t kHeaderBytes = 64, kLeafBytes = 7 * 4 + 2 * 8, kNodeBytes = 4 * (4 + 2);

// The depth of an S-tree (children[2 i], children[2 i + 1]; 0, 0 = a leaf; a child's index is above its parent's: one forward pass) —
// levels below the root of its deepest leaf — and whether the box spatial filter's splat can walk it (include/ppg_testhooks.h
// PPG_STREE_MAX_DEPTH).  kErrInvalid: a child index that is not above its parent's or beyond the array.
inline int streeDepthCheck(const uint32_t *children, uint32_t n_nodes, int32_t spatial_filter, uint32_t *depth) {
    std::vector<uint32_t> d(n_nodes, 0u);
    uint32_t deepest = 0;
    for (uint32_t i = 0; i < n_nodes; ++i) {
        if (children[2 * (size_t)i] == 0) { deepest = d[i] > deepest ? d[i] : deepest; continue; }
        for (int c = 0; c < 2; ++c) {
            const uint32_t k = children[2 * (size_t)i + c];
            if (k <= i || k >= n_nodes) return kErrInvalid;
            d[k] = d[i] + 1u;
        }
    }
    *depth = deepest;
    return (spatial_filter == kSpatialFilterBox && deepest > kStreeMaxDepth) ? kErrNoMem : kOk;
}

struct Limits {
    uint64_t maxStreeNodes = (1ull << 27) - 1;  // uploadTree / refineDevice: "S-tree exceeds 2^27 nodes"
    uint64_t maxSamplingNodes = 0xfffffff0ull;  // node indices of the pools are 32 bits
};

struct Node {  // one quadtree node, as the file holds it
    float sum[4];
    uint16_t child[4];
};

struct Leaf {  // per S-tree node; all zero for an interior node
    uint32_t base = 0, num = 0;  // the D-tree's block in Tree::nodes
    float sum = 0, statw = 0;    // DTree::m_atomic of the sampling tree
    int32_t depth = 0;           // m_maxDepth
    int64_t fileLeaf = -1;       // index of the leaf in the file; -1: a hole (or an interior node)
};

struct Tree {
    std::vector<int32_t> axis;            // per S-tree node, numbered in preorder (child 0's subtree before child 1's)
    std::vector<uint32_t> children;       // [2 i], [2 i + 1]; 0, 0 = a leaf
    std::vector<Leaf> hdr;                // per S-tree node
    std::vector<Node> nodes;              // the sampling pool: the leaves' D-trees in preorder
    std::vector<uint32_t> dfsRightFirst;  // the leaves in the order STree::refine visits them (child 1 before child 0)
    uint32_t depth = 0;                   // levels below the root of the deepest leaf
    uint64_t fileLeaves = 0, holes = 0;
    uint64_t reservedNodes = 0;           // quadtree nodes memory was asked for (0 while only sizes have been checked)
    void clear() { *this = Tree(); }
};

namespace detail {

struct FileLeaf {
    size_t offset;  // of the leaf's record in the file
    float p[3], s[3], mean;
    uint64_t weight, numNodes;
};
struct Box { float p[3], s[3]; };

template <typename T> inline T rd(const uint8_t *b, size_t off) { T v; std::memcpy(&v, b + off, sizeof(T)); return v; }
inline bool equalBox(const FileLeaf &l, const Box &r) {
    for (int a = 0; a < 3; ++a) if (l.p[a] != r.p[a] || l.s[a] != r.s[a]) return false;
    return true;
}
// Can l be a region below r?  Its size is r's halved some times along every axis — halving is exact, so sizes compare exactly — and at
// least once along one; its centre lies in r.  The corners are NOT compared: a child's p is a rounded float sum (p[axis] += size[axis]), so
// a descendant's far corner may lie an ulp outside its ancestor's.  Whether l IS a region is then decided by exact equality further down.
inline bool within(const Box &r, const FileLeaf &l) {
    bool smaller = false;
    for (int a = 0; a < 3; ++a) {
        if (l.s[a] > r.s[a]) return false;
        if (l.s[a] < r.s[a]) smaller = true;
        const double c = (double)l.p[a] + 0.5 * (double)l.s[a];
        if (!(c > (double)r.p[a] && c < (double)r.p[a] + (double)r.s[a])) return false;
    }
    return smaller;
}
// the dump's own float arithmetic (dumpSDTreeFile; STreeNode::forEachLeaf GP:796-813)
inline void split(const Box &r, int axis, Box &c0, Box &c1) {
    c0 = r; c1 = r;
    c0.s[axis] /= 2; c1.s[axis] = c0.s[axis];
    c1.p[axis] += c1.s[axis];
}
inline std::string where(uint64_t leaf, size_t offset) { return "leaf " + std::to_string(leaf) + " at offset " + std::to_string(offset) + ": "; }
// is the box one of the regions the tree box can be split into?
inline bool isRegion(const FileLeaf &l, Box r) {
    for (int axis = 0, level = 0; level < 4096; ++level, axis = (axis + 1) % 3) {
        if (equalBox(l, r)) return true;
        if (!within(r, l)) return false;
        Box c0, c1;
        split(r, axis, c0, c1);
        r = (double)l.p[axis] + 0.5 * (double)l.s[axis] < (double)c1.p[axis] ? c0 : c1;
    }
    return false;
}

}  // namespace detail

// The sampling SD-tree of the file `bytes[0 .. size)` for a context whose tree box is [treeMin, treeMax].  kOk and `out`, or a refusal —
// kErrInvalid for a file that is malformed or belongs to another box, kErrNoMem for one that exceeds a limit — with `error` set and `out` empty.
inline int importTree(const uint8_t *bytes, size_t size, const float treeMin[3], const float treeMax[3], int32_t spatialFilter, const Limits &lim,
                      Tree &out, std::string &error) {
    using namespace detail;
    out.clear();
    auto refuse = [&](int code, const std::string &msg) { const uint64_t r = out.reservedNodes; out.clear(); out.reservedNodes = r; error = msg; return code; };
    if (!bytes || size < kHeaderBytes) return refuse(kErrInvalid, "truncated file: " + std::to_string(size) + " bytes, the camera matrix alone takes 64");

    // 1. the leaf records: sizes first — nothing is allocated for a node count the file cannot hold
    std::vector<FileLeaf> leaves;
    uint64_t fileNodes = 0;
    for (size_t off = kHeaderBytes; off < size;) {
        const uint64_t k = leaves.size();
        if (size - off < kLeafBytes) return refuse(kErrInvalid, where(k, off) + "truncated file: " + std::to_string(size - off) + " trailing bytes do not form a leaf");
        FileLeaf l;
        l.offset = off;
        for (int a = 0; a < 3; ++a) { l.p[a] = rd<float>(bytes, off + 4 * a); l.s[a] = rd<float>(bytes, off + 12 + 4 * a); }
        l.mean = rd<float>(bytes, off + 24);
        l.weight = rd<uint64_t>(bytes, off + 28);
        l.numNodes = rd<uint64_t>(bytes, off + 36);
        off += kLeafBytes;
        if (l.numNodes == 0) return refuse(kErrInvalid, where(k, l.offset) + "numNodes is 0");
        if (l.numNodes > (size - off) / kNodeBytes)
            return refuse(kErrInvalid, where(k, l.offset) + "truncated file: numNodes " + std::to_string(l.numNodes) + " needs more than the " + std::to_string(size - off) + " bytes that remain");
        if (l.numNodes > kDTreeMaxNodes) return refuse(kErrInvalid, where(k, l.offset) + "numNodes " + std::to_string(l.numNodes) + " exceeds 65536 (children are 16 bits)");
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(l.p[a]) || !std::isfinite(l.s[a]) || !(l.s[a] > 0)) return refuse(kErrInvalid, where(k, l.offset) + "the box is not finite with a positive size");
        if (!std::isfinite(l.mean)) return refuse(kErrInvalid, where(k, l.offset) + "mean is not finite");
        off += (size_t)l.numNodes * kNodeBytes;
        fileNodes += l.numNodes;
        leaves.push_back(l);
    }

    // 2. the S-tree from the leaf boxes: at each region the next leaf of the file IS the region, lies inside it (split), or the region is a
    //    hole — the leaves of weight 0 that the dump skips.  Nodes are numbered in preorder: a child's index is above its parent's.
    struct Frame { Box box; int axis; uint32_t parent; int which; };
    const uint32_t kNone = 0xffffffffu;
    std::vector<Frame> stack;
    Frame root;
    for (int a = 0; a < 3; ++a) { root.box.p[a] = treeMin[a]; root.box.s[a] = treeMax[a] - treeMin[a]; }
    root.axis = 0; root.parent = kNone; root.which = 0;
    stack.push_back(root);
    size_t next = 0;
    while (!stack.empty()) {
        const Frame f = stack.back();
        stack.pop_back();
        const uint64_t idx = out.axis.size();
        if (idx >= lim.maxStreeNodes) return refuse(kErrNoMem, "the S-tree exceeds " + std::to_string(lim.maxStreeNodes) + " nodes");
        out.axis.push_back(f.axis);
        out.children.push_back(0u); out.children.push_back(0u);
        out.hdr.push_back(Leaf());
        if (f.parent != kNone) out.children[2 * (size_t)f.parent + f.which] = (uint32_t)idx;
        if (next < leaves.size()) {
            const FileLeaf &l = leaves[next];
            if (equalBox(l, f.box)) { out.hdr[idx].fileLeaf = (int64_t)next++; out.hdr[idx].num = (uint32_t)l.numNodes; continue; }
            if (within(f.box, l)) {
                Frame c0, c1;
                split(f.box, f.axis, c0.box, c1.box);
                c0.axis = c1.axis = (f.axis + 1) % 3;
                c0.parent = c1.parent = (uint32_t)idx;
                c0.which = 0; c1.which = 1;
                stack.push_back(c1); stack.push_back(c0);
                continue;
            }
        }
        out.hdr[idx].num = 1;  // a hole: one leaf with an empty D-tree
        ++out.holes;
    }
    if (next < leaves.size()) {
        const FileLeaf &l = leaves[next];
        if (!isRegion(l, root.box)) return refuse(kErrInvalid, where(next, l.offset) + "the box is not a region of this context's SD-tree box: the tree was trained on another scene");
        return refuse(kErrInvalid, where(next, l.offset) + "out of depth-first order, or overlapping an earlier leaf");
    }
    out.fileLeaves = leaves.size();
    const uint32_t nS = (uint32_t)out.axis.size();
    {
        const int rc = streeDepthCheck(out.children.data(), nS, spatialFilter, &out.depth);
        if (rc == kErrInvalid) return refuse(kErrInvalid, "internal: an S-tree child that is not above its parent");
        if (rc) return refuse(rc, "S-tree deeper than " + std::to_string(kStreeMaxDepth) + " levels (" + std::to_string(out.depth) + ") with the box spatial filter");
    }
    if (fileNodes + out.holes > lim.maxSamplingNodes) return refuse(kErrNoMem, "the sampling D-trees exceed " + std::to_string(lim.maxSamplingNodes) + " nodes in total");

    // 3. the D-trees, in preorder of their leaves; every child index is checked before anything may follow it
    out.reservedNodes = fileNodes + out.holes;
    out.nodes.reserve((size_t)out.reservedNodes);
    std::vector<uint8_t> level;
    for (uint32_t i = 0; i < nS; ++i) {
        if (out.children[2 * (size_t)i] != 0) continue;
        Leaf &h = out.hdr[i];
        h.base = (uint32_t)out.nodes.size();
        if (h.fileLeaf < 0) {
            out.nodes.push_back(Node{{0, 0, 0, 0}, {0, 0, 0, 0}});
            h.num = 1; h.depth = 1;
            continue;
        }
        const FileLeaf &l = leaves[(size_t)h.fileLeaf];
        const uint32_t n = (uint32_t)l.numNodes;
        // (messages are put together only when something is refused: this loop sees every node of the file)
        auto at = [&] { return where((uint64_t)h.fileLeaf, l.offset); };
        auto slot = [&](uint32_t k, int j, size_t off) {
            return at() + "node " + std::to_string(k) + " slot " + std::to_string(j) + " (offset " + std::to_string(off + 6 * (size_t)j) + "): ";
        };
        level.assign(n, 0);
        level[0] = 1;
        int deepest = 1;
        for (uint32_t k = 0; k < n; ++k) {
            const size_t off = l.offset + kLeafBytes + (size_t)k * kNodeBytes;
            if (level[k] == 0) return refuse(kErrInvalid, at() + "node " + std::to_string(k) + " is referenced by no node");
            Node nd;
            for (int j = 0; j < 4; ++j) {
                nd.sum[j] = rd<float>(bytes, off + 6 * (size_t)j);
                nd.child[j] = rd<uint16_t>(bytes, off + 6 * (size_t)j + 4);
                if (!std::isfinite(nd.sum[j]) || nd.sum[j] < 0) return refuse(kErrInvalid, slot(k, j, off) + "the sum is negative or not finite");
                const uint32_t c = nd.child[j];
                if (c == 0) continue;
                if (c >= n) return refuse(kErrInvalid, slot(k, j, off) + "child " + std::to_string(c) + " is beyond the " + std::to_string(n) + " nodes");
                if (c <= k) return refuse(kErrInvalid, slot(k, j, off) + "child " + std::to_string(c) + " is not above its parent");
                if (level[c] != 0) return refuse(kErrInvalid, slot(k, j, off) + "child " + std::to_string(c) + " is referenced twice");
                if (level[k] + 1 > kDTreeMaxDepth) return refuse(kErrInvalid, slot(k, j, off) + "the D-tree is deeper than " + std::to_string(kDTreeMaxDepth) + " levels");
                level[c] = (uint8_t)(level[k] + 1);
                deepest = level[c] > deepest ? level[c] : deepest;
            }
            out.nodes.push_back(nd);
        }
        h.num = n; h.depth = deepest;
        h.statw = (float)l.weight;
        h.sum = l.mean * (kPi * 4 * h.statw);  // the inverse of the dump's mean = 1 / (pi * 4 * statw) * sum
        if (!std::isfinite(h.sum)) return refuse(kErrInvalid, at() + "mean times 4 pi times the weight is not finite");
    }

    // 4. the leaves as STree::refine's stack visits them (GP:957-998: child 0 pushed first, child 1 popped first)
    {
        std::vector<uint32_t> st(1, 0u);
        while (!st.empty()) {
            const uint32_t i = st.back();
            st.pop_back();
            if (out.children[2 * (size_t)i] == 0) { out.dfsRightFirst.push_back(i); continue; }
            st.push_back(out.children[2 * (size_t)i]); st.push_back(out.children[2 * (size_t)i + 1]);
        }
    }
    return kOk;
}

}  // namespace ppg_sdt
