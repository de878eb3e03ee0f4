"""An exact restatement of the commit of path vertices into the SD-tree, for tests/test_commit.py and tests/test_commit_gpu.py (not a test module).

Plain Python over the arrays Engine.read_sdtree() returns; no code shared with the product or the oracle.  Every float expression of
Vertex::commit (GP:1730-1768), DTreeWrapper::record (GP:575-584), DTree::recordIrradiance (GP:395-413), QuadTreeNode::record (GP:303-338),
STreeNode::record (GP:823-839) and STree::record (GP:935-943) is one np.float32 operation at a time, in the reference's order; every sum is a
Python int per (leaf, node, slot) and per leaf weight.  dir_to_canonical is handed in (the oracle's ppgo_dir_to_canonical, pinned by
tests/test_oracle_reference_pins.py); ppg_rand is written from the sampler contract (include/ppg_rng.h, pinned by tests/test_detmath.py).

Beside every float32 value that ends in a sum the same expression is carried in float64 ("irr64", "w64"): the conservation identities of
tests/test_commit.py are checked on those.

splat_routes() derives, from the sorted keys of a round and the leaves' node counts, which way k_splat_sorted (csrc/ppg_kernels.h) takes
every chunk and run, and wave_arms() which arms of wave_key_add the record-by-record chunks reach: the tests assert with them that their
inputs reach the branch they were written for.
"""
import math

import numpy as np

f32 = np.float32
EPSILON = f32(1e-4)            # PPG_EPSILON (mitsuba Epsilon, single precision)
THIRD = f32(1.0) / f32(3.0)    # Spectrum::average multiplies by (1.0f / 3)
LEAF_SHIFT, CODE_BITS, CODE_VERTEX = 40, 13, 4096   # include/ppg.h: key = leaf << 40 | path << 13 | code
CHUNK, BLOCK, MAX_RUNS, RUN_FACTOR, LDS_NODES = 2048, 256, 64, 4, 512  # k_splat_sorted (csrc/ppg_kernels.h)
M32 = 0xffffffff


def _hash32(x):
    x &= M32
    x ^= x >> 16; x = (x * 0x7feb352d) & M32
    x ^= x >> 15; x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def ppg_rand(key, dim):
    r = _hash32(int(key) ^ _hash32((int(dim) * 0x9e3779b1 + 0x7f4a7c15) & M32))
    return np.array([(r >> 9) | 0x3f800000], np.uint32).view(f32)[0] - f32(1.0)


def to_fixed(x):
    """ppg_to_fixed: round-half-even of x * 2^24; NaN and negatives 0, from 2^26 on (and +inf) 2^50."""
    x = float(x)
    if x != x or x < 0.0:
        return 0
    v = x * 16777216.0
    if not v < 1125899906842624.0:
        return 1 << 50
    return int(round(v))  # Python rounds halves to even; v is exact (a float32 scaled by a power of two)


def _finite(x):
    return not (math.isinf(float(x)) or math.isnan(float(x)))


def _mx(a, b):  # std::max
    return b if a < b else a


def _mn(a, b):  # std::min
    return b if b < a else a


class Tree:
    """The arrays of read_sdtree() the commit reads: S-tree topology and box, building D-trees' topology."""

    def __init__(self, t):
        self.axis = [int(a) for a in t["axis"]]
        self.children = [(int(a), int(b)) for a, b in t["children"]]
        self.mn = [f32(v) for v in t["aabb_min"]]
        self.mx = [f32(v) for v in t["aabb_max"]]
        self.ext = [self.mx[a] - self.mn[a] for a in range(3)]  # AABB::getExtents
        b = t["building"]
        self.offset = [int(o) for o in b["offset"]]
        self.num_nodes = [int(n) for n in b["num_nodes"]]
        self.dchild = b["node_children"].tolist()
        self.is_leaf = [c[0] == 0 for c in self.children]

    def lookup(self, p):
        """STree::dTreeWrapper (GP:897-905, 761-769): leaf and voxel size."""
        size = list(self.ext)
        q = [(f32(p[a]) - self.mn[a]) / size[a] for a in range(3)]
        node = 0
        while not self.is_leaf[node]:
            a = self.axis[node]
            size[a] = size[a] / f32(2)
            if q[a] < f32(0.5):
                q[a] = q[a] * f32(2)
                node = self.children[node][0]
            else:
                q[a] = (q[a] - f32(0.5)) * f32(2)
                node = self.children[node][1]
        return node, size

    def dnode(self, leaf, n):
        return self.dchild[self.offset[leaf] + n]


def _child_index(p):  # QuadTreeNode::childIndex, GP:205-217
    res = 0
    for i in range(2):
        if p[i] < f32(0.5):
            p[i] = p[i] * f32(2)
        else:
            p[i] = (p[i] - f32(0.5)) * f32(2)
            res |= 1 << i
    return res


class Result:
    def __init__(self):
        self.fixed = {}      # (leaf, node, slot) -> int
        self.weight = {}     # leaf -> int
        self.records = []    # (key, product, woPdf, bsdfPdf, dTreePdf, weight) of the optimiser
        self.committed = 0
        self.splats = []     # per DTreeWrapper::record call: dict(leaf, vertex, path, v, w, w64, irr, irr64, px, py, canon64, live, depth, addends)
        self.vertex_w64 = {}  # vertex -> [w64 of the vertex, sum of its leaves' w64] (box spatial filter)
        self.n_addends = {}  # leaf -> additions into its slots


def _record_irradiance(tree, res, leaf, p, irradiance, w, dfilter, info):
    """DTree::recordIrradiance, GP:395-413."""
    if not (_finite(w) and w > 0):
        return
    res.weight[leaf] = res.weight.get(leaf, 0) + to_fixed(w)
    info["live"] = False
    if not (_finite(irradiance) and irradiance > 0):
        return
    info["live"] = True

    info["fixed_sum"], info["addends"] = 0, 0

    def add(node, slot, value):
        k = (leaf, node, slot)
        fx = to_fixed(value)
        res.fixed[k] = res.fixed.get(k, 0) + fx
        res.n_addends[leaf] = res.n_addends.get(leaf, 0) + 1
        info["fixed_sum"] += fx
        info["addends"] += 1

    if dfilter == "nearest":  # QuadTreeNode::record, GP:303-312
        q = [p[0], p[1]]
        value = irradiance * w
        node = 0
        while True:
            i = _child_index(q)
            c = tree.dnode(leaf, node)[i]
            if c == 0:
                add(node, i, value)
                return
            node = c
    q = [p[0], p[1]]
    depth, node = 0, 0
    while True:  # depthAt, GP:247-255
        i = _child_index(q)
        depth += 1
        c = tree.dnode(leaf, node)[i]
        if c == 0:
            break
        node = c
    info["depth"] = depth
    size = f32(math.ldexp(1.0, -depth))  # std::pow(0.5f, depth), exact
    origin = [p[0] - size / f32(2), p[1] - size / f32(2)]
    value = irradiance * w / (size * size)
    info["inside"] = bool(origin[0] >= 0 and origin[1] >= 0 and origin[0] + size <= f32(1) and origin[1] + size <= f32(1))

    def rec(node, no, ns):  # GP:322-338
        cs = ns / f32(2)
        ch = tree.dnode(leaf, node)
        for i in range(4):
            co = [no[0], no[1]]
            if i & 1:
                co[0] = co[0] + cs
            if i & 2:
                co[1] = co[1] + cs
            lx = _mx(_mn(origin[0] + size, co[0] + cs) - _mx(origin[0], co[0]), f32(0))
            ly = _mx(_mn(origin[1] + size, co[1] + cs) - _mx(origin[1], co[1]), f32(0))
            ww = lx * ly
            if ww > f32(0):
                if ch[i] == 0:
                    add(node, i, value * ww)
                else:
                    rec(ch[i], co, cs)

    rec(0, [f32(0), f32(0)], f32(1))


def commit(t, cfg, inp, dir_to_canonical):
    """All vertices of `inp` through Vertex::commit.  cfg: spatial ('nearest' | 'stochastic' | 'box'), directional ('nearest' | 'box'),
    loss (bool: a loss is set AND the tree is built), weight (1.0 | 0.5).  inp: the arrays of Engine.debug_commit."""
    tree = t if isinstance(t, Tree) else Tree(t)
    res = Result()
    sw0 = f32(cfg["weight"])
    k = 0
    with np.errstate(all="ignore"):
        for i, nv in enumerate(inp["nv"]):
            for v in range(int(nv)):
                _commit_vertex(tree, res, cfg, inp, dir_to_canonical, sw0, i, v, k)
                k += 1
    res.records.sort(key=lambda r: r[0])
    return res


def _commit_vertex(tree, res, cfg, inp, dir_to_canonical, sw0, i, v, k):
    rad = [f32(x) for x in inp["radiance"][k]]
    thr = [f32(x) for x in inp["throughput"][k]]
    bsdf = [f32(x) for x in inp["bsdf_val"][k]]
    wo, bp, dp = f32(inp["wo_pdf"][k]), f32(inp["bsdf_pdf"][k]), f32(inp["dtree_pdf"][k])
    delta = bool(inp["is_delta"][k])
    p = [f32(x) for x in inp["p"][k]]
    d = [f32(x) for x in inp["d"][k]]
    leaf0, vox = tree.lookup(p)
    # GP:1730-1744
    if not (wo > 0) or any((not _finite(x)) or x < 0 for x in rad) or any((not _finite(x)) or x < 0 for x in bsdf):
        return
    res.committed += 1
    lr = [f32(0)] * 3
    lr64 = [0.0] * 3
    for c in range(3):
        if thr[c] * wo > EPSILON:
            lr[c] = rad[c] / thr[c]
            lr64[c] = float(rad[c]) / float(thr[c])
    prod = [lr[c] * bsdf[c] for c in range(3)]
    radiance = (((f32(0) + lr[0]) + lr[1]) + lr[2]) * THIRD
    product = (((f32(0) + prod[0]) + prod[1]) + prod[2]) * THIRD
    rad64 = (lr64[0] + lr64[1] + lr64[2]) / 3.0

    def wrapper_record(leaf, w, w64):  # DTreeWrapper::record, GP:575-584
        if not delta:
            irradiance = radiance / wo
            px, py = dir_to_canonical(d)
            info = dict(leaf=leaf, vertex=k, path=i, v=v, w=w, w64=w64, irr=irradiance, irr64=rad64 / float(wo), px=px, py=py, live=None)
            _record_irradiance(tree, res, leaf, [f32(px), f32(py)], irradiance, w, cfg["directional"], info)
            res.splats.append(info)
        if cfg["loss"] and product > 0:
            key = (leaf << LEAF_SHIFT) | (i << CODE_BITS) | (CODE_VERTEX + v)
            res.records.append((key, product, wo, bp, dp, w))

    if cfg["spatial"] == "nearest":
        wrapper_record(leaf0, sw0, float(sw0))
    elif cfg["spatial"] == "stochastic":  # GP:1746-1763
        key, dim = int(inp["key"][i]), int(inp["dim"][i]) + 3 * v
        o = [p[a] + vox[a] * (ppg_rand(key, dim + a) - f32(0.5)) for a in range(3)]
        o = [_mn(_mx(o[a], tree.mn[a]), tree.mx[a]) for a in range(3)]  # AABB::clip
        leaf, _ = tree.lookup(o)
        wrapper_record(leaf, sw0, float(sw0))
    else:  # STree::record, GP:935-943
        volume = f32(1)
        for a in range(3):
            volume = volume * vox[a]
        w = sw0 / volume
        w64 = float(sw0) / (float(vox[0]) * float(vox[1]) * float(vox[2]))
        min1 = [p[a] - vox[a] * f32(0.5) for a in range(3)]
        max1 = [p[a] + vox[a] * f32(0.5) for a in range(3)]
        inside = all(min1[a] >= tree.mn[a] and max1[a] <= tree.mx[a] for a in range(3))
        tot = [float(sw0), 0.0, inside]
        res.vertex_w64[k] = tot

        def node_record(node, min2, size2):  # STreeNode::record, GP:823-839
            ls = [_mx(_mn(max1[a], min2[a] + size2[a]) - _mx(min1[a], min2[a]), f32(0)) for a in range(3)]
            ov = ls[0] * ls[1] * ls[2]
            if not ov > 0:
                return
            if tree.is_leaf[node]:
                ls64 = [max(min(float(max1[a]), float(min2[a]) + float(size2[a])) - max(float(min1[a]), float(min2[a])), 0.0) for a in range(3)]
                lw64 = w64 * ls64[0] * ls64[1] * ls64[2]
                tot[1] += lw64
                wrapper_record(node, w * ov, lw64)
                return
            a = tree.axis[node]
            size2 = list(size2)
            min2 = list(min2)
            size2[a] = size2[a] / f32(2)
            for c in range(2):
                if c & 1:
                    min2[a] = min2[a] + size2[a]
                node_record(tree.children[node][c], min2, size2)

        node_record(0, list(tree.mn), list(tree.ext))


# ------------------------------------------------------------------------------------------------
# The round's records as k_commit_records lays them out, and what k_splat_sorted does with them
# ------------------------------------------------------------------------------------------------
def round_keys(res, inp, n_stree_nodes, late=None, max_vertices=32, with_weights=False):
    """The sorted key array of a record route: positions = exclusive scan of the vertex counts (a late path reserves max_vertices), a key
    per DTreeWrapper::record call that has a weight or an optimiser record, 'splat only' ones flagged just above the leaf bits, stable sort
    by (flag, leaf), holes (~0) behind.  -> (keys list with holes, leaf_bits[, per sorted position: its splat record has a weight])."""
    leaf_bits = 1
    while (1 << leaf_bits) <= n_stree_nodes:
        leaf_bits += 1
    flag = 1 << (LEAF_SHIFT + leaf_bits)
    base, pos = [], 0
    for i, nv in enumerate(inp["nv"]):
        base.append(pos)
        pos += max_vertices if (late is not None and late[i]) else int(nv)
    n = pos
    keys = [None] * n
    opt = {r[0] for r in res.records}
    for s in res.splats:
        key = (s["leaf"] << LEAF_SHIFT) | (s["path"] << CODE_BITS) | (CODE_VERTEX + s["v"])
        if key in opt:
            keys[base[s["path"]] + s["v"]] = key
        elif s["live"] is not None:  # (a weight was added)
            keys[base[s["path"]] + s["v"]] = key | flag
    for r in res.records:  # (a delta vertex leaves a record and no splat)
        path, v = (r[0] >> CODE_BITS) & ((1 << 27) - 1), (r[0] & ((1 << CODE_BITS) - 1)) - CODE_VERTEX
        keys[base[path] + v] = r[0]
    weighted = set()  # positions whose splat record carries a statistical weight
    for s in res.splats:
        if s["live"] is not None:
            weighted.add(base[s["path"]] + s["v"])
    valid = [(kk >> LEAF_SHIFT, j) for j, kk in enumerate(keys) if kk is not None]
    valid.sort()  # (stable in the position j)
    out = [keys[j] for _, j in valid] + [(1 << 64) - 1] * (n - len(valid))
    if with_weights:
        return out, leaf_bits, [j in weighted for _, j in valid] + [False] * (n - len(valid))
    return out, leaf_bits


def splat_routes(keys, leaf_bits, num_nodes, lds_nodes=LDS_NODES):
    """Which way k_splat_sorted takes the chunks and runs of `keys` -> (set of route names, the record-by-record chunks' first positions)."""
    leaf_mask, field_mask = (1 << leaf_bits) - 1, (2 << leaf_bits) - 1
    field = [(kk >> LEAF_SHIFT) & field_mask for kk in keys]
    routes, by_record = set(), []
    n = len(keys)
    for lo in range(0, n, CHUNK):
        hi = min(n, lo + CHUNK)
        f_first, f_last = field[lo], field[hi - 1]
        count_runs = (f_last & leaf_mask) == leaf_mask or f_last - f_first >= MAX_RUNS
        routes.add("runs counted" if count_runs else "run count skipped")
        if count_runs:
            runs = sum(1 for p in range(lo, hi) if (field[p] & leaf_mask) != leaf_mask and (p == 0 or field[p - 1] != field[p]))
            if runs == MAX_RUNS:
                routes.add("exactly 64 runs")
            if runs == MAX_RUNS + 1:
                routes.add("65 runs")
            if runs > MAX_RUNS:
                routes.add("record by record")
                by_record.append(lo)
                continue
        pos = lo
        while pos < hi:
            f0 = field[pos]
            if (f0 & leaf_mask) == leaf_mask:
                routes.add("holes at the end")
                break
            end = pos
            while end < hi and field[end] <= f0:
                end += 1
            if pos == lo and lo > 0 and field[lo - 1] == f0:
                routes.add("run continued across chunks")
            nn = num_nodes[f0 & leaf_mask]
            if nn > lds_nodes:
                routes.add("unstaged: large")
            elif (end - pos) * RUN_FACTOR < nn:
                routes.add("unstaged: short")
            else:
                routes.add("staged")
            pos = end
    return routes, by_record


def wave_arms(lanes):
    """wave_key_add<3> over one wave: lanes = [(key, value) or None] * 64 -> the arms reached ('equal', 'reduced', 'direct')."""
    arms = set()
    todo = [x for x in lanes if x is not None]
    for _ in range(3):
        if not todo:
            break
        k0, v0 = todo[0]
        grp = [x for x in todo if x[0] == k0]
        arms.add("equal" if all(x[1] == v0 for x in grp) else "reduced")
        todo = [x for x in todo if x[0] != k0]
    if todo:
        arms.add("direct")
    return arms


def commit_wave_arms(res, inp, n_paths, grid=2048):
    """The arms k_commit's wave_key_add reaches (nearest / stochastic spatial filter): work item w = slot * n_paths + path, a wave is 64
    consecutive items of a workgroup of 256, key = leaf * 32 + (workgroup & 31)."""
    by = {}
    for s in res.splats:
        if s["live"] is not None:
            w = s["v"] * n_paths + s["path"]
            by.setdefault(w // 64, {})[w % 64] = (s["leaf"] * 32 + ((w // 256) % grid) % 32, to_fixed(s["w"]))
    arms = set()
    for lanes in by.values():
        arms |= wave_arms([lanes.get(j) for j in range(64)])
    return arms


def record_wave_arms(keys, weighted, leaf_bits, by_record, weight_fixed):
    """The arms wave_key_add<3> reaches in k_splat_sorted's record-by-record chunks (first positions `by_record`, from splat_routes): lane t
    of the workgroup of 256 takes positions lo + t + 256 j, j < 8; per j a wave of 64 lanes adds (leaf, the launch's weight) for its records
    that carry a weight."""
    leaf_mask = (1 << leaf_bits) - 1
    arms = set()
    for lo in by_record:
        hi = min(len(keys), lo + CHUNK)
        for j in range(CHUNK // BLOCK):
            for wave in range(BLOCK // 64):
                lanes = []
                for lane in range(64):
                    p = lo + wave * 64 + lane + j * BLOCK
                    leaf = (keys[p] >> LEAF_SHIFT) & leaf_mask if p < hi else leaf_mask
                    lanes.append((leaf, weight_fixed) if p < hi and leaf != leaf_mask and weighted[p] else None)
                arms |= wave_arms(lanes)
    return arms
