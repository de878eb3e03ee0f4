"""The trees, contexts and explicit vertices of tests/test_commit.py and tests/test_commit_gpu.py (not a test module).

The tree: CBOX 32x32, budgetType spp, five iterations of 1, 2, 4, 8, 16 passes of 4 samples with sTreeThreshold 300 and dTreeThreshold
0.0015, then begin_iteration(False).  Chosen on the CPU with the oracle; with the kl loss and weight 1 it gives
    nearest / nearest  319 S-tree leaves, building D-trees of 341 / 525 / 777 nodes (min / median / max), 173 above 512, deepest 13
    nearest / box      314 S-tree leaves, building D-trees of 341 / 521 / 675 nodes, 182 above 512, deepest 12
and about half as many leaves under the kick-start's weight of 0.5.  assert_shape() holds every context's tree to at least MIN_LEAVES
leaves, a building D-tree of depth MIN_DEPTH and three D-trees below SMALL nodes, and says whether one lies above: the record routes meet
staged and large D-trees in the same tree, and tests/test_commit_gpu.py runs them again with PPG_SPLAT_LDS_NODES=4, which makes every
D-tree large.
"""
import ctypes as C

import numpy as np

TREE = dict(res=32, iters=5, sTreeThreshold=300, dTreeThreshold=0.0015, seed=7)
MIN_LEAVES, MIN_DEPTH, SMALL = 64, 8, 512
SPATIAL, DIRECTIONAL, LOSSES, WEIGHTS = ("nearest", "stochastic", "box"), ("nearest", "box"), ("none", "kl"), (1.0, 0.5)
ROUTES = ("commit", "commit_split", "records", "records_split")
MAX_VERTICES = 9  # CBOX_PROPS: maxDepth 10


def contexts():
    return [(s, d, l, w) for s in SPATIAL for d in DIRECTIONAL for l in LOSSES for w in WEIGHTS]


def props(spatial, directional, loss, weight):
    from conftest import CBOX_PROPS
    return dict(CBOX_PROPS, budget=4096, seed=TREE["seed"], sTreeThreshold=TREE["sTreeThreshold"], dTreeThreshold=TREE["dTreeThreshold"],
                spatialFilter=spatial, directionalFilter=directional, bsdfSamplingFractionLoss=loss, nee="kickstart" if weight == 0.5 else "never")


def grow(engine, weight):
    """The module's tree on `engine`: rendered iterations, then an open training iteration."""
    import ppg_host
    engine.set_scene(ppg_host.cbox_scene(TREE["res"], TREE["res"]))
    engine.begin_render()
    for it in range(TREE["iters"]):
        engine.set_do_nee(weight == 0.5)  # (kickstart: luminaire sampling while spp < 128; here for every iteration, on both engines alike)
        engine.begin_iteration(False)
        engine.render_passes(1 << it)
        engine.build_sdtree()
        engine.end_iteration()
    engine.set_do_nee(weight == 0.5)
    engine.begin_iteration(False)


def admitted(spatial, loss, weight):
    """The routes a context runs: the record routes need a round (a loss) and known record positions."""
    return ROUTES if (loss != "none" and spatial != "box" and weight == 1.0) else ROUTES[:2]


def assert_shape(t):
    leaves = t["children"][:, 0] == 0
    nn = t["building"]["num_nodes"][leaves]
    assert leaves.sum() >= MIN_LEAVES, leaves.sum()
    assert t["building"]["max_depth"].max() >= MIN_DEPTH
    assert (nn < SMALL).sum() >= 3
    return bool((nn > SMALL).any())


class Oracle:
    """ppgo_canonical_to_dir / ppgo_dir_to_canonical of the oracle library."""

    def __init__(self, lib):
        self.lib = lib
        lib.ppgo_canonical_to_dir.restype = None
        lib.ppgo_dir_to_canonical.restype = None
        lib.ppgo_canonical_to_dir.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_float)]
        lib.ppgo_dir_to_canonical.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]

    def to_dir(self, x, y):
        d = (C.c_float * 3)()
        self.lib.ppgo_canonical_to_dir(C.c_float(x), C.c_float(y), d)
        return [d[0], d[1], d[2]]

    def to_canonical(self, d):
        a, o = (C.c_float * 3)(*[float(x) for x in d]), (C.c_float * 2)()
        self.lib.ppgo_dir_to_canonical(a, o)
        return np.float32(o[0]), np.float32(o[1])


# ------------------------------------------------------------------------------------------------
# Inputs
# ------------------------------------------------------------------------------------------------
def _pack(nv, verts, rng, late=None):
    """verts: list of dicts (p, d, radiance, throughput, bsdf_val, wo_pdf, bsdf_pdf, dtree_pdf, is_delta), path after path."""
    n = len(nv)
    f3 = lambda k: np.array([v[k] for v in verts], np.float32).reshape(-1, 3)
    f1 = lambda k: np.array([v[k] for v in verts], np.float32).reshape(-1)
    return dict(nv=np.array(nv, np.uint32), key=rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32),
                dim=rng.integers(0, 200, n).astype(np.uint32), late=None if late is None else np.array(late, np.uint8),
                p=f3("p"), d=f3("d"), radiance=f3("radiance"), throughput=f3("throughput"), bsdf_val=f3("bsdf_val"),
                wo_pdf=f1("wo_pdf"), bsdf_pdf=f1("bsdf_pdf"), dtree_pdf=f1("dtree_pdf"), is_delta=np.array([v["is_delta"] for v in verts], np.uint8))


def _vertex(rng, box, **over):
    mn, mx = box
    z = rng.uniform(-1, 1)
    phi = rng.uniform(0, 2 * np.pi)
    s = np.sqrt(max(0.0, 1 - z * z))
    v = dict(p=[rng.uniform(mn[a], mx[a]) for a in range(3)], d=[s * np.cos(phi), s * np.sin(phi), z],
             radiance=list(rng.uniform(0.0, 4.0, 3)), throughput=list(rng.uniform(0.05, 1.0, 3)), bsdf_val=list(rng.uniform(0.0, 1.0, 3)),
             wo_pdf=rng.uniform(0.05, 2.0), bsdf_pdf=rng.uniform(0.0, 1.0), dtree_pdf=rng.uniform(0.0, 1.0), is_delta=False)
    v.update(over)
    return v


def _paths(rng, nvs, make):
    verts = []
    for i, n in enumerate(nvs):
        verts += [make(i, v) for v in range(n)]
    return _pack(nvs, verts, rng)


def case_guards(t, orc, rng):
    """Every guard of Vertex::commit, DTreeWrapper::record and ppg_to_fixed, one vertex each, 65 paths."""
    box = (t["aabb_min"], t["aabb_max"])
    nan, inf = float("nan"), float("inf")
    eps = float(np.float32(1e-4))
    over = [dict(wo_pdf=w) for w in (0.0, -1.0, nan, inf, 1e-30)]
    for c in range(3):
        for bad in (nan, inf, -0.5):
            r, b = [1.0, 2.0, 3.0], [0.5, 0.25, 0.125]
            r[c] = bad
            over.append(dict(radiance=r))
            b[c] = bad
            over.append(dict(bsdf_val=b))
        for f in (0.5, 1.0, float(np.nextafter(np.float32(1), np.float32(2))), 2.0):  # throughput * woPdf below, at, just above, above PPG_EPSILON
            th = [0.5, 0.5, 0.5]
            th[c] = eps * f
            over.append(dict(throughput=th, wo_pdf=1.0))
    over += [dict(is_delta=True), dict(is_delta=True, radiance=[0.0, 0.0, 0.0]),
             dict(radiance=[3e38, 3e38, 3e38], throughput=[1.0, 1.0, 1.0], wo_pdf=1e-3, bsdf_val=[0.0, 0.0, 0.0]),  # radiance / woPdf overflows to inf (no optimiser record: case_inf_product)
             dict(radiance=[0.0, 0.0, 0.0]), dict(bsdf_val=[0.0, 0.0, 0.0]),                     # product = 0 with and without irradiance
             dict(throughput=[-1.0, -1.0, -1.0])]                                                # no channel passes the throughput test
    for x in (2.0 ** 26 * 0.999, 2.0 ** 26, 2.0 ** 26 * 1.001, 2.0 ** 27, 2.0 ** -25, 2.0 ** -26, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24):
        over.append(dict(radiance=[x, x, x], throughput=[1.0, 1.0, 1.0], wo_pdf=1.0))           # irradiance * weight around the clamp and the ties
    while len(over) < 65:
        over.append({})
    verts = [_vertex(rng, box, **o) for o in over]
    return _pack([1] * len(verts), verts, rng)


def case_inf_product(t, orc, rng):
    """One vertex whose optimiser record has product = inf: its Adam step turns the leaf's variable into a NaN.  Run LAST in a context, so
    that no later step of that leaf is compared NaN against NaN."""
    box = (t["aabb_min"], t["aabb_max"])
    return _pack([1], [_vertex(rng, box, radiance=[3e38, 3e38, 3e38], throughput=[1.0, 1.0, 1.0], wo_pdf=1e-3, bsdf_val=[0.5, 0.5, 0.5])], rng)


def case_wave_leaves(t, orc, rng, n_leaves):
    """64 paths of one vertex each — one wave of k_commit's slot 0 — at the centres of n_leaves distinct S-tree leaves, path i in leaf
    i mod n_leaves: wave_key_add<3> combines up to three keys and adds the fourth and later ones directly."""
    mn, mx = np.array(t["aabb_min"], np.float64), np.array(t["aabb_max"], np.float64)
    centres = leaf_centres(t)
    ids = sorted(centres)
    assert len(ids) >= n_leaves
    pick = [ids[int(j * (len(ids) - 1) // max(1, n_leaves - 1))] for j in range(n_leaves)]
    assert len(set(pick)) == n_leaves
    return _paths(rng, [1] * 64, lambda i, v: _vertex(rng, (mn, mx), p=list(centres[pick[i % n_leaves]]), is_delta=False, radiance=[1.0, 1.0, 1.0]))


def state(engine):
    """The optimiser's state of every S-tree node now (a call without paths)."""
    e3, e1 = np.zeros((0, 3), np.float32), np.zeros(0, np.float32)
    z = np.zeros(0, np.uint32)
    return engine.debug_commit("commit", z, z, z, e3, e3, e3, e3, e3, e1, e1, e1, np.zeros(0, np.uint8))["adam_state"]


def leaves_per_vertex(res):
    """How many leaves every vertex's record went to (the restatement's splats, box spatial filter)."""
    n = {}
    for s in res.splats:
        n[s["vertex"]] = n.get(s["vertex"], 0) + 1
    return n


def case_directions(t, orc, rng):
    """Poles, signed zeros, phi = 0 and pi, dyadic cell borders, overhanging box footprints, unnormalised and zero vectors: 63 paths."""
    box = (t["aabb_min"], t["aabb_max"])
    ds = [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [-0.0, 0.0, 1.0], [-0.0, -0.0, 1.0], [-0.0, 0.0, -1.0], [-0.0, -0.0, -1.0],
          [1.0, 0.0, 0.0], [1.0, -0.0, 0.0], [-1.0, 0.0, 0.0], [-1.0, -0.0, 0.0], [0.6, 0.0, 0.8], [0.6, -0.0, -0.8],
          [3.0, 4.0, 12.0], [0.0, 0.0, 5.0], [0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [1e-30, 1e-30, 1e-30], [0.3, 0.4, 2.0], [float("inf"), 0.0, 0.0],
          [0.0, float("nan"), 1.0]]
    dy = [0.0, 0.5, 0.25, 0.75, 0.125, 1.0 - 2.0 ** -20, 2.0 ** -20, 1.0, 2.0 ** -12, 0.5 - 2.0 ** -13]
    for x in dy:
        for y in (0.0, 0.5, 0.25, 1.0 - 2.0 ** -20, 2.0 ** -11):
            ds.append(orc.to_dir(x, y))
    ds = ds[:63]
    while len(ds) < 63:
        ds.append(orc.to_dir(rng.uniform(0, 1), rng.uniform(0, 1)))
    verts = [_vertex(rng, box, d=d) for d in ds]
    return _pack([1] * 63, verts, rng)


def case_positions(t, orc, rng):
    """On S-tree split planes, on faces, edges and corners of the box, one voxel outside it: 64 paths of two vertices."""
    mn, mx = np.array(t["aabb_min"], np.float64), np.array(t["aabb_max"], np.float64)
    ext = mx - mn
    ps = []
    for a in range(3):
        for f in (0.5, 0.25, 0.75, 0.125, 0.375):  # planes of the first levels along axis a
            p = mn + ext * rng.uniform(0.05, 0.95, 3)
            p[a] = mn[a] + ext[a] * f
            ps.append(p)
    for bits in range(8):  # corners
        ps.append(np.where([(bits >> a) & 1 for a in range(3)], mx, mn))
    for a in range(3):
        for side in (mn, mx):
            p = mn + ext * rng.uniform(0.05, 0.95, 3)
            p[a] = side[a]
            ps.append(p)          # faces
            q = p.copy()
            q[(a + 1) % 3] = side[(a + 1) % 3]
            ps.append(q)          # edges
            o = p.copy()
            o[a] = side[a] + (ext[a] / 16) * (1 if side is mx else -1)
            ps.append(o)          # outside
    ps.append(mn + ext * 0.5)
    ps.append(mn + ext * 2.0)      # far outside: the box filter finds no overlap
    while len(ps) < 128:
        ps.append(mn + ext * rng.uniform(0, 1, 3))
    verts = [_vertex(rng, (mn, mx), p=list(p)) for p in ps[:128]]
    return _pack([2] * 64, verts, rng)


def case_random(t, orc, rng, n_paths, mean_nv=1.5, late=None):
    """Random vertices; whole waves of paths without vertices (paths 64 .. 191 where there are that many) and one path at the maximum."""
    box = (t["aabb_min"], t["aabb_max"])
    nvs = [int(min(MAX_VERTICES, x)) for x in rng.poisson(mean_nv, n_paths)]
    for i in range(64, min(192, n_paths)):
        nvs[i] = 0
    nvs[n_paths // 2] = MAX_VERTICES
    c = _paths(rng, nvs, lambda i, v: _vertex(rng, box, is_delta=bool(rng.uniform() < 0.05), radiance=list(rng.uniform(0.0, 4.0, 3) * (rng.uniform() < 0.8))))
    if late == "all":
        c["late"] = np.ones(n_paths, np.uint8)
    elif late == "third":
        c["late"] = (np.arange(n_paths) % 3 == 0).astype(np.uint8)
    return c


def case_one_leaf(t, orc, rng, total, point=None):
    """`total` vertices at one point (`point`: where, in world coordinates) (one S-tree leaf under the nearest filter), one per path: one run, across chunk borders from 2049 on."""
    mn, mx = np.array(t["aabb_min"], np.float64), np.array(t["aabb_max"], np.float64)
    p = list(mn + (mx - mn) * np.array([0.31, 0.27, 0.64]) if point is None else point)
    return _paths(rng, [1] * total, lambda i, v: _vertex(rng, (mn, mx), p=p))


def case_leaves(t, orc, rng, n_leaves, per_leaf, tree):
    """per_leaf vertices in each of n_leaves S-tree leaves spread over the whole index range (their centres): a chunk of n_leaves runs."""
    mn, mx = np.array(t["aabb_min"], np.float64), np.array(t["aabb_max"], np.float64)
    centres = leaf_centres(t)
    ids = sorted(centres)
    pick = [ids[int(round(j * (len(ids) - 1) / (n_leaves - 1)))] for j in range(n_leaves)]
    assert len(set(pick)) == n_leaves
    ps = [centres[l] for l in pick for _ in range(per_leaf)]
    return _paths(rng, [1] * len(ps), lambda i, v: _vertex(rng, (mn, mx), p=list(ps[i]), is_delta=False, radiance=[1.0, 1.0, 1.0]))


def leaf_centres(t):
    mn, mx = np.array(t["aabb_min"], np.float64), np.array(t["aabb_max"], np.float64)
    out = {}

    def walk(node, lo, size):
        c0, c1 = (int(x) for x in t["children"][node])
        if c0 == 0:
            out[node] = lo + size / 2
            return
        a = int(t["axis"][node])
        size = size.copy()
        size[a] /= 2
        walk(c0, lo, size)
        lo = lo.copy()
        lo[a] += size[a]
        walk(c1, lo, size)

    walk(0, mn, mx - mn)
    return out


def call(engine, route, c, **kw):
    return engine.debug_commit(route, c["nv"], c["key"], c["dim"], c["p"], c["d"], c["radiance"], c["throughput"], c["bsdf_val"], c["wo_pdf"],
                               c["bsdf_pdf"], c["dtree_pdf"], c["is_delta"], late=c.get("late"), **kw)


def delta(before, after):
    """What a call added: fixed sums per building node slot, fixed weights per S-tree node; the topology must not have moved."""
    for k in ("children", "axis"):
        assert np.array_equal(before[k], after[k]), k
    for k in ("num_nodes", "node_children", "max_depth", "offset"):
        assert np.array_equal(before["building"][k], after["building"][k]), k
    for k in ("num_nodes", "node_children", "node_sums", "sum", "stat_weight"):
        assert np.array_equal(before["sampling"][k], after["sampling"][k]), k
    dw = np.rint((after["building"]["stat_weight"] - before["building"]["stat_weight"]) * 16777216.0).astype(np.int64)
    return after["building"]["node_fixed"].astype(np.int64) - before["building"]["node_fixed"].astype(np.int64), dw


def expected_arrays(res, t):
    """The restatement's sums in the layout of delta()."""
    fx = np.zeros(t["building"]["node_fixed"].shape, np.int64)
    for (leaf, node, slot), v in res.fixed.items():
        fx[int(t["building"]["offset"][leaf]) + node, slot] += v
    w = np.zeros(len(t["axis"]), np.int64)
    for leaf, v in res.weight.items():
        w[leaf] += v
    return fx, w
