"""The SD-tree of the oracle AND of the HIP kernels against the reference's own compiled classes.

Every other parity test compares libppg_hip.so with oracle/libppg_oracle.so — two restatements by the same hands that share
include/ppg_detmath.h and include/ppg_rng.h.  Here the judge is the reference's text itself: AdamOptimizer, QuadTreeNode, DTree,
DTreeWrapper, STreeNode, STree of guided_path.cpp, cut out at build time and compiled under strict IEEE-754 float evaluation behind the C ABI
of oracle/ref_sdtree/harness.cpp (oracle/_ref/libppg_ref_sdtree.so; never committed).  One set of checks, written against an engine, runs
with the oracle (CPU) and with the HIP engine (-m gpu).  A render is driven phase by phase; at every iteration boundary the engine's trees are
loaded into the reference's classes (Engine.read_sdtree()), the reference runs the same step, and the results are compared:

  refine + reset  S-tree topology in the reference's numbering, building D-tree topology (the LIFO numbering of DTree::reset), max depth,
                  halved statistical weights, inherited theta: exactly equal.
  pdf             Engine.query_pdf against STree::dTreeWrapper -> DTreeWrapper::pdf, bit for bit, on 20 000 random queries plus listed edges.
                  A query is *boundary-flagged* — by the reference alone — if its pdf changes when dirToCanonical(dir) moves by +-DELTA in x or y
                  (DELTA: the 4e-7 atan2 bound of test_detmath.py / 2 pi, rounded up to one float ulp at 1.0); a flagged query must return
                  the value of a neighbouring cell.  At most 1 % of the random queries may be flagged (asserted; printed).
  sample          Engine.query_sample against DTree::sample on the same stream: same canonical leaf cell (within DELTA), direction within the
                  sincos bound of test_detmath.py + 2 ulp per component — which an engine that consumed other draws than the reference cannot
                  meet (it returns only the direction).  That the reference itself draws depth-of-the-leaf + 2 numbers is checked on the
                  harness, as a check of the stream handed to it, not of the engine.
  build           DTreeWrapper::build on the engine's accumulated leaf sums: interior node sums, tree sums bit-equal; min / avg / max mean
                  radiance of the tree statistics within 1 float ulp of DTree::mean().
  splat (CPU)     ppgo_dtree_exercise against the reference's recordIrradiance / build / reset / pdf / sample.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ref_sdtree as R
from conftest import CBOX_PROPS, IMPROVED, ROOT, make_oracle

needs_ref = pytest.mark.skipif(not R.reference_available(), reason=R.SKIP_REASON)  # (no side effects here: Ref() builds on first use)
ENGINES = [pytest.param("oracle", id="oracle"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
BOXBOX = dict(spatialFilter="box", directionalFilter="box", bsdfSamplingFractionLoss="var", sTreeThreshold=600, sampleCombination="discard")
QUARTER_PI_INV = np.float32(1 / (4 * np.pi))


def _engine(kind, oracle_lib, **props):
    if kind == "hip":
        import ppg_host
        return ppg_host.Engine.hip(**props)
    return make_oracle(oracle_lib, threads=min(16, os.cpu_count() or 8), **props)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _leaf_cells(tree):
    """(node, lo, size) of every S-tree leaf in world coordinates (float64 walk; only used to pick positions)"""
    lo0, ext = tree["aabb_min"].astype(np.float64), (tree["aabb_max"] - tree["aabb_min"]).astype(np.float64)
    out, stack = [], [(0, lo0, ext)]
    while stack:
        i, lo, sz = stack.pop()
        c = tree["children"][i]
        if c[0] == 0 and c[1] == 0:
            out.append((i, lo, sz))
            continue
        a = int(tree["axis"][i])
        sz = sz.copy(); sz[a] /= 2
        hi = lo.copy(); hi[a] += sz[a]
        stack.append((int(c[0]), lo, sz)); stack.append((int(c[1]), hi, sz))
    return out


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _positions(rng, tree, n):
    lo, hi = tree["aabb_min"], tree["aabb_max"]
    return np.clip((lo + rng.rand(n, 3).astype(np.float32) * (hi - lo)).astype(np.float32), lo, hi)


# ---- check 1: pdf -------------------------------------------------------------------------------------------------------------------
def _neighbour_pdfs(ref, pos, c):
    """reference pdf at the canonical point moved by +-DELTA: columns 0-3 the axis moves (they define the flag), 4-7 the diagonals"""
    d = R.DELTA
    cols = []
    for dx, dy in ((d, 0), (-d, 0), (0, d), (0, -d), (d, d), (d, -d), (-d, d), (-d, -d)):
        x = np.clip(c[:, 0] + np.float32(dx), np.float32(0), np.float32(1)).astype(np.float32)
        y = (c[:, 1] + np.float32(dy)).astype(np.float32)
        y = np.where(y < 0, y + np.float32(1), np.where(y > 1, y - np.float32(1), y)).astype(np.float32)  # phi wraps
        cols.append(ref.pdf_canonical(pos, np.stack([x, y], 1))[0])
    return np.stack(cols, 1)


def check_pdf(e, ref, tree, rng, seen):
    n = 20000
    pos, dirs = _positions(rng, tree, n), _unit(rng, n)
    lo, hi = tree["aabb_min"], tree["aabb_max"]
    # the edges, one by one: (label, positions, directions, exact) — exact = must be bit-equal whatever the flag says, because no atan2 rounding
    # is involved (atan2(+-0, x > 0) = +-0, atan2(+-0, x < 0) = +-pi, atan2(+-0, +0) = +-0, atan2(+-0, -0) = +-pi by C99 F.9.1.4; non-finite -> (0, 0), GP:598-600)
    edges = []
    for a in range(3):
        p = _positions(rng, tree, 9)
        p[:, a] = [np.float32(lo[a] + (hi[a] - lo[a]) * np.float32(k / 8)) for k in range(9)]  # k = 0, 8: the box faces; 1..7: split planes of the first levels
        edges.append(("position on planes of axis %d" % a, p, _unit(rng, 9), False))
    cells = _leaf_cells(tree)
    pick = [cells[i] for i in rng.choice(len(cells), min(16, len(cells)), replace=False)]
    for a in range(3):  # split planes of the deepest levels: the faces of leaf cells
        p = np.array([c[1] + c[2] * rng.rand(3) for c in pick])
        p[:, a] = [c[1][a] + c[2][a] for c in pick]
        edges.append(("position on leaf faces of axis %d" % a, np.clip(p.astype(np.float32), lo, hi), _unit(rng, len(pick)), False))
    special = np.float32([[0, 0, 1], [0, 0, -1], [-0.0, -0.0, 1], [1, 0.0, 0], [1, -0.0, 0], [0.6, 0.0, 0.8], [0.6, -0.0, -0.8], [-1, 0.0, 0], [-1, -0.0, 0],
                          [np.nan, 0, 1], [0, np.inf, 0], [0, 1, -np.inf], [np.nan, np.nan, np.nan], [0, 0, 0], [0, 0, 2], [0, 0, -3]])
    edges.append(("poles, phi = 0 with y = +0 / -0, phi = pi, non-finite, zero and over-long directions", _positions(rng, tree, len(special)), special, True))
    means = ref.read()["sampling"]["mean"]
    dark = [c for c in cells if not means[c[0]] > 0]
    if dark:
        seen["dark"] = True
        dk = [dark[i] for i in rng.choice(len(dark), min(8, len(dark)), replace=False)]
        p = np.array([c[1] + c[2] * 0.5 for c in dk]).astype(np.float32)
        edges.append(("leaf whose mean() is 0: uniform pdf (GP:415-418)", p, _unit(rng, len(p)), True))
    allp = np.concatenate([pos] + [x[1] for x in edges]).astype(np.float32)
    alld = np.concatenate([dirs] + [x[2] for x in edges]).astype(np.float32)
    got, want = e.query_pdf(allp, alld), ref.pdf(allp, alld)
    c = ref.dir_to_canonical(alld)
    centre = ref.pdf_canonical(allp, c)[0]
    assert np.array_equal(_bits(centre), _bits(want))  # the harness's two routes agree: the flag below speaks about the same cell
    nb = _neighbour_pdfs(ref, allp, c)
    flagged = (_bits(nb[:, :4]) != _bits(want)[:, None]).any(1)
    equal = _bits(got) == _bits(want)
    near = equal | (_bits(nb) == _bits(got)[:, None]).any(1)
    share = float(flagged[:n].mean())
    assert share <= 0.01, share
    bad = ~flagged[:n] & ~equal[:n]
    assert not bad.any(), ("pdf differs from the reference on unflagged queries", int(bad.sum()), got[:n][bad][:5], want[:n][bad][:5], allp[:n][bad][:5], alld[:n][bad][:5])
    assert near[:n].all(), "a flagged query returned the value of no neighbouring cell"
    off = n
    for label, p, d, exact in edges:
        k = slice(off, off + len(p)); off += len(p)
        if exact:
            assert equal[k].all(), (label, got[k], want[k])
        else:
            assert (equal[k] | (flagged[k] & near[k])).all(), (label, got[k], want[k], flagged[k])
        seen.setdefault("edge_flagged", {}).setdefault(label, 0)
        seen["edge_flagged"][label] += int((flagged[k] & ~equal[k]).sum())
    if dark:
        assert (got[off - len(p):off] == QUARTER_PI_INV).all()
    return share


# ---- check 2: sample ----------------------------------------------------------------------------------------------------------------
def check_sample(e, ref, tree, rng, seed):
    n = 5000
    pos = _positions(rng, tree, n)
    got = e.query_sample(pos, seed)
    want, canon, dims = ref.sample(pos, seed)
    _, depth, node = ref.pdf_canonical(pos, canon)
    lit = ref.read()["sampling"]["mean"][node] > 0
    # one next1D per level and one next2D at the leaf (GP:257-301); a tree without data draws one next2D (GP:431-434)
    expect = np.where(lit, depth + 2, 2).astype(np.uint32)
    # (origin + 0.5f * child's point, level after level, rounds: at depth 20 a float keeps 4 bits inside the cell, and the point may round up onto
    # the cell's far edge, which depthAt counts to the neighbour — hence "or within DELTA of it": the depths of the cells DELTA away count too)
    d = R.DELTA
    near_depths = [depth]
    for dx, dy in ((d, 0), (-d, 0), (0, d), (0, -d), (d, d), (d, -d), (-d, d), (-d, -d)):
        c2 = np.clip(canon + np.float32([dx, dy]), np.float32(0), np.float32(1)).astype(np.float32)
        near_depths.append(ref.pdf_canonical(pos, c2)[1])
    matches = np.stack([np.where(lit, x + 2, 2).astype(np.uint32) == dims for x in near_depths]).any(0)
    for i in np.nonzero(~matches)[0]:
        # the one other way out of QuadTreeNode::sample: a node whose four sums total 0 draws its next2D there (GP:265-268, "numerical
        # instabilities": sums that underflowed at great depth).  Walk the loaded tree along the canonical point to that node and see that it is one.
        s_, off = tree["sampling"], int(tree["sampling"]["offset"][node[i]])
        k, x, y = 0, float(canon[i, 0]), float(canon[i, 1])
        for _ in range(int(dims[i]) - 2):
            j = (1 if x >= 0.5 else 0) | (2 if y >= 0.5 else 0)
            x, y = (x * 2 if x < 0.5 else (x - 0.5) * 2), (y * 2 if y < 0.5 else (y - 0.5) * 2)
            k = int(s_["node_children"][off + k, j])
            assert k != 0, "the reference drew fewer dimensions than the leaf is deep"
        q = s_["node_sums"][off + k]
        assert lit[i] and dims[i] < expect[i] and not np.float32(np.float32(np.float32(q[0] + q[2]) + q[1]) + q[3]) > 0, (i, dims[i], expect[i], q)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    assert err <= R.SINCOS_TOL, ("direction differs from the reference's beyond the sincos bound", err)
    back = ref.dir_to_canonical(got).astype(np.float64)
    size = np.where(lit, 0.5 ** (dims.astype(np.float64) - 2), 1.0)  # the cell the reference's walk ended in
    origin = np.floor(canon.astype(np.float64) / size[:, None]) * size[:, None]
    origin = np.minimum(origin, 1 - size[:, None])  # a canonical point at exactly 1.0 lies in the last cell
    d = float(R.DELTA)
    size = size + d  # the reference's own point may have rounded onto the far edge (above)
    dy = back[:, 1] - origin[:, 1]
    dy = np.where(dy > 1 - d, dy - 1, dy)  # phi = 2 pi is phi = 0
    inside = (back[:, 0] >= origin[:, 0] - d) & (back[:, 0] <= origin[:, 0] + size + d) & (dy >= -d) & (dy <= size + d)
    polar = np.abs(got[:, 2]) > 1 - 1e-6  # at the poles phi is not determined by the direction: x alone locates the cell
    inside |= polar & (back[:, 0] >= origin[:, 0] - d) & (back[:, 0] <= origin[:, 0] + size + d)
    assert (inside | ~lit).all(), ("sampled direction maps outside the reference's leaf cell", int((~inside & lit).sum()))
    return err


def check_sample_ties(e, ref, tree, seen):
    """`sample < boundary` (GP:275) with sample == boundary: a draw in 2^23 per level, which random queries never meet.  The first boundary of a
    D-tree is fl(fl(sum0 + sum2) / total) of its root; where that is a multiple of 2^-23 a stream whose first draw equals it exists: look for one
    (a few thousand seeds at most) and sample that leaf with it.  `<=` there sends the sample to the other half of the sphere."""
    r = ref.read()["sampling"]
    cells = [c for c in _leaf_cells(tree) if r["mean"][c[0]] > 0]
    if len(cells) < 8:
        return
    q = r["node_sums"][[int(r["offset"][c[0]]) for c in cells]]
    partial = (q[:, 0] + q[:, 2]).astype(np.float32)
    total = ((partial + q[:, 1]).astype(np.float32) + q[:, 3]).astype(np.float32)
    ok = total > 0
    b = np.where(ok, partial / np.where(ok, total, np.float32(1)), np.float32(0)).astype(np.float32)
    ok &= (b > 0) & (b < 1) & (b * np.float32(2 ** 23) == np.floor(b * np.float32(2 ** 23)))
    if not ok.any():
        return
    targets, n = np.unique(b[ok]), 4096
    for seed in range(1 << 20, (1 << 20) + int(40 * 2 ** 23 / (len(targets) * n)) + 1):
        u = ref.stream(seed, n, 0)
        hit = np.flatnonzero(np.isin(u, targets))
        if len(hit):
            break
    else:
        return
    i = int(hit[0])
    leaf = cells[int(np.flatnonzero(ok & (b == u[i]))[0])]
    pos = np.tile((leaf[1] + leaf[2] * 0.5).astype(np.float32), (i + 1, 1))
    got, (want, canon, dims) = e.query_sample(pos, seed), ref.sample(pos, seed)
    assert ref.pdf_canonical(pos[i:], canon[i:])[2][0] == leaf[0] and canon[i, 0] >= 0.5  # the tie goes to the right half (`<` is false)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    assert err <= R.SINCOS_TOL, ("a sample that ties with the boundary went the other way", err, got[i], want[i])
    seen["ties"] = seen.get("ties", 0) + 1


# ---- check 3: build -----------------------------------------------------------------------------------------------------------------
def check_build(e, ref):
    t = e.read_sdtree()
    ref.load(t)
    ref.build()
    st = e.build_sdtree()
    a, b = e.read_sdtree()["sampling"], ref.read()["sampling"]
    assert np.array_equal(a["num_nodes"], b["num_nodes"]) and np.array_equal(a["node_children"], b["node_children"])
    assert np.array_equal(_bits(a["node_sums"]), _bits(b["node_sums"])), "built node sums differ from the reference's DTree::build"
    assert np.array_equal(_bits(a["sum"]), _bits(b["sum"]))
    assert np.array_equal(a["stat_weight"].astype(np.float32), b["stat_weight"])
    leaf = b["num_nodes"] > 0
    m = b["mean"][leaf]
    acc = np.float32(0)
    for v in m:
        acc = np.float32(acc + v)
    for name, got, want in (("min", st.min_mean_radiance, m.min()), ("max", st.max_mean_radiance, m.max()), ("avg", st.avg_mean_radiance, np.float32(acc / np.float32(len(m))))):
        assert abs(float(got) - float(want)) <= R.ulp(want), (name, got, want)
    return st


# ---- check 4: refine + reset --------------------------------------------------------------------------------------------------------
def _size_footprint(tree):
    """GP:516-518, 655-657 with capacity = size: a lower bound of the reference's approxMemoryFootprint (a vector's capacity is at most
    twice its size, so twice this is an upper bound).  Interior S-tree nodes hold two one-node trees."""
    n_int = len(tree["axis"]) - tree["n_leaves"]
    nodes = int(tree["sampling"]["num_nodes"].sum()) + int(tree["building"]["num_nodes"].sum()) + 2 * n_int
    return nodes * 24 + len(tree["axis"]) * 2 * 40


def check_refine_reset(e, ref, props, final, seen=None):
    before = e.read_sdtree()
    spp, thr0 = props.get("sppPerPass", 4), props.get("sTreeThreshold", 12000)
    thr = int(np.sqrt(2.0 ** int(before["iter"]) * spp / 4) * thr0)  # GP:1111, evaluated in double and truncated
    cap = props.get("sdTreeMaxMemory", -1)
    if cap < 0:
        caps = [-1]
    elif cap == 0:
        caps = [0]
    else:  # the reference's footprint counts vector capacities, which arrays cannot carry: decided where the bounds decide it
        f = _size_footprint(before)
        caps = [0] if f // 1000000 >= cap else [-1] if (2 * f) // 1000000 < cap else [0, -1]
        if seen is not None:
            seen.setdefault("cap", []).append("stops" if caps == [0] else "refines" if caps == [-1] else "undecided")
    e.begin_iteration(final)
    after = e.read_sdtree()
    ok = []
    for c in caps:
        ref.load(before)
        ref.refine_reset(thr, c, 20, props.get("dTreeThreshold", 0.01))
        r = ref.read()
        same = (np.array_equal(after["axis"], r["axis"]) and np.array_equal(after["children"], r["children"])
                and np.array_equal(after["building"]["num_nodes"], r["building"]["num_nodes"])
                and np.array_equal(after["building"]["node_children"], r["building"]["node_children"])
                and np.array_equal(after["building"]["max_depth"], r["building"]["max_depth"])
                and np.array_equal(after["building"]["stat_weight"].astype(np.float32), r["building"]["stat_weight"])
                and np.array_equal(_bits(after["theta"]), _bits(r["theta"]))
                and np.array_equal(after["sampling"]["node_children"], r["sampling"]["node_children"])
                and np.array_equal(_bits(after["sampling"]["node_sums"]), _bits(r["sampling"]["node_sums"])))
        ok.append(same)
    if not any(ok):
        assert np.array_equal(after["children"], r["children"]), "S-tree topology differs from the reference's refine"
        assert np.array_equal(after["axis"], r["axis"])
        assert np.array_equal(after["building"]["num_nodes"], r["building"]["num_nodes"]), "D-tree node counts differ from the reference's reset"
        assert np.array_equal(after["building"]["node_children"], r["building"]["node_children"]), "D-tree numbering differs from the reference's reset"
        assert np.array_equal(after["building"]["max_depth"], r["building"]["max_depth"])
        assert np.array_equal(after["building"]["stat_weight"].astype(np.float32), r["building"]["stat_weight"]), "statistical weights differ"
        assert np.array_equal(_bits(after["theta"]), _bits(r["theta"])), "inherited theta differs"
        assert False, "sampling trees differ after refine"
    return before, after


def drive(kind, oracle_lib, scene, props, budget, seed):
    """One render, phase by phase, every check at every iteration boundary.  Returns what was seen."""
    props = dict(props, budget=budget, seed=seed)
    e, ref, rng = _engine(kind, oracle_lib, **props), R.Ref(), np.random.RandomState(seed)
    log0 = ref.log_calls()  # (the counter belongs to the library, which the tests of a process share)
    e.set_scene(scene)
    e.begin_render()
    spp = props.get("sppPerPass", 4)
    passes, it, done = int(np.ceil(budget / spp)), 0, 0
    seen = dict(flagged=[], sample_err=[], leaves=[], depth=[], dark=False)
    while done < passes:
        p = min(passes - done, 1 << it)
        if passes - done - p < 2 * p:
            p = passes - done
        final = p >= passes - done
        before, after = check_refine_reset(e, ref, props, final, seen)
        ref.load(after)
        seen["flagged"].append(check_pdf(e, ref, after, rng, seen))
        seen["sample_err"].append(check_sample(e, ref, after, rng, seed + it))
        check_sample_ties(e, ref, after, seen)
        e.set_do_nee(props.get("nee", "never") == "always" or (props.get("nee") == "kickstart" and done * spp < 128))  # GP:1331-1340
        e.render_passes(p)
        st = check_build(e, ref)
        seen["leaves"].append(int(st.n_leaves)); seen["depth"].append(int(st.max_depth))
        e.end_iteration()
        done += p; it += 1
    # the final sampling trees once more (built from the last iteration's statistics)
    t = e.read_sdtree()
    ref.load(t)
    seen["flagged"].append(check_pdf(e, ref, t, rng, seen))
    seen["sample_err"].append(check_sample(e, ref, t, rng, seed + 99))
    e.end_render()
    assert ref.log_calls() == log0, "an SAssert of the reference's text fired"
    print("\n[%s] leaves %s, max D-tree depth %s, flagged share of the random pdf queries %s (limit 0.01), max |direction error| %.3g (limit %.3g), "
          "edge queries excused by the flag: %s, samples tying with a boundary: %d" % (kind, seen["leaves"], seen["depth"], ["%.5f" % f for f in seen["flagged"]], max(seen["sample_err"]),
                                                     R.SINCOS_TOL, {k: v for k, v in seen["edge_flagged"].items() if v}, seen.get("ties", 0)))
    return seen


@needs_ref
@pytest.mark.parametrize("kind", ENGINES)
@pytest.mark.parametrize("preset", ["improved", "boxbox"])
def test_cbox_sdtree_against_reference_classes(oracle_lib, kind, preset):
    import ppg_host
    extra, budget = (IMPROVED, 31) if preset == "improved" else (BOXBOX, 60)
    seen = drive(kind, oracle_lib, ppg_host.cbox_scene(96, 96), dict(CBOX_PROPS, **extra), budget, 7)
    assert seen["dark"] and max(seen["leaves"]) >= 4 and max(seen["depth"]) >= 6 and seen.get("ties", 0) >= 1


@needs_ref
@pytest.mark.parametrize("kind", ENGINES)
def test_room_sdtree_against_reference_classes(oracle_lib, kind):
    """Hundreds of S-tree leaves, unbounded path depth, glossy materials."""
    import ppg_host
    scene = ppg_host.room_scene(96, 54, n_boxes=60, tess=2, glossy=True)
    props = dict(budgetType="spp", maxDepth=-1, rrDepth=5, strictNormals=1, **IMPROVED)
    seen = drive(kind, oracle_lib, scene, props, 63, 17)
    assert max(seen["leaves"]) >= 100 and max(seen["depth"]) >= 6 and seen.get("ties", 0) >= 1


@needs_ref
@pytest.mark.parametrize("kind", ENGINES)
@pytest.mark.parametrize("cap", [0, 1])
def test_memory_cap_against_reference_refine(oracle_lib, kind, cap):
    """sdTreeMaxMemory (GP:958-967): 0 never refines; 1 MB refines while the trees are small and stops once they are not.  The reference's
    footprint counts vector capacities, which trees loaded from arrays do not carry; capacity lies between size and twice the size, so the
    decision is known wherever both bounds fall on the same side of the cap — the scene is chosen so that both decided cases occur (it grows to
    256 leaves of ~200 nodes: ~2.5 MB by size alone) — and there the engine must do exactly what the reference does with that decision.  An
    iteration between the bounds may go either way and is reported as undecided."""
    import ppg_host
    seen = drive(kind, oracle_lib, ppg_host.cbox_scene(48, 48), dict(CBOX_PROPS, sTreeThreshold=200, sdTreeMaxMemory=cap), 124, 2)
    print("memory cap %d MB: per iteration %s, leaves %s" % (cap, seen.get("cap"), seen["leaves"]))
    if cap == 0:
        assert max(seen["leaves"]) == 1
    else:
        assert "refines" in seen["cap"] and "stops" in seen["cap"], seen["cap"]
        first_stop = seen["cap"].index("stops")
        assert len(set(seen["leaves"][first_stop - 1:])) == 1 and seen["leaves"][first_stop - 1] > 1, "the S-tree grew after the cap was reached"


@needs_ref
@pytest.mark.parametrize("kind", ENGINES)
def test_dtree_depth_limit_against_reference_reset(oracle_lib, kind):
    """A subdivision threshold small enough that DTree::reset runs into newMaxDepth = 20 (GP:487)."""
    import ppg_host
    from test_oracle_known_answers import _floor_and_lamp
    # a tiny lamp high above a floor patch seen through a very narrow camera, lit by next-event estimation: the energy of a D-tree sits in one
    # cell level after level (lamp and patch subtend ~1e-8 of the sphere: a cell of depth ~13; rho = 2e-5 then subdivides 7 levels further)
    scene = _floor_and_lamp(32, lamp_half=0.0005, lamp_h=10.0)
    scene.emitters = [dict(radiance=(1e8, 1e8, 1e8))]  # irradiance of order 1 at the floor: well above the 2^-24 quantum of the accumulators
    scene.camera = ppg_host.perspective_camera((0.0, 30.0, 0.0), (0.0, 0.0, 0.0), (0, 0, 1), 0.01, "x", 0.1, 100.0, 32, 32)
    seen = drive(kind, oracle_lib, scene, dict(CBOX_PROPS, dTreeThreshold=DEEP_THRESHOLD, directionalFilter="nearest", nee="kickstart", sTreeThreshold=100000), 124, 5)
    assert max(seen["depth"]) == 20


DEEP_THRESHOLD = 2e-5


# ---- check 5: the optimiser's arithmetic ---------------------------------------------------------------------------------------------
def _read_i64(kind, ptr, n):
    """n 64-bit words at ptr: device memory of the HIP engine, host memory of the oracle"""
    if n == 0:
        return np.zeros(0, np.int64)
    if kind == "hip":
        import torch
        from ppg_host.distributed import _view
        v = _view(torch, ptr, n, "<i8", torch.device("cuda", 0)).clone()
        torch.cuda.synchronize()
        return v.cpu().numpy()
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int64)), shape=(int(n),)).copy()


def _nudge(a, rng):
    """every finite float moved by one ulp, up or down by a fixed pseudo-random sign"""
    a = np.ascontiguousarray(a, np.float32)
    sign = rng.randint(0, 2, a.shape) * 2 - 1
    moved = np.nextafter(a, np.where(sign > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    return np.where(np.isfinite(a), moved, a).astype(np.float32)


STATE_FIELDS = ("theta", "iter", "firstMoment", "secondMoment", "batchGradient", "batchAccumulation")


def drive_optimiser(kind, oracle_lib, scene, props, budget, seed, defer_depth=None):
    """Per round and per leaf: the leaf's records, in key order, through DTreeWrapper::optimizeBsdfSamplingFraction / AdamOptimizer of the
    reference, from the state the engine reported after the previous round; compared with the state the engine reports after this one.
    Arithmetic on given inputs in a given order: the schedule (which records a round holds, stragglers one round late) is the engine's."""
    props = dict(props, budget=budget, seed=seed)
    loss = {"kl": 1, "var": 2}[props["bsdfSamplingFractionLoss"]]
    e, ref = _engine(kind, oracle_lib, **props), R.Ref()
    log0 = ref.log_calls()
    if defer_depth is not None:
        e._call("debug_set_defer_depth", C.c_int32(defer_depth))
    e.set_scene(scene)
    e.begin_render()
    rounds, cur = [], {}

    def hook():  # a world of one owner (include/ppg.h "Sharded optimiser"): phase 0 hands the records over in key order, phase 1 the state
        if e.hook_phase() == 0:
            ptr, counts = e.adam_records_by_owner(1)
            cur["recs"] = _read_i64(kind, ptr, 4 * counts[0]).reshape(-1, 4)
        else:
            ptr, seg = e.adam_state(1)
            rounds.append((cur.pop("recs"), _read_i64(kind, ptr, 3 * seg).view(np.uint32).reshape(-1, 6).copy()))
    e.set_pass_hook(hook)
    spp = props.get("sppPerPass", 4)
    passes, it, done = int(np.ceil(budget / spp)), 0, 0
    state = np.zeros((1, 6), np.uint32)
    scale = np.zeros(6)       # s: the reference's own conditioning, maximum over rounds and leaves
    worst = np.zeros(6)       # |engine - reference| / (4 s + 1 ulp), maximum
    worst_ulp = np.zeros(6)   # |engine - reference| in ulps of the reference's value, maximum (printed only)
    n_rounds = n_replays = n_deferred = n_steps = n_flipped = 0
    while done < passes:
        p = min(passes - done, 1 << it)
        if passes - done - p < 2 * p:
            p = passes - done
        final = p >= passes - done
        before = e.read_sdtree()
        thr = int(np.sqrt(2.0 ** int(before["iter"]) * spp / 4) * props.get("sTreeThreshold", 12000))
        ref.load(before, adam=state)
        ref.refine_reset(thr, -1, 20, props.get("dTreeThreshold", 0.01))
        state = ref.read()["adam"]  # subdivided leaves inherit the whole optimiser (GP:890)
        e.begin_iteration(final)
        after = e.read_sdtree()
        assert np.array_equal(after["children"], ref.read()["children"])
        is_leaf = (after["children"] == 0).all(1)
        assert np.array_equal(_bits(after["theta"])[is_leaf], state[is_leaf, 0])
        del rounds[:]
        e.render_passes(p)
        for recs, st in rounds:
            n_rounds += 1
            assert len(st) >= len(state)
            keys = recs[:, 0].view(np.uint64)
            assert (keys[1:] > keys[:-1]).all()  # key order, keys unique
            leaf = (keys >> np.uint64(40)).astype(np.int64)
            n_deferred += int((((keys >> np.uint64(13)) & np.uint64(1 << 26)) != 0).sum())
            vals = np.ascontiguousarray(recs[:, 1:]).view(np.float32).reshape(-1, 6)[:, :5]
            touched = np.zeros(len(state), bool)
            touched[np.unique(leaf)] = True
            quiet = is_leaf & ~touched
            assert np.array_equal(st[:len(state)][quiet], state[quiet]), "a leaf without records changed its optimiser state"
            starts = np.flatnonzero(np.r_[True, leaf[1:] != leaf[:-1]]) if len(leaf) else np.zeros(0, np.int64)
            ends = np.r_[starts[1:], len(leaf)]
            replays = []
            for a, b in zip(starts, ends):
                l, r = int(leaf[a]), vals[a:b]
                assert is_leaf[l]
                runs = [ref.adam_replay(state[l], r, loss)]
                for k in (1, 2):  # the same records twice more, every float input moved by +-1 ulp (fixed pseudo-random signs)
                    rng = np.random.RandomState(1000 * k + l % 997)
                    s_in = state[l].copy()
                    s_in[[0, 2, 3, 4, 5]] = _nudge(s_in[[0, 2, 3, 4, 5]].view(np.float32), rng).view(np.uint32)
                    r_in = _nudge(r, rng)
                    # The statistical weights of a render are 1 / sppPerPass exactly, so batchAccumulation reaches batchSize = 1 EXACTLY and
                    # `> batchSize` (GP:89) sits on its boundary: a weight moved up by an ulp makes the reference take another number of
                    # steps, and the distance between such runs measures the step rule, not rounding (`iter` is asserted exact below).
                    # The signs of the weights are therefore chosen so that the rule is not crossed: pseudo-random if that keeps the step
                    # count, else all down, else all up; a run that still differs in `iter` is left out of s.
                    for w_in in (r_in[:, 4], np.nextafter(r[:, 4], np.float32(-np.inf)), np.nextafter(r[:, 4], np.float32(np.inf))):
                        r_try = r_in.copy()
                        r_try[:, 4] = np.where(np.isfinite(r[:, 4]), w_in, r[:, 4])
                        out = ref.adam_replay(s_in, r_try, loss)
                        acc0, acc1 = float(runs[0][5:6].view(np.float32)[0]), float(out[5:6].view(np.float32)[0])
                        # (same number of steps AND the same residue in the batch: mixed signs can move a step from one record to the next
                        # and still end at the same count — then the accumulation differs by a whole weight, not by ulps)
                        if out[1] == runs[0][1] and abs(acc1 - acc0) <= 1e-3 * float(np.min(np.abs(r[:, 4]))):
                            runs.append(out)
                            break
                    else:
                        n_flipped += 1
                replays.append((l, np.stack(runs)))
                n_replays += 1
                n_steps += int(runs[0][1]) - int(state[l, 1])
            # s of this round, per state field: the largest difference between the reference runs of a leaf, maximum over the leaves
            s_round = np.zeros(6)
            for l, runs in replays:
                v = runs.view(np.float32).astype(np.float64)
                d_ = np.abs(v[:, None, :] - v[None, :, :]).max((0, 1))
                s_round = np.maximum(s_round, np.where(np.isfinite(d_), d_, 0))
            scale = np.maximum(scale, s_round)
            for l, runs in replays:
                assert st[l, 1] == runs[0][1], ("iter", l, int(st[l, 1]), [int(x[1]) for x in runs])
                for f in (0, 2, 3, 4, 5):
                    want = float(runs[0][f:f + 1].view(np.float32)[0])
                    got = float(st[l, f:f + 1].view(np.float32)[0])
                    tol = 4 * s_round[f] + float(R.ulp(np.float32(want)))
                    assert abs(got - want) <= tol, (STATE_FIELDS[f], "leaf", l, "engine", got, "reference", want, "tolerance", tol, "s", s_round[f])
                    worst[f] = max(worst[f], abs(got - want) / tol)
                    worst_ulp[f] = max(worst_ulp[f], abs(got - want) / float(R.ulp(np.float32(want))))
            state = st[:len(state)].copy()
        e.build_sdtree()
        e.end_iteration()
        done += p; it += 1
    e.end_render()
    assert ref.log_calls() == log0, "an SAssert of the reference's text fired"
    print("\n[%s] optimiser: %d rounds, %d leaf replays, %d Adam steps, %d deferred records, %d nudged runs left out of s (their steps fell on other records whatever the weights' signs); reference conditioning s = %s; worst |engine - reference| / (4 s + 1 ulp) = %s, in ulps of the value = %s"
          % (kind, n_rounds, n_replays, n_steps, n_deferred, n_flipped, {STATE_FIELDS[f]: "%.3g" % scale[f] for f in (0, 2, 3, 4, 5)},
             {STATE_FIELDS[f]: "%.3g" % worst[f] for f in (0, 2, 3, 4, 5)}, {STATE_FIELDS[f]: "%.3g" % worst_ulp[f] for f in (0, 2, 3, 4, 5)}))
    return dict(rounds=n_rounds, replays=n_replays, steps=n_steps, deferred=n_deferred, scale=scale, worst=worst, left_out=n_flipped)


@needs_ref
@pytest.mark.parametrize("kind", ENGINES)
@pytest.mark.parametrize("case", ["kl", "var", "stragglers"])
def test_optimiser_against_reference_adam(oracle_lib, kind, case):
    """Check 5.  `iter` exact; theta, both moments, batchGradient, batchAccumulation within 4 s + 1 ulp of the reference's replay, s = the
    reference's own conditioning per round (drive_optimiser: the same records twice more with every float input moved by +-1 ulp, the signs of
    the weights chosen so that `batchAccumulation > batchSize` is not crossed, because render weights are exactly 1 / sppPerPass and sit on it).
    Measured s, maximum over the rounds of each case (oracle and HIP engine give the same figures):
      kl          CBOX 96^2, improved preset (sppPerPass 1, weights 1):   theta 3.6e-7, firstMoment 4.8e-7, secondMoment 9.5e-7,
                  batchGradient 2.4e-6, batchAccumulation 6.0e-8;  engine at most 0.24 of the tolerance, 1 ulp in theta
      var         CBOX 96^2, box / box preset (sppPerPass 4, fractional weights): theta 4.8e-7, firstMoment 1.5e-4, secondMoment 1.6e-2,
                  batchGradient 4.6e-5, batchAccumulation 1.2e-7;  engine at most 0.24 of the tolerance, 1 ulp in theta
      stragglers  room 96x54, unbounded depth, straggler depth 8 (94 071 deferred records, 61 241 steps): theta 4.8e-7, firstMoment 1.4e-6,
                  secondMoment 2.9e-6, batchGradient 5.7e-6, batchAccumulation 6.0e-8;  engine at most 0.23 of the tolerance, 2 ulp in theta
    Maximum over the scenes: theta 4.8e-7, firstMoment 1.5e-4, secondMoment 1.6e-2, batchGradient 4.6e-5, batchAccumulation 1.2e-7."""
    import ppg_host
    if case == "kl":
        out = drive_optimiser(kind, oracle_lib, ppg_host.cbox_scene(96, 96), dict(CBOX_PROPS, **IMPROVED), 31, 7)
    elif case == "var":
        out = drive_optimiser(kind, oracle_lib, ppg_host.cbox_scene(96, 96), dict(CBOX_PROPS, **BOXBOX), 60, 7)
    else:  # paths deeper than the (lowered) straggler depth hand their records in one round late: their place in the key order is replayed too
        scene = ppg_host.room_scene(96, 54, n_boxes=60, tess=2, glossy=True)
        props = dict(budgetType="spp", maxDepth=-1, rrDepth=3, strictNormals=1, **IMPROVED)
        out = drive_optimiser(kind, oracle_lib, scene, props, 63, 29, defer_depth=8)
        assert out["deferred"] > 1000, "the test needs stragglers"
    assert out["rounds"] >= 4 and out["steps"] > 100


# ---- check 6: the splat, CPU only (the engines take records only through a render; the kernels are bit-equal to the oracle on node_fixed) -------
def _slot_cells(children):
    """(node, quadrant) -> (origin x, origin y, size) for every slot of a quadtree"""
    out, stack = {}, [(0, 0.0, 0.0, 1.0)]
    while stack:
        k, x, y, s = stack.pop()
        h = s / 2
        for j in range(4):
            ox, oy = x + (h if j & 1 else 0), y + (h if j & 2 else 0)
            out[(k, j)] = (ox, oy, h)
            if children[k, j]:
                stack.append((int(children[k, j]), ox, oy, h))
    return out


def _depth_at(children, x, y):
    node, d = 0, 0
    while True:
        d += 1
        i = (1 if x >= 0.5 else 0) | (2 if y >= 0.5 else 0)
        x, y = (x * 2 if x < 0.5 else (x - 0.5) * 2), (y * 2 if y < 0.5 else (y - 0.5) * 2)
        if children[node, i] == 0:
            return d
        node = children[node, i]


def _splat_inputs():
    rng = np.random.RandomState(11)
    xy = np.clip(np.concatenate([rng.normal([0.7, 0.2], 0.03, (6000, 2)), rng.rand(2000, 2)]), 0, 0.999999)
    cases = {"peaked": (xy, rng.uniform(0.5, 1.5, len(xy)), np.ones(len(xy)))}  # test_dtree_pdf_integrates_to_one_and_matches_samples
    rng = np.random.RandomState(2)
    xy = rng.uniform(0.3, 0.7, (3000, 2))
    cases["interior"] = (xy, rng.uniform(0.5, 1.5, len(xy)), np.ones(len(xy)))  # test_dtree_box_filter_conserves_interior_energy
    b = np.float32([[0, 0], [1, 1], [0, 1], [1, 0], [0.5, 0.5], [0.5, 0], [0, 0.5], [1, 0.5], [0.25, 0.75], [0.001, 0.001], [0.9995, 0.9999], [0.999999, 0.5]])
    xy = np.concatenate([np.tile(b, (40, 1)), rng.rand(500, 2)])
    cases["borders and corners"] = (xy, rng.uniform(0.5, 1.5, len(xy)), rng.uniform(0.25, 2.0, len(xy)))
    xy = rng.rand(600, 2)
    irr, w = rng.uniform(0.5, 1.5, 600).astype(np.float32), rng.uniform(0.25, 2.0, 600).astype(np.float32)
    irr[0:40:4], irr[1:40:4], irr[2:40:4], irr[3:40:4] = 0, -1, np.nan, np.inf   # the guards of GP:395-399
    w[40:80:4], w[41:80:4], w[42:80:4], w[43:80:4] = 0, -1, np.nan, np.inf
    w[80:84], irr[80:84] = -np.inf, -np.inf
    cases["guards"] = (xy, irr, w)
    return cases


@needs_ref
@pytest.mark.parametrize("dfilter", [0, 1], ids=["nearest", "box"])
@pytest.mark.parametrize("case", ["peaked", "interior", "borders and corners", "guards"])
def test_oracle_splat_against_reference_record(oracle_lib, case, dfilter):
    ref = R.Ref()
    log0 = ref.log_calls()  # (the counter belongs to the library, which other tests of this process share)
    xy, irr, w = _splat_inputs()[case]
    q = np.random.RandomState(4).rand(2000, 2).astype(np.float32)
    q[:8] = [[0, 0], [1, 1], [0.5, 0.5], [1, 0], [0, 1], [0.25, 0.5], [0.999999, 0.999999], [0.5, 1]]
    r = R.exercise(ref.lib.ppgr_dtree_exercise, 1, dfilter, xy, irr, w, q)
    a = R.exercise(oracle_lib.ppgo_dtree_exercise, 1, dfilter, xy, irr, w, q)  # the oracle's float accumulation, same order: bit-equal
    assert a["n"] == r["n"] and np.array_equal(a["children"], r["children"])
    assert np.array_equal(_bits(a["sums"]), _bits(r["sums"])), np.abs(a["sums"] - r["sums"]).max()
    assert _bits(np.float32([a["statw"], a["total"]])).tolist() == _bits(np.float32([r["statw"], r["total"]])).tolist()
    assert np.array_equal(_bits(a["pdf"]), _bits(r["pdf"])) and np.array_equal(_bits(a["samples"]), _bits(r["samples"]))
    f = R.exercise(oracle_lib.ppgo_dtree_exercise, 0, dfilter, xy, irr, w, q)  # 2^-24 fixed point: what the kernels use
    assert f["n"] == r["n"] and np.array_equal(f["children"], r["children"])
    # per slot |delta| <= (records touching it) * 2^-25 [our quantisation, half a step per addend] + n * 2^-24 * slot sum [the reference's
    # float accumulation of n addends, each rounding to at most half an ulp of a partial sum <= the slot sum, doubled for the two roundings of
    # irradiance * weight (* overlap)]: derived, not measured
    xf, wf, irf = np.float32(xy).astype(np.float64), np.float32(w), np.float32(irr)
    live = np.isfinite(wf) & (wf > 0) & np.isfinite(irf) & (irf > 0)
    px, py = xf[live, 0], xf[live, 1]
    if dfilter:
        half = np.array([0.5 ** _depth_at(r["children"], np.float32(x), np.float32(y)) for x, y in zip(px, py)]) / 2
    n = int(live.sum())
    for (k, j), (ox, oy, s) in _slot_cells(r["children"]).items():
        if dfilter:
            touch = int(((np.minimum(px + half, ox + s) > np.maximum(px - half, ox)) & (np.minimum(py + half, oy + s) > np.maximum(py - half, oy))).sum())
        else:
            touch = int(((px >= ox) & (px <= ox + s) & (py >= oy) & (py <= oy + s)).sum())
        bound = touch * 2.0 ** -25 + n * 2.0 ** -24 * float(r["sums"][k, j])
        assert abs(float(f["sums"][k, j]) - float(r["sums"][k, j])) <= bound, (k, j, f["sums"][k, j], r["sums"][k, j], bound, touch)
    assert ref.log_calls() == log0, "an SAssert of the reference's text fired"


# ---- the reference's text stays out of the repository ------------------------------------------------------------------------------
def test_nothing_of_the_reference_is_tracked():
    git = subprocess.run(["git", "-C", ROOT, "ls-files", "oracle/_ref"], capture_output=True, text=True)
    if git.returncode != 0:
        pytest.skip("not a git checkout")
    assert git.stdout.strip() == ""
    tracked = subprocess.run(["git", "-C", ROOT, "ls-files", "oracle/ref_sdtree"], capture_output=True, text=True).stdout.split()
    on_disk = [os.path.relpath(os.path.join(d, f), ROOT) for d, _, fs in os.walk(os.path.join(ROOT, "oracle", "ref_sdtree")) for f in fs]
    if not os.path.isfile(R.REFERENCE_SRC):
        return
    src = open(R.REFERENCE_SRC, encoding="utf-8", errors="replace").read().splitlines()
    b = next(i for i, l in enumerate(src) if l.startswith("MTS_NAMESPACE_BEGIN"))
    en = next(i for i, l in enumerate(src) if l.startswith("static StatsCounter avgPathLength"))

    def norm(lines):  # non-trivial lines: more than braces, blanks and one-word lines
        out = ["".join(l.split()) for l in lines]
        return [l for l in out if len(l) >= 12 and not l.startswith("#include")]
    ext = norm(src[b:en])
    runs = {tuple(ext[i:i + 3]) for i in range(len(ext) - 2)}
    for f in sorted(set(tracked) | set(on_disk)):
        mine = norm(open(os.path.join(ROOT, f), encoding="utf-8", errors="replace").read().splitlines())
        hits = [mine[i:i + 3] for i in range(len(mine) - 2) if tuple(mine[i:i + 3]) in runs]
        assert not hits, (f, hits[:2])


# ---- include/ppg.h "Limits": a round's paths must fit below PPG_ADAM_DEFER_PATH_BIT -------------------------------------------------
def _limit_case(make, spp, loss):
    import ppg_host
    from ppg_host.bindings import PPGError
    e = make(sppPerPass=spp, budget=spp, maxDepth=2, **({"bsdfSamplingFractionLoss": loss} if loss else {}))
    try:
        e.set_scene(ppg_host.cbox_scene(1024, 1024))
    except PPGError as ex:
        return str(ex)
    finally:
        e.close()
    return None


def _limit_checks(make, can_hold_2_26_paths):
    msg = _limit_case(make, 65, "kl")  # 1024 * 1024 * 65 > 2^26: refused before anything of that size is allocated
    assert msg is not None and "2^26" in msg and "67108864" in msg, msg
    msg = _limit_case(make, 128, "var")  # between 2^26 and the former limit 2^27: bit 26 of the path field is the straggler flag
    assert msg is not None and "2^26" in msg, msg
    msg = _limit_case(make, 64, "kl")  # exactly 2^26: accepted by the check (the HIP engine then sizes buffers for 2^26 paths, which may fail on its own)
    assert msg is None or ("2^26" not in msg and not can_hold_2_26_paths), msg


def test_round_path_limit_oracle(oracle_lib):
    _limit_checks(lambda **p: make_oracle(oracle_lib, **dict(CBOX_PROPS, **p)), True)
    assert _limit_case(lambda **p: make_oracle(oracle_lib, **dict(CBOX_PROPS, **p)), 65, None) is None  # no loss, no keys, no limit


@pytest.mark.gpu
def test_round_path_limit_hip():
    import ppg_host
    _limit_checks(lambda **p: ppg_host.Engine.hip(**dict(CBOX_PROPS, **p)), False)
