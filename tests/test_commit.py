"""Explicit vertices through the oracle's commit (ppgo_debug_commit) against the exact restatement of tests/commit_ref.py, on the CPU.

Per spatial filter x directional filter x loss x statistical weight the oracle grows the tree of tests/commit_cases.py, then every case is
committed through the hook and the building sums, the statistical weights, the committed count and the optimiser's records must EQUAL
the restatement's — integers and float bit patterns.  The HIP engine is held to both in tests/test_commit_gpu.py.

Conservation (float64, pins the restatement itself), with the bound per sum
    addends * 2^-25  +  K * 2^-24 * sum
K = the float32 roundings on the longest expression that ends in an addend.  Nearest directional filter: radiance / throughput (1), the two
additions of Spectrum::average (2), the float constant 1/3 and the product with it (2), / woPdf (1), * statisticalWeight (1): K = 7.
Box spatial filter, weights: the volume's two products (2), weight / volume (1), the two products of the three overlap lengths (2), the
product with the weight (1) and, per length, the roundings of p -+ voxel / 2 and of the node's corner additions, each of at most half an ulp
of a coordinate of magnitude |x| <= c relative to a length of at least the voxel's side s: 3 * 4 * (c / s) halves of an ulp:
K = 6 + 6 * c / s, evaluated per vertex.
"""
import numpy as np
import pytest

import commit_cases as cc
import commit_ref as cr
from conftest import make_oracle

K_NEAREST = 7


@pytest.fixture(scope="module")
def orc(oracle_lib):
    return cc.Oracle(oracle_lib)


_grown = {}


def grown(oracle_lib, ctx):
    """The oracle with the module's tree in an open iteration, one per context for the whole module."""
    if ctx not in _grown:
        o = make_oracle(oracle_lib, threads=8, **cc.props(*ctx))
        cc.grow(o, ctx[3])
        t = o.read_sdtree()
        cc.assert_shape(t)
        _grown[ctx] = (o, t, cr.Tree(t))
    return _grown[ctx]


def cases(t, orc, tree):
    rng = np.random.default_rng(2024)
    yield "guards", cc.case_guards(t, orc, rng)
    yield "directions", cc.case_directions(t, orc, rng)
    yield "positions", cc.case_positions(t, orc, rng)
    yield "one path", cc.case_random(t, orc, rng, 1)
    yield "three paths", cc.case_random(t, orc, rng, 3)
    yield "1000 paths", cc.case_random(t, orc, rng, 1000, mean_nv=1.0)
    for k in (1, 3, 4, 64):
        yield "wave of %d leaves" % k, cc.case_wave_leaves(t, orc, rng, k)
    yield "inf product", cc.case_inf_product(t, orc, rng)  # (last: it leaves a NaN in its leaf's optimiser)


def check(o, t, tree, cfg, c, orc):
    before, state = o.read_sdtree(), cc.state(o)
    got = cc.call(o, "commit", c)
    fx, w = cc.delta(before, o.read_sdtree())
    res = cr.commit(tree, cfg, c, orc.to_canonical)
    efx, ew = cc.expected_arrays(res, t)
    assert got["committed"] == res.committed
    assert np.array_equal(w, ew), np.flatnonzero(w != ew)[:8]
    assert np.array_equal(fx, efx), np.argwhere(fx != efx)[:8]
    rec = got["records"]
    assert len(rec) == len(res.records)
    exp = np.zeros(len(res.records), rec.dtype)
    for j, r in enumerate(res.records):
        exp[j] = (r[0], r[1], r[2], r[3], r[4], r[5], 0.0)
    assert rec.tobytes() == exp.tobytes()
    assert np.array_equal(got["keys"], exp["key"])
    untouched = np.ones(len(state), bool)
    untouched[[r[0] >> cr.LEAF_SHIFT for r in res.records]] = False
    assert np.array_equal(got["adam_state"][untouched], state[untouched])  # leaves without records keep their optimiser's state
    assert cfg["loss"] or untouched.all()
    return res


@pytest.mark.parametrize("spatial,directional,loss,weight", cc.contexts())
def test_oracle_equals_restatement(oracle_lib, orc, spatial, directional, loss, weight):
    o, t, tree = grown(oracle_lib, (spatial, directional, loss, weight))
    cfg = dict(spatial=spatial, directional=directional, loss=loss != "none", weight=weight)
    for name, c in cases(t, orc, tree):
        res = check(o, t, tree, cfg, c, orc)
        if name.startswith("wave of") and spatial == "nearest":  # both sides of wave_key_add<3>'s third round, and the full wave
            k = int(name.split()[2])
            assert len({s["leaf"] for s in res.splats}) == k
            assert cr.commit_wave_arms(res, c, 64) == ({"equal"} if k <= 3 else {"equal", "direct"}), name
        if spatial == "box":  # a voxel centred in its leaf lies inside it; the random vertices' voxels span many leaves
            n = cc.leaves_per_vertex(res)
            if name.startswith("wave of"):
                # (inside up to rounding: the centre and the node corners are rounded to an ulp of a coordinate, |x| <= 2^11 here, so a face may
                # leave a sliver of at most 4 ulps = 2^-10 with the neighbours, against a voxel side of at least extent / 2^7 > 2^3: a share
                # of 2^-13 per face, three faces)
                share, total = {}, {}
                for sp in res.splats:
                    share[sp["vertex"]] = max(share.get(sp["vertex"], 0.0), sp["w64"])
                    total[sp["vertex"]] = total.get(sp["vertex"], 0.0) + sp["w64"]
                assert all(share[v] >= total[v] * (1 - 3 * 2.0 ** -13) for v in share), name
                assert float(max(abs(x) for x in tree.mn + tree.mx)) <= 2 ** 11 and min(float(min(tree.lookup(q)[1])) for q in c["p"]) > 2 ** 3
            if name == "1000 paths":
                assert max(n.values()) >= 8 and min(n.values()) >= 1, (min(n.values()), max(n.values()))


@pytest.mark.parametrize("spatial", cc.SPATIAL)
def test_conservation_nearest_directional_filter(oracle_lib, orc, spatial):
    """Sum of the slots of a D-tree = sum of irradiance * weight of its live records, in float64."""
    o, t, tree = grown(oracle_lib, (spatial, "nearest", "kl", 1.0))
    rng = np.random.default_rng(5)
    c = cc.case_random(t, orc, rng, 1000, mean_nv=1.0)
    res = cr.commit(tree, dict(spatial=spatial, directional="nearest", loss=True, weight=1.0), c, orc.to_canonical)
    want, addends = {}, {}
    for s in res.splats:
        if s["live"]:
            want[s["leaf"]] = want.get(s["leaf"], 0.0) + s["irr64"] * s["w64"]
            addends[s["leaf"]] = addends.get(s["leaf"], 0) + 1
    have = {}
    for (leaf, _, _), v in res.fixed.items():
        have[leaf] = have.get(leaf, 0) + v
    assert set(have) == set(want) and len(want) > 20
    for leaf, x in want.items():
        assert addends[leaf] == res.n_addends[leaf]
        k = K_NEAREST + (6 if spatial == "box" else 0)  # (box spatial filter: the weight is w / volume * overlap, six more roundings; its lengths below)
        bound = addends[leaf] * 2.0 ** -25 + k * 2.0 ** -24 * x
        if spatial == "box":
            bound += x * 2.0 ** -24 * 6 * 2 ** 8  # c / s <= 2^8: |coordinate| / extent < 2 in the CBOX, voxels of at least extent / 2^7
        assert abs(have[leaf] / 16777216.0 - x) <= bound, (leaf, have[leaf] / 16777216.0, x, bound)


K_BOX = K_NEAREST + 5


@pytest.mark.parametrize("spatial", ("nearest", "stochastic"))
def test_conservation_box_directional_filter(oracle_lib, orc, spatial):
    """A box footprint inside the unit square hands irradiance * weight out whole: per record, the sum of its additions = irradiance *
    weight in float64.  K: the seven roundings of the nearest filter's value, the division by size^2 (1), per overlap the two subtractions
    that give its side lengths, their product and the product with the value (4): K = 12 = K_BOX.  Beyond K the footprint itself is
    rounded: origin = p - size / 2 by at most 2^-25 and origin + size by at most 2^-24 per axis (|p| <= 1), against a side of
    size = 2^-depth — the footprint's area, and with it the sum, is off by at most 2 * 1.5 * 2^-24 / size relative, taken as 4 * 2^(depth - 24).
    Records within 2^-22 of a cell border of their D-tree (float64 canonical point) are left out."""
    import math
    o, t, tree = grown(oracle_lib, (spatial, "box", "kl", 1.0))
    rng = np.random.default_rng(9)
    c = cc.case_random(t, orc, rng, 1000, mean_nv=1.0)
    res = cr.commit(tree, dict(spatial=spatial, directional="box", loss=True, weight=1.0), c, orc.to_canonical)
    checked = 0
    for s in res.splats:
        if not s["live"] or not s["inside"]:
            continue
        d = [float(x) for x in c["d"][s["vertex"]]]
        x = (min(max(d[2], -1.0), 1.0) + 1) / 2
        phi = math.atan2(d[1], d[0])
        y = (phi + 2 * math.pi if phi < 0 else phi) / (2 * math.pi)
        cell = 2.0 ** -s["depth"]
        if any(min(v % cell, cell - v % cell) < 2.0 ** -22 for v in (x, y)):
            continue
        want = s["irr64"] * s["w64"]
        bound = s["addends"] * 2.0 ** -25 + (K_BOX * 2.0 ** -24 + 4 * 2.0 ** (s["depth"] - 24)) * want
        assert abs(s["fixed_sum"] / 16777216.0 - want) <= bound, (s["vertex"], s["depth"], s["addends"], s["fixed_sum"] / 16777216.0, want, bound)
        checked += 1
    assert checked > 400, checked


def test_conservation_box_spatial_filter_weights(oracle_lib, orc):
    """A voxel inside the box hands its statistical weight out whole: the leaves' weights of one record sum to w."""
    o, t, tree = grown(oracle_lib, ("box", "nearest", "kl", 1.0))
    rng = np.random.default_rng(6)
    c = cc.case_random(t, orc, rng, 1000, mean_nv=1.0)
    res = cr.commit(tree, dict(spatial="box", directional="nearest", loss=True, weight=1.0), c, orc.to_canonical)
    inside = [v for v in res.vertex_w64.values() if v[2]]
    assert len(inside) > 100
    bound = max(abs(float(x)) for x in list(tree.mn) + list(tree.mx)) / min(float(min(tree.lookup(p)[1])) for p in c["p"])
    assert bound <= 2 ** 8  # c / s of the module's docstring
    for w, total, _ in inside:
        assert abs(total - w) <= w * 2.0 ** -24 * (6 + 6 * 2 ** 8), (w, total)


def test_unsure_share_of_random_records(oracle_lib, orc):
    """Records whose float64 canonical point lies within 2^-22 of a cell border of their D-tree: at most 1 % of the random cases'."""
    import math
    o, t, tree = grown(oracle_lib, ("nearest", "box", "kl", 1.0))
    rng = np.random.default_rng(7)
    c = cc.case_random(t, orc, rng, 1000, mean_nv=1.0)
    res = cr.commit(tree, dict(spatial="nearest", directional="box", loss=True, weight=1.0), c, orc.to_canonical)
    live = [s for s in res.splats if s["live"]]
    unsure = 0
    for s in live:
        d = [float(x) for x in c["d"][s["vertex"]]]
        x = (min(max(d[2], -1.0), 1.0) + 1) / 2
        phi = math.atan2(d[1], d[0])
        y = (phi + 2 * math.pi if phi < 0 else phi) / (2 * math.pi)
        cell = 2.0 ** -s["depth"]
        unsure += any(min(v % cell, cell - v % cell) < 2.0 ** -22 for v in (x, y))
    assert len(live) > 500 and unsure <= 0.01 * len(live), (unsure, len(live))


def test_refusals_name_the_argument_and_leave_the_context_usable(oracle_lib, orc):
    import ppg_host
    o, t, tree = grown(oracle_lib, ("box", "box", "kl", 1.0))
    rng = np.random.default_rng(8)
    c = cc.case_random(t, orc, rng, 3)
    with pytest.raises(ppg_host.PPGError, match="route"):
        cc.call(o, "records", c)          # the box spatial filter has no known record positions
    with pytest.raises(ppg_host.PPGError, match="route"):
        cc.call(o, 7, c)
    with pytest.raises(ppg_host.PPGError, match="n_vertices"):
        cc.call(o, "commit", c, n_vertices=len(c["wo_pdf"]) + 1)
    o.set_pass_hook(lambda: None)
    with pytest.raises(ppg_host.PPGError, match="round hook"):
        cc.call(o, "commit", c)          # a round hook may replace the round's records
    o.set_pass_hook(None)
    many = dict(c, nv=c["nv"].copy())
    many["nv"][0] = cc.MAX_VERTICES + 1
    with pytest.raises(ppg_host.PPGError, match="nv"):
        cc.call(o, "commit", many, n_vertices=int(many["nv"].sum()))
    fresh = make_oracle(oracle_lib, threads=2, **cc.props("nearest", "nearest", "none", 1.0))
    fresh.set_scene(ppg_host.cbox_scene(8, 8))
    fresh.begin_render()
    with pytest.raises(ppg_host.PPGError, match="begin_iteration"):
        cc.call(fresh, "commit", c)       # outside an iteration
    check(o, t, tree, dict(spatial="box", directional="box", loss=True, weight=1.0), c, orc)


def _chain(depth):
    """An S-tree whose child 0 is split again and again: 2 * depth + 1 nodes, its deepest leaves `depth` levels below the root."""
    ch = np.zeros((2 * depth + 1, 2), np.uint32)
    for k in range(depth):
        ch[2 * k] = (2 * k + 2, 2 * k + 1)
    return ch


def test_the_host_refuses_an_stree_the_box_splat_cannot_walk(hip_lib_path):
    """stree_record_box holds 96 stack entries: the refine step refuses a tree deeper than PPG_STREE_MAX_DEPTH = 94 under the box filter."""
    import ctypes as C
    lib = C.CDLL(hip_lib_path)
    f = lib.ppg_debug_stree_depth
    f.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.c_int32, C.POINTER(C.c_uint32)]

    def ask(ch, sf):
        d = C.c_uint32(0)
        return f(ch.ctypes.data_as(C.POINTER(C.c_uint32)), len(ch), sf, C.byref(d)), d.value

    assert ask(_chain(94), 2) == (0, 94)
    assert ask(_chain(95), 2) == (-5, 95)      # PPG_ERR_NOMEM
    assert ask(_chain(95), 0) == (0, 95) and ask(_chain(300), 1) == (0, 300)
    assert ask(np.zeros((1, 2), np.uint32), 2) == (0, 0)
    bad = _chain(3)
    bad[2] = (1, 9)
    assert ask(bad, 2)[0] == -1                # PPG_ERR_INVALID: a child that is not above its parent, a child beyond the array
