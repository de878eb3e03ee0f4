"""Explicit vertices through the HIP engine's commit and splat kernels (ppg_debug_commit, include/ppg_testhooks.h) against the oracle's
ppgo_debug_commit and the exact restatement of tests/commit_ref.py: equal bits, route by route.

Both engines grow the tree of tests/commit_cases.py (the parity contract makes the two trees equal; asserted), then every case goes through
every route the context admits — k_commit over all paths, k_commit split into ended and late paths, k_commit_records + sort +
k_splat_sorted + k_adam_apply, the same with the late paths through the list launch — and each call must add the same fixed sums and
statistical weights, count the same vertices, leave the same optimiser records in the same order and the same optimiser state in every
leaf header as the oracle; sums, count, records and the keys of the record routes must also be the restatement's.  Which way k_splat_sorted
takes a chunk or run, and which arm of wave_key_add a wave reaches, is derived by the restatement from the keys; a case that does not reach
the branch it was written for fails.

wave_key_add's shuffle reduction (a group of equal keys with DIFFERENT values) is not reachable through any commit route: the kernels that
call it pass the launch's one statistical weight (1 or 0.5) as the value, and the box spatial filter, whose weights differ, adds without
it.  Reached and asserted: the all-equal shortcut and the direct addition of a fourth distinct key.

NaN.  The guards case holds a vertex whose optimiser record has product = inf (radiance 3e38, woPdf 1e-3).  Its Adam step has an infinite
gradient, both moments become inf and the variable lr * inf / (inf + eps) = NaN — on both engines, in the same leaf, after the same step.
The NaN's SIGN differs: k_adam_apply on gfx950 leaves 0x7fc00000, the oracle on x86-64 0xffc00000 (SSE's default NaN has the sign set).
IEEE 754 leaves sign and payload of a generated NaN open and nothing in the project reads them (logistic(NaN) is a NaN either way), so
state_equal() takes a word that is a NaN on both engines as equal; every other word, and every word of every other leaf, is compared by
its bits.  Found by this test on its first run; neither implementation was changed.
"""
import numpy as np
import pytest

import commit_cases as cc
import commit_ref as cr
from conftest import make_oracle
from test_gpu_parity import assert_tree_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc(oracle_lib):
    return cc.Oracle(oracle_lib)


def pair(oracle_lib, ctx):
    import ppg_host
    g, o = ppg_host.Engine.hip(**cc.props(*ctx)), make_oracle(oracle_lib, threads=16, **cc.props(*ctx))
    cc.grow(g, ctx[3]); cc.grow(o, ctx[3])
    tg, to = g.read_sdtree(), o.read_sdtree()
    assert_tree_equal(tg, to)
    assert np.array_equal(tg["building"]["node_fixed"], to["building"]["node_fixed"])
    large = cc.assert_shape(tg)
    return g, o, tg, cr.Tree(tg), large


def expected_records(res, dtype):
    exp = np.zeros(len(res.records), dtype)
    for j, r in enumerate(res.records):
        exp[j] = (r[0], r[1], r[2], r[3], r[4], r[5], 0.0)
    return exp


def state_equal(a, b):
    """The optimiser's state words, bit for bit; a float word that is a NaN on BOTH engines counts as equal whatever its sign and payload
    (module docstring: 'NaN')."""
    fa, fb = a.view(np.float32), b.view(np.float32)
    both_nan = np.isnan(fa) & np.isnan(fb)
    both_nan[:, 1] = False  # (the iteration count is an integer)
    return (a == b) | both_nan


def run_case(g, o, t, tree, cfg, c, orc, routes, lds_nodes=cr.LDS_NODES):
    """One case through `routes` on both engines; -> (restatement, {route: k_splat_sorted routes reached})."""
    res = cr.commit(tree, cfg, c, orc.to_canonical)
    efx, ew = cc.expected_arrays(res, t)
    reached = {}
    for route in routes:
        bg, bo = g.read_sdtree(), o.read_sdtree()
        sg, so = cc.state(g), cc.state(o)
        a, b = cc.call(g, route, c), cc.call(o, route, c)
        fg, wg = cc.delta(bg, g.read_sdtree())
        fo, wo = cc.delta(bo, o.read_sdtree())
        assert a["committed"] == b["committed"] == res.committed, route
        assert np.array_equal(wg, wo) and np.array_equal(wg, ew), (route, np.flatnonzero(wg != ew)[:8])
        assert np.array_equal(fg, fo) and np.array_equal(fg, efx), (route, np.argwhere(fg != efx)[:8])
        assert a["records"].tobytes() == b["records"].tobytes() == expected_records(res, a["records"].dtype).tobytes(), route
        same = state_equal(a["adam_state"], b["adam_state"])
        assert same.all(), (route, np.flatnonzero(~same.all(1))[:8])
        untouched = np.ones(len(sg), bool)  # leaves without records keep their optimiser's state, word for word
        untouched[[r[0] >> cr.LEAF_SHIFT for r in res.records]] = False
        assert np.array_equal(a["adam_state"][untouched], sg[untouched]) and np.array_equal(b["adam_state"][untouched], so[untouched]), route
        assert cfg["loss"] or untouched.all()
        if route.startswith("records"):
            late = c.get("late") if route.endswith("split") else None
            keys, leaf_bits = cr.round_keys(res, c, len(t["axis"]), late=late, max_vertices=cc.MAX_VERTICES)
            valid = np.array([k for k in keys if k != (1 << 64) - 1], np.uint64)
            assert np.array_equal(a["keys"], valid), route
            keys, leaf_bits, weighted = cr.round_keys(res, c, len(t["axis"]), late=late, max_vertices=cc.MAX_VERTICES, with_weights=True)
            reached[route], by_record = cr.splat_routes(keys, leaf_bits, tree.num_nodes, lds_nodes)
            reached[route + " arms"] = cr.record_wave_arms(keys, weighted, leaf_bits, by_record, cr.to_fixed(cfg["weight"]))
        elif cfg["loss"]:
            assert np.array_equal(a["keys"], b["keys"]), route
    return res, reached


def general_cases(t, orc):
    rng = np.random.default_rng(2024)
    yield "guards", cc.case_guards(t, orc, rng)
    yield "directions", cc.case_directions(t, orc, rng)
    yield "positions", cc.case_positions(t, orc, rng)
    yield "one path", cc.case_random(t, orc, rng, 1)
    yield "three paths", cc.case_random(t, orc, rng, 3, late="third")
    yield "1000 paths", cc.case_random(t, orc, rng, 1000, mean_nv=1.0, late="third")
    for k in (1, 3, 4, 64):
        yield "wave of %d leaves" % k, cc.case_wave_leaves(t, orc, rng, k)
    yield "inf product", cc.case_inf_product(t, orc, rng)  # (last: it leaves a NaN in its leaf's optimiser)


@pytest.mark.parametrize("spatial,directional,loss,weight", cc.contexts())
def test_hip_equals_oracle_and_restatement(oracle_lib, orc, spatial, directional, loss, weight):
    g, o, t, tree, _ = pair(oracle_lib, (spatial, directional, loss, weight))
    cfg = dict(spatial=spatial, directional=directional, loss=loss != "none", weight=weight)
    arms = set()
    for name, c in general_cases(t, orc):
        res, _ = run_case(g, o, t, tree, cfg, c, orc, cc.admitted(spatial, loss, weight))
        if spatial != "box":
            arms |= cr.commit_wave_arms(res, c, len(c["nv"]))
        if name.startswith("wave of") and spatial == "nearest":  # k_commit's wave: both sides of wave_key_add<3>'s third round, the full wave
            k = int(name.split()[2])
            assert len({s["leaf"] for s in res.splats}) == k
            assert cr.commit_wave_arms(res, c, 64) == ({"equal"} if k <= 3 else {"equal", "direct"}), name
        if spatial == "box" and name == "1000 paths":  # voxels spanning many leaves (voxels inside one: the waves' leaf centres, tests/test_commit.py)
            assert max(cc.leaves_per_vertex(res).values()) >= 8
    if spatial != "box":
        assert {"equal", "direct"} <= arms, arms  # waves of one leaf and of more than three (the 1000 random paths)


@pytest.mark.parametrize("directional", cc.DIRECTIONAL)
def test_every_route_of_the_sorted_splat(oracle_lib, orc, directional):
    """Record totals of 2048 k - 1, 2048 k, 2048 k + 1 in one run; a run across a chunk border; chunks of exactly 64 and of 65 runs; sparse
    records leaf by leaf; holes at the end; 4096 + 17 paths with every third one late.  The record-by-record chunks are the second caller
    of wave_key_add; a chunk gets there with more than 64 runs in 2048 records, so some wave of 64 consecutive records always meets a fourth
    leaf: of 65 runs of 31 records most waves hold three leaves (the shortcut alone) and the one from record 960 on four, and 65 leaves of
    one record each put 64 distinct leaves into one wave.  Both arms are derived from the sorted keys and asserted."""
    ctx = ("nearest", directional, "kl", 1.0)
    g, o, t, tree, large = pair(oracle_lib, ctx)
    cfg = dict(spatial="nearest", directional=directional, loss=True, weight=1.0)
    rng = np.random.default_rng(11)
    seen = set()
    routes = ("records", "records_split")
    centres = cc.leaf_centres(t)
    small = min(centres, key=lambda l: tree.num_nodes[l])  # (a D-tree the kernel stages: at most 512 nodes)
    assert tree.num_nodes[small] <= cr.LDS_NODES
    for total in (2047, 2048, 2049):
        c = cc.case_one_leaf(t, orc, rng, total, point=centres[small])
        _, r = run_case(g, o, t, tree, cfg, c, orc, ("commit", "records"))
        assert "run count skipped" in r["records"] and ({"staged", "unstaged: large"} & r["records"]), r
        assert ("run continued across chunks" in r["records"]) == (total > 2048), (total, r)
        seen |= r["records"]
    c = cc.case_leaves(t, orc, rng, 64, 32, tree)
    _, r = run_case(g, o, t, tree, cfg, c, orc, ("commit", "records"))
    assert {"runs counted", "exactly 64 runs"} <= r["records"] and "record by record" not in r["records"], r
    seen |= r["records"]
    c = cc.case_leaves(t, orc, rng, 65, 31, tree)
    _, r = run_case(g, o, t, tree, cfg, c, orc, ("commit", "records"))
    assert {"runs counted", "65 runs", "record by record"} <= r["records"], r
    assert r["records arms"] == {"equal", "direct"}, r
    seen |= r["records"]
    c = cc.case_leaves(t, orc, rng, 65, 1, tree)
    _, r = run_case(g, o, t, tree, cfg, c, orc, ("commit", "records"))
    assert "record by record" in r["records"] and r["records arms"] == {"equal", "direct"}, r
    for n, late in ((63, None), (64, "all"), (65, "third"), (4096 + 17, "third")):
        c = cc.case_random(t, orc, rng, n, mean_nv=1.2, late=late)
        _, r = run_case(g, o, t, tree, cfg, c, orc, cc.ROUTES if n < 4096 else routes)
        seen |= r["records"] | r["records_split"]
        if late == "third":  # (the late paths reserve max_vertices positions each)
            assert "holes at the end" in r["records_split"], (n, r)
    want = {"staged", "unstaged: short", "record by record", "run continued across chunks", "holes at the end", "run count skipped", "runs counted"}
    assert want <= seen, want - seen
    assert ("unstaged: large" in seen) == large  # (a tree without a D-tree above 512 nodes: PPG_SPLAT_LDS_NODES=4 below makes them all large)


@pytest.mark.parametrize("switch,value", [("PPG_SPLAT_LDS_NODES", "4"), ("PPG_NO_SORTED_COMMIT", "1"), ("PPG_BLOCKS", "512")])
@pytest.mark.parametrize("spatial,directional", [("nearest", "box"), ("stochastic", "nearest")])
def test_switches_change_no_bit(oracle_lib, orc, monkeypatch, switch, value, spatial, directional):
    """PPG_SPLAT_LDS_NODES and PPG_BLOCKS change what the hook's routes launch (the staging limit, the grid).  PPG_NO_SORTED_COMMIT changes
    how the RENDERS that grow the tree commit their rounds (k_commit instead of records + sort + k_splat_sorted) and must leave the same
    tree; the hook's routes are the caller's choice and run the same kernels with and without it."""
    monkeypatch.setenv(switch, value)  # (read by ppg_create)
    g, o, t, tree, _ = pair(oracle_lib, (spatial, directional, "kl", 1.0))
    cfg = dict(spatial=spatial, directional=directional, loss=True, weight=1.0)
    rng = np.random.default_rng(12)
    lds = 4 if switch == "PPG_SPLAT_LDS_NODES" else cr.LDS_NODES
    seen = set()
    for c in (cc.case_random(t, orc, rng, 1000, mean_nv=1.0, late="third"), cc.case_one_leaf(t, orc, rng, 2049), cc.case_guards(t, orc, rng)):
        _, r = run_case(g, o, t, tree, cfg, c, orc, cc.ROUTES, lds_nodes=lds)
        seen |= r["records"] | r["records_split"]
    if lds == 4:
        assert "unstaged: large" in seen and "staged" not in seen, seen


def test_refusals_name_the_argument_and_leave_the_context_usable(oracle_lib, orc):
    import ppg_host
    g, o, t, tree, _ = pair(oracle_lib, ("box", "box", "kl", 1.0))
    rng = np.random.default_rng(8)
    c = cc.case_random(t, orc, rng, 3)
    with pytest.raises(ppg_host.PPGError, match="route"):
        cc.call(g, "records", c)          # the box spatial filter has no known record positions
    with pytest.raises(ppg_host.PPGError, match="route"):
        cc.call(g, 7, c)
    with pytest.raises(ppg_host.PPGError, match="n_vertices"):
        cc.call(g, "commit", c, n_vertices=len(c["wo_pdf"]) + 1)
    g.set_pass_hook(lambda: None)
    with pytest.raises(ppg_host.PPGError, match="round hook"):
        cc.call(g, "commit", c)          # a round hook may replace the round's records
    g.set_pass_hook(None)
    many = dict(c, nv=c["nv"].copy())
    many["nv"][0] = cc.MAX_VERTICES + 1
    with pytest.raises(ppg_host.PPGError, match="nv"):
        cc.call(g, "commit", many, n_vertices=int(many["nv"].sum()))
    fresh = ppg_host.Engine.hip(**cc.props("nearest", "nearest", "none", 1.0))
    fresh.set_scene(ppg_host.cbox_scene(8, 8))
    fresh.begin_render()
    with pytest.raises(ppg_host.PPGError, match="begin_iteration"):
        cc.call(fresh, "commit", c)       # outside an iteration
    g.build_sdtree(); o.build_sdtree()
    with pytest.raises(ppg_host.PPGError, match="begin_iteration"):
        cc.call(g, "commit", c)           # the iteration's tree has been built
    g.end_iteration(); o.end_iteration()
    g.begin_iteration(False); o.begin_iteration(False)
    t = g.read_sdtree()
    run_case(g, o, t, cr.Tree(t), dict(spatial="box", directional="box", loss=True, weight=1.0), c, orc, ("commit", "commit_split"))
