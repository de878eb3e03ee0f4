"""GPU parity tests (run with -m gpu on an MI355X).  Everything goes through the C-ABI of libppg_hip.so.

Bar: bit-exact against the CPU oracle — film pixels (per-pixel L2 = 0), SD-tree
topology, fixed-point statistics, learned sampling fractions, ray / path-length / record counters —
because both sides evaluate the same IEEE-754 expression sequence (include/ppg_detmath.h, no FMA
contraction) on the same counter-based sampler, and all shared accumulation is integer.
"""
import ctypes as C
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from conftest import CBOX_PROPS, GOLDEN, IMPROVED, ROOT, make_oracle

pytestmark = pytest.mark.gpu


def hip(**props):
    import ppg_host
    return ppg_host.Engine.hip(**props)


def assert_tree_equal(a, b):
    assert np.array_equal(a["children"], b["children"]) and np.array_equal(a["axis"], b["axis"])
    for k in ("sampling", "building"):
        assert np.array_equal(a[k]["num_nodes"], b[k]["num_nodes"]), k
        assert np.array_equal(a[k]["node_children"], b[k]["node_children"]), k
        assert np.array_equal(a[k]["max_depth"], b[k]["max_depth"]), k
    assert np.array_equal(a["building"]["node_fixed"], b["building"]["node_fixed"])  # raw 2^-24 fixed-point accumulators
    assert np.array_equal(a["sampling"]["node_sums"], b["sampling"]["node_sums"])    # built float sums incl. interior nodes
    assert np.array_equal(a["sampling"]["sum"], b["sampling"]["sum"])
    assert np.array_equal(a["sampling"]["stat_weight"], b["sampling"]["stat_weight"])
    assert np.array_equal(a["theta"], b["theta"])


@pytest.mark.parametrize("case,extra", [("default", {}), ("improved", IMPROVED),
                                        ("boxbox", dict(spatialFilter="box", directionalFilter="box", bsdfSamplingFractionLoss="var",
                                                        sTreeThreshold=600, sampleCombination="discard"))])
def test_against_committed_golden_vectors(case, extra):
    import ppg_host
    g = np.load(os.path.join(GOLDEN, "oracle_cbox_%s.npz" % case))
    e = hip(budget=float(g["budget"]), seed=int(g["seed"]), **dict(CBOX_PROPS, **extra))
    gpt = ppg_host.GuidedPathTracer(engine=e)
    film = gpt.render(ppg_host.cbox_scene(int(g["res"]), int(g["res"])))
    assert np.array_equal(film, g["film"]), np.abs(film - g["film"]).max()
    t = e.read_sdtree()
    assert np.array_equal(t["children"], g["stree_children"]) and np.array_equal(t["axis"], g["stree_axis"])
    assert np.array_equal(t["sampling"]["node_children"], g["dtree_children"])
    assert np.array_equal(t["sampling"]["node_sums"], g["dtree_sums"])
    assert np.array_equal(t["sampling"]["num_nodes"], g["dtree_num"]) and np.array_equal(t["theta"], g["theta"])
    stats = np.array([[s["rays"], s["path_length_sum"], s["vertices_committed"]] for it in gpt.iterations for s in it["stats"]], np.uint64)
    assert np.array_equal(stats, g["stats"])
    var = np.array([s["variance"] for it in gpt.iterations for s in it["stats"]], np.float32)
    assert np.array_equal(var, g["variance"], equal_nan=True)
    assert [it["passes"] for it in gpt.iterations] == list(g["passes"])


@pytest.mark.parametrize("res,budget,extra", [((160, 90), 60, {}), ((96, 96), 31, IMPROVED), ((64, 64), 124, dict(maxDepth=-1, rrDepth=5, strictNormals=0)),
                                              ((64, 40), 28, dict(maxDepth=2)), ((48, 48), 40, dict(sppPerPass=8, dTreeThreshold=0.002, sTreeThreshold=300))])
def test_stepwise_against_live_oracle(oracle_lib, res, budget, extra):
    """Every phase of every iteration compared: reset topology, accumulated statistics, built trees, film."""
    import ppg_host
    props = dict(CBOX_PROPS, budget=budget, seed=99, **extra)
    scene = ppg_host.cbox_scene(*res)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    g.set_scene(scene); o.set_scene(scene)
    g.begin_render(); o.begin_render()
    spp = props.get("sppPerPass", 4)
    passes, it, done = int(np.ceil(budget / spp)), 0, 0
    while done < passes:
        p = min(passes - done, 1 << it)
        if passes - done - p < 2 * p:
            p = passes - done
        final = p >= passes - done
        g.begin_iteration(final); o.begin_iteration(final)
        a, b = g.read_sdtree(), o.read_sdtree()
        assert np.array_equal(a["children"], b["children"]) and np.array_equal(a["building"]["node_children"], b["building"]["node_children"])
        sg, so = g.render_passes(p), o.render_passes(p)
        for f in ("samples", "rays", "path_length_sum", "vertices_committed", "passes_rendered_total"):
            assert getattr(sg, f) == getattr(so, f), f
        assert sg.variance == so.variance or (np.isnan(sg.variance) and np.isnan(so.variance)) or (np.isinf(sg.variance) and np.isinf(so.variance))
        a, b = g.read_sdtree(), o.read_sdtree()
        assert np.array_equal(a["building"]["node_fixed"], b["building"]["node_fixed"])
        tg, to = g.build_sdtree(), o.build_sdtree()
        assert tg.as_dict() == to.as_dict()
        g.end_iteration(); o.end_iteration()
        assert_tree_equal(g.read_sdtree(), o.read_sdtree())
        assert np.array_equal(g.read_film(), o.read_film())
        assert np.array_equal(g.read_variance(), o.read_variance(), equal_nan=True)
        done += p; it += 1
    g.end_render(); o.end_render()
    assert np.array_equal(g.read_film(), o.read_film())


def test_full_size_720p_against_oracle(oracle_lib):
    """BASELINE.json configs[1] at its real size (1280x720, 4 spp/pass), first three iterations."""
    import ppg_host
    props = dict(CBOX_PROPS, budget=28, seed=1234)
    scene = ppg_host.cbox_scene(1280, 720)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    ig = ppg_host.GuidedPathTracer(engine=g).render(scene)
    io = ppg_host.GuidedPathTracer(engine=o).render(scene)
    assert np.array_equal(ig, io)
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())


def test_full_size_invariants():
    """Size-independent properties at 1280x720 that need no oracle: run-to-run determinism, the statistical-weight
    checksum (Σ leaf weights == records committed, nearest filters, weight 1), interior sums == Σ children,
    guiding pdfs integrate to one."""
    import ppg_host
    scene = ppg_host.cbox_scene(1280, 720)
    runs = []
    for _ in range(2):
        e = hip(budget=60, seed=5, **CBOX_PROPS)
        e.set_scene(scene); e.begin_render()
        for it, p in enumerate([1, 2, 4]):
            e.begin_iteration(False)
            st = e.render_passes(p)
            t = e.read_sdtree()
            leaf = t["children"][:, 0] == 0
            assert int(round(t["building"]["stat_weight"][leaf].sum())) == st.vertices_committed
            assert st.samples == 1280 * 720 * 4 * p and st.rays == st.path_length_sum
            e.build_sdtree(); e.end_iteration()
        runs.append((e.read_film(), e.read_sdtree()))
        t = runs[-1][1]["sampling"]
        off = 0
        for n in t["num_nodes"][runs[-1][1]["children"][:, 0] == 0][:200]:
            sums, ch = t["node_sums"][off:off + n], t["node_children"][off:off + n]
            for k in range(n):
                for j in range(4):
                    if ch[k, j]:
                        assert abs(sums[k, j] - sums[ch[k, j]].sum()) <= 2e-6 * max(1.0, sums[k, j])
            off += n
    assert np.array_equal(runs[0][0], runs[1][0])
    assert_tree_equal(runs[0][1], runs[1][1])
    # pdf over the sphere integrates to 1 in every populated leaf we probe
    e = hip(budget=60, seed=5, **CBOX_PROPS)
    img = ppg_host.GuidedPathTracer(engine=e).render(scene)
    assert np.array_equal(img[..., :], img) and img.mean() > 0.05
    rng = np.random.RandomState(0)
    pos = np.array([[278, 5, 280], [5, 270, 280], [278, 540, 280]], np.float32)
    u = rng.rand(200000, 2)
    z = 2 * u[:, 0] - 1; phi = 2 * np.pi * u[:, 1]; r = np.sqrt(1 - z * z)
    dirs = np.stack([r * np.cos(phi), r * np.sin(phi), z], -1).astype(np.float32)
    for p in pos:
        pdf = e.query_pdf(np.repeat(p[None], len(dirs), 0), dirs)
        assert abs(pdf.mean() * 4 * np.pi - 1) < 0.02


def test_cpp_render_loop_equals_python_driver():
    import ppg_host
    scene = ppg_host.cbox_scene(80, 60)
    for extra in ({}, IMPROVED):
        props = dict(CBOX_PROPS, budget=60, seed=3, **extra)
        a = hip(**props); a.set_scene(scene); a.render()
        b = hip(**props)
        img = ppg_host.GuidedPathTracer(engine=b).render(scene)
        assert np.array_equal(a.read_film(), img)
        assert_tree_equal(a.read_sdtree(), b.read_sdtree())


def test_queries_match_oracle(oracle_lib):
    import ppg_host
    props = dict(CBOX_PROPS, budget=60, seed=21)
    scene = ppg_host.cbox_scene(64, 64)
    g, o = hip(**props), make_oracle(oracle_lib, **props)
    for e in (g, o):
        e.set_scene(scene); e.render()
    rng = np.random.RandomState(4)
    pos = (rng.rand(5000, 3) * [550, 540, 550]).astype(np.float32)
    d = rng.randn(5000, 3); d /= np.linalg.norm(d, axis=1, keepdims=True)
    assert np.array_equal(g.query_pdf(pos, d.astype(np.float32)), o.query_pdf(pos, d.astype(np.float32)))
    sg, so = g.query_sample(pos, 77), o.query_sample(pos, 77)
    assert np.array_equal(sg, so) and np.allclose(np.linalg.norm(sg, axis=1), 1, atol=1e-5)


def test_large_scene_bvh_against_oracle(oracle_lib):
    """~50k triangles: the product's SAH BVH and the oracle's own median-split BVH must agree on every closest hit."""
    import ppg_host
    scene = ppg_host.room_scene(160, 90, n_boxes=260, tess=4)
    assert scene.n_triangles > 45000
    props = dict(budgetType="spp", budget=28, maxDepth=8, rrDepth=5, seed=8, sTreeThreshold=2000)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    ig = ppg_host.GuidedPathTracer(engine=g).render(scene)
    io = ppg_host.GuidedPathTracer(engine=o).render(scene)
    assert ig.mean() > 1e-3
    assert np.array_equal(ig, io)
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())


def test_room_stand_in_improved_unbounded_against_oracle(oracle_lib):
    """BASELINE configs[2] class (KITCHEN scene-improved: inverse-variance film, stochastic/box filters, KL-learned sampling fraction,
    unbounded depth) on the full-geometry room stand-in — 384k triangles, one rough-metal and two plastic materials, all light
    indirect — at a film size the oracle covers."""
    import ppg_host
    scene = ppg_host.room_scene(128, 72, glossy=True)
    assert scene.n_triangles == 384024
    props = dict(budgetType="spp", budget=31, maxDepth=-1, rrDepth=5, strictNormals=1, seed=17, **IMPROVED)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    assert _stats(gg) == _stats(go) and [i["passes"] for i in gg.iterations] == [1, 2, 4, 8, 16]
    assert np.array_equal(ig, io, equal_nan=True) and np.isfinite(ig).all() and ig.mean() > 1e-3
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())


def spaceship_class_scene(width, height, n_boxes=1400):
    """BASELINE configs[3] class stand-in (the reference's SPACESHIP: 257k triangles, one sphere — the emitting sky dome with flipped
    normals —, rough conductor / plastic / glass / diffuse): the room's boxes (268,824 triangles with n_boxes = 1400) with a third of
    them glass, the ceiling and its lamp removed, under a dome."""
    import ppg_host
    scene = ppg_host.room_scene(width, height, n_boxes=n_boxes, glossy=True)
    scene.materials = list(scene.materials)
    scene.materials[7] = dict(type="dielectric", eta=1.5, reflectance=(1, 1, 1), specular=(1, 1, 1))            # "b2"
    scene.materials.append(dict(type="diffuse", reflectance=(0.5, 0.5, 0.5)))
    keep = np.ones(len(scene.indices), bool); keep[10:24] = False                                           # ceiling, lamp, lamp housing
    scene.indices, scene.tri_material, scene.tri_emitter = scene.indices[keep], scene.tri_material[keep], scene.tri_emitter[keep]
    scene.emitters = [dict(radiance=(1.2, 1.3, 1.5))]
    scene.spheres = [dict(center=(2.0, 1.5, 2.5), radius=60.0, material=len(scene.materials) - 1, emitter=0, flip_normals=True)]
    return scene


def test_spaceship_class_improved_against_oracle(oracle_lib):
    """>= 250k triangles + 1 sphere with the SPACESHIP material mix, improved preset with the scene's own depth settings
    (spaceship-improved.xml: maxDepth 10, rrDepth 10)."""
    import ppg_host
    scene = spaceship_class_scene(160, 90)
    assert scene.n_triangles == 268810 and len(scene.spheres) == 1
    props = dict(budgetType="spp", budget=31, maxDepth=10, rrDepth=10, strictNormals=1, seed=23, **IMPROVED)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    assert _stats(gg) == _stats(go)
    assert np.array_equal(ig, io, equal_nan=True) and np.isfinite(ig).all() and ig.mean() > 1e-2
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())


@pytest.mark.parametrize("which", ["room-720p", "spaceship-class-1080p", "torus-1080p"])
def test_full_size_invariants_improved_configs(which):
    """Properties that need no oracle, at the real film sizes of BASELINE configs[2] / configs[3] with the improved preset: run-to-run
    determinism of film and SD-tree (atomics are fixed point, the optimiser's records are applied in key order), sample / ray
    bookkeeping, a finite film, every guiding pdf integrating to one."""
    import ppg_host
    if which == "room-720p":
        scene, spp = ppg_host.room_scene(1280, 720, glossy=True), 1280 * 720
        props = dict(budgetType="spp", budget=31, maxDepth=-1, rrDepth=5, strictNormals=1, seed=5, **IMPROVED)
    elif which == "torus-1080p":
        # BASELINE configs[4] at its size and settings (TORUS itself is a download, not bundled: the labelled stand-in of bench.py --scene torus):
        # 1920x1080, sppPerPass = 1, sTreeThreshold = 4000, unbounded specular-diffuse-specular chains — the persistent-thread tail at 2 M paths
        scene, spp = ppg_host.torus_scene(1920, 1080), 1920 * 1080
        props = dict(budgetType="spp", budget=31, sppPerPass=1, sTreeThreshold=4000, maxDepth=-1, rrDepth=5, strictNormals=0, seed=5)
    else:
        scene, spp = spaceship_class_scene(1920, 1080), 1920 * 1080
        props = dict(budgetType="spp", budget=31, maxDepth=10, rrDepth=10, strictNormals=1, seed=5, **IMPROVED)
    runs = []
    for _ in range(2):
        e = hip(**props)
        gpt = ppg_host.GuidedPathTracer(engine=e)
        img = gpt.render(scene)
        assert [i["passes"] for i in gpt.iterations] == [1, 2, 4, 8, 16]      # (fewer than 16 passes: inverse-variance over the one-sample
        for i in gpt.iterations:                                                #  first iteration is NaN, in the reference as well)
            st = i["stats"][0]
            assert st["samples"] == spp * i["passes"] and st["rays"] == st["path_length_sum"]
            assert (st["vertices_committed"] > 0) == (i is not gpt.iterations[-1])      # the last iteration only renders (GP:1524, isFinalIter)
        assert np.isfinite(img).all() and img.mean() > 1e-3
        runs.append((img, e.read_sdtree(), e))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert_tree_equal(runs[0][1], runs[1][1])
    e = runs[0][2]
    rng = np.random.RandomState(1)
    u = rng.rand(100000, 2)
    z = 2 * u[:, 0] - 1; phi = 2 * np.pi * u[:, 1]; r = np.sqrt(1 - z * z)
    dirs = np.stack([r * np.cos(phi), r * np.sin(phi), z], -1).astype(np.float32)
    lo, hi = np.asarray(scene.positions).min(0), np.asarray(scene.positions).max(0)
    pts = (np.array([[2.0, 0.02, 2.5], [0.02, 1.5, 3.0], [2.0, 1.5, 0.5]], np.float32) if which != "torus-1080p"
           else (lo + (hi - lo) * np.array([[0.5, 0.5, 0.5], [0.3, 0.1, 0.6], [0.7, 0.45, 0.2]])).astype(np.float32))
    for p in pts:
        pdf = e.query_pdf(np.repeat(p[None], len(dirs), 0), dirs)
        assert abs(pdf.mean() * 4 * np.pi - 1) < 0.03


def test_tuning_switches_do_not_change_results(monkeypatch):
    """DESIGN.md "Tuning switches": the environment switches ppg_create reads select schedules and layouts, never results.  A BVH scene
    with the full material set, improved preset, unbounded depth (tail + commit on two streams, BSDF-type sort, optimiser rounds)."""
    import ppg_host
    scene = ppg_host.room_scene(96, 54, n_boxes=60, tess=2, glossy=True)
    props = dict(budgetType="spp", budget=31, maxDepth=-1, rrDepth=5, strictNormals=1, seed=3, **IMPROVED)

    def run():
        e = hip(**props)
        img = ppg_host.GuidedPathTracer(engine=e).render(scene)
        return img, e.read_sdtree()

    base_img, base_tree = run()
    assert np.isfinite(base_img).all() and base_img.mean() > 1e-3
    for env in (dict(PPG_PATH_LAYOUT="aos"), dict(PPG_PATH_LAYOUT="soa"), dict(PPG_NO_SPLIT="1"), dict(PPG_NO_SORT_FIRST="1"),
                dict(PPG_NO_TOPCUT="1"), dict(PPG_NO_OVERLAP="1"), dict(PPG_NO_SORT="1"), dict(PPG_TAIL_MIN="1", PPG_TAIL_DIV="1000000"),
                dict(PPG_TAIL_THRESHOLD="100000000"), dict(PPG_BLOCKS="512"), dict(PPG_BATCH_PATHS="20000"), dict(PPG_TAIL_BLOCKS="64"),
                dict(PPG_BULK_BOUNCES="0"), dict(PPG_BULK_BOUNCES="3"), dict(PPG_BOUNCE_MARGIN="0"), dict(PPG_TAIL_MIN="200", PPG_TAIL_DIV="1000000"),
                dict(PPG_BVH_LEAF="3"), dict(PPG_BVH_LEAF="8"), dict(PPG_BLOCKS_SMALL="1024", PPG_SMALL_PATHS="100000000"), dict(PPG_BLOCKS_SMALL="0"), dict(PPG_NO_SORTED_COMMIT="1"), dict(PPG_ADAM_UNORDERED="1"), dict(PPG_SPLAT_LDS_NODES="4"), dict(PPG_NO_ASIDE="1"),
                dict(PPG_SPLIT_DEPTH="0"), dict(PPG_SPLIT_DEPTH="6"), dict(PPG_FINAL_HALVES="1", PPG_SPLIT_DEPTH="4"), dict(PPG_SPLIT_DEPTH="6", PPG_NO_OVERLAP="1"), dict(PPG_SPLIT_DEPTH="2", PPG_BULK_BOUNCES="5")):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            img, tree = run()
        assert np.array_equal(img, base_img), env
        assert_tree_equal(tree, base_tree)



def _length_histogram(oracle_lib, o):
    h = (C.c_uint64 * 4096)()
    oracle_lib.ppgo_path_length_histogram(o.ctx, h)
    return np.array(h)


@pytest.mark.parametrize("scene_name,depth,extra", [("cbox", 6, {}), ("cbox", 3, dict(nee="always")), ("room", 8, {}), ("room", 5, dict(sampleCombination="automatic")),
                                                    ("room", 8, dict(bsdfSamplingFractionLoss="var", spatialFilter="nearest", directionalFilter="nearest"))])
def test_stragglers_records_one_round_late_against_oracle(oracle_lib, scene_name, depth, extra):
    """include/ppg.h "STRAGGLERS": with maxDepth = -1 a path whose final depth exceeds PPG_ADAM_DEFER_DEPTH leaves k_tail, is finished beside the
    next round, and its optimiser records are applied one round late (the last round's in a round of their own).  One path in 10^4 gets to depth
    64 in a real scene and almost none here, so the tests' switch lowers the depth — in product and oracle alike — until THOUSANDS of paths go
    that way; film, SD-tree, learned fractions and counters must still be the oracle's bit for bit, and the rule must show in the fractions
    (the oracle at the shipped depth gives different ones)."""
    import ppg_host
    scene = ppg_host.cbox_scene(96, 96) if scene_name == "cbox" else ppg_host.room_scene(96, 54, n_boxes=60, tess=2, glossy=True)
    props = dict(budgetType="spp", budget=63, maxDepth=-1, rrDepth=3, strictNormals=1, seed=29, **dict(IMPROVED, **extra))
    threads = min(32, os.cpu_count() or 8)  # (96 x 54 pixels are six blocks: more threads only wait for each other)
    g, o = hip(**props), make_oracle(oracle_lib, threads=threads, **props)
    g._call("debug_set_defer_depth", C.c_int32(depth))
    o._call("debug_set_defer_depth", C.c_int32(depth))
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    hist = _length_histogram(oracle_lib, o)
    assert hist[depth + 1:].sum() > 2000, "the test needs stragglers"
    assert _stats(gg) == _stats(go)
    assert np.array_equal(ig, io, equal_nan=True) and np.isfinite(ig).all()
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())
    o64 = make_oracle(oracle_lib, threads=threads, **props)
    ppg_host.GuidedPathTracer(engine=o64).render(scene)
    assert not np.array_equal(o64.read_sdtree()["theta"], o.read_sdtree()["theta"])


@pytest.mark.parametrize("extra,env", [(dict(nee="always", **IMPROVED), {}), (dict(nee="always"), dict(PPG_SPLIT_DEPTH="3", PPG_BATCH_PATHS="6000"))], ids=["rounds", "scheduling-only"])
def test_stragglers_under_an_environment_emitter_with_luminaire_sampling(oracle_lib, monkeypatch, extra, env):
    """The per-path cosine that ConstantBackgroundEmitter::pdfDirect needs (`PathState::nee_cos`, scenes with an environment emitter and
    luminaire sampling only) must travel with a straggler into its set: an open scene under a constant sky, unbounded paths, nee = always —
    once with rounds of the optimiser (the tests' switch lowers the depth of the rule to 4) and once without a learned fraction, where the
    split is scheduling only (PPG_SPLIT_DEPTH = 3, batches of 6000 paths so that every batch but the last hands its stragglers over) and
    must not show in any result."""
    import ppg_host
    scene = _pane_scene((56, 56))
    keep = np.ones(len(scene.indices), bool)
    keep[4:8] = False          # drop ceiling and back wall
    scene.indices, scene.tri_material, scene.tri_emitter = scene.indices[keep], scene.tri_material[keep], scene.tri_emitter[keep]
    scene.environment = (0.5, 0.7, 1.1)
    props = dict(budgetType="spp", budget=60 if "sppPerPass" not in extra else 31, maxDepth=-1, rrDepth=3, strictNormals=1, seed=41, **extra)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    if not env:
        g._call("debug_set_defer_depth", C.c_int32(4))
        o._call("debug_set_defer_depth", C.c_int32(4))
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    assert _length_histogram(oracle_lib, o)[5:].sum() > 1000
    assert _stats(gg) == _stats(go)
    assert np.array_equal(ig, io, equal_nan=True) and np.isfinite(ig).all()
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())


def test_stragglers_phase_calls_and_time_budget(oracle_lib):
    """The same through ppg_render() in one call, and with a time budget (every batch may be the last: whatever is owed is settled at the end
    of each ppg_render_passes): deterministic from run to run."""
    import ppg_host
    scene = ppg_host.room_scene(96, 54, n_boxes=60, tess=2, glossy=True)
    props = dict(budgetType="spp", budget=63, maxDepth=-1, rrDepth=3, strictNormals=1, seed=31, **IMPROVED)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    for e in (g, o):
        e._call("debug_set_defer_depth", C.c_int32(6))
        e.set_scene(scene)
        e.render()
    assert np.array_equal(g.read_film(), o.read_film(), equal_nan=True)
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())
    props = dict(props, budgetType="seconds", budget=1.0)
    e = hip(**props)
    e._call("debug_set_defer_depth", C.c_int32(6))
    img = ppg_host.GuidedPathTracer(engine=e).render(scene)
    assert np.isfinite(img).all() and img.mean() > 1e-3


@pytest.mark.parametrize("leaf,depth", [(8, 6), (1, 6), (8, -1), (3, -1)])
def test_closest_hit_with_coincident_triangles_and_full_leaves_against_oracle(oracle_lib, monkeypatch, leaf, depth):
    """k_trace tests compacted (ray, triangle) pairs: the wave's leaves are dealt to all its lanes and a pair's result reaches its ray
    through an LDS minimum on (t, original index) (leaf_pairs, ppg_device.h); k_tail suspends a wave's last traversals and resumes them
    beside the lanes' next rays (trace_closest4_resume).  The closest hit must stay the reference's — the FIRST of several triangles hit at the
    same distance (skdtree.cpp:112-142 visits a leaf's triangles in order and keeps a hit only if it is closer).  Every box of the scene is
    there TWICE, the copy with another material and its triangles in reverse order, so that every hit on a box is a tie whose loser shows
    in the picture; leaves of 8 triangles make a wave collect more than 64 pairs (several rounds), leaves of 1 the other extreme.
    Bounded paths run in k_trace only, unbounded ones mostly in k_tail (the batches are smaller than its hand-over threshold)."""
    import ppg_host
    scene = ppg_host.room_scene(96, 54, n_boxes=50, tess=2, glossy=True)
    idx, mat, em = np.asarray(scene.indices).reshape(-1, 3), np.asarray(scene.tri_material), np.asarray(scene.tri_emitter)
    boxes = np.arange(24, len(idx))  # (the room itself is the first 24 triangles)
    nmat = len(scene.materials)
    twin_mat = np.where(mat[boxes] == nmat - 1, nmat - 3, mat[boxes] + 1).astype(mat.dtype)  # b0 -> b1 -> b2 -> b0: metal / plastic / diffuse swap
    scene.indices = np.concatenate([idx, idx[boxes][::-1]]).astype(idx.dtype)
    scene.tri_material = np.concatenate([mat, twin_mat[::-1]])
    scene.tri_emitter = np.concatenate([em, em[boxes][::-1]])
    monkeypatch.setenv("PPG_BVH_LEAF", str(leaf))
    props = dict(budgetType="spp", budget=31, maxDepth=depth, rrDepth=4, strictNormals=1, seed=41, **IMPROVED)
    g, o = hip(**props), make_oracle(oracle_lib, threads=min(32, os.cpu_count() or 8), **props)
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    assert _stats(gg) == _stats(go)
    assert np.isfinite(ig).all() and ig.mean() > 1e-3
    assert np.array_equal(ig, io)
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())
    # ... and the tie rule is visible: with the copies FIRST the picture is another one
    order = np.concatenate([np.arange(24), np.arange(len(idx), len(scene.indices)), boxes])
    scene.indices, scene.tri_material, scene.tri_emitter = scene.indices[order], scene.tri_material[order], scene.tri_emitter[order]
    g2 = hip(**props)
    i2 = ppg_host.GuidedPathTracer(engine=g2).render(scene)
    assert not np.array_equal(i2, ig)


@pytest.mark.parametrize("dfilter", ["nearest", "box"])
def test_sorted_splat_with_dtrees_beyond_the_lds_stage_and_runs_across_chunks(oracle_lib, dfilter):
    """k_splat_sorted (ppg_kernels.h "The commit of a ROUND") stages the building D-tree of a run of equal leaves in LDS when it has at most
    PPG_SPLAT_NODES = 512 nodes and splats in the pool otherwise, and a run may span many chunks of 2048 records.  A coarse S-tree (a
    handful of leaves: tens of thousands of records per run, i.e. dozens of chunks) with fine D-trees (dTreeThreshold 0.0015: 561 - 587 nodes in
    the largest) puts both branches and the chunk boundaries on the path, for the nearest and the box directional filter."""
    import ppg_host
    scene = ppg_host.cbox_scene(64, 64)
    props = dict(CBOX_PROPS, budget=124, seed=13, sppPerPass=4, sTreeThreshold=40000, dTreeThreshold=0.0015, bsdfSamplingFractionLoss="kl", spatialFilter="stochastic",
                 directionalFilter=dfilter, sampleCombination="inversevar")
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    t = o.read_sdtree()
    assert t["building"]["num_nodes"].max() > 512 and t["building"]["num_nodes"].min() <= 512 and t["n_leaves"] <= 16
    assert _stats(gg) == _stats(go)
    assert np.array_equal(ig, io, equal_nan=True)
    assert_tree_equal(g.read_sdtree(), t)


@pytest.mark.parametrize("scene_name,regions,extra,depth", [("cbox", 8, {}, 0), ("cbox-96", 9, dict(directionalFilter="nearest", bsdfSamplingFractionLoss="var"), 0),
                                                            ("room", 5, dict(maxDepth=-1, rrDepth=3), 6), ("cbox-96", 1000, dict(seed=20), 0)])
def test_rounds_by_image_region_against_oracle(oracle_lib, scene_name, regions, extra, depth):
    """include/ppg.h "Rounds by image region" (ppg_set_adam_regions, an extension, off by default): in the iterations of at most 16 passes a
    round is one pass over one of R groups of 32x32 blocks in the spiral order of the reference's scheduler, the optimiser applied after every
    group.  Film, SD-tree, fractions and counters are the oracle's bit for bit — bounded paths, unbounded paths with stragglers whose records
    travel from group to group (the tests' switch lowers the depth), R clamped to the number of blocks — and differ from the render without
    regions (the rule acts)."""
    import ppg_host
    scene = (ppg_host.cbox_scene(160, 160) if scene_name == "cbox" else ppg_host.cbox_scene(96, 96) if scene_name == "cbox-96"
             else ppg_host.room_scene(160, 96, n_boxes=60, tess=2, glossy=True))
    props = dict(CBOX_PROPS, budget=31.0, seed=19, **IMPROVED)
    props.update(extra)
    threads = min(16, os.cpu_count() or 8)  # (a round over one group of blocks is a few blocks of work: hundreds of threads only wait for each other)
    g, o = hip(**props), make_oracle(oracle_lib, threads=threads, **props)
    for e in (g, o):
        e.set_adam_regions(regions)
        if depth:
            e._call("debug_set_defer_depth", C.c_int32(depth))
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    assert _stats(gg) == _stats(go)
    assert np.array_equal(ig, io, equal_nan=True) and np.isfinite(ig).all()
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())
    plain = make_oracle(oracle_lib, threads=threads, **props)
    if depth:
        plain._call("debug_set_defer_depth", C.c_int32(depth))
    ppg_host.GuidedPathTracer(engine=plain).render(scene)
    assert not np.array_equal(plain.read_sdtree()["theta"], o.read_sdtree()["theta"])


def test_edge_cases(oracle_lib):
    import ppg_host
    # 1x1 film; 1 spp and a single pass (N - 1 = 0 → non-finite variance like the reference's "-1.#INF"); maxDepth = 1
    for res, props in (((1, 1), dict(budget=12)), ((33, 17), dict(budget=1, sppPerPass=1)), ((16, 16), dict(budget=8, maxDepth=1))):
        p = dict(CBOX_PROPS, seed=2, **props)
        g, o = hip(**p), make_oracle(oracle_lib, **p)
        scene = ppg_host.cbox_scene(*res)
        ig = ppg_host.GuidedPathTracer(engine=g).render(scene)
        io = ppg_host.GuidedPathTracer(engine=o).render(scene)
        assert np.array_equal(ig, io)
    # every ray misses: empty image, untouched SD-tree
    scene = ppg_host.cbox_scene(32, 32)
    scene.camera = ppg_host.perspective_camera((278, 273, -800), (278, 273, -2000), (0, 1, 0), 39.3, "x", 10, 2800, 32, 32)
    g = hip(budget=8, seed=1, **CBOX_PROPS)
    img = ppg_host.GuidedPathTracer(engine=g).render(scene)
    assert img.max() == 0 and g.read_sdtree()["n_leaves"] == 1
    # vertex normals present (shading frame from interpolated normals, skdtree.h:388-401)
    scene = ppg_host.cbox_scene(40, 40)
    idx = scene.indices.reshape(-1)
    fn = np.cross(scene.positions[scene.indices[:, 1]] - scene.positions[scene.indices[:, 0]], scene.positions[scene.indices[:, 2]] - scene.positions[scene.indices[:, 0]])
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    nrm = np.zeros_like(scene.positions)
    nrm[idx] = np.repeat(fn, 3, 0) + 0.05 * np.random.RandomState(0).randn(len(idx), 3)
    scene.normals = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    p = dict(CBOX_PROPS, budget=28, seed=6)
    g, o = hip(**p), make_oracle(oracle_lib, **p)
    assert np.array_equal(ppg_host.GuidedPathTracer(engine=g).render(scene), ppg_host.GuidedPathTracer(engine=o).render(scene))
    # errors: calls out of order, unsupported property value
    e = hip(budget=4, **CBOX_PROPS)
    with pytest.raises(ppg_host.PPGError) as ei:
        e.render()
    assert ei.value.code == -3
    with pytest.raises(ppg_host.PPGError):
        hip(nee="sometimes")


def test_sharded_contexts_on_one_gpu_equal_unsharded():
    """Two contexts render rank 0 / rank 1 of a 2-way tile shard on the same GPU; the exchange the RCCL driver
    performs (int64 sums of the building statistics, float sums of disjoint image tiles) is done by hand."""
    import ppg_host
    import torch
    from ppg_host.distributed import _view
    dev = torch.device("cuda", 0)
    scene = ppg_host.cbox_scene(96, 64)
    props = dict(CBOX_PROPS, budget=111, sppPerPass=1, seed=31)  # iterations 1, 2, 4, 8, 16 and a final one of 80 passes = five groups of 16
    ref = hip(**props)
    ref_gpt = ppg_host.GuidedPathTracer(engine=ref)
    ref_img = ref_gpt.render(scene)
    schedule = [it["passes"] for it in ref_gpt.iterations]
    assert schedule == [1, 2, 4, 8, 16, 80]

    class PairReducer:  # all-reduce over the two local contexts
        def __init__(self, engines):
            self.engines = engines
            self.pending = {}

        def _sum(self, key, views):
            total = views[0].clone()
            for v in views[1:]:
                total += v
            for v in views:
                v.copy_(total)
            torch.cuda.synchronize()

        def reduce_sdtree(self):
            bufs = [e.stat_buffers() for e in self.engines]
            for k in range(2):
                if bufs[0][k][1]:
                    self._sum(k, [_view(torch, b[k][0], b[k][1], "<i8", dev) for b in bufs])

        def reduce_images(self):
            n = 96 * 64
            for sel in (0, 1):
                self._sum(sel, [_view(torch, e.image_buffers()[sel], 3 * n, "<f4", dev) for e in self.engines])
            self._sum(2, [_view(torch, e.image_weight_buffer(), n, "<f4", dev) for e in self.engines])

        def reduce_final_partials(self):
            # the final iteration: every context rendered every second GROUP of passes over the whole film (include/ppg.h "Final iteration:
            # groups of passes"); the slots are summed — each is non-zero in one context only — and added in group order by the library
            bufs = [e.final_partials() for e in self.engines]
            assert bufs[0][1] == bufs[1][1] == 4 * 96 * 64 + 5 * 7 * 96 * 64
            self._sum(0, [_view(torch, b[0], b[1], "<f4", dev) for b in bufs])
            for e in self.engines:
                e.final_partials_commit()

    engines = [hip(**props) for _ in range(2)]
    for r, e in enumerate(engines):
        e.set_scene(scene); e.set_shard(r, 2, 16); e.begin_render()
    red = PairReducer(engines)
    for it, p in enumerate(schedule):
        final = it == len(schedule) - 1
        for e in engines:
            e.begin_iteration(final)
        for e in engines:
            e.render_passes_nostat(p)
        if final:
            red.reduce_final_partials()
        else:
            red.reduce_images()
        stats = [e.finish_passes() for e in engines]
        assert stats[0].variance == stats[1].variance or (np.isnan(stats[0].variance) and np.isnan(stats[1].variance))  # (1 spp: no estimate)
        if final:  # groups 0, 2 and 4 (48 passes) in context 0, groups 1 and 3 in context 1, all pixels each
            assert [st.samples for st in stats] == [96 * 64 * 48, 96 * 64 * 32]
        else:
            red.reduce_sdtree()
        for e in engines:
            e.build_sdtree(); e.end_iteration()
    for e in engines:  # (the exchange of the final iteration's groups left the complete film in both contexts: no film exchange)
        e.end_render()
        assert np.array_equal(e.read_film(), ref_img)
        assert_tree_equal(e.read_sdtree(), ref.read_sdtree())


def test_cancel_from_another_thread():
    import ppg_host
    e = hip(budgetType="spp", budget=40000, maxDepth=10, rrDepth=10, strictNormals=1)
    e.set_scene(ppg_host.cbox_scene(640, 360))
    threading.Timer(0.3, e.cancel).start()
    t0 = time.time()
    with pytest.raises(ppg_host.PPGError) as ei:
        e.render()
    assert ei.value.code == -4 and time.time() - t0 < 30  # render() returns false when cancelled (GP:1584, 1643-1648)


def test_sdt_dump_equals_oracle_bytes(oracle_lib, tmp_path):
    import ppg_host
    props = dict(CBOX_PROPS, budget=28, seed=12)
    scene = ppg_host.cbox_scene(48, 48)
    g, o = hip(**props), make_oracle(oracle_lib, **props)
    for e in (g, o):
        e.set_scene(scene); e.render()
    g.dump_sdtree(str(tmp_path / "g.sdt")); o.dump_sdtree(str(tmp_path / "o.sdt"))
    assert open(tmp_path / "g.sdt", "rb").read() == open(tmp_path / "o.sdt", "rb").read()


def test_round_hook_sees_the_records_of_every_round():
    """The multi-GPU exchange point of the sampling-fraction optimiser (include/ppg.h): the hook runs once per round after the
    round's records were collected and before they are applied.  An identity hook must not change anything; a hook that hands the
    same records back in another order exercises the whole-key sort of the union and must not change anything either."""
    import ppg_host
    import torch
    from ppg_host.distributed import _view
    dev = torch.device("cuda", 0)
    scene = ppg_host.cbox_scene(64, 64)
    props = dict(CBOX_PROPS, budget=31, seed=4, **IMPROVED)
    ref = hip(**props)
    ref_img = ppg_host.GuidedPathTracer(engine=ref).render(scene)
    for shuffle in (False, True):
        e = hip(**props)
        seen = []

        def hook():
            ptr, n = e.adam_records()
            recs = _view(torch, ptr, 4 * n, "<i8", dev).reshape(n, 4)
            keys = recs[:, 0]
            assert bool((keys[1:] > keys[:-1]).all())  # handed over in key order, keys unique
            leaf, path, code = keys >> 40, (keys >> 13) & ((1 << 27) - 1), keys & 8191
            assert int(leaf.max()) < e.sdtree_info().n_stree_nodes and int(code.min()) >= 4096 and int(code.max()) < 4096 + 32
            seen.append((n, int(path.max())))
            if shuffle:
                perm = torch.randperm(n, device=dev)
                mixed = recs[perm].contiguous()
                e.adam_records_replace(mixed.data_ptr(), n)

        e.set_scene(scene)
        e.begin_render()
        e.set_pass_hook(hook)
        passes = [1, 2, 4, 8, 16]
        for it, p in enumerate(passes):
            e.begin_iteration(it == len(passes) - 1)
            e.render_passes(p)
            e.build_sdtree(); e.end_iteration()
        e.end_render()
        assert np.array_equal(e.read_film(), ref_img)
        assert np.array_equal(e.read_sdtree()["theta"], ref.read_sdtree()["theta"])
        # rounds: none before the first build, 2 x 1 pass, 2 x 2 passes, 2 x 4 passes, none in the final iteration
        assert len(seen) == 6 and min(n for n, _ in seen) > 0
        assert [p // (64 * 64) for _, p in seen] == [0, 0, 1, 1, 3, 3]  # path id = sample-in-round * pixels + pixel


NCCL_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
import ppg_host
from ppg_host.distributed import TorchReducer
dist.init_process_group("nccl")
props = dict(budgetType="spp", maxDepth=10, rrDepth=10, strictNormals=1, budget=45, seed=17, sampleCombination="inversevar", bsdfSamplingFractionLoss="kl",
             spatialFilter="stochastic", directionalFilter="box", sTreeThreshold=2000, sppPerPass=1)
e = ppg_host.Engine.hip(**props)
e.set_scene(ppg_host.cbox_scene(64, 48)); e.set_shard(dist.get_rank(), dist.get_world_size(), 16)
gpt = ppg_host.GuidedPathTracer(engine=e, reducer=TorchReducer(dist, torch.device("cuda", 0)))
img = gpt.render()
t = e.read_sdtree()
np.savez(sys.argv[2], film=img, children=t["children"], dch=t["sampling"]["node_children"], dsum=t["sampling"]["node_sums"], theta=t["theta"])
dist.barrier(); dist.destroy_process_group()
"""


def test_torch_reducer_over_rccl_one_rank_equals_unsharded(tmp_path):
    """The reducer `bench.py --gpus N` renders with (ppg_host.distributed.TorchReducer: torch.distributed, backend "nccl" = RCCL, tensors
    viewed over the library's device buffers) on a real communicator of ONE rank: the whole sharded control flow — SD-tree all-reduce,
    the optimiser's records to the owners and their state back (round hook, both phases), the final iteration's groups of passes through
    ppg_final_partials / all-reduce / ppg_final_partials_commit, the status word — with every exchange the identity.  Film, SD-tree and the
    learned fractions equal the plain render's.  (Two ranks need two GPUs; the gloo tests of tests/test_host_logic.py cover world 2 and 4
    with the host reducer.)"""
    import ppg_host
    script = tmp_path / "worker.py"
    script.write_text(NCCL_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29500 + os.getpid() % 2000), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "practical-path-guiding_amd"), str(tmp_path / "rank0.npz")], env=env, timeout=600,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    props = dict(CBOX_PROPS, budget=45, seed=17, sampleCombination="inversevar", bsdfSamplingFractionLoss="kl", spatialFilter="stochastic", directionalFilter="box",
                 sTreeThreshold=2000, sppPerPass=1)
    e = hip(**props)
    ref_img = ppg_host.GuidedPathTracer(engine=e).render(ppg_host.cbox_scene(64, 48))
    ref_t = e.read_sdtree()
    got = np.load(tmp_path / "rank0.npz")
    assert np.array_equal(got["children"], ref_t["children"])
    assert np.array_equal(got["dch"], ref_t["sampling"]["node_children"]) and np.array_equal(got["dsum"], ref_t["sampling"]["node_sums"])
    assert np.array_equal(got["theta"], ref_t["theta"])
    assert np.array_equal(got["film"], ref_img, equal_nan=True)


@pytest.mark.parametrize("scheme", ["owner", "gather"])
def test_sharded_contexts_with_learned_fraction_equal_unsharded(scheme):
    """Two tile-sharded contexts on one GPU with the improved preset (KL-learned sampling fraction): the two render threads meet in
    the round hook.  "owner" (include/ppg.h "Sharded optimiser"): every D-tree has one owner; phase 0 sends each record to the owner of
    its D-tree, which sorts and applies only those, phase 1 copies the owners' optimiser state to the other context.  "gather": each
    context applies the union of both ranks' records.  Fractions, SD-tree and image equal the unsharded render either way."""
    import threading
    import ppg_host
    import torch
    from ppg_host.distributed import _view
    dev = torch.device("cuda", 0)
    scene = ppg_host.cbox_scene(64, 48)
    props = dict(CBOX_PROPS, budget=31, seed=9, **IMPROVED)
    ref = hip(**props)
    ref_img = ppg_host.GuidedPathTracer(engine=ref).render(scene)
    engines = [hip(**props) for _ in range(2)]
    barrier = threading.Barrier(2)
    slots = [None, None]

    def make_owner_hook(r):
        e = engines[r]

        def hook():
            if e.hook_phase() == 0:
                ptr, counts = e.adam_records_by_owner(2)
                recs = _view(torch, ptr, 4 * sum(counts), "<i8", dev).reshape(-1, 4) if sum(counts) else torch.zeros((0, 4), dtype=torch.int64, device=dev)
                seg = (e.sdtree_info().n_stree_nodes + 1) // 2
                assert bool(((recs[:counts[0], 0] >> 40) < seg).all()) and bool(((recs[counts[0]:, 0] >> 40) >= seg).all())
                slots[r] = (recs[:counts[0]].clone(), recs[counts[0]:].clone())
                torch.cuda.synchronize()
                barrier.wait()
                mine = torch.cat([slots[0][r], slots[1][r]]).contiguous()
                keep.append(mine)
                torch.cuda.synchronize()
                e.adam_records_replace(mine.data_ptr(), mine.shape[0])
                barrier.wait()
            else:
                ptr, seg = e.adam_state(2)
                state = _view(torch, ptr, 3 * seg * 2, "<i8", dev)
                slots[r] = state[3 * seg * r:3 * seg * (r + 1)].clone()
                torch.cuda.synchronize()
                barrier.wait()
                o = 1 - r
                state[3 * seg * o:3 * seg * (o + 1)] = slots[o]
                torch.cuda.synchronize()
                e.adam_state_commit()
                barrier.wait()
        return hook
    keep = []

    def make_hook(r):
        if scheme == "owner":
            return make_owner_hook(r)

        def hook():
            ptr, n = engines[r].adam_records()
            slots[r] = _view(torch, ptr, 4 * n, "<i8", dev).clone() if n else torch.zeros(0, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            barrier.wait()
            union = torch.cat(slots).contiguous()
            torch.cuda.synchronize()
            engines[r].adam_records_replace(union.data_ptr(), union.numel() // 4)
            barrier.wait()
        return hook

    def both(fn):
        errs = []

        def run(r):
            try:
                fn(r)
            except Exception as ex:  # pragma: no cover
                errs.append(ex)
                barrier.abort()
        ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
        [t.start() for t in ts]; [t.join() for t in ts]
        assert not errs, errs

    def sum_views(views):
        total = views[0].clone()
        for v in views[1:]:
            total += v
        for v in views:
            v.copy_(total)
        torch.cuda.synchronize()

    n = 64 * 48
    for r, e in enumerate(engines):
        e.set_scene(scene); e.set_shard(r, 2, 16); e.begin_render(); e.set_pass_hook(make_hook(r))
    for it, p in enumerate([1, 2, 4, 8, 16]):
        final = it == 4
        for e in engines:
            e.begin_iteration(final)
        both(lambda r: engines[r].render_passes_nostat(p))
        if final:  # one group of 16 passes, rendered by context 0 over the whole film (include/ppg.h "Final iteration: groups of passes")
            bufs = [e.final_partials() for e in engines]
            sum_views([_view(torch, b[0], b[1], "<f4", dev) for b in bufs])
            for e in engines:
                e.final_partials_commit()
        else:
            for sel in (0, 1):
                sum_views([_view(torch, e.image_buffers()[sel], 3 * n, "<f4", dev) for e in engines])
            sum_views([_view(torch, e.image_weight_buffer(), n, "<f4", dev) for e in engines])
        stats = [e.finish_passes() for e in engines]
        assert stats[0].variance == stats[1].variance or (np.isnan(stats[0].variance) and np.isnan(stats[1].variance))
        if not final:
            bufs = [e.stat_buffers() for e in engines]
            for k in range(2):
                if bufs[0][k][1]:
                    sum_views([_view(torch, b[k][0], b[k][1], "<i8", dev) for b in bufs])
        for e in engines:
            e.build_sdtree(); e.end_iteration()
    for e in engines:
        e.end_render()
        assert np.array_equal(e.read_film(), ref_img, equal_nan=True)
        assert_tree_equal(e.read_sdtree(), ref.read_sdtree())
        assert np.array_equal(e.read_sdtree()["theta"], ref.read_sdtree()["theta"])


def _materials_scene(res):
    """CBOX with the tall box turned into an ideal mirror (conductor, material "none") and the short box into a
    two-sided diffuse surface whose faces are wound inside-out (so the flipped side is the one that is seen)."""
    import ppg_host
    scene = ppg_host.cbox_scene(*res)
    scene.materials = list(scene.materials) + [dict(type=2, reflectance=(0.95, 0.93, 0.88)), dict(type=1, reflectance=(0.3, 0.5, 0.8))]
    tm = scene.tri_material.copy()
    tm[24:36] = 5                       # tall box  -> mirror
    tm[12:24] = 6                       # short box -> twosided diffuse
    scene.tri_material = tm
    idx = scene.indices.copy()
    idx[12:24] = idx[12:24][:, ::-1]    # flip the winding: the geometric normal now points into the box
    scene.indices = idx
    return scene


@pytest.mark.parametrize("extra", [{}, IMPROVED])
def test_mirror_and_twosided_materials_against_oracle(oracle_lib, extra):
    """First slice of SURVEY.md §8(f1): a delta BSDF (never guided, no vertex recorded, no Russian roulette clamp —
    GP:1654, 1942-1944, 2093, 2126) and twosided(diffuse)."""
    import ppg_host
    scene = _materials_scene((96, 96))
    props = dict(CBOX_PROPS, budget=60, seed=77, **extra)
    props.update(maxDepth=12, rrDepth=4)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    ig = ppg_host.GuidedPathTracer(engine=g).render(scene)
    io = ppg_host.GuidedPathTracer(engine=o).render(scene)
    assert np.array_equal(ig, io)
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())
    plain = ppg_host.GuidedPathTracer(engine=hip(**props)).render(ppg_host.cbox_scene(96, 96))
    assert np.abs(ig - plain).mean() > 1e-3  # the materials are really in effect


def _stats(gpt):
    return [[s["rays"], s["path_length_sum"], s["vertices_committed"]] for it in gpt.iterations for s in it["stats"]]


@pytest.mark.parametrize("res,budget,extra", [
    ((64, 64), 60, dict(nee="always")),
    ((48, 48), 508, dict(nee="kickstart")),  # the 128-spp switch of doNeeWithSpp (GP:1331-1340) is crossed: the last iteration starts at 252 spp
    ((64, 64), 60, dict(nee="kickstart", **IMPROVED)),
    ((48, 48), 60, dict(nee="kickstart", spatialFilter="box", directionalFilter="box", bsdfSamplingFractionLoss="var", sTreeThreshold=600)),
    ((64, 64), 124, dict(nee="always", maxDepth=-1, rrDepth=5, strictNormals=0)),
])
def test_next_event_estimation_against_oracle(oracle_lib, res, budget, extra):
    """nee = always / kickstart (GP:1962-2021, 2083-2088): luminaire sampling with the shadow ray traced inside Li's loop,
    MIS against the mixture pdf, the direct-light vertex committed in place with statistical weight 0.5."""
    import ppg_host
    props = dict(CBOX_PROPS, budget=budget, seed=5)
    props.update(extra)
    scene = ppg_host.cbox_scene(*res)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    assert _stats(gg) == _stats(go)
    assert np.array_equal(ig, io)
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())
    never = ppg_host.GuidedPathTracer(engine=hip(**dict(props, nee="never"))).render(scene)
    assert np.abs(ig - never).mean() > 1e-3 and abs(ig.mean() / never.mean() - 1) < 0.05  # a different, equally unbiased estimator


def test_next_event_estimation_bvh_scene_and_materials(oracle_lib):
    """Shadow rays through the BVH4 (any-hit) on a ~50k-triangle scene; twosided receivers (dRec.refN = 0) and a mirror."""
    import ppg_host
    scene = ppg_host.room_scene(120, 68, n_boxes=260, tess=4)
    props = dict(budgetType="spp", budget=28, maxDepth=8, rrDepth=5, seed=8, sTreeThreshold=2000, nee="kickstart")
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    ig = ppg_host.GuidedPathTracer(engine=g).render(scene)
    io = ppg_host.GuidedPathTracer(engine=o).render(scene)
    assert ig.mean() > 1e-3 and np.array_equal(ig, io)
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())
    scene = _materials_scene((64, 64))
    props = dict(CBOX_PROPS, budget=60, seed=78, nee="always", maxDepth=12, rrDepth=4, **IMPROVED)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    assert np.array_equal(ppg_host.GuidedPathTracer(engine=g).render(scene), ppg_host.GuidedPathTracer(engine=o).render(scene))
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())


def _full_materials_scene(res):
    """CBOX with the BSDFs of SURVEY.md §8(f1): GGX gold floor, copper back wall (smooth conductor), plastic short box,
    glass tall box, a two-sided rough aluminium-like ceiling."""
    import ppg_host
    scene = ppg_host.cbox_scene(*res)
    base = len(scene.materials)
    scene.materials = list(scene.materials) + [
        dict(type="roughconductor", alpha=0.2, eta=(0.143, 0.375, 1.442), k=(3.983, 2.386, 1.603), reflectance=(1, 1, 1)),          # +0 floor
        dict(type="conductor", eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14), reflectance=(0.95, 0.95, 0.95)),                         # +1 back wall
        dict(type="plastic", reflectance=(0.2, 0.35, 0.7), specular=(1, 1, 1), eta=1.49),                                           # +2 short box
        dict(type="dielectric", eta=1.5, reflectance=(1, 1, 1), specular=(0.98, 0.99, 0.98)),                                       # +3 tall box
        dict(type="roughconductor", alpha=0.45, eta=(1.66, 0.88, 0.52), k=(9.2, 6.3, 4.8), reflectance=(0.9, 0.9, 0.9), twosided=True,
             distribution="beckmann"),                                                                                              # +4 ceiling
    ]
    tm = scene.tri_material.copy()
    tm[2:4] = base + 0      # floor
    tm[4:6] = base + 4      # ceiling
    tm[6:8] = base + 1      # back wall
    tm[12:24] = base + 2    # short box
    tm[24:36] = base + 3    # tall box
    scene.tri_material = tm
    return scene


@pytest.mark.parametrize("extra", [{}, IMPROVED, dict(nee="kickstart", bsdfSamplingFractionLoss="var"), dict(maxDepth=-1, rrDepth=3, strictNormals=0)],
                         ids=["default", "improved", "nee-kickstart-var", "unbounded-rr"])
def test_glossy_plastic_and_glass_materials_against_oracle(oracle_lib, extra):
    """roughconductor (GGX, visible normals) is smooth ⇒ guided, with the learned BSDF sampling fraction
    doing real work; plastic mixes a delta lobe into a guided BSDF (GP:1672-1676, delta vertices recorded for Adam, GP:2093);
    the dielectric is all-delta, transmits, and scales eta for Russian roulette (GP:2040, 2130)."""
    import ppg_host
    scene = _full_materials_scene((72, 72))
    assert [int(t) for t in np.bincount(scene.tri_material)] and scene.tri_emitter[0] == 0
    props = dict(CBOX_PROPS, budget=60, seed=12)
    props.update(maxDepth=14, rrDepth=5)
    props.update(extra)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    assert _stats(gg) == _stats(go)
    assert np.array_equal(ig, io, equal_nan=True)
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())
    plain = ppg_host.GuidedPathTracer(engine=hip(**props)).render(ppg_host.cbox_scene(72, 72))
    assert np.nanmean(np.abs(ig - plain)) > 5e-3


@pytest.mark.parametrize("extra", [{}, dict(nee="always", **IMPROVED), dict(maxDepth=-1, rrDepth=3, strictNormals=0, nee="kickstart")],
                         ids=["default", "nee-always-improved", "unbounded-kickstart"])
def test_rough_dielectric_against_oracle(oracle_lib, extra):
    """roughdielectric (roughdielectric.cpp:268-606): a smooth ⇒ guided BSDF that transmits — guided directions below the surface,
    eta carried for Russian roulette, and sample() drawing its reflect/refract choice from the path's sampler (one extra
    dimension per BSDF sample), which shifts every later dimension of the path."""
    import ppg_host
    scene = ppg_host.cbox_scene(64, 64)
    base = len(scene.materials)
    scene.materials = list(scene.materials) + [
        dict(type="roughdielectric", alpha=0.2, eta=1.5, reflectance=(1, 1, 1), specular=(0.95, 0.98, 0.95)),                         # tall box: frosted glass
        dict(type="roughdielectric", alpha=0.08, eta=1.33, reflectance=(0.9, 0.9, 1), specular=(1, 1, 1), distribution="beckmann")]   # short box
    tm = scene.tri_material.copy()
    tm[12:24] = base + 1
    tm[24:36] = base + 0
    scene.tri_material = tm
    props = dict(CBOX_PROPS, budget=60, seed=33)
    props.update(maxDepth=12, rrDepth=5)
    props.update(extra)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    assert _stats(gg) == _stats(go)
    assert np.array_equal(ig, io, equal_nan=True)
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())
    glass = ppg_host.cbox_scene(64, 64)
    glass.materials = list(glass.materials) + [dict(type="dielectric", eta=1.5, reflectance=(1, 1, 1), specular=(0.95, 0.98, 0.95))]
    tmg = glass.tri_material.copy(); tmg[24:36] = base; glass.tri_material = tmg
    assert np.nanmean(np.abs(ig - ppg_host.GuidedPathTracer(engine=hip(**props)).render(glass))) > 5e-3


def _roughplastic_scene(res):
    import ppg_host
    from test_bsdfs import rtrans_slice
    scene = ppg_host.cbox_scene(*res)
    base = len(scene.materials)
    scene.rtrans = np.stack([rtrans_slice("ggx", 0.1, 1.5), rtrans_slice("beckmann", 0.2, 1.49), rtrans_slice("ggx", 0.3, 1.49)]).astype(np.float32)
    scene.materials = list(scene.materials) + [
        dict(type="roughplastic", alpha=0.1, eta=1.5, reflectance=(0.45, 0.3, 0.15), specular=(1, 1, 1), rtrans=0),                                  # floor: varnished wood
        dict(type="roughplastic", alpha=0.2, eta=1.49, reflectance=(0.2, 0.5, 0.7), specular=(0.8, 0.9, 1.0), distribution="beckmann", nonlinear=True,
             twosided=True, rtrans=1),                                                                                                             # short box
        dict(type="roughplastic", alpha=0.3, eta=1.49, reflectance=(0.7, 0.7, 0.7), specular=(1, 1, 1), rtrans=2)]                                   # tall box
    tm = scene.tri_material.copy()
    tm[2:4] = base + 0
    tm[12:24] = base + 1
    tm[24:36] = base + 2
    scene.tri_material = tm
    return scene


@pytest.mark.parametrize("extra", [{}, dict(nee="always", **IMPROVED)], ids=["default", "nee-always-improved"])
def test_rough_plastic_against_oracle(oracle_lib, extra):
    """roughplastic (roughplastic.cpp:330-501): glossy coating + diffuse base, both guided; the energy split comes from the material's
    rough-transmittance slice (ppg_scene.rtrans — cut from Mitsuba's data/microfacet tables, committed as tests/golden/rtrans_slices.npz),
    read through the reference's cubic interpolation on the warped cosine."""
    import ppg_host
    scene = _roughplastic_scene((64, 64))
    props = dict(CBOX_PROPS, budget=60, seed=41)
    props.update(maxDepth=10, rrDepth=5)
    props.update(extra)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    assert _stats(gg) == _stats(go)
    assert np.array_equal(ig, io, equal_nan=True)
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())
    plain = ppg_host.GuidedPathTracer(engine=hip(**props)).render(ppg_host.cbox_scene(64, 64))
    assert np.nanmean(np.abs(ig - plain)) > 5e-3
    bad = _roughplastic_scene((16, 16))
    bad.materials[-1]["rtrans"] = 7
    with pytest.raises(ppg_host.PPGError, match="rtrans"):
        ppg_host.GuidedPathTracer(engine=hip(**props)).render(bad)


def _sphere_scene(res, sky=False):
    """CBOX whose tall box is replaced by nothing and which gains three analytic spheres (shapes/sphere.cpp): a glass ball, a rotated
    rough-gold ball (its (theta, phi) tangent frame steers the microfacet sampling) and a small sphere LAMP; `sky`: everything sits
    inside a large emitting sphere with flipped normals, the sky dome of the reference's SPACESHIP scene."""
    import ppg_host
    scene = ppg_host.cbox_scene(*res)
    base = len(scene.materials)
    scene.materials = list(scene.materials) + [
        dict(type="dielectric", eta=1.5, reflectance=(1, 1, 1), specular=(1, 1, 1)),
        dict(type="roughconductor", alpha=0.15, eta=(0.143, 0.375, 1.442), k=(3.983, 2.386, 1.603), reflectance=(1, 1, 1)),
        dict(type="diffuse", reflectance=(0.5, 0.5, 0.5))]
    scene.emitters = list(scene.emitters) + [dict(radiance=(40.0, 30.0, 20.0))]
    a = np.float32(0.6)
    rot = [float(np.cos(a)), 0.0, float(np.sin(a)), 0.0, 1.0, 0.0, float(-np.sin(a)), 0.0, float(np.cos(a))]
    scene.spheres = [dict(center=(370.0, 90.0, 200.0), radius=90.0, material=base + 0),
                     dict(center=(150.0, 250.0, 320.0), radius=70.0, material=base + 1, to_world=rot),
                     dict(center=(420.0, 400.0, 380.0), radius=25.0, material=base + 2, emitter=1)]
    keep = np.ones(len(scene.indices), bool); keep[24:36] = False          # drop the tall box (the glass ball stands there)
    scene.indices, scene.tri_material, scene.tri_emitter = scene.indices[keep], scene.tri_material[keep], scene.tri_emitter[keep]
    if sky:
        scene.emitters = scene.emitters + [dict(radiance=(0.3, 0.3, 0.35))]
        scene.spheres.append(dict(center=(278.0, 273.0, 280.0), radius=3000.0, material=base + 2, emitter=2, flip_normals=True))
        keep = np.ones(len(scene.indices), bool); keep[4:6] = False        # open the ceiling towards the dome
        scene.indices, scene.tri_material, scene.tri_emitter = scene.indices[keep], scene.tri_material[keep], scene.tri_emitter[keep]
    return scene


@pytest.mark.parametrize("extra,sky", [({}, False), (dict(nee="always", **IMPROVED), False), (dict(nee="kickstart", bsdfSamplingFractionLoss="kl"), True),
                                       (dict(maxDepth=-1, rrDepth=3, strictNormals=0), True)],
                         ids=["default", "nee-always-improved", "sky-dome-kickstart", "sky-dome-unbounded"])
def test_analytic_spheres_against_oracle(oracle_lib, extra, sky):
    """shapes/sphere.cpp as a primitive next to the triangles: the reference's double-precision quadratic (sphere.cpp:164-189) after the
    BVH's closest triangle, intersection records re-projected onto the sphere with the (theta, phi) tangent (:213-263), sphere emitters
    sampled by cone (outside) or area (inside) with the matching pdfDirect in the MIS weights (:291-378), and a scene box / S-tree
    that now spans the dome."""
    import ppg_host
    scene = _sphere_scene((64, 64), sky)
    props = dict(CBOX_PROPS, budget=60, seed=52)
    props.update(maxDepth=10, rrDepth=5)
    props.update(extra)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    assert _stats(gg) == _stats(go)
    assert np.array_equal(ig, io, equal_nan=True)
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())
    plain = ppg_host.GuidedPathTracer(engine=hip(**props)).render(ppg_host.cbox_scene(64, 64))
    assert np.nanmean(np.abs(ig - plain)) > 5e-3
    if not sky:
        bad = _sphere_scene((16, 16))
        bad.spheres[2]["emitter"] = 0                                      # the ceiling lamp's emitter
        with pytest.raises(ppg_host.PPGError, match="shared"):
            ppg_host.GuidedPathTracer(engine=hip(**props)).render(bad)


def _envmap_scene(res, pane=False):
    """CBOX without its ceiling and lamp under an image-based sky (a noisy map with a small, 60x brighter "sun", rotated about an oblique
    axis); `pane`: a thin-dielectric pane closes the opening, so the sky is found THROUGH a null surface."""
    import ppg_host
    from test_envmap import _sun_map
    scene = ppg_host.cbox_scene(*res)
    keep = np.ones(len(scene.indices), bool); keep[0:2] = False; keep[4:6] = False     # the luminaire and the ceiling
    scene.indices, scene.tri_material, scene.tri_emitter = scene.indices[keep], scene.tri_material[keep], scene.tri_emitter[keep]
    scene.emitters = []
    ax = np.float64([1, 2, 3]) / np.sqrt(14.0); a = 0.7
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    scene.envmap = dict(rgb=_sun_map(), scale=0.5, to_world=R.astype(np.float32).reshape(-1))
    if pane:
        base_v = len(scene.positions)
        quad = np.array([(0, 548, 0), (556, 548, 0), (556, 548, 559), (0, 548, 559)], np.float32)
        scene.positions = np.vstack([scene.positions, quad]).astype(np.float32)
        scene.indices = np.vstack([scene.indices, [[base_v, base_v + 1, base_v + 2], [base_v, base_v + 2, base_v + 3]]]).astype(np.uint32)
        scene.materials = list(scene.materials) + [dict(type="thindielectric", eta=1.5, reflectance=(1, 1, 1), specular=(0.95, 0.97, 0.95))]
        scene.tri_material = np.concatenate([scene.tri_material, np.full(2, len(scene.materials) - 1)]).astype(np.uint32)
        scene.tri_emitter = np.concatenate([scene.tri_emitter, np.full(2, -1)]).astype(np.int32)
    return scene


@pytest.mark.parametrize("extra,pane", [({}, False), (dict(nee="always", **IMPROVED), False), (dict(nee="kickstart", maxDepth=-1, rrDepth=3, strictNormals=0), True),
                                        (dict(nee="always", maxDepth=6), True)],
                         ids=["default", "nee-always-improved", "pane-kickstart-unbounded", "pane-nee-always"])
def test_environment_map_against_oracle(oracle_lib, extra, pane):
    """emitters/envmap.cpp: level-0 bilinear lookups for rays that leave the scene (also through null surfaces, GP:2236-2243), luminance x
    sin(theta) importance sampling with tent-filtered pixel positions (envmap.cpp:557-595) for next-event estimation, its solid-angle
    density in the MIS weights (:598-633), the emitter's rotation; the cdfs are built on the host in the oracle's float operations."""
    import ppg_host
    scene = _envmap_scene((64, 64), pane)
    props = dict(CBOX_PROPS, budget=60, seed=63)
    props.update(maxDepth=10, rrDepth=5)
    props.update(extra)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    assert _stats(gg) == _stats(go)
    assert np.array_equal(ig, io, equal_nan=True)
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())
    assert np.nanmean(ig) > 0.02
    if not pane:
        scene.environment = (1.0, 1.0, 1.0)
        with pytest.raises(ppg_host.PPGError, match="one environment emitter"):
            ppg_host.GuidedPathTracer(engine=hip(**props)).render(scene)


def test_torus_class_stand_in_against_oracle(oracle_lib):
    """ppg_host.torus_scene (bench.py --scene torus, BASELINE configs[4] stand-in): unbounded specular chains inside the glass cube, the
    k_tail path, 1 spp per pass."""
    import ppg_host
    scene = ppg_host.torus_scene(64, 36, n_major=24, n_minor=12)
    props = dict(budgetType="spp", budget=31, sppPerPass=1, sTreeThreshold=4000, maxDepth=-1, rrDepth=5, seed=7)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    assert _stats(gg) == _stats(go)
    assert np.array_equal(ig, io, equal_nan=True) and np.isfinite(ig).all() and ig.mean() > 0.05
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())


def _pane_scene(res):
    """CBOX + two thin-dielectric panes: a horizontal one between the (upward-facing) luminaire and the ceiling and a vertical
    "window" across the room — most paths cross a null component, emitters are found through one or two panes."""
    import ppg_host
    scene = ppg_host.cbox_scene(*res)
    base_v = len(scene.positions)
    quads = [[(150, 510, 170), (400, 510, 170), (400, 510, 390), (150, 510, 390)],   # above the luminaire
             [(20, 20, 300), (530, 20, 300), (530, 500, 300), (20, 500, 300)]]       # the window
    pos = np.array([p for q in quads for p in q], np.float32)
    idx = np.array([[base_v + 4 * k + a for a in tri] for k in range(len(quads)) for tri in ((0, 1, 2), (0, 2, 3))], np.uint32)
    scene.positions = np.vstack([scene.positions, pos]).astype(np.float32)
    scene.indices = np.vstack([scene.indices, idx]).astype(np.uint32)
    scene.materials = list(scene.materials) + [dict(type="thindielectric", eta=1.5, reflectance=(1, 1, 1), specular=(0.95, 0.97, 0.95))]
    scene.tri_material = np.concatenate([scene.tri_material, np.full(len(idx), len(scene.materials) - 1)]).astype(np.uint32)
    scene.tri_emitter = np.concatenate([scene.tri_emitter, np.full(len(idx), -1)]).astype(np.int32)
    return scene


@pytest.mark.parametrize("extra", [{}, dict(nee="always"), dict(nee="kickstart", **IMPROVED), dict(maxDepth=-1, rrDepth=3, strictNormals=0, nee="kickstart"),
                                   dict(maxDepth=3)],
                         ids=["default", "nee-always", "nee-kickstart-improved", "unbounded", "depth3-budget"])
def test_null_component_bsdf_against_oracle(oracle_lib, extra):
    """thindielectric: Li's null branch (GP:2045-2075: no MIS, no roulette, emission re-enabled only before the first real
    scattering), emitters found THROUGH null surfaces (GP:2184-2245) within the interaction budget maxDepth - depth - 1, shadow
    rays attenuated by them (scene.cpp:619-679)."""
    import ppg_host
    scene = _pane_scene((64, 64))
    props = dict(CBOX_PROPS, budget=60, seed=21)
    props.update(maxDepth=12, rrDepth=5)
    props.update(extra)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    assert _stats(gg) == _stats(go)
    assert np.array_equal(ig, io, equal_nan=True)
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())
    plain = ppg_host.GuidedPathTracer(engine=hip(**props)).render(ppg_host.cbox_scene(64, 64))
    assert np.nanmean(np.abs(ig - plain)) > 2e-3


def test_null_component_bsdf_on_a_bvh_scene(oracle_lib):
    import ppg_host
    scene = ppg_host.room_scene(96, 54, n_boxes=200, tess=4)
    # a large pane across the room below the slit light
    base_v = len(scene.positions)
    pos = np.array([(0.2, 2.2, 0.2), (3.8, 2.2, 0.2), (3.8, 2.2, 4.8), (0.2, 2.2, 4.8)], np.float32)
    scene.positions = np.vstack([scene.positions, pos]).astype(np.float32)
    scene.indices = np.vstack([scene.indices, [[base_v, base_v + 1, base_v + 2], [base_v, base_v + 2, base_v + 3]]]).astype(np.uint32)
    scene.materials = list(scene.materials) + [dict(type="thindielectric", eta=1.33, reflectance=(1, 1, 1), specular=(1, 1, 1))]
    scene.tri_material = np.concatenate([scene.tri_material, [len(scene.materials) - 1] * 2]).astype(np.uint32)
    scene.tri_emitter = np.concatenate([scene.tri_emitter, [-1, -1]]).astype(np.int32)
    props = dict(budgetType="spp", budget=28, maxDepth=9, rrDepth=5, seed=8, sTreeThreshold=2000, nee="kickstart")
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    assert _stats(gg) == _stats(go) and ig.mean() > 1e-3 and np.array_equal(ig, io)
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())


@pytest.mark.parametrize("extra", [dict(nee="never"), dict(nee="always"), dict(nee="kickstart", **IMPROVED), dict(nee="always", hideEmitters=1, maxDepth=-1, rrDepth=3)],
                         ids=["never", "nee-always", "nee-kickstart-improved", "hidden-unbounded"])
def test_constant_environment_emitter_against_oracle(oracle_lib, extra):
    """emitters/constant.cpp: an open scene (CBOX without ceiling and back wall) under a constant sky next to the area light — Li's
    miss branch (GP:1902-1914), the escape branch of rayIntersectAndLookForEmitter (GP:2236-2243), luminaire sampling over two
    emitters with the environment's cosine / uniform-sphere sampling, and its pdf in the MIS weights (constant.cpp:176-231).  A pane
    makes escaping rays pass a null surface first; a two-sided floor exercises refN = 0 (uniform-sphere sampling)."""
    import ppg_host
    scene = _pane_scene((56, 56))
    keep = np.ones(len(scene.indices), bool)
    keep[4:8] = False          # drop ceiling and back wall
    scene.indices, scene.tri_material, scene.tri_emitter = scene.indices[keep], scene.tri_material[keep], scene.tri_emitter[keep]
    scene.materials = list(scene.materials) + [dict(type="diffuse", reflectance=(0.6, 0.6, 0.6), twosided=True)]
    tm = scene.tri_material.copy(); tm[2:4] = len(scene.materials) - 1; scene.tri_material = tm   # floor
    scene.environment = (0.5, 0.7, 1.1)
    props = dict(CBOX_PROPS, budget=60, seed=33)
    props.update(maxDepth=9, rrDepth=5)
    props.update(extra)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    assert _stats(gg) == _stats(go)
    assert np.array_equal(ig, io, equal_nan=True)
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())
    scene.environment = None
    dark = ppg_host.GuidedPathTracer(engine=hip(**props)).render(scene)
    assert np.nanmean(ig) > 1.3 * np.nanmean(dark)


@pytest.mark.parametrize("extra", [dict(bsdfSamplingFractionLoss="kl"), dict(nee="kickstart", **IMPROVED), dict(nee="always", maxDepth=-1, rrDepth=3, strictNormals=0)],
                         ids=["kl", "nee-kickstart-improved", "nee-always-unbounded"])
def test_mask_bsdf_against_oracle(oracle_lib, extra):
    """mask (a smooth/null hybrid): the surface is guided, its sampled pass-through is a delta vertex recorded for the sampling-fraction
    optimiser (GP:2047-2068), emitters are seen through it (GP:2184-2245) and shadow rays are attenuated by 1 - opacity."""
    import ppg_host
    scene = _pane_scene((56, 56))
    scene.materials[-1] = dict(type="diffuse", reflectance=(0.7, 0.7, 0.7), twosided=True, opacity=(0.35, 0.4, 0.45))   # the panes: masked, two-sided
    scene.materials = list(scene.materials) + [dict(type="roughconductor", alpha=0.3, eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.1), opacity=(0.8, 0.8, 0.8))]
    tm = scene.tri_material.copy(); tm[12:24] = len(scene.materials) - 1; scene.tri_material = tm   # short box: masked GGX
    props = dict(CBOX_PROPS, budget=60, seed=45)
    props.update(maxDepth=11, rrDepth=5)
    props.update(extra)
    g, o = hip(**props), make_oracle(oracle_lib, threads=os.cpu_count() or 8, **props)
    gg, go = ppg_host.GuidedPathTracer(engine=g), ppg_host.GuidedPathTracer(engine=o)
    ig, io = gg.render(scene), go.render(scene)
    assert _stats(gg) == _stats(go)
    assert np.array_equal(ig, io, equal_nan=True)
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())


def test_time_budget_automatic_dumps_and_memory_cap(oracle_lib, tmp_path):
    """budgetType = seconds (the reference's default) on the GPU; the automatic per-iteration .sdt dumps; sdTreeMaxMemory — the latter two
    compared with the oracle."""
    import ppg_host
    from test_host_logic import _time_budget_checks
    _time_budget_checks(lambda **p: hip(**p), ppg_host.cbox_scene(160, 90), 0.5)
    scene = ppg_host.cbox_scene(48, 48)
    for name, mk in (("g", hip), ("o", lambda **p: make_oracle(oracle_lib, **p))):
        e = mk(budget=60, seed=2, dumpSDTree=1, dumpPrefix=str(tmp_path / name), **CBOX_PROPS)
        ppg_host.GuidedPathTracer(engine=e).render(scene)
    gf, of = sorted(f for f in os.listdir(tmp_path) if f.startswith("g-")), sorted(f for f in os.listdir(tmp_path) if f.startswith("o-"))
    assert len(gf) == 3 and [f[1:] for f in gf] == [f[1:] for f in of]
    for a, b in zip(gf, of):
        assert open(tmp_path / a, "rb").read() == open(tmp_path / b, "rb").read()
    for cap, leaves in ((0, 1), (1, None)):
        p = dict(CBOX_PROPS, budget=124, seed=2, sTreeThreshold=200, sdTreeMaxMemory=cap)
        g, o = hip(**p), make_oracle(oracle_lib, **p)
        assert np.array_equal(ppg_host.GuidedPathTracer(engine=g).render(scene), ppg_host.GuidedPathTracer(engine=o).render(scene))
        assert_tree_equal(g.read_sdtree(), o.read_sdtree())
        assert leaves is None or g.read_sdtree()["n_leaves"] == leaves
