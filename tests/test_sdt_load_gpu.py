"""Loading a dumped SD-tree on the GPU (include/ppg.h "Loading a dumped SD-tree", Engine.load_sdtree):

  * the oracle's file, loaded by the HIP engine, answers pdf and sample queries as the oracle's own tree does, bit for bit;
  * a render split at a dump — final iteration from the file — equals the uninterrupted one: film, variance, pass statistics;
  * training continued from a file leaves the same next dump, byte for byte;
  * dump -> load -> dump is the identity up to 4 ulp of each leaf's mean (also with the `improved` preset, where queries stay bit-equal);
  * a hand-written file with a missing leaf: the hole samples uniformly, the present leaf as a numpy descent of its quadtree says;
  * the refusals through the API leave the context rendering what an untouched one renders;
  * `python -m ppg_host --sdtree FILE --guide-only` writes the image of the stepwise guide-only render;
  * GuidedPathTracer(sdtree=...) goes on with the usual schedule from either dump of a whole render and ends with its film; guide_only
    spends an spp or a time budget on one final iteration.

cbox at 48x48 with budget 28 = 7 passes: two training iterations of 1 and 2 passes, a final one of 4 (renderSPP, GP:1367-1374)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import CBOX_PROPS, GOLDEN, IMPROVED, PKG, make_oracle

f32 = np.float32
pytestmark = pytest.mark.gpu
RES = 48
PROPS = dict(CBOX_PROPS, budget=28, seed=9)
# With the preset's sTreeThreshold (12000) this render never splits the S-tree: one leaf.  The same cases therefore run a second time with a
# threshold that gives dozens of leaves — some of weight 0, which the dump skips: holes on the way back in.
FINE = dict(sTreeThreshold=300)
TREES = [("preset", {}), ("fine", FINE)]


def hip(**props):
    import ppg_host
    return ppg_host.Engine.hip(**props)


def scene():
    import ppg_host
    return ppg_host.cbox_scene(RES, RES)


def train(e, first, count):
    """training iterations first .. first + count - 1 of the usual schedule (2^i passes each); the last one's pass statistics"""
    st = None
    for it in range(first, first + count):
        e.set_do_nee(False)
        e.begin_iteration(False)
        st = e.render_passes(1 << it)
        e.build_sdtree()
        e.end_iteration()
    return st


def final(e, passes):
    e.set_do_nee(False)
    e.begin_iteration(True)
    st = e.render_passes(passes)
    e.build_sdtree(); e.end_iteration(); e.end_render()
    return st


def queries(n=5000, seed=4):
    rng = np.random.RandomState(seed)
    pos = (rng.rand(n, 3) * [550, 540, 550]).astype(f32)
    d = rng.randn(n, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return pos, d.astype(f32)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("name,extra", TREES)
def test_the_oracles_file_answers_queries_as_the_oracle_does(oracle_lib, tmp_path, name, extra):
    sc = scene()
    PROPS = dict(globals()["PROPS"], **extra)
    o = make_oracle(oracle_lib, **PROPS)
    o.set_scene(sc); o.begin_render()
    st = train(o, 0, 2)
    path = str(tmp_path / "oracle-01.sdt")
    o.dump_sdtree(path)
    g = hip(**PROPS)
    g.set_scene(sc); g.begin_render()
    g.load_sdtree(path, iter=o.sdtree_info().iter, passes_rendered=st.passes_rendered_total)
    info = g.sdtree_info()
    assert info.iter == 2 and info.is_built == 1 and info.n_leaves >= (10 if name == "fine" else 1)
    pos, d = queries()
    want = o.query_pdf(pos, d)
    assert len(np.unique(want)) > 100  # (a trained tree, not the uniform answer)
    assert np.array_equal(bits(g.query_pdf(pos, d)), bits(want))
    assert np.array_equal(bits(g.query_sample(pos, 77)), bits(o.query_sample(pos, 77)))


@pytest.mark.parametrize("name,extra", TREES)
def test_a_render_split_at_a_dump_equals_the_uninterrupted_one(tmp_path, name, extra):
    sc = scene()
    PROPS = dict(globals()["PROPS"], **extra)
    a = hip(**PROPS)
    a.set_scene(sc); a.begin_render()
    st = train(a, 0, 2)
    path = str(tmp_path / "a-01.sdt")
    a.dump_sdtree(path)
    it, passes = a.sdtree_info().iter, st.passes_rendered_total
    assert (it, passes) == (2, 3)
    sa = final(a, 4)
    b = hip(**PROPS)
    b.set_scene(sc); b.begin_render()
    b.load_sdtree(path, iter=it, passes_rendered=passes)
    print(name, "leaves in the file:", len(__import__("ppg_host").read_sdt(path)["leaves"]), "leaves loaded:", b.sdtree_info().n_leaves, "of", a.sdtree_info().n_leaves)
    sb = final(b, 4)
    assert np.array_equal(bits(a.read_film()), bits(b.read_film())) and a.read_film().mean() > 0.01
    assert np.array_equal(bits(a.read_variance()), bits(b.read_variance()))
    for k in ("rays", "path_length_sum", "vertices_committed", "samples", "passes_rendered_total"):
        assert getattr(sa, k) == getattr(sb, k), k
    assert sa.variance == sb.variance
    # and the file made a difference: the same final passes on the untrained tree give another film
    c = hip(**PROPS)
    c.set_scene(sc); c.begin_render()
    c.load_sdtree(_empty_file(tmp_path), iter=it, passes_rendered=passes)
    final(c, 4)
    assert not np.array_equal(c.read_film(), a.read_film())


def _empty_file(tmp_path):
    path = str(tmp_path / "empty.sdt")
    open(path, "wb").write(struct.pack("<16f", *np.eye(4).ravel()))
    return path


@pytest.mark.parametrize("name,extra", TREES)
def test_training_continued_from_a_file_leaves_the_same_next_dump(tmp_path, name, extra):
    sc = scene()
    PROPS = dict(globals()["PROPS"], **extra)
    a = hip(**PROPS)
    a.set_scene(sc); a.begin_render()
    st = train(a, 0, 1)
    first = str(tmp_path / "a-00.sdt")
    a.dump_sdtree(first)
    it, passes = a.sdtree_info().iter, st.passes_rendered_total
    train(a, 1, 1)
    a.dump_sdtree(str(tmp_path / "a-01.sdt"))
    b = hip(**PROPS)
    b.set_scene(sc); b.begin_render()
    b.load_sdtree(first, iter=it, passes_rendered=passes)
    train(b, 1, 1)
    b.dump_sdtree(str(tmp_path / "b-01.sdt"))
    want, got = open(tmp_path / "a-01.sdt", "rb").read(), open(tmp_path / "b-01.sdt", "rb").read()
    assert len(want) > 64 + 44 + 24 * 10 and want != open(first, "rb").read()
    assert got == want
    assert b.sdtree_info().iter == a.sdtree_info().iter == 2


@pytest.mark.parametrize("preset,iters", [("default", 2), ("fine", 2), ("improved", 3)])
def test_dump_load_dump_is_the_identity_up_to_the_mean(tmp_path, preset, iters):
    """mean = 1 / (4 pi w) * sum on the way out, sum' = mean * (4 pi w) on the way in, mean' = 1 / (4 pi w) * sum' on the way out again: the float
    roundings of 4 pi w, mean * t, 1 / t and factor * sum' lie between mean and mean', half an ulp each at most — 4 ulp bound them."""
    import ppg_host
    props = dict(PROPS, **(IMPROVED if preset == "improved" else FINE if preset == "fine" else {}))
    sc = scene()
    a = hip(**props)
    a.set_scene(sc); a.begin_render()
    st = train(a, 0, iters)
    one, two = str(tmp_path / "one.sdt"), str(tmp_path / "two.sdt")
    a.dump_sdtree(one)
    pos, d = queries()
    before = a.query_pdf(pos, d)
    b = hip(**props)
    b.set_scene(sc); b.begin_render()
    b.load_sdtree(one, iter=a.sdtree_info().iter, passes_rendered=st.passes_rendered_total)
    assert np.array_equal(bits(b.query_pdf(pos, d)), bits(before)) and len(np.unique(before)) > 100
    b.dump_sdtree(two)
    x, y = ppg_host.read_sdt(one), ppg_host.read_sdt(two)
    assert np.array_equal(x["camera"], y["camera"]) and len(x["leaves"]) == len(y["leaves"]) >= (1 if preset == "default" else 4)
    worst = 0
    for p, q in zip(x["leaves"], y["leaves"]):
        assert np.array_equal(bits(p["p"]), bits(q["p"])) and np.array_equal(bits(p["size"]), bits(q["size"]))
        assert p["weight"] == q["weight"] and p["num_nodes"] == q["num_nodes"]
        assert np.array_equal(p["node_children"], q["node_children"]) and np.array_equal(bits(p["node_sums"]), bits(q["node_sums"]))
        worst = max(worst, abs(int(bits(p["mean"])[0]) - int(bits(q["mean"])[0])))
    print("largest difference of a mean: %d ulp" % worst)
    assert worst <= 4
    # apart from the means the two files are the same bytes
    raw_one, raw_two = bytearray(open(one, "rb").read()), bytearray(open(two, "rb").read())
    for leaf in x["leaves"]:
        raw_one[leaf["offset"] + 24:leaf["offset"] + 28] = raw_two[leaf["offset"] + 24:leaf["offset"] + 28] = b"mean"
    assert raw_one == raw_two


def test_a_hand_written_file_with_a_hole(tmp_path):
    """the root split along x: the lower half is a leaf with a two-level quadtree, the upper half is not in the file"""
    e = hip(**PROPS)
    e.set_scene(scene()); e.begin_render()
    info = e.sdtree_info()
    lo, hi = np.array(info.aabb_min[:], f32), np.array(info.aabb_max[:], f32)
    size = (hi - lo).astype(f32)
    half = size.copy()
    half[0] = half[0] / f32(2)
    sums = [[1, 2, 1, 4], [0.5, 0.5, 1, 0]]  # node 1 hangs below slot 1 of the root; its slot 3 is empty
    children = [[0, 1, 0, 0], [0, 0, 0, 0]]
    path = str(tmp_path / "hand.sdt")
    with open(path, "wb") as f:
        f.write(struct.pack("<16f", *np.eye(4).ravel()))
        f.write(struct.pack("<7fQQ", *lo, *half, 0.25, 5, 2))
        for s, c in zip(sums, children):
            for j in range(4):
                f.write(struct.pack("<fH", s[j], c[j]))
    e.load_sdtree(path, iter=1, passes_rendered=1)
    t = e.read_sdtree()
    assert t["children"].tolist() == [[1, 2], [0, 0], [0, 0]] and t["axis"].tolist() == [0, 1, 1]
    assert t["sampling"]["num_nodes"].tolist() == [0, 2, 1] and t["sampling"]["stat_weight"].tolist() == [0, 5, 0]
    # directions at the centres of the 4 x 4 canonical cells (DTreeWrapper::canonicalToDir, GP:586-597), positions well inside either half
    cx, cy = np.meshgrid((np.arange(4) + 0.5) / 4, (np.arange(4) + 0.5) / 4, indexing="ij")
    cx, cy = cx.ravel(), cy.ravel()
    cos_t, phi = 2 * cx - 1, 2 * np.pi * cy
    sin_t = np.sqrt(1 - cos_t * cos_t)
    d = np.stack([sin_t * np.cos(phi), sin_t * np.sin(phi), cos_t], 1).astype(f32)
    mid = (lo + size / 2).astype(f32)
    uniform = f32(1) / (f32(4) * f32(np.pi))
    inside, hole = mid.copy(), mid.copy()
    inside[0], hole[0] = lo[0] + size[0] * 0.25, lo[0] + size[0] * 0.75
    got_hole = e.query_pdf(np.repeat(hole[None], 16, 0), d)
    assert np.array_equal(bits(got_hole), bits(np.full(16, uniform, f32)))

    def descend(px, py):  # QuadTreeNode::pdf (GP:232-245) in float32, factors multiplied from the leaf upwards
        node, factors = 0, []
        while True:
            idx = (1 if px >= 0.5 else 0) | (2 if py >= 0.5 else 0)
            px, py = (px * 2) % 1.0, (py * 2) % 1.0
            s = [f32(v) for v in sums[node]]
            if not s[idx] > 0:
                return f32(0)
            factors.append(f32(4) * s[idx] / (s[0] + s[1] + s[2] + s[3]))
            if children[node][idx] == 0:
                break
            node = children[node][idx]
        r = factors.pop()
        while factors:
            r = factors.pop() * r
        return r / (f32(4) * f32(np.pi))

    want = np.array([descend(x, y) for x, y in zip(cx, cy)], f32)
    assert len(np.unique(want)) == 4 and (want == 0).sum() == 1  # 0.5, 1, 2 and 0, over 4 pi
    assert np.array_equal(bits(e.query_pdf(np.repeat(inside[None], 16, 0), d)), bits(want))
    # samples: uniform directions in the hole are unit vectors all over the sphere; in the leaf none falls into the empty cell
    s = e.query_sample(np.repeat(inside[None], 4000, 0), 5)
    px, py = (s[:, 2] + 1) / 2, (np.arctan2(s[:, 1], s[:, 0]) % (2 * np.pi)) / (2 * np.pi)
    assert np.allclose(np.linalg.norm(s, axis=1), 1, atol=1e-5)
    assert not np.any((px > 0.76) & (px < 0.99) & (py > 0.26) & (py < 0.49))  # slot 1 of the root (x upper, y lower), slot 3 below it
    frac = np.mean((px >= 0.5) & (py >= 0.5))  # slot 3 of the root holds 4 of 8
    assert abs(frac - 0.5) < 5 * np.sqrt(0.25 / 4000)


def test_refusals_leave_the_context_as_it_was(tmp_path):
    import ppg_host
    sc = scene()
    ref = hip(**PROPS)
    ref.set_scene(sc); ref.begin_render()
    st = train(ref, 0, 1)
    good = str(tmp_path / "good-00.sdt")
    ref.dump_sdtree(good)
    train(ref, 1, 1); final(ref, 4)
    want = ref.read_film()

    e = hip(**PROPS)
    e.set_scene(sc)
    with pytest.raises(ppg_host.PPGError) as ei:  # before begin_render
        e.load_sdtree(good, 1, 1)
    assert ei.value.code == -3 and "render not begun" in str(ei.value)
    e.begin_render()
    e.set_do_nee(False); e.begin_iteration(False)
    with pytest.raises(ppg_host.PPGError) as ei:  # with an iteration open
        e.load_sdtree(good, 1, 1)
    assert ei.value.code == -3 and "an iteration is open" in str(ei.value)
    assert e.render_passes(1).passes_rendered_total == st.passes_rendered_total
    e.build_sdtree(); e.end_iteration()
    # a file whose boxes belong to another box
    info = e.sdtree_info()
    lo, size = np.array(info.aabb_min[:], f32), np.array(info.aabb_max[:], f32) - np.array(info.aabb_min[:], f32)
    other = str(tmp_path / "other.sdt")
    with open(other, "wb") as f:
        f.write(struct.pack("<16f", *np.eye(4).ravel()))
        f.write(struct.pack("<7fQQ", *lo, *(size * f32(0.7)), 0.25, 5, 1))
        f.write(struct.pack("<fHfHfHfH", 1, 0, 1, 0, 1, 0, 1, 0))
    with pytest.raises(ppg_host.PPGError) as ei:
        e.load_sdtree(other, 1, 1)
    assert ei.value.code == -1 and "the tree was trained on another scene" in str(ei.value) and "leaf 0 at offset 64" in str(ei.value)
    # a truncated file
    cut = str(tmp_path / "cut.sdt")
    open(cut, "wb").write(open(good, "rb").read()[:-5])
    with pytest.raises(ppg_host.PPGError) as ei:
        e.load_sdtree(cut, 1, 1)
    assert ei.value.code == -1 and "truncated" in str(ei.value)
    with pytest.raises(ppg_host.PPGError) as ei:
        e.load_sdtree(str(tmp_path / "missing.sdt"), 1, 1)
    assert ei.value.code == -1 and "cannot open" in str(ei.value)
    with pytest.raises(ppg_host.PPGError) as ei:
        e.load_sdtree(good, 31, 1)
    assert ei.value.code == -1
    # the context kept its tree and its counters: the rest of the render is the untouched one's
    assert e.sdtree_info().iter == 1
    train(e, 1, 1); final(e, 4)
    assert np.array_equal(bits(e.read_film()), bits(want))
    # a sharded context is refused by name
    s = hip(**PROPS)
    s.set_shard(0, 2, 8)
    s.set_scene(sc); s.begin_render()
    with pytest.raises(ppg_host.PPGError) as ei:
        s.load_sdtree(good, 1, 1)
    assert ei.value.code == -1 and "not supported yet" in str(ei.value)


def test_guide_only_cli_writes_the_stepwise_guide_only_render(tmp_path):
    import ppg_host
    from ppg_host.imageio import read_pfm
    xml = os.path.join(GOLDEN, "cbox", "cbox.xml")
    desc, props, _ = ppg_host.load_scene(xml, {}, width=16, height=12)
    props = dict(props, budget=12.0)
    a = hip(**props)
    a.set_scene(desc); a.begin_render()
    st = train(a, 0, 2)
    tree = str(tmp_path / "cbox-01.sdt")  # the name the dumpSDTree property gives the dump of iteration 1: the CLI goes on with 2
    a.dump_sdtree(tree)
    assert a.sdtree_info().iter == 2 and st.passes_rendered_total == 3
    b = hip(**props)
    b.set_scene(desc); b.begin_render()
    b.load_sdtree(tree, iter=2, passes_rendered=3)
    final(b, 3)  # the whole budget: 12 spp = 3 passes
    want = b.read_film()
    out = str(tmp_path / "out.pfm")
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "ppg_host", xml, "--size", "16x12", "-P", "budget=12", "--sdtree", tree, "--guide-only", "-q", "-o", out],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(bits(read_pfm(out)), bits(want)) and want.mean() > 0.01


def test_the_integrator_goes_on_with_the_usual_schedule_from_a_file(tmp_path):
    """a whole render that dumps as it goes (the dumpSDTree property: "<prefix>-NN.sdt" at the end of training iteration NN) against
    GuidedPathTracer(sdtree=...) started from either dump: the rest of the schedule, the same film"""
    import ppg_host
    from ppg_host.__main__ import sdtree_iter_from_name
    sc = scene()
    prefix = str(tmp_path / "whole")
    a = ppg_host.GuidedPathTracer(engine=hip(dumpSDTree=1, dumpPrefix=prefix, **PROPS))
    want = a.render(sc)
    assert [r["passes"] for r in a.iterations] == [1, 2, 4] and sorted(os.listdir(tmp_path)) == ["whole-00.sdt", "whole-01.sdt"]
    for name, rest in (("whole-00.sdt", [2, 4]), ("whole-01.sdt", [4])):
        path = str(tmp_path / name)
        b = ppg_host.GuidedPathTracer(engine=hip(**PROPS), sdtree=path, sdtree_iter=sdtree_iter_from_name(path))
        got = b.render(sc)
        assert [r["passes"] for r in b.iterations] == rest and [r["iter"] for r in b.iterations] == list(range(3 - len(rest), 3))
        assert np.array_equal(bits(got), bits(want)), name
        assert b.iterations[-1]["stats"][-1]["passes_rendered_total"] == 7


@pytest.mark.parametrize("budget_type,budget", [("spp", 12), ("seconds", 0.05)])
def test_guide_only_spends_the_whole_budget_on_one_final_iteration(tmp_path, budget_type, budget):
    import ppg_host
    sc = scene()
    a = hip(**PROPS)
    a.set_scene(sc); a.begin_render()
    train(a, 0, 2)
    tree = str(tmp_path / "t-01.sdt")
    a.dump_sdtree(tree)
    props = dict(PROPS, budgetType=budget_type, budget=budget)
    g = ppg_host.GuidedPathTracer(engine=hip(**props), sdtree=tree, sdtree_iter=2, guide_only=True)
    img = g.render(sc)
    assert len(g.iterations) == 1 and g.iterations[0]["iter"] == 2 and np.isfinite(img).all() and img.mean() > 0.01
    stats = g.iterations[0]["stats"]
    assert all(s["vertices_committed"] == 0 for s in stats)  # a final iteration records nothing
    if budget_type == "spp":  # 12 spp = 3 passes behind the 3 of the training: the stepwise render's film
        assert len(stats) == 1 and stats[0]["passes_rendered_total"] == 6
        b = hip(**props)
        b.set_scene(sc); b.begin_render()
        b.load_sdtree(tree, iter=2, passes_rendered=3)
        final(b, 3)
        assert np.array_equal(bits(img), bits(b.read_film()))
    else:
        assert len(stats) >= 1 and g.iterations[0]["passes"] == 4 * len(stats)
