"""Every form of the closest-hit traversal, ray by ray, through ppg_debug_intersect_mode (include/ppg_testhooks.h):

    lane, lane_any, lane_vote   trace_closest4<ANY, SPH, VOTE>            (csrc/ppg_device.h)
    resume                      trace_closest4_resume under k_tail's protocol, suspend_lanes 1 and 8
    wave                        trace_closest4_wave with the render's 24-row stack and with one row (the prim = -2 fallback)
    ktrace                      the real k_trace of the scene's family: trace_slice_bvh4 + leaf_pairs, or trace_small  (csrc/ppg_kernels.h)

on scenes that reach what a render rarely does — the lanes' overflow arrays (the nested soup's rays walk 33 entries deep), a full top cut, ties
in every leaf, a parked traversal, the wave stack's overrun — and on rays chosen for the edges of the arithmetic (tests/traversal_ref.py
ray_classes).  Asserted, with no ray left out: every closest-hit mode returns LANE's record byte for byte (prim, t, and p / frame / wi,
which are functions of (prim, u, v): the record has no room for u, v themselves), lane_any reports a hit exactly where LANE does,
and LANE's (t, original triangle) equal the host walker's, which tests/test_traversal.py holds to an all-triangles closest hit.
Against float64: within 8 x the measured float32-float64 figure of the ray's class, unsure rays left out (tests/traversal_ref.py).

Before any launch a test asks the host hooks for the stack need of the very tree (<= 48): a tree beyond it would write out of bounds.

Measured float32-float64 figures per scene (largest over the classes that are compared; relative in t, absolute in u, v):
    cbox 1.7e-03   floor-and-clutter-502 3.4e-04   doubled-600 6.9e-05   doubled-room 1.3e-03   nested-400-0.8 9.4e-06
    full-top-cut 1.0e-03   coincident-600 5.4e-05
Intersection records (floor-and-clutter-502 with normals), float32 against float64 restatement of fill_isect: see
test_intersection_records_against_float64, which prints them.
"""
import contextlib
import os
import sys

import numpy as np
import pytest

import traversal_ref as tr
from conftest import ROOT
from test_bvh_host import build

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bvh_quality as bq  # noqa: E402

pytestmark = pytest.mark.gpu

CLOSEST = [("lane_vote", 0), ("resume", 1), ("resume", 8), ("wave", 0), ("wave", 1), ("ktrace", 0), ("ktrace", 3)]
# scene, leaf size, further environment of the context
CONFIGS = {
    "cbox": ("cbox", 4, {}),
    "cbox-force-bvh": ("cbox", 4, {"PPG_FORCE_BVH": "1"}),
    "floor-and-clutter-502": ("floor-and-clutter-502", 4, {}),
    "doubled-600": ("doubled-600", 4, {}),
    "doubled-room-leaf-1": ("doubled-room", 1, {}),
    "doubled-room-leaf-4": ("doubled-room", 4, {}),
    "doubled-room-leaf-8": ("doubled-room", 8, {}),
    "nested-400-0.8": ("nested-400-0.8", 4, {}),
    "full-top-cut": ("full-top-cut", 4, {}),
    "full-top-cut-no-topcut": ("full-top-cut", 4, {"PPG_NO_TOPCUT": "1"}),
    "coincident-600": ("coincident-600", 4, {}),
}


@contextlib.contextmanager
def _environment(leaf, extra):
    env = dict(extra, PPG_BVH_LEAF=str(leaf))
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _description(scene, pos, idx):
    import ppg_host
    if scene == "cbox":
        return ppg_host.cbox_scene(32, 32)
    if scene == "doubled-room":
        return tr.doubled_room()
    return tr.desc_of(pos, idx)


def _pad64(rays):
    extra = (-rays.shape[0]) % 64
    return np.concatenate([rays, rays[:extra]]) if extra else rays


class Run:
    """one context of one configuration: the rays through every mode"""

    def __init__(self, hip_lib_path, config):
        import ppg_host
        scene, leaf, extra = CONFIGS[config]
        self.pos, self.idx = tr.SOUPS[scene]()
        lib = bq.bind(hip_lib_path)
        pad = bq.scene_pad(self.pos)
        # the bound first, on the host: nothing is launched on a tree that needs more stack than the kernels have
        self.stack_need = bq.stats(lib, self.pos, self.idx, pad, leaf)["stack_need"]
        assert 0 < self.stack_need <= 48
        nodes, self.order = build(hip_lib_path, self.pos, self.idx, pad, leaf)
        self.rays, self.classes = tr.ray_classes(lib, self.pos, self.idx, nodes, leaf, tr.SEEDS[scene])
        self.n = self.rays.shape[0]
        self.t_host, self.orig_host, _, _, self.deepest = bq.trace(lib, self.pos, self.idx, pad, leaf, self.rays)
        padded = _pad64(self.rays)
        assert padded.shape[0] <= 4096
        with _environment(leaf, extra):
            eng = ppg_host.Engine.hip(budgetType="spp", budget=1, maxDepth=2, seed=1)
            eng.set_scene(_description(scene, self.pos, self.idx))
        self.out, self.stats = {}, {}
        for mode, param in [("lane", 0), ("lane_any", 0)] + CLOSEST:
            o, s = eng.debug_intersect_mode(padded, mode, param)
            self.out[mode, param], self.stats[mode, param] = o[: self.n], s
        self.old_hook = eng.debug_intersect(self.rays)
        if scene == "doubled-room":
            # the parked traversals: 4096 rays, every eighth from inside the room in a random direction (a walk of 3 to 20 steps), the
            # others from outside flying away (one step).  A wave parks what is left when most of its lanes are done, and a ray is parked
            # a second time only if it outlasts the next round's rays as well: with rays of similar lengths, and one ray to a round
            # (suspend_lanes = 1), that happens twice in 12288 rays; with this mix the short rays end a round at once.
            rng = np.random.default_rng(77 + leaf)
            lo, hi = self.pos.min(0).astype(np.float64), self.pos.max(0).astype(np.float64)
            d = rng.normal(size=(4096, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            o = rng.uniform(lo, hi, (4096, 3))
            short = np.arange(4096) % 8 != 0
            o[short] = (0.5 * (lo + hi) + d * 2.0 * (hi - lo).max())[short]
            self.long_rays = tr._rays(o, d)
            self.long_lane = eng.debug_intersect_mode(self.long_rays, "lane", 0)[0]
            self.long_resume = {p: eng.debug_intersect_mode(self.long_rays, "resume", p) for p in (1, 8)}
        eng.close()

    def orig(self, rec):
        return np.where(rec["prim"] >= 0, self.order[np.maximum(rec["prim"], 0)].astype(np.int32), -1)


@pytest.fixture(scope="module")
def runs(hip_lib_path):
    cache = {}

    def get(config):
        if config not in cache:
            cache[config] = Run(hip_lib_path, config)
        return cache[config]
    return get


def _same(a, b):
    return a.tobytes() == b.tobytes()


def _first_difference(a, b):
    bad = np.nonzero((a["prim"] != b["prim"]) | (a["t"].view(np.uint32) != b["t"].view(np.uint32)))[0]
    return bad[:8], a[bad[:4]], b[bad[:4]]


@pytest.mark.parametrize("config", list(CONFIGS))
def test_lane_equals_the_host_walker(runs, config):
    r = runs(config)
    lane = r.out["lane", 0]
    assert (lane["prim"] >= 0).sum() > r.n // 4
    assert np.array_equal(r.orig(lane), r.orig_host), np.nonzero(r.orig(lane) != r.orig_host)[0][:8]
    hit = r.orig_host >= 0
    assert np.array_equal(lane["t"][hit].view(np.uint32), r.t_host[hit].view(np.uint32))
    assert _same(lane, r.old_hook)  # ppg_debug_intersect runs the same traversal
    print(config, "stack need", r.stack_need, "deepest stack of these rays", r.deepest)
    if config.startswith("nested"):
        assert r.deepest > 24  # the rays of this scene do walk into the overflow arrays (k_trace's begin at 12)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_every_mode_equals_lane(runs, config):
    r = runs(config)
    lane = r.out["lane", 0]
    for key in CLOSEST:
        assert _same(r.out[key], lane), (key, _first_difference(r.out[key], lane))
    assert np.array_equal(r.out["lane_any", 0]["prim"] >= 0, lane["prim"] >= 0)
    assert r.stats["ktrace", 0][3] == (1 if config == "cbox" else 0)  # SMALL exactly where a render would use it
    assert r.stats["wave", 0][0] == 0  # with the render's stack the wave traversal abandons no ray


@pytest.mark.parametrize("config", list(CONFIGS))
def test_lane_against_float64_brute_force(runs, config):
    r = runs(config)
    ref = tr.Reference64(r.pos, r.idx, r.rays, r.classes)
    counted = ref.counted()
    print(config, "figure %.3g" % ref.scene_figure, "unsure %.4f" % ref.unsure_fraction(), {c: "%.2g" % ref.figure[c] for c in counted})
    assert ref.unsure_fraction() <= 0.02 and min(counted.values()) >= 50
    lane = r.out["lane", 0]
    assert ref.check(lane["t"], r.orig(lane)) == int((~ref.unsure & ref.applies).sum())


def test_resume_parks_traversals(runs):
    """scene (c).  With suspend_lanes = 1 a round of a wave parks one ray and 4096 rays are some 65 rounds: the counts are summed over
    the scene's three leaf sizes, per value of suspend_lanes."""
    once, twice = {1: 0, 8: 0}, {1: 0, 8: 0}
    for leaf in (1, 4, 8):
        r = runs("doubled-room-leaf-%d" % leaf)
        for p in (1, 8):
            rec, stats = r.long_resume[p]
            assert _same(rec, r.long_lane), (leaf, p, _first_difference(rec, r.long_lane))
            once[p] += int(stats[0])
            twice[p] += int(stats[1])
    print("parked once", once, "twice", twice)
    for p in (1, 8):
        assert once[p] >= 100 and twice[p] >= 10, (p, once, twice)


def test_wave_stack_overrun_falls_back_to_one_lane(runs):
    r = runs("coincident-600")
    print("fallbacks with one row", r.stats["wave", 1][0], "with 24 rows", r.stats["wave", 0][0], "steps", r.stats["wave", 1][1], r.stats["wave", 0][1])
    assert r.stats["wave", 1][0] >= 10 and r.stats["wave", 0][0] == 0
    assert _same(r.out["wave", 1], r.out["lane", 0])


def test_top_cut_full_and_absent(runs):
    full, none = runs("full-top-cut"), runs("full-top-cut-no-topcut")
    assert full.stats["wave", 0][2] == 64 and none.stats["wave", 0][2] == 0
    assert _same(full.out["wave", 0], none.out["wave", 0])


def test_ktrace_small_equals_ktrace_bvh(runs):
    small, bvh = runs("cbox"), runs("cbox-force-bvh")
    assert small.stats["ktrace", 0][3] == 1 and bvh.stats["ktrace", 0][3] == 0
    for key in (("ktrace", 0), ("ktrace", 3)):
        assert _same(small.out[key], bvh.out[key]), _first_difference(small.out[key], bvh.out[key])


def test_intersection_records_against_float64(hip_lib_path):
    """fill_isect of the closest-hit modes on floor-and-clutter-502 with per-vertex normals (every fourth triangle's flipped against the
    geometric normal) and one zero-area triangle, against a float64 restatement: within 8 x the largest difference between the
    restatement in float32 and in float64 on the counted rays, per field.  Hits within the bound of an edge (unsure rays) are left out;
    the zero-area triangle is never hit.
    Measured on the counted rays (float32 against float64 restatement, each with its own evaluation's barycentrics): p 2.3e-05, geo_n 4.6e-07,
    n 2.3e-04, s 1.1e-04, wi 2.1e-04."""
    import ppg_host
    pos, idx = tr.SOUPS["floor-and-clutter-502"]()
    pos, idx, nrm = tr.with_normals(pos, idx)
    degenerate = idx.shape[0] - 1
    lib = bq.bind(hip_lib_path)
    pad = bq.scene_pad(pos)
    assert 0 < bq.stats(lib, pos, idx, pad, 4)["stack_need"] <= 48
    _, order = build(hip_lib_path, pos, idx, pad, 4)
    rng = np.random.default_rng(611)
    k = 1024
    tri = pos[idx].astype(np.float64)
    target = np.einsum("mk,mkc->mc", rng.dirichlet([1.0, 1.0, 1.0], k), tri[rng.integers(0, idx.shape[0], k)])
    o = rng.uniform(pos.min(0), pos.max(0), (k, 3))  # (from inside the scene's box, aimed at points of triangles)
    rays = tr._rays(o, tr._unit(target - o))
    desc = tr.desc_of(pos, idx, normals=nrm)
    with _environment(4, {}):
        eng = ppg_host.Engine.hip(budgetType="spp", budget=1, maxDepth=2, seed=1)
        eng.set_scene(desc)
    lane = eng.debug_intersect_mode(rays, "lane", 0)[0]
    for mode, param in CLOSEST:
        assert _same(eng.debug_intersect_mode(rays, mode, param)[0], lane), (mode, param)
    eng.close()
    ref = tr.Reference64(pos, idx, rays, {"all": slice(0, k)})
    orig = np.where(lane["prim"] >= 0, order[np.maximum(lane["prim"], 0)].astype(np.int32), -1)
    assert not (orig == degenerate).any() and not (ref.i == degenerate).any()
    sel = ~ref.unsure & (ref.i >= 0) & (orig == ref.i)
    assert ref.unsure.mean() <= 0.02 and sel.sum() >= 500
    d = rays[sel, 4:7]
    want = tr.fill_isect_np(pos, idx, nrm, ref.i[sel], ref.uv[sel, 0], ref.uv[sel, 1], d, np.float64)
    in32 = tr.fill_isect_np(pos, idx, nrm, ref.i[sel], ref.uv32[sel, 0], ref.uv32[sel, 1], d, np.float32)
    flipped = (np.einsum("ij,ij->i", np.cross(tri[ref.i[sel], 1] - tri[ref.i[sel], 0], tri[ref.i[sel], 2] - tri[ref.i[sel], 0]), want["geo_n"]) < 0).sum()
    assert flipped >= 50  # hits on triangles whose normals point against the winding
    for field in ("p", "geo_n", "n", "s", "wi"):
        figure = float(np.abs(in32[field].astype(np.float64) - want[field]).max())
        err = float(np.abs(lane[field][sel].astype(np.float64) - want[field]).max())
        print(field, "figure %.3g" % figure, "device error %.3g" % err)
        assert err <= 8.0 * max(figure, 2.0 ** -24), field
    assert np.array_equal(lane["material"][sel], np.asarray(desc.tri_material)[ref.i[sel]].astype(np.int32))
    assert np.array_equal(lane["emitter"][sel], np.asarray(desc.tri_emitter)[ref.i[sel]].astype(np.int32))


def test_hook_refuses_what_it_cannot_run():
    import ppg_host
    eng = ppg_host.Engine.hip(budgetType="spp", budget=1, maxDepth=2, seed=1)
    eng.set_scene(ppg_host.cbox_scene(32, 32))
    rays = tr._rays(np.full((65, 3), 278.0), np.tile([[0.0, 0.0, 1.0]], (65, 1)))
    with pytest.raises(ppg_host.bindings.PPGError, match="multiple of 64"):
        eng.debug_intersect_mode(rays, "lane_vote")
    with pytest.raises(ppg_host.bindings.PPGError, match="negative"):
        eng.debug_intersect_mode(rays, "lane", -1)
    with pytest.raises(ppg_host.bindings.PPGError, match="above 31"):
        eng.debug_intersect_mode(rays, "resume", 32)
    out, stats = eng.debug_intersect_mode(rays[:0], "ktrace")
    assert out.shape == (0,) and not stats.any()
    for mode in ("lane", "resume", "wave", "ktrace"):  # a partial wave, a partial chunk
        assert _same(eng.debug_intersect_mode(rays, mode, 0)[0], eng.debug_intersect(rays)), mode
    eng.close()
