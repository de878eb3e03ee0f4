"""The closest-hit traversal on the CPU (no GPU needed), through the host-only hooks of include/ppg_testhooks.h.

1. The traversal stack's bound.  The kernels' per-lane stacks hold 48 entries without a range check (csrc/ppg_device.h TStack); the
   builder keeps the STACK NEED of every tree it hands them — the most entries the ordered walk can leave behind — within that
   (csrc/ppg_hip.hip BvhBuilder::boundStack).  Nested triangles, on which the SAH sweep peels one triangle per level, gave
   trees that needed up to 78 before the bound was kept.
2. The host walker (ppg_debug_bvh_trace), which the GPU tests compare the kernels with bit for bit, against an all-triangles closest hit
   in numpy: in float32 exactly, and in float64 within 8 x the measured float32-float64 figure (tests/traversal_ref.py), on the ray
   classes of tests/test_traversal_gpu.py.

   Measured figures per scene (the largest over the ray classes that are compared; relative in t, absolute in u, v):
     cbox 1.7e-03   floor-and-clutter-502 3.4e-04   doubled-600 6.9e-05   doubled-room 1.3e-03   nested-400-0.8 9.4e-06
     full-top-cut 1.0e-03   coincident-600 5.4e-05
   The largest belong to rays from far away (1e4 scene extents: 1e-3; two extents, aimed at triangles of a hundredth of the scene: 1e-3 to
   3e-4); rays from inside the scene are between 1e-7 and 5e-5.  Where float32 cannot resolve a class at all — 8 x figure above a tenth
   of a triangle — only the exact comparisons are made (tests/traversal_ref.py RESOLVE).
"""
import os
import sys

import numpy as np
import pytest

import traversal_ref as tr
from conftest import ROOT
from test_bvh_host import build

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bvh_quality as bq  # noqa: E402

STACK = 48  # entries of the kernels' traversal stacks


@pytest.fixture(scope="module")
def lib(hip_lib_path):
    return bq.bind(hip_lib_path)


def _stack(lib, pos, idx, rays, max_leaf):
    pad = bq.scene_pad(pos)
    st = bq.stats(lib, pos, idx, pad, max_leaf)
    deepest = bq.trace(lib, pos, idx, pad, max_leaf, rays)[4]
    print("triangles", idx.shape[0], "leaf", max_leaf, "depth", st["depth"], "stack_need", st["stack_need"], "max_stack", deepest)
    assert deepest <= STACK  # (what the kernels would have written out of bounds)
    assert 0 < st["stack_need"] <= STACK
    assert deepest <= st["stack_need"]
    return st["stack_need"], deepest


@pytest.mark.parametrize("max_leaf", [1, 4, 8])
@pytest.mark.parametrize("name", list(bq.FIXTURES))
def test_stack_need_of_the_fixtures(lib, name, max_leaf):
    pos, idx, rays = bq.fixture(name)
    _stack(lib, pos, idx, rays, max_leaf)


@pytest.mark.parametrize("which", ["room", "torus"])
def test_stack_need_of_the_scenes(lib, which):
    import ppg_host
    desc = ppg_host.room_scene(64, 48, n_boxes=300) if which == "room" else ppg_host.torus_scene(64, 48)
    pos, idx = tr.pos_idx(desc)
    o, d = bq.camera_rays(desc.camera, np.random.default_rng(3), nx=24, ny=16)
    _stack(lib, pos, idx, bq.make_rays(o, d), 4)


@pytest.mark.parametrize("max_leaf", [1, 4, 8])
@pytest.mark.parametrize("n,r", tr.NESTED)
def test_stack_need_of_nested_triangles(lib, n, r, max_leaf):
    """the chain the SAH builds of them is rebuilt with medians where it would overrun; what is left of it still walks deep into the
    lanes' overflow arrays (more than 24 entries)"""
    pos, idx = tr.nested_soup(n, r)
    need, deepest = _stack(lib, pos, idx, tr.nested_rays(n, r), max_leaf)
    assert deepest > 24


def test_nested_triangles_keep_the_closest_hit(lib):
    """the rebuilt tree returns what an all-triangles closest hit returns"""
    for n, r in tr.NESTED:
        pos, idx = tr.nested_soup(n, r)
        rays = tr.nested_rays(n, r)
        t, orig = bq.trace(lib, pos, idx, bq.scene_pad(pos), 4, rays)[:2]
        t_ref, i_ref = tr.brute32(pos, idx, rays)
        assert (i_ref >= 0).sum() >= 32
        assert np.array_equal(orig, i_ref) and np.array_equal(t, t_ref)


@pytest.mark.parametrize("name", list(tr.SOUPS))
def test_host_walker_against_float64_brute_force(hip_lib_path, lib, name):
    pos, idx = tr.SOUPS[name]()
    pad = bq.scene_pad(pos)
    nodes, _ = build(hip_lib_path, pos, idx, pad, 4)
    rays, classes = tr.ray_classes(lib, pos, idx, nodes, 4, tr.SEEDS[name])
    t, orig = bq.trace(lib, pos, idx, pad, 4, rays)[:2]
    ref = tr.Reference64(pos, idx, rays, classes)
    # float32, all triangles: exact, no ray left out
    assert np.array_equal(orig, ref.i32), np.nonzero(orig != ref.i32)[0][:8]
    assert np.array_equal(t, ref.t32)
    # float64
    counted = ref.counted()
    print(name, "rays", rays.shape[0], "unsure %.4f" % ref.unsure_fraction(), "figure %.3g" % ref.scene_figure)
    for c in counted:
        print("   %-32s figure %.3g counted %d hits %d" % (c, ref.figure[c], counted[c], int((ref.i[classes[c]] >= 0).sum())))
    assert ref.unsure_fraction() <= 0.02
    assert min(counted.values()) >= 50
    assert ref.check(t, orig) == int((~ref.unsure & ref.applies).sum())


def test_the_bound_leaves_a_large_scene_its_tree(lib):
    """bench.py's room (1820 boxes, 1.4 M triangles): the SAH tree of it needs a few entries more than the kernels have.  The repair is
    local — subtrees of some dozen triangles at the bottom of the offending paths — and costs the traversal nothing: the same rays take the
    node steps they took in the unbounded tree (21723 for these 1296 camera rays, measured with the builder before the bound was kept).
    A repair that gives up the top of the tree for medians passes every other test here and renders a fifth slower."""
    import ppg_host
    desc = ppg_host.room_scene(1280, 720, n_boxes=1820, tess=8)
    pos, idx = tr.pos_idx(desc)
    o, d = bq.camera_rays(desc.camera, np.random.default_rng(3), nx=48, ny=27)
    pad = bq.scene_pad(pos)
    need = bq.stats(lib, pos, idx, pad, 4)["stack_need"]
    _, _, steps, _, deepest = bq.trace(lib, pos, idx, pad, 4, bq.make_rays(o, d))
    print("stack need", need, "deepest", deepest, "node steps", int(steps.sum()))
    assert deepest <= need <= STACK
    assert int(steps.sum()) <= 21723 * 1.01
