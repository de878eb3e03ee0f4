"""The re-optimised, cost-collapsed BVH under the traversal kernels: two scenes just above the 64-triangle LDS path that contain re-inserted
subtrees, merged leaves and ties — two room-sized triangles over 500 small ones, and every triangle twice — rendered by the GPU and by
the oracle (which walks a tree of its own).  Film and SD-tree must be equal bit for bit."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, make_oracle
from test_gpu_parity import assert_tree_equal, hip

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bvh_quality as bq  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 64, 48
PROPS = dict(budgetType="spp", budget=8, sppPerPass=4, maxDepth=6, rrDepth=5, seed=31)


def _scene(name):
    """the fixture's triangles, diffuse, one emitter (the two large triangles; of the doubled soup its first tenth), seen from outside"""
    import ppg_host
    pos, idx, _ = bq.fixture(name)
    n = idx.shape[0]
    emitter = np.full(n, -1, np.int32)
    emitter[: 2 if name.startswith("floor") else n // 10] = 0
    cam = ppg_host.scenes.perspective_camera((0.3, -3.2, 1.1), (0.0, 0.0, -0.1), (0, 0, 1), 45.0, "x", 0.01, 100.0, W, H)
    return ppg_host.SceneDesc(pos, idx, np.zeros(n, np.uint32), emitter, [dict(type=0, reflectance=(0.7, 0.6, 0.5))], [dict(radiance=(12.0, 12.0, 12.0))], cam)


@pytest.mark.parametrize("name", ["floor-and-clutter-502", "doubled-600"])
def test_film_and_sdtree_equal_the_oracle(oracle_lib, name):
    scene = _scene(name)
    g, o = hip(**PROPS), make_oracle(oracle_lib, threads=8, **PROPS)
    for e in (g, o):
        e.set_scene(scene)
        e.render()
    film, ref = g.read_film(), o.read_film()
    assert np.isfinite(ref).all() and (ref > 0).mean() > 0.05  # the camera sees lit surfaces
    assert np.array_equal(film, ref), np.abs(film - ref).max()
    assert_tree_equal(g.read_sdtree(), o.read_sdtree())
