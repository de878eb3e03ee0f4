"""A filtered film rendered by TWO PROCESSES sharing one MI355X (run with -m gpu): the launcher of tests/test_two_ranks_one_gpu.py with
`StagedReducer`, whose footprint hook (TorchReducer.reduce_footprint, installed before the scene's filter meets the shard) carries the
border slots of the ranks' footprints through host memory over gloo — exchanges that really wait for another process, at the end of every
training call and once per group of the final iteration.  The film equals the unsharded filtered render bit for bit; a cancelled rank takes
its peer out of the render with it."""
import numpy as np
import pytest

import test_two_ranks_one_gpu as base
from conftest import CBOX_PROPS, IMPROVED

pytestmark = pytest.mark.gpu

_SHARD = 'e.set_scene(scene); e.set_shard(rank, world, case.get("tile", 32))\n'
_TRACER = 'gpt = ppg_host.GuidedPathTracer(engine=e, reducer=StagedReducer(dist, torch.device("cuda:0")))\n'
assert base.WORKER.count(_SHARD) == 1 and base.WORKER.count(_TRACER) == 1
# the same worker; the scene carries the case's film filter and the reducer installs its footprint hook before scene and shard are set
WORKER = base.WORKER.replace(_SHARD, 'scene.rfilter = case.get("rfilter")\nred = StagedReducer(dist, torch.device("cuda:0"))\nred.install(e)\n' + _SHARD) \
                    .replace(_TRACER, 'gpt = ppg_host.GuidedPathTracer(engine=e, reducer=red)\n')

# 63 spp: training iterations of 1 .. 16 passes in rounds of the optimiser, then 32 final passes = 2 groups, rendered by tiles (2 < 2 * world)
CASE = dict(scene="cbox", res=[96, 96], tile=16, rfilter={"type": "gaussian"}, props=dict(CBOX_PROPS, budget=63.0, seed=6, **IMPROVED))


def test_two_ranks_with_a_film_filter_equal_the_unsharded_render(tmp_path, monkeypatch):
    import ppg_host
    monkeypatch.setattr(base, "WORKER", WORKER)
    ranks = base._launch(tmp_path, CASE)
    scene = ppg_host.cbox_scene(*CASE["res"])
    scene.rfilter = CASE["rfilter"]
    e = ppg_host.Engine.hip(**CASE["props"])
    gpt = ppg_host.GuidedPathTracer(engine=e)
    img = gpt.render(scene)
    tree = e.read_sdtree()
    assert np.isfinite(img).all() and img.mean() > 1e-3
    for r in ranks:
        assert np.array_equal(r["passes"], [it["passes"] for it in gpt.iterations])
        assert np.array_equal(r["children"], tree["children"]) and np.array_equal(r["theta"], tree["theta"])
        assert np.array_equal(r["film"], img)
    box = ppg_host.GuidedPathTracer(engine=ppg_host.Engine.hip(**CASE["props"])).render(ppg_host.cbox_scene(*CASE["res"]))
    assert not np.array_equal(box, img)  # the filter is really in effect


@pytest.mark.parametrize("cancel_rank", [1, 0])
def test_two_ranks_with_a_film_filter_cancel(tmp_path, monkeypatch, cancel_rank):
    """cancel() on one rank after iteration 2: the peer learns of it in the next exchange — a round hook's, or the footprint hook's — and
    both leave with RenderAborted or a PPGError; neither hangs in a collective."""
    monkeypatch.setattr(base, "WORKER", WORKER)
    ranks = base._launch(tmp_path, dict(CASE, cancel_rank=cancel_rank, cancel_after=2), timeout=300)
    outcomes = [str(r["outcome"]) for r in ranks]
    assert all(o == "aborted" or o == "cancelled" or o.startswith("error: ppg error") for o in outcomes), outcomes
    assert all(int(r["iterations"]) == 3 for r in ranks)
