"""What renderBatch LAUNCHES, counted by the library's kernel timer (ppg_enable_kernel_timing / ppg_kernel_times).  Every schedule renders the
same bits, so the parity tests cannot see a kernel launched twice or not at all: these assertions follow from the plan of a batch
(csrc/ppg_batch_plan.h, DESIGN.md "Launch structure on MI355X") with kernel timing on — one stream, no split tail outside a round."""
import ctypes as C
import os

import pytest

pytestmark = pytest.mark.gpu

RES, SPP = 32, 4
TRAIN_THEN_FINAL = ((1, False), (2, False), (4, True))  # passes of an iteration, whether it is the final one: renderSPP's schedule for 28 spp
# the wavefront runs more than one bounce on so small a film: k_tail takes over below 200 live paths instead of 2 M
ENV = dict(PPG_TAIL_MIN="200", PPG_TAIL_DIV="1000000")
BASE = dict(budgetType="spp", budget=SPP * 7, maxDepth=-1, rrDepth=5, strictNormals=1, seed=7, sppPerPass=SPP)


def launch_table(case):
    """case: props (over BASE), env (over ENV), iterations (default TRAIN_THEN_FINAL), defer_depth, adam_regions, rfilter; timing=False renders
    the product's schedule instead (side streams: for a profiler to look at — the tables are empty then).
    Returns ({kernel name: (launches, units)} of the whole render, the same after each iteration)."""
    import ppg_host
    env = dict(ENV, **case.get("env", {}))
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        e = ppg_host.Engine.hip(**dict(BASE, **case.get("props", {})))  # (ppg_create reads the switches)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    if "defer_depth" in case:
        e._call("debug_set_defer_depth", C.c_int32(case["defer_depth"]))
    if "adam_regions" in case:
        e.set_adam_regions(case["adam_regions"])
    scene = ppg_host.cbox_scene(RES, RES)
    if "rfilter" in case:
        scene.rfilter = case["rfilter"]
    e.set_scene(scene)
    e.enable_kernel_timing(case.get("timing", True))
    nee = e.props["nee"]
    table = lambda: {k["name"]: (k["launches"], k["units"]) for k in e.kernel_times()}
    after = []
    e.begin_render()
    passes = 0
    for n, final in case.get("iterations", TRAIN_THEN_FINAL):
        e.set_do_nee(nee == "always" or (nee == "kickstart" and passes * SPP < 128))
        e.begin_iteration(final)
        e.render_passes(n)
        e.build_sdtree()
        e.end_iteration()
        passes += n
        after.append(table())
    e.end_render()
    total = table()
    e.close()
    return total, after


def launches(t, name):
    return t.get(name, (0, 0))[0]


def test_unbounded_paths_one_tail_one_commit_one_film_kernel_per_batch():
    total, after = launch_table({})
    assert total["k_generate"][1] == RES * RES * SPP * 7  # every path of every pass, once
    assert launches(total, "k_generate") >= 3
    assert launches(total, "k_tail") == launches(total, "k_generate")
    assert launches(total, "k_film") == launches(total, "k_generate")
    # without a loss nothing but k_commit commits, once per training batch — and nothing is committed in the final iteration
    training = after[1]
    assert launches(training, "k_commit") == launches(training, "k_generate") and launches(total, "k_commit") == launches(training, "k_commit")
    assert "k_commit_records" not in total and "k_tail(stragglers)" not in total
    assert launches(total, "k_trace") > launches(total, "k_generate")  # (the hand-over threshold above did its work)


def test_bounded_paths_have_no_tail():
    total, _ = launch_table(dict(props=dict(maxDepth=3)))
    assert total["k_generate"][1] == RES * RES * SPP * 7
    assert "k_tail" not in total and "k_tail(stragglers)" not in total
    assert launches(total, "k_trace") <= 3 * launches(total, "k_generate")
    assert launches(total, "k_film") == launches(total, "k_generate")


def test_a_final_iteration_commits_nothing():
    total, _ = launch_table(dict(props=dict(budget=SPP * 4), iterations=((4, True),)))
    assert total["k_generate"][1] == RES * RES * SPP * 4
    assert not [k for k in total if k.startswith("k_commit")]
    assert launches(total, "k_tail") == launches(total, "k_generate") == launches(total, "k_film")
