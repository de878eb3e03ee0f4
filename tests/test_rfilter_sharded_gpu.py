"""A filtered film in a render sharded by tiles (include/ppg.h "Footprint hook"; ppg_kernels.h k_halo_pack / k_halo_unpack /
k_film_resolve_owned): the ranks — in-process contexts on threads, their exchanges summed on the host behind a barrier — exchange the
border slots of their footprints and reproduce the unsharded filtered render bit for bit: every iteration's image, squared image and
weights, and the film.  (The unsharded film itself is pinned to the exact numpy splat by tests/test_rfilter_gpu.py.)"""
import threading

import numpy as np
import pytest

from conftest import CBOX_PROPS, IMPROVED
from test_rfilter_gpu import hip

pytestmark = pytest.mark.gpu

RES = (40, 28)  # no multiple of any tile size used here
TENT, GAUSS, LANCZOS = {"type": "tent"}, {"type": "gaussian"}, {"type": "lanczos", "lobes": 3}  # borders 1, 2, 3
BORDER = {"tent": 1, "gaussian": 2, "lanczos": 3}

# schedule -> (properties, passes per iteration — the last one final; GuidedPathTracer's own for the budget)
SCHEDULES = {
    # rounds of the optimiser with a learned fraction in the training iterations; the final iteration is ONE group, rendered by tiles
    "improved-31": (dict(CBOX_PROPS, budget=31, seed=9, **IMPROVED), [1, 2, 4, 8, 16]),
    # a final iteration of 64 passes = 4 groups: dealt whole at world = 2 (no exchange there), by tiles at world = 3 (one exchange per group)
    "plain-127": (dict(CBOX_PROPS, budget=127, seed=5, sppPerPass=1), [1, 2, 4, 8, 16, 32, 64]),
    # the final group of 16 passes cut into launches of a few passes each (PPG_BATCH_PATHS, read when the context is created)
    "plain-31-cut": (dict(CBOX_PROPS, budget=31, seed=6, sppPerPass=1), [1, 2, 4, 8, 16]),
}


def _dev():
    import torch
    return torch.device("cuda", 0)


def _np(ptr, n):
    import torch
    from ppg_host.distributed import _view
    return _view(torch, ptr, n, "<f4", _dev()).cpu().numpy().copy()


def _sum_views(views):
    import torch
    total = views[0].clone()
    for v in views[1:]:
        total += v
    for v in views:
        v.copy_(total)
    torch.cuda.synchronize()


class Run:
    """`world` contexts rendering `schedule` of cbox with film filter `rf`, tile-sharded; what the footprint hook saw."""

    def __init__(self, rf, schedule, world=1, tile=16, hook=True, cancel=None):
        import ppg_host
        import torch
        from ppg_host.distributed import RenderAborted, _view
        props, passes = SCHEDULES[schedule]
        dev, n = _dev(), RES[0] * RES[1]
        scene = ppg_host.cbox_scene(*RES)
        scene.rfilter = rf
        self.engines = engines = [hip(**props) for _ in range(world)]
        barrier = threading.Barrier(world, timeout=120)  # (a rank that misses an exchange breaks the barrier instead of hanging the test)
        self.calls = [[] for _ in range(world)]       # per rank: (index of the render_passes_nostat call, n_floats, local_status)
        self.max_owners = 0                           # most ranks that held a non-zero float at one position of the halo buffer
        halos, statuses, slots = [None] * world, [0] * world, [None] * world
        self.iteration = -1

        def foot_hook(r):
            def fn(ptr, count, status):
                self.calls[r].append((self.iteration, count, status))
                view = _view(torch, ptr, count, "<f4", dev) if ptr else torch.zeros(count, dtype=torch.float32, device=dev)
                halos[r], statuses[r] = view.cpu().numpy().copy(), status
                barrier.wait()
                if r == 0:
                    self.max_owners = max(self.max_owners, int(sum((h != 0).astype(np.int32) for h in halos).max()))
                total = halos[0].copy()
                for h in halos[1:]:
                    total = total + h
                bad = any(statuses)
                view.copy_(torch.from_numpy(total))
                torch.cuda.synchronize()
                barrier.wait()
                if bad:
                    raise RenderAborted("a rank reported a failure")
            return fn

        def round_hook(r):  # every context applies the union of all ranks' records (include/ppg.h ppg_set_pass_hook)
            def fn():
                ptr, cnt = engines[r].adam_records()
                slots[r] = _view(torch, ptr, 4 * cnt, "<i8", dev).clone() if cnt else torch.zeros(0, dtype=torch.int64, device=dev)
                torch.cuda.synchronize()
                barrier.wait()
                union = torch.cat(slots).contiguous()
                keep.append(union)
                torch.cuda.synchronize()
                engines[r].adam_records_replace(union.data_ptr(), union.numel() // 4)
                barrier.wait()
            return fn
        keep = []

        def both(fn):
            errs = [None] * world

            def run(r):
                try:
                    fn(r)
                except Exception as ex:
                    errs[r] = ex
            ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
            [t.start() for t in ts]; [t.join() for t in ts]
            return errs

        for r, e in enumerate(engines):
            if hook:
                e.set_footprint_hook(foot_hook(r))
            e.set_scene(scene)
            if world > 1:
                e.set_shard(r, world, tile)
            e.begin_render()
            if world > 1 and props.get("bsdfSamplingFractionLoss", "none") != "none":
                e.set_pass_hook(round_hook(r))
        self.images, self.errors = [], None
        for it, p in enumerate(passes):
            final = it == len(passes) - 1
            self.iteration = it
            for e in engines:
                e.begin_iteration(final)
            if cancel is not None and cancel[0] == it:
                engines[cancel[1]].cancel()
            errs = both(lambda r: engines[r].render_passes_nostat(p))
            if any(errs):
                self.errors = errs
                return
            if world > 1:
                if final:
                    bufs = [e.final_partials() for e in engines]
                    assert all(b[1] == engines[0].final_partials_expected(p) for b in bufs)
                    _sum_views([_view(torch, b[0], b[1], "<f4", dev) for b in bufs])
                    for e in engines:
                        e.final_partials_commit()
                else:
                    for sel in (0, 1):
                        _sum_views([_view(torch, e.image_buffers()[sel], 3 * n, "<f4", dev) for e in engines])
                    _sum_views([_view(torch, e.image_weight_buffer(), n, "<f4", dev) for e in engines])
            per_rank = [(_np(e.image_buffers()[0], 3 * n), _np(e.image_buffers()[1], 3 * n), _np(e.image_weight_buffer(), n)) for e in engines]
            for other in per_rank[1:]:
                assert all(np.array_equal(a, b) for a, b in zip(per_rank[0], other))
            self.images.append(per_rank[0])
            for e in engines:
                e.finish_passes()
            if not final and world > 1:
                bufs = [e.stat_buffers() for e in engines]
                for k in range(2):
                    if bufs[0][k][1]:
                        _sum_views([_view(torch, b[k][0], b[k][1], "<i8", dev) for b in bufs])
            for e in engines:
                e.build_sdtree(); e.end_iteration()
        self.films = []
        for e in engines:
            e.end_render()
            self.films.append(e.read_film())

    def close(self):
        for e in self.engines:
            e.close()
        self.engines = []


def _calls_per_iteration(run, schedule, rank):
    counts = [0] * len(SCHEDULES[schedule][1])
    for it, _, _ in run.calls[rank]:
        counts[it] += 1
    return counts


_cache = {}


def _run(rf, schedule, world=1, tile=16, **kw):
    """one render per configuration and test session, shared by the tests below and left unchanged"""
    key = (None if rf is None else rf["type"], schedule, world, tile, tuple(sorted(kw.items())))
    if key not in _cache:
        run = Run(rf, schedule, world, tile, **kw)
        run.close()
        _cache[key] = run
    return _cache[key]


def _assert_equal_renders(got, ref):
    assert ref.errors is None and got.errors is None, got.errors
    assert len(got.images) == len(ref.images)
    for it, (a, b) in enumerate(zip(got.images, ref.images)):
        for name, x, y in zip(("image", "squared image", "weights"), a, b):
            assert np.array_equal(x, y), (it, name, float(np.abs(x - y).max()))
    assert np.isfinite(ref.films[0]).all() and ref.films[0].mean() > 1e-3
    for film in got.films:
        assert np.array_equal(film, ref.films[0])


# world 2 in tiles of 16: 3 tile columns, a checkerboard — horizontal and vertical borders cross ranks; world 3 in tiles of 8: 5 columns, the
# diagonal neighbours differ as well; tiles of 4 under lanczos' border of 3: a target lies two tiles from its source
LAYOUTS = [(2, 16, TENT), (2, 16, GAUSS), (2, 16, LANCZOS), (3, 8, TENT), (3, 8, GAUSS), (3, 8, LANCZOS), (3, 4, LANCZOS)]


@pytest.mark.parametrize("world,tile,rf", LAYOUTS, ids=lambda v: v["type"] if isinstance(v, dict) else str(v))
def test_sharded_filtered_render_equals_unsharded_with_learned_fraction(world, tile, rf):
    """training iterations in rounds of the optimiser (their images are what the inverse-variance film is made of), then a final
    iteration of one group rendered by tiles"""
    _assert_equal_renders(_run(rf, "improved-31", world, tile), _run(rf, "improved-31"))


def test_final_groups_dealt_whole_need_no_exchange():
    """64 final passes = 4 groups >= 2 per rank at world 2: every rank renders whole groups over the whole film and resolves them itself"""
    got = _run(GAUSS, "plain-127", 2, 16)
    _assert_equal_renders(got, _run(GAUSS, "plain-127"))
    for r in range(2):
        assert _calls_per_iteration(got, "plain-127", r) == [1, 1, 1, 1, 1, 1, 0]


def test_final_groups_by_tiles_exchange_once_per_group():
    """the same 4 groups at world 3 (fewer than two per rank): every rank renders every group on its tiles, one exchange per group"""
    got = _run(TENT, "plain-127", 3, 8)
    _assert_equal_renders(got, _run(TENT, "plain-127"))
    for r in range(3):
        assert _calls_per_iteration(got, "plain-127", r) == [1, 1, 1, 1, 1, 1, 4]


@pytest.mark.parametrize("world,tile,rf", [(2, 16, GAUSS), (3, 8, LANCZOS)], ids=lambda v: v["type"] if isinstance(v, dict) else str(v))
def test_a_group_cut_into_several_launches(monkeypatch, world, tile, rf):
    """the final group arrives in parts (launches of at most 2000 paths); its footprint is exchanged once, when it is complete"""
    ref = _run(rf, "plain-31-cut")
    monkeypatch.setenv("PPG_BATCH_PATHS", "2000")
    got = Run(rf, "plain-31-cut", world, tile)  # (not from the cache: the switch is read when a context is created)
    got.close()
    _assert_equal_renders(got, ref)
    for r in range(world):
        assert _calls_per_iteration(got, "plain-31-cut", r) == [1, 1, 1, 1, 1]


@pytest.mark.parametrize("world,tile,rf", [(2, 16, GAUSS), (3, 8, LANCZOS), (3, 4, LANCZOS)], ids=lambda v: v["type"] if isinstance(v, dict) else str(v))
def test_halo_buffers_have_disjoint_supports(world, tile, rf):
    from ppg_host.bindings import footprint_halo_floats
    run = _run(rf, "improved-31", world, tile)
    want = footprint_halo_floats(RES[0], RES[1], tile, world, BORDER[rf["type"]])
    assert want > 0 and run.max_owners == 1
    for r in range(world):
        assert run.calls[r] and all(count == want and status == 0 for _, count, status in run.calls[r])
        assert _calls_per_iteration(run, "improved-31", r) == [1, 1, 1, 1, 1]


def test_no_hook_calls_without_borders_to_exchange():
    """one rank, or the default box: the installed hook is never called (and the default box still shards as it did)"""
    assert _run(GAUSS, "improved-31", 1, 16).calls == [[]]
    box = _run(None, "improved-31", 2, 16)
    assert box.calls == [[], []]
    _assert_equal_renders(box, _run(None, "improved-31", 1, 16, hook=False))


def test_hook_decides_whether_the_combination_is_accepted():
    import ppg_host
    from ppg_host.bindings import PPGError
    desc = ppg_host.cbox_scene(16, 16)
    for order in ("filter-first", "shard-first"):
        e = hip(budgetType="spp", budget=4)
        e.set_scene(desc)
        e.set_footprint_hook(lambda ptr, n, status: None)
        if order == "filter-first":
            e.set_rfilter(GAUSS); e.set_shard(1, 2, 8)
        else:
            e.set_shard(1, 2, 8); e.set_rfilter(GAUSS)
        with pytest.raises(PPGError, match="footprint") as ex:
            e.set_footprint_hook(None)  # the render set up here cannot do without it
        assert ex.value.code == -1
        e.set_rfilter(None)
        e.set_footprint_hook(None)      # the default box can
        with pytest.raises(PPGError, match="sharded filtered renders are not supported yet.*ppg_set_footprint_hook") as ex:
            e.set_rfilter(GAUSS)
        assert ex.value.code == -1
        e.close()


def test_a_cancelled_rank_still_makes_its_due_call():
    """rank 1 is cancelled before the third iteration's passes: it makes that call's one exchange with zeros and its status, both ranks
    learn of it there and return an error; no further calls"""
    from ppg_host.bindings import PPGError
    run = Run(GAUSS, "plain-31-cut", 2, 16, cancel=(2, 1))
    run.close()
    assert run.errors is not None and all(isinstance(ex, PPGError) for ex in run.errors), run.errors
    assert run.errors[1].code == -4 and "footprint hook failed" in str(run.errors[0])
    for r in range(2):
        assert _calls_per_iteration(run, "plain-31-cut", r) == [1, 1, 1, 0, 0]
    assert run.calls[1][-1][2] != 0 and run.calls[0][-1][2] == 0
