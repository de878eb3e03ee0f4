"""Heterogeneous participating media on the GPU (include/ppg.h ppg_set_media_volumes; the hetmedia kernel family, csrc PPG_HETMEDIA):
  1. the family's volume lookups item by item against the float64 restatement (tests/hetmedium_ref.py; its margins and what "undecided"
     means are written there: 8 x the float32 / float64 figure of the restatement per quantity, measured on the CPU);
  2. its two tracking routines item by item: success, draw counts and the tracked transmittance equal, the numbers within the margins;
  3. reduction: a heterogeneous medium bound where no path goes renders, bit for bit, what the media family renders without it;
  4. an absorbing ramp in closed form, inside a null-bounded slab and on the sensor;
  5. reduction in expectation: a const density and albedo against the homogeneous medium of the same sigmaT and albedo;
  6. shadow rays through an absorbing affine density against a float64 quadrature;
  7. the furnace: an albedo-1 grid of uneven density in a constant environment returns the environment;
  8. the refusals of the device path.
"""
import numpy as np
import pytest

import hetmedium_ref as R
from test_media_gpu import LE, EMITTER_QUAD, _box_quads, _camera, _cbox_with_hidden_quad, _outward, _render, _scene, _secant_bounds, _slab_scene, _word, hip

f32, f64 = np.float32, np.float64
pytestmark = pytest.mark.gpu


def _het(density, albedo, scale=1.0, **phase):
    return dict(type="heterogeneous", density=density, albedo=albedo, scale=scale, **phase)


# ------------------------------------------------------------------------------------------------ 1. and 2. item by item
@pytest.fixture(scope="module")
def hook_engine():
    """one scene that binds every medium of the item-by-item tests: media 0.. = hetmedium_ref.TRACK_MEDIA, then two media over the lookup
    grids; the volumes are numbered in the order bindings.flatten_media_volumes meets them (density, albedo per medium)"""
    import ppg_host
    from ppg_host.bindings import flatten_media_volumes
    desc = ppg_host.cbox_scene(8, 8)
    _, vols = R.lookup_items()
    desc.media = [m for _, m in R.TRACK_MEDIA] + [_het(vols[0], vols[1], 1.0)]
    desc.camera_medium = 1
    volumes, entries, _ = flatten_media_volumes(desc.media)
    index = {"exact": entries[-1].density, "rgb": entries[-1].albedo}
    e = hip(budgetType="spp", budget=4)
    e.set_scene(desc)
    yield e, index
    e.close()


def test_volume_lookups_against_float64(hook_engine):
    """ppg_debug_volume over 4096 points — random interior ones, every node exactly, points on the six faces and just outside them, far
    outside — of a 5 x 4 x 3 one-channel grid (placed exactly: a quarter turn, power-of-two scales) and a 3 x 3 x 2 RGB grid (a general
    rotation): within 8 x hetmedium_ref.FIGURES["lookup"] = 1.6e-07 of float64 (measured on the CPU), at most 1 % of the items undecided"""
    e, index = hook_engine
    items, vols = R.lookup_items()
    assert len(items) == 4096
    want, undecided = R.evaluate_lookup(items, vols, f64)
    send = items.copy()
    send["volume"] = np.where(items["volume"] == 0, index["exact"], index["rgb"])
    got = e.debug_volume(send)["value"].astype(f64)
    assert undecided.mean() <= 0.01
    d = R.deviation("lookup", got, want)
    sure = ~undecided
    zero = (want == 0).all(1)
    print("lookup: largest difference", float(d[sure].max()), "margin", R.MARGIN["lookup"], "items", int(sure.sum()), "undecided", int(undecided.sum()),
          "answering 0", int((zero & sure).sum()))
    assert (zero & sure).sum() > 100 and (~zero & sure).sum() > 3000
    assert np.all(got[sure & zero] == 0)  # outside the nodes the answer is 0 exactly
    assert d[sure].max() <= R.MARGIN["lookup"]


@pytest.mark.parametrize("index", range(len(R.TRACK_MEDIA)), ids=[name for name, _ in R.TRACK_MEDIA])
def test_tracking_against_float64(hook_engine, index):
    """ppg_debug_hetmedium against tests/hetmedium_ref.py in float64: on every item float64 can decide (at most 1 % it cannot) success, the
    draw counts of sampleDistance and of evalTransmittance and the tracked transmittance (one of 0, 0.5, 1) are equal, and t, sigma_s and
    transmittance lie within 8 x the restatement's float32 / float64 figures (hetmedium_ref.FIGURES: t 1.8e-07, sigma_s 4.6e-07,
    transmittance 1.0e-06 — measured on the CPU, never from the kernel)"""
    e, _ = hook_engine
    name, medium = R.TRACK_MEDIA[index]
    items = R.track_items(index, medium)
    got = e.debug_hetmedium(items)
    want = R.evaluate_track(medium, items, f64)
    undecided = want["undecided"]
    assert undecided.mean() <= 0.01
    sure = ~undecided
    print(name, "items", len(items), "undecided", int(undecided.sum()), "events", int(want["success"][sure].sum()), "mean draws", float(want["draws"][sure].mean()),
          "transmittance 0 / 0.5 / 1:", [int((want["eval_transmittance"][sure] == v).sum()) for v in (0.0, 0.5, 1.0)])
    for q in ("success", "draws", "eval_draws", "eval_transmittance"):
        assert np.array_equal(np.asarray(got[q])[sure], np.asarray(want[q])[sure].astype(np.asarray(got[q]).dtype)), q
    for q in ("t", "sigma_s", "transmittance"):
        d = R.deviation(q, got[q], want[q])
        print(name, q, "largest difference", float(d[sure].max()), "margin", R.MARGIN[q])
        assert d[sure].max() <= R.MARGIN[q], q
    if name == "const":  # a zero direction component against the default box: AABB::rayIntersect answers false, nothing is drawn
        zero = (items["d"] == 0).any(1)
        assert zero.sum() > 100 and not got["success"][zero].any() and not got["draws"][zero].any() and np.all(got["eval_transmittance"][zero] == 1)


# ------------------------------------------------------------------------------------------------ 3. reduction
def _foggy_cbox_with_hidden_quad(het):
    desc = _cbox_with_hidden_quad(True)  # (its medium 0 on the hidden quad)
    fog = dict(sigma_a=0.0001, sigma_s=0.0004, phase="hg", g=0.3)
    n = desc.n_triangles - 2
    if het:
        desc.media = [fog, _het(R.ramp_grid(R.placement(np.eye(3), 10.0, (180.0, 75.0, 160.0))), dict(value=0.5), 0.5)]
        desc.tri_media = np.concatenate([np.zeros(n, np.uint32), np.full(2, _word(interior=1), np.uint32)])
    else:
        desc.media, desc.tri_media = [fog], None
    desc.camera_medium = 1
    return desc


@pytest.mark.parametrize("nee", ["never", "always"])
def test_a_heterogeneous_binding_no_path_reaches_renders_the_same_bits(nee):
    """the foggy Cornell box (a homogeneous fog on the sensor) with and without a heterogeneous medium bound to the quad inside the closed
    short box: the hetmedia family against the media family, film and variance equal byte for byte"""
    props = dict(budgetType="spp", budget=60, sppPerPass=4, maxDepth=10, rrDepth=5, seed=11, nee=nee)
    a, va, ia = _render(_foggy_cbox_with_hidden_quad(False), **props)
    b, vb, ib = _render(_foggy_cbox_with_hidden_quad(True), **props)
    assert a.mean() > 0.01 and ia.is_built and ib.is_built
    assert np.array_equal(a.astype(f32).view(np.uint32), b.astype(f32).view(np.uint32))
    assert np.array_equal(va.astype(f32).view(np.uint32), vb.astype(f32).view(np.uint32))
    assert (ia.n_leaves, ia.n_sampling_nodes) == (ib.n_leaves, ib.n_sampling_nodes)


# ------------------------------------------------------------------------------------------------ 4. an absorbing ramp in closed form
RAMP_Z = (0.1, 0.3, 0.5, 0.7)  # the density at the nodes z = 1, 2, 3, 4
RAMP_SCALE = 2.0
STAT_PROPS = dict(budgetType="spp", budget=508, sppPerPass=4, seed=3, sampleCombination="discard")


def _ramp_medium():
    data = np.broadcast_to(np.asarray(RAMP_Z, f32)[:, None, None], (4, 2, 2)).copy()
    return _het(dict(data=data, min=(-40.0, -40.0, 1.0), max=(40.0, 40.0, 4.0), to_world=None), dict(value=0.0), RAMP_SCALE)


def _check_ramp(film, var, last, depth):
    """depth: the integral of the density between the two planes the medium acts between, per unit of z"""
    lo, hi = _secant_bounds(16, 16)
    le = np.asarray(LE, f64)
    upper = (le * np.exp(-RAMP_SCALE * depth * lo[..., None])).reshape(-1, 3).mean(0)
    lower = (le * np.exp(-RAMP_SCALE * depth * hi[..., None])).reshape(-1, 3).mean(0)
    mean = film.reshape(-1, 3).mean(0)
    se = np.sqrt((var / last).reshape(-1, 3).sum(0)) / 256
    print("ramp: mean", mean, "interval", lower, upper, "standard error", se)
    assert np.all(se > 0) and np.all(se < 0.05 * lower)
    assert np.all(mean >= lower - 5 * se) and np.all(mean <= upper + 5 * se)


def test_an_absorbing_ramp_in_closed_form():
    """the null-bounded slab z in [2, 3] holding a grid that spans z in [1, 4], nodes at z = 1, 2, 3, 4, the density rising linearly, albedo
    0: each pixel expects Le exp(-scale secant (rho(2) + rho(3)) / 2) over its footprint's secants, and the film's mean lies within 5
    standard errors of the interval's means.  Then the same medium on the sensor with the emitter inside the grid, at z = 3: the grid acts
    from z = 1 on, (rho(1) + rho(3)) / 2 over two units."""
    from test_coatings_gpu import _last_iteration_spp
    last = _last_iteration_spp(STAT_PROPS["budget"], STAT_PROPS["sppPerPass"])
    w = _word(interior=0)
    film, var, _ = _render(_slab_scene(w, w, media=[_ramp_medium()]), maxDepth=8, **STAT_PROPS)
    _check_ramp(film, var, last, (RAMP_Z[1] + RAMP_Z[2]) / 2)
    inside = [(-20, -20, 3), (-20, 20, 3), (20, 20, 3), (20, -20, 3)]  # faces the camera, like EMITTER_QUAD
    assert np.allclose(np.asarray(inside)[:, :2], np.asarray(EMITTER_QUAD)[:, :2])
    desc = _scene([(inside, 0, 0, 0)], [dict(type=0, reflectance=(0, 0, 0))], [dict(radiance=LE)], _camera(16, 16), media=[_ramp_medium()], camera_medium=1)
    film, var, _ = _render(desc, maxDepth=4, **STAT_PROPS)
    _check_ramp(film, var, last, (RAMP_Z[0] + RAMP_Z[2]) / 2 * 2)


# ------------------------------------------------------------------------------------------------ 5. reduction in expectation
def test_a_const_volume_reduces_to_the_homogeneous_medium_in_expectation():
    """the fog Cornell box of test_guiding_survives_fog at 32 x 32 with the homogeneous fog (sigmaT 0.0005, albedo 0.8) and with a
    heterogeneous one of const density 0.5 x scale 0.001 and const albedo 0.8: the means agree within 5 combined standard errors, and both
    renders build their SD-tree"""
    import ppg_host
    from test_coatings_gpu import _last_iteration_spp
    # (four times the samples of that test: at its 124 spp the last iteration's 64 leave a standard error of 6 % of the mean, too much for
    # "the standard error below 5 % of the mean", which keeps the comparison from passing by noise)
    props = dict(budgetType="spp", budget=508, sppPerPass=4, maxDepth=-1, rrDepth=5, seed=8, sampleCombination="discard")
    last = _last_iteration_spp(props["budget"], props["sppPerPass"])
    out = {}
    for key, medium in (("homogeneous", dict(sigma_a=0.0001, sigma_s=0.0004, phase="hg", g=0.3)),
                        ("heterogeneous", _het(dict(value=0.5), dict(value=0.8), 0.001, phase="hg", g=0.3))):
        desc = ppg_host.cbox_scene(32, 32)
        desc.media, desc.camera_medium = [medium], 1
        film, var, info = _render(desc, **props)
        assert np.isfinite(film).all() and info.is_built and info.n_leaves >= 1
        out[key] = film.reshape(-1, 3).mean(0), np.sqrt((var / last).reshape(-1, 3).sum(0)) / (32 * 32)
    (mh, sh), (mv, sv) = out["homogeneous"], out["heterogeneous"]
    print("fog: homogeneous", mh, "+-", sh, "heterogeneous", mv, "+-", sv)
    assert np.all(sh > 0) and np.all(sv > 0) and np.all(sv < 0.05 * mv)
    assert np.all(np.abs(mh - mv) <= 5 * np.sqrt(sh * sh + sv * sv))


# ------------------------------------------------------------------------------------------------ 6. shadow rays against quadrature
def test_direct_light_through_an_absorbing_affine_density_against_quadrature():
    """the direct-light scene of the homogeneous suite — a diffuse floor under a small quad emitter, maxDepth = 2, nee = always — inside an
    absorbing grid the sensor lies in, whose density rho = a + b x + c y trilinear interpolation reproduces: the optical depth of a segment
    is scale |AB| rho(midpoint), exactly.  The mean of the central 8 x 8 pixels against a float64 quadrature of
    rho_floor / pi  Le  T(eye -> p)  int T(p -> e) cos cos / r^2 dA  within 5 standard errors; and the standard error below 5 % of the value,
    so that the test cannot pass by noise."""
    import ppg_host
    from test_coatings_gpu import _last_iteration_spp
    rho_floor, le, scale = 0.7, np.asarray(LE, f64) * 20, 1.0
    a, b, c = 0.12, 0.004, 0.02  # rho = a + b x + c y: 0.02 .. 0.32 over the box
    lo, hi = np.array([-25.0, -0.5, -25.0]), np.array([25.0, 5.0, 25.0])
    rho = lambda p: a + b * p[..., 0] + c * p[..., 1]  # noqa: E731
    zz, yy, xx = np.meshgrid(np.linspace(lo[2], hi[2], 2), np.linspace(lo[1], hi[1], 3), np.linspace(lo[0], hi[0], 3), indexing="ij")
    data = (a + b * xx + c * yy).astype(f32)
    assert data.min() > 0 and data.max() < 1
    medium = _het(dict(data=data, min=tuple(lo), max=tuple(hi), to_world=None), dict(value=0.0), scale)
    floor = [(-20, 0, -20), (-20, 0, 20), (20, 0, 20), (20, 0, -20)]
    half, height = 0.5, 4.0
    emitter = [(-half, height, -half), (half, height, -half), (half, height, half), (-half, height, half)]
    eye, target = np.array([0.0, 3.0, -6.0]), np.array([0.0, 0.0, 0.0])
    cam = ppg_host.perspective_camera(eye, target, (0, 1, 0), 30.0, "x", 0.01, 100.0, 32, 32)
    desc = _scene([(emitter, 0, 0, 0), (floor, 1, -1, 0)], [dict(type=0, reflectance=(0, 0, 0)), dict(type=0, reflectance=(rho_floor,) * 3)], [dict(radiance=tuple(le))], cam,
                  media=[medium], camera_medium=1)
    props = dict(budgetType="spp", budget=508, sppPerPass=4, maxDepth=2, seed=21, nee="always", sampleCombination="discard")
    last = _last_iteration_spp(props["budget"], props["sppPerPass"])
    film, var, _ = _render(desc, **props)
    block = (slice(12, 20), slice(12, 20))
    mean = film[block].reshape(-1, 3).mean(0)
    se = np.sqrt((var[block] / last).reshape(-1, 3).sum(0)) / 64
    d = (target - eye) / np.linalg.norm(target - eye)
    left = np.cross((0.0, 1.0, 0.0), d); left /= np.linalg.norm(left)
    up = np.cross(d, left)
    t = np.tan(np.radians(30.0) / 2)
    sub = (np.arange(6) + 0.5) / 6
    px = (12 + (np.arange(8)[:, None] + sub[None, :]).reshape(-1)) / 32
    X, Y = np.meshgrid((1 - 2 * px) * t, (1 - 2 * px) * t)
    gx, gw = np.polynomial.legendre.leggauss(24)
    ex, ez = np.meshgrid(gx * half, gx * half)
    ew = np.outer(gw, gw) * half * half
    dirs = d[None, None, :] + X[..., None] * left[None, None, :] + Y[..., None] * up[None, None, :]
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    tc = -eye[1] / dirs[..., 1]
    p = eye + tc[..., None] * dirs
    e = np.stack([ex, np.full_like(ex, height), ez], -1).reshape(-1, 3)
    r = e[None, None, :, :] - p[:, :, None, :]
    dist = np.linalg.norm(r, axis=-1)
    geom = (r[..., 1] / dist) ** 2 / dist ** 2
    t_cam = np.exp(-scale * tc * rho((eye + p) / 2))
    t_shadow = np.exp(-scale * dist * rho((e[None, None, :, :] + p[:, :, None, :]) / 2))
    inner = np.sum(t_shadow * geom * ew.reshape(-1)[None, None, :], axis=-1)
    total = (rho_floor / np.pi * t_cam * inner).mean() * le
    # (the block's pixel columns are symmetric about the film's centre: the sign of the film's x axis does not matter, whatever the slope b)
    print("block mean", mean, "quadrature", total, "standard error", se, "difference in standard errors", (mean - total) / se)
    assert np.all(se > 0) and np.all(se < 0.05 * total)
    assert np.all(np.abs(mean - total) <= 5 * se)


# ------------------------------------------------------------------------------------------------ 7. the furnace
FURNACE = [("isotropic, nee never", {}, "never"), ("isotropic, nee always", {}, "always"),
           ("hg 0.8, nee never", dict(phase="hg", g=0.8), "never"), ("hg 0.8, nee always", dict(phase="hg", g=0.8), "always")]


@pytest.mark.parametrize("name,phase,nee", FURNACE, ids=[f[0] for f in FURNACE])
def test_furnace(name, phase, nee):
    """the null-bounded cube (edge 2) of the homogeneous suite in a constant environment of radiance 1 with an albedo-1 grid of uneven
    density (3 x 3 x 3 nodes between 0 and 1, empty ones among them, scale 2): the film's mean is 1 within 5 standard errors, no pixel is
    NaN or negative"""
    import ppg_host
    from test_coatings_gpu import _last_iteration_spp
    w = _word(interior=0)
    quads = [(q, 0, -1, w) for q in _outward(_box_quads((-1, -1, -1), (1, 1, 1)), (-1, -1, -1), (1, 1, 1))]
    cam = ppg_host.perspective_camera((0, 0, -6), (0, 0, 0), (0, 1, 0), 30.0, "x", 0.01, 100.0, 16, 16)
    data = np.random.RandomState(5).uniform(0.0, 1.0, (3, 3, 3)).astype(f32)
    data[0, 0, 0] = data[1, 1, 1] = data[2, 0, 1] = 0.0
    medium = _het(dict(data=data, min=(-1.25, -1.25, -1.25), max=(1.25, 1.25, 1.25), to_world=R.placement(R.rotation((1.0, 1.0, 0.0), 15.0), 1.0, (0.0, 0.0, 0.0))),
                  dict(value=1.0), 2.0, **phase)
    desc = _scene(quads, [dict(type="null")], [], cam, media=[medium], environment=(1.0, 1.0, 1.0))
    props = dict(budgetType="spp", budget=508, sppPerPass=4, maxDepth=-1, rrDepth=5, seed=31, nee=nee, sampleCombination="discard")
    last = _last_iteration_spp(props["budget"], props["sppPerPass"])
    film, var, _ = _render(desc, **props)
    assert np.isfinite(film).all() and (film >= 0).all()
    mean = film.reshape(-1, 3).mean(0)
    se = np.sqrt((var / last).reshape(-1, 3).sum(0)) / 256
    print(name, "mean", mean, "standard error", se, "difference in standard errors", (mean - 1) / np.maximum(se, 1e-30))
    assert np.all(se > 0) and np.all(se < 0.05)
    assert np.all(np.abs(mean - 1) <= 5 * se)


# ------------------------------------------------------------------------------------------------ 8. refusals of the device path
def test_the_device_path_refuses_by_code():
    import ppg_host
    from ppg_host.bindings import flatten_media_volumes
    e = hip(budgetType="spp", budget=8, sppPerPass=4, maxDepth=6, seed=2)
    desc = ppg_host.cbox_scene(16, 16)
    e.set_scene(desc)
    e.render()
    before = e.read_film().copy()
    smoke = _het(R.ramp_grid(), dict(value=0.5), 0.01)
    # a list against the wrong scene — binding words for more triangles than it has — and a grid too long to track: PPG_ERR_INVALID, and the
    # previous scene still renders, bit for bit
    other = ppg_host.cbox_scene(16, 16)
    other.media = [smoke]
    other.tri_media = np.full(other.n_triangles + 3, _word(interior=0), np.uint32)
    with pytest.raises(ppg_host.PPGError, match=r"media: tri_media has \d+ entries, the scene \d+ triangles") as err:
        e.set_scene(other)
    assert err.value.code == -1
    long = ppg_host.cbox_scene(16, 16)
    long.media, long.camera_medium = [_het(R.ramp_grid(), dict(value=0.5), 1e5)], 1
    with pytest.raises(ppg_host.PPGError, match="media volumes: entry 0: the grid is too long to track") as err:
        e.set_scene(long)
    assert err.value.code == -1
    e.render()  # (Engine.set_scene has taken the refused lists out of the context again)
    assert np.array_equal(e.read_film(), before)
    volumes, entries, keep = flatten_media_volumes([smoke])
    # between begin and end of a render: PPG_ERR_STATE
    e.begin_render()
    with pytest.raises(ppg_host.PPGError, match="media volumes: not between ppg_begin_render and ppg_end_render") as err:
        e.set_media_volumes(volumes, entries)
    assert err.value.code == -3
    e.end_render()
    # the hooks need a scene that binds a heterogeneous medium: a homogeneous one does not do
    fog = ppg_host.cbox_scene(16, 16)
    fog.media, fog.camera_medium = [dict(sigma_a=0.0001, sigma_s=0.0004)], 1
    for scene in (ppg_host.cbox_scene(16, 16), fog):
        e.set_scene(scene)
        with pytest.raises(ppg_host.PPGError, match="ppg_debug_volume: the scene binds no heterogeneous medium") as err:
            e.debug_volume(np.zeros(2, R.LOOKUP_ITEM_DTYPE))
        assert err.value.code == -3
        with pytest.raises(ppg_host.PPGError, match="ppg_debug_hetmedium: the scene binds no heterogeneous medium") as err:
            e.debug_hetmedium(np.zeros(2, R.TRACK_ITEM_DTYPE))
        assert err.value.code == -3
    # ... and refuse an index out of range, and a medium that is not heterogeneous
    both = ppg_host.cbox_scene(16, 16)
    both.media, both.camera_medium = [dict(sigma_a=0.0001, sigma_s=0.0004), smoke], 2
    e.set_scene(both)
    item = np.zeros(1, R.LOOKUP_ITEM_DTYPE)
    item["volume"] = 2
    with pytest.raises(ppg_host.PPGError, match="ppg_debug_volume: item 0: volume out of range") as err:
        e.debug_volume(item)
    assert err.value.code == -1
    track = np.zeros(1, R.TRACK_ITEM_DTYPE)
    track["d"] = (0, 0, 1)
    for medium, message in ((2, "medium out of range"), (0, "the medium is not heterogeneous")):
        track["medium"] = medium
        with pytest.raises(ppg_host.PPGError, match="ppg_debug_hetmedium: item 0: " + message) as err:
            e.debug_hetmedium(track)
        assert err.value.code == -1
    # a sharded render refuses a scene with a heterogeneous medium, whichever call comes second
    with pytest.raises(ppg_host.PPGError, match="participating media are not supported in a sharded render") as err:
        e.set_shard(0, 2, 8)
    assert err.value.code == -1
    e.set_scene(ppg_host.cbox_scene(16, 16))
    e.set_shard(0, 2, 8)
    with pytest.raises(ppg_host.PPGError, match="participating media are not supported in a sharded render") as err:
        e.set_scene(both)
    assert err.value.code == -1
    e.close()
