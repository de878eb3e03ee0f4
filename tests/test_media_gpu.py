"""Homogeneous participating media on the GPU (include/ppg.h ppg_set_media; the media kernel family, csrc PPG_MEDIA):
  1. the family's device functions item by item against the float64 restatement (tests/medium_ref.py; its margins and what "unsure" means
     are written there: 8 x the float32 / float64 figure of the restatement, per quantity and item class, measured on the CPU);
  2. reduction: a media list whose only binding no path reaches renders, bit for bit, what the scene renders without it;
  3. an absorbing medium in closed form — on the sensor, inside a null-bounded slab, and an inconsistent pair;
  4. shadow rays through an absorber against a float64 quadrature of the direct-lighting integral;
  5. the furnace: an albedo-1 medium in a constant environment returns the environment;
  6. guiding survives fog;
  7. the refusals of the device path.
"""
import numpy as np
import pytest

import medium_ref as R

f32, f64 = np.float32, np.float64
pytestmark = pytest.mark.gpu


def hip(**props):
    import ppg_host
    return ppg_host.Engine.hip(**props)


def _word(**sides):
    from ppg_host.bindings import media_word
    return media_word(**sides)


# ------------------------------------------------------------------------------------------------ scenes of quads
def _box_quads(lo, hi):
    """the six faces of an axis-aligned box, wound to face outwards"""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    return [[(x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)], [(x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)],
            [(x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)], [(x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)],
            [(x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)], [(x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)]]


def _scene(quads, materials, emitters, camera, **more):
    """quads: (four vertices, material index, emitter index, binding word)"""
    import ppg_host
    pos, idx, tmat, tem, words = [], [], [], [], []
    for verts, mat, em, word in quads:
        b = len(pos)
        pos.extend(verts)
        idx.extend([(b, b + 1, b + 2), (b, b + 2, b + 3)])
        tmat.extend([mat] * 2); tem.extend([em] * 2); words.extend([word] * 2)
    return ppg_host.SceneDesc(np.array(pos, f32), np.array(idx, np.uint32), np.array(tmat, np.uint32), np.array(tem, np.int32), materials, emitters, camera,
                              tri_media=np.array(words, np.uint32) if any(words) else None, **more)


def _outward(quads, lo, hi):
    c = (np.asarray(lo, f64) + np.asarray(hi, f64)) / 2
    for q in quads:
        v = np.asarray(q, f64)
        assert np.dot(np.cross(v[1] - v[0], v[2] - v[0]), v.mean(0) - c) > 0
    return quads


def _render(desc, **props):
    e = hip(**props)
    e.set_scene(desc)
    e.render()
    film, var, info = e.read_film().astype(f64), e.read_variance().astype(f64), e.sdtree_info()
    e.close()
    return film, var, info


# ------------------------------------------------------------------------------------------------ 1. item by item
@pytest.fixture(scope="module")
def medium_runs():
    """every medium's items through ppg_debug_medium, once: {index: (items, device output)}"""
    import ppg_host
    desc = ppg_host.cbox_scene(8, 8)
    desc.media = [m for _, m in R.MEDIA]
    desc.camera_medium = 1
    e = hip(budgetType="spp", budget=4)
    e.set_scene(desc)
    runs = {}
    for k, (_, medium) in enumerate(R.MEDIA):
        items = R.items_for(k, medium)
        runs[k] = (items, e.debug_medium(items))
    e.close()
    return runs


@pytest.mark.parametrize("index", range(len(R.MEDIA)), ids=[name for name, _ in R.MEDIA])
def test_device_functions_against_float64(medium_runs, index):
    """ppg_debug_medium against tests/medium_ref.py in float64: the success flag equal on every item float64 can decide (at most 1 % cannot),
    every returned number within 8 x the restatement's own float32 / float64 figure of its quantity and item class (medium_ref.FIGURES:
    edge t 4.3e-06, pdf_success 3.0e-05, pdf_failure 8.7e-08, transmittance 3.9e-07, eval_transmittance 8.6e-08, wo 9.1e-04, phase 8.5e-05;
    random t 2.3e-04, pdf_success 1.8e-05, pdf_failure 1.4e-07, transmittance 6.2e-07, eval_transmittance 1.1e-07, wo 2.7e-05, phase 1.2e-04
    — measured on the CPU, never from the kernel)."""
    items, got = medium_runs[index]
    medium = R.MEDIA[index][1]
    want = R.evaluate(medium, items, f64)
    unsure = R.unsure(want, items, max(R.MARGIN[c]["t"] for c in R.CLASSES))
    assert unsure.mean() <= 0.01
    sure = ~unsure
    assert np.array_equal(got["success"][sure] != 0, want["success"][sure])
    cls = R.item_class(len(items))
    for q in R.QUANTITIES:
        d = R.difference(q, got[q], want[q])
        finite = np.isfinite(np.asarray(want[q], f64).reshape(len(items), -1)).all(axis=1)
        # where float64 is not finite (0 * inf of a channel without extinction) the device is not finite either
        assert not np.isfinite(np.asarray(got[q], f64).reshape(len(items), -1)[sure & ~finite]).all(axis=1).any(), q
        for ci, c in enumerate(R.CLASSES):
            sel = sure & finite & (cls == ci)
            worst = float(np.nanmax(d[sel])) if sel.any() else 0.0
            print(R.MEDIA[index][0], q, c, "largest difference", worst, "margin", R.MARGIN[c][q], "items", int(sel.sum()))
            assert worst <= R.MARGIN[c][q], (q, c, worst)


# ------------------------------------------------------------------------------------------------ 2. reduction
def _cbox_with_hidden_quad(bind):
    """the Cornell box with a small quad inside the closed short box, where no path goes; bind: the quad carries a medium"""
    import ppg_host
    desc = ppg_host.cbox_scene(32, 32)
    b, n = len(desc.positions), desc.n_triangles
    quad = np.array([[180, 80, 160], [190, 80, 160], [190, 80, 170], [180, 80, 170]], f32)
    desc.positions = np.concatenate([np.asarray(desc.positions, f32), quad])
    desc.indices = np.concatenate([np.asarray(desc.indices, np.uint32), np.array([[b, b + 1, b + 2], [b, b + 2, b + 3]], np.uint32)])
    desc.tri_material = np.concatenate([np.asarray(desc.tri_material, np.uint32), np.zeros(2, np.uint32)])
    desc.tri_emitter = np.concatenate([np.asarray(desc.tri_emitter, np.int32), np.full(2, -1, np.int32)])
    if bind:
        desc.media = [dict(sigma_a=0.01, sigma_s=0.02, phase="hg", g=0.3)]
        desc.tri_media = np.concatenate([np.zeros(n, np.uint32), np.full(2, _word(interior=0), np.uint32)])
    return desc


@pytest.mark.parametrize("nee", ["never", "always"])
def test_a_binding_no_path_reaches_renders_the_same_bits(nee):
    """three training iterations and the final one at 4 spp per pass (15 passes: 1, 2, 4, 8): the scene with the list runs the media family's
    kernels, the scene without it the base family's; film and variance are equal byte for byte"""
    props = dict(budgetType="spp", budget=60, sppPerPass=4, maxDepth=10, rrDepth=5, seed=11, nee=nee)
    a, va, ia = _render(_cbox_with_hidden_quad(False), **props)
    b, vb, ib = _render(_cbox_with_hidden_quad(True), **props)
    assert a.mean() > 0.01 and ia.is_built and ib.is_built
    assert np.array_equal(a.astype(f32).view(np.uint32), b.astype(f32).view(np.uint32))
    assert np.array_equal(va.astype(f32).view(np.uint32), vb.astype(f32).view(np.uint32))
    assert (ia.n_leaves, ia.n_sampling_nodes) == (ib.n_leaves, ib.n_sampling_nodes)


# ------------------------------------------------------------------------------------------------ 3. an absorber in closed form
LE = (1.0, 2.0, 3.0)
SIGMA_A = (0.05, 0.2, 0.4)
FOV = 40.0


def _camera(w, h):
    import ppg_host
    return ppg_host.perspective_camera((0, 0, 0), (0, 0, 1), (0, 1, 0), FOV, "x", 0.01, 100.0, w, h)


def _secant_bounds(w, h):
    """per pixel, the smallest and the largest sqrt(1 + X^2 + Y^2) over its footprint: the length of a camera ray between two planes z = const,
    one unit apart"""
    t = np.tan(np.radians(FOV) / 2)
    ex = (2 * np.arange(w + 1) / w - 1) * t
    ey = (2 * np.arange(h + 1) / h - 1) * t * h / w
    def lo_hi(e):
        a, b = np.abs(e[:-1]), np.abs(e[1:])
        lo = np.where(e[:-1] * e[1:] <= 0, 0.0, np.minimum(a, b))
        return lo, np.maximum(a, b)
    (xl, xh), (yl, yh) = lo_hi(ex), lo_hi(ey)
    return np.sqrt(1 + xl[None, :] ** 2 + yl[:, None] ** 2), np.sqrt(1 + xh[None, :] ** 2 + yh[:, None] ** 2)


def _check_absorbed(film, thickness):
    lo, hi = _secant_bounds(16, 16)
    sigma, le = np.asarray(SIGMA_A, f64), np.asarray(LE, f64)
    slack = 8 * R.FIGURES["random"]["transmittance"]  # 8 x the float32 / float64 figure of the restatement's transmittance
    upper = le * (np.exp(-sigma * thickness * lo[..., None]) + slack)
    lower = le * (np.exp(-sigma * thickness * hi[..., None]) - slack)
    print("absorber, thickness", thickness, "centre pixel", film[8, 8], "bounds", lower[8, 8], upper[8, 8])
    assert np.all(film >= lower) and np.all(film <= upper)


ABSORBER = dict(sigma_a=SIGMA_A, sigma_s=0.0)
EMITTER_QUAD = [(-20, -20, 5), (-20, 20, 5), (20, 20, 5), (20, -20, 5)]  # faces the camera (normal -z)


def test_absorbing_fog_on_the_sensor_in_closed_form():
    """the camera inside an absorbing fog, facing an emitter 5 units away: every pixel lies in [Le exp(-sigma d_max), Le exp(-sigma d_min)]
    over its footprint"""
    desc = _scene([(EMITTER_QUAD, 0, 0, 0)], [dict(type=0, reflectance=(0, 0, 0))], [dict(radiance=LE)], _camera(16, 16), media=[ABSORBER], camera_medium=1)
    film, _, _ = _render(desc, budgetType="spp", budget=8, sppPerPass=8, maxDepth=4, seed=3)
    _check_absorbed(film, 5.0)


def _slab_scene(front, back, camera=None, extra=(), **more):
    """a null-bounded slab z in [2, 3] between the camera and the emitter; front / back: the binding words of the face towards the camera
    and of the other five"""
    quads = [(EMITTER_QUAD, 0, 0, 0)] + list(extra)
    for k, q in enumerate(_outward(_box_quads((-30, -30, 2), (30, 30, 3)), (-30, -30, 2), (30, 30, 3))):
        quads.append((q, 1, -1, front if k == 0 else back))
    return _scene(quads, [dict(type=0, reflectance=(0, 0, 0)), dict(type="null")], [dict(radiance=LE)], camera or _camera(16, 16), **more)


def test_absorbing_slab_behind_null_boundaries_in_closed_form():
    """the same fog as the interior of a null-bounded slab one unit thick: two medium transitions, no medium outside"""
    w = _word(interior=0)
    film, _, _ = _render(_slab_scene(w, w, media=[ABSORBER]), budgetType="spp", budget=8, sppPerPass=8, maxDepth=8, seed=3)
    _check_absorbed(film, 1.0)


def test_absorbing_interior_of_an_analytic_sphere_behind_index_matched_glass():
    """the binding word of an analytic primitive: a unit sphere of the absorbing fog behind a `dielectric` boundary with intIOR = extIOR (no
    reflection, no bending), five units from the camera, in a constant environment of radiance Le and nothing else.  A camera ray at angle
    theta to the axis runs 2 sqrt(1 - 25 sin^2 theta) through the sphere, so every pixel lies in [Le exp(-sigma chord_max), Le exp(-sigma
    chord_min)] over its footprint; a pixel the sphere's outline crosses has chord_min = 0, one beside the sphere shows Le"""
    import ppg_host
    glass = dict(type="dielectric", eta=(1.0, 1.0, 1.0), reflectance=(1.0, 1.0, 1.0), specular=(1.0, 1.0, 1.0))
    sphere = dict(center=(0.0, 0.0, 5.0), radius=1.0, material=0, emitter=-1)
    desc = ppg_host.SceneDesc(np.zeros((0, 3), f32), np.zeros((0, 3), np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.int32), [glass], [], _camera(16, 16),
                              spheres=[sphere], environment=LE, media=[ABSORBER], sphere_media=np.array([_word(interior=0)], np.uint32))
    film, _, _ = _render(desc, budgetType="spp", budget=8, sppPerPass=8, maxDepth=8, seed=3)
    lo, hi = _secant_bounds(16, 16)
    chord = lambda sec: 2 * np.sqrt(np.maximum(0.0, 1 - 25 * (1 - 1 / sec ** 2)))  # noqa: E731
    sigma, le = np.asarray(SIGMA_A, f64), np.asarray(LE, f64)
    slack = 8 * R.FIGURES["random"]["transmittance"]
    upper = le * (np.exp(-sigma * chord(hi)[..., None]) + slack)
    lower = le * (np.exp(-sigma * chord(lo)[..., None]) - slack)
    print("sphere: centre pixel", film[8, 8], "bounds", lower[8, 8], upper[8, 8], "corner pixel", film[0, 0])
    assert chord(lo)[8, 8] > 1.99 and chord(lo)[0, 0] == 0
    assert np.all(film >= lower) and np.all(film <= upper)


def _floor_under_slab(front, back, media):
    """a diffuse floor at z = 9 lit by an emitter at z = 0 through the null-bounded slab z in [2, 3]; the camera sits between slab and floor
    and looks at the floor, so the slab lies between floor and emitter only.  front: the word of the face towards the emitter"""
    import ppg_host
    floor = [(-20, -20, 9), (-20, 20, 9), (20, 20, 9), (20, -20, 9)]  # faces -z, towards slab and emitter
    emitter = [(-5, -5, 0), (5, -5, 0), (5, 5, 0), (-5, 5, 0)]       # faces +z, towards slab and floor
    quads = [(emitter, 0, 0, 0), (floor, 2, -1, 0)]
    for k, q in enumerate(_outward(_box_quads((-30, -30, 2), (30, 30, 3)), (-30, -30, 2), (30, 30, 3))):
        quads.append((q, 1, -1, front if k == 0 else back))
    cam = ppg_host.perspective_camera((0, 0, 5), (0, 0, 6), (0, 1, 0), FOV, "x", 0.01, 100.0, 16, 16)
    return _scene(quads, [dict(type=0, reflectance=(0, 0, 0)), dict(type="null"), dict(type=0, reflectance=(0.8, 0.8, 0.8))], [dict(radiance=LE)], cam, media=media)


def test_an_inconsistent_pair_of_media_blocks_shadow_rays():
    """interior A on the slab's face towards the emitter, interior B on the others: a shadow segment that enters medium A finds itself leaving
    medium B, and Scene::evalTransmittance answers 0 — the floor behind the slab is black under emitter sampling with maxDepth = 2.
    With maxDepth = 2 the interaction cap alone blackens it, so a control lifts the cap (maxDepth = 6).  A and B have the same coefficients
    there, so only the rule tells the two renders apart: the consistent slab lights the floor by both strategies, the inconsistent one by
    BSDF-sampled paths alone, which follow the path's own medium and know no such rule.  Both strategies estimate the same integral I.
    The emitter samples carry the weight pE^2 / (pE^2 + pB^2) with pE = r^3 / (A h) >= 9^3 / (100 * 9) = 0.81 (r >= h = 9 the distance,
    A = 100 the emitter's area) and pB = cos / pi <= 1 / pi: at least 0.866.  The BSDF samples carry a weight w <= 1.  So the inconsistent
    mean is at most w / (0.866 + w) <= 0.536 of the consistent one; 0.75 leaves room for the noise of 8 x 256 samples."""
    two = [ABSORBER, dict(ABSORBER)]
    props = dict(budgetType="spp", budget=8, sppPerPass=8, seed=5, nee="always")
    black, _, _ = _render(_floor_under_slab(_word(interior=0), _word(interior=1), two), maxDepth=2, **props)
    assert np.all(black == 0)
    lit, _, _ = _render(_floor_under_slab(_word(interior=0), _word(interior=0), two), maxDepth=6, **props)
    blocked, _, _ = _render(_floor_under_slab(_word(interior=0), _word(interior=1), two), maxDepth=6, **props)
    print("floor means: consistent", lit.mean((0, 1)), "inconsistent", blocked.mean((0, 1)))
    assert np.all(lit.mean((0, 1)) > 0.01) and np.all(blocked.mean((0, 1)) < 0.75 * lit.mean((0, 1)))


# ------------------------------------------------------------------------------------------------ 4. shadow rays through an absorber
def test_direct_light_through_absorbing_fog_against_quadrature():
    """a diffuse floor under a small quad emitter, both inside an absorbing fog the sensor lies in; maxDepth = 2, nee = always: the mean of the
    central 8 x 8 pixels against a float64 quadrature of  rho / pi  Le  exp(-sigma d_cam)  int exp(-sigma r) cos cos / r^2 dA,  within 5
    standard errors of that mean (ppg_read_variance of the last iteration's 256 samples, as the other statistical tests take it)"""
    import ppg_host
    from test_coatings_gpu import _last_iteration_spp
    rho, sigma, le = 0.7, np.asarray((0.05, 0.1, 0.2), f64), np.asarray(LE, f64) * 20
    floor = [(-20, 0, -20), (-20, 0, 20), (20, 0, 20), (20, 0, -20)]            # y = 0, faces +y
    half, height = 0.5, 4.0
    emitter = [(-half, height, -half), (half, height, -half), (half, height, half), (-half, height, half)]  # faces -y
    for q, up in ((floor, 1), (emitter, -1)):
        v = np.asarray(q, f64)
        assert np.sign(np.cross(v[1] - v[0], v[2] - v[0])[1]) == up
    eye, target = np.array([0.0, 3.0, -6.0]), np.array([0.0, 0.0, 0.0])
    cam = ppg_host.perspective_camera(eye, target, (0, 1, 0), 30.0, "x", 0.01, 100.0, 32, 32)
    desc = _scene([(emitter, 0, 0, 0), (floor, 1, -1, 0)], [dict(type=0, reflectance=(0, 0, 0)), dict(type=0, reflectance=(rho,) * 3)], [dict(radiance=tuple(le))], cam,
                  media=[dict(sigma_a=tuple(sigma), sigma_s=0.0)], camera_medium=1)
    props = dict(budgetType="spp", budget=508, sppPerPass=4, maxDepth=2, seed=21, nee="always", sampleCombination="discard")
    last = _last_iteration_spp(props["budget"], props["sppPerPass"])
    assert last == 256
    film, var, _ = _render(desc, **props)
    block = (slice(12, 20), slice(12, 20))
    mean = film[block].reshape(-1, 3).mean(0)
    se = np.sqrt((var[block] / last).reshape(-1, 3).sum(0)) / 64
    # the quadrature: 6 x 6 positions per pixel, 24 x 24 Gauss points on the emitter
    d = (target - eye) / np.linalg.norm(target - eye)
    left = np.cross((0.0, 1.0, 0.0), d); left /= np.linalg.norm(left)
    up = np.cross(d, left)
    t = np.tan(np.radians(30.0) / 2)
    sub = (np.arange(6) + 0.5) / 6
    px = (12 + (np.arange(8)[:, None] + sub[None, :]).reshape(-1)) / 32
    X, Y = np.meshgrid((1 - 2 * px) * t, (1 - 2 * px) * t)  # (the central block is symmetric about the film's centre: the axes' signs do not matter)
    gx, gw = np.polynomial.legendre.leggauss(24)
    ex, ez = np.meshgrid(gx * half, gx * half)
    ew = np.outer(gw, gw) * half * half
    total = np.zeros(3)
    dirs = d[None, None, :] + X[..., None] * left[None, None, :] + Y[..., None] * up[None, None, :]
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    tc = -eye[1] / dirs[..., 1]
    p = eye + tc[..., None] * dirs
    e = np.stack([ex, np.full_like(ex, height), ez], -1).reshape(-1, 3)
    r = e[None, None, :, :] - p[:, :, None, :]
    dist = np.linalg.norm(r, axis=-1)
    cos_f = r[..., 1] / dist
    geom = cos_f * cos_f / dist ** 2  # the emitter faces straight down: both cosines are r_y / |r|
    for c in range(3):
        inner = np.sum(np.exp(-sigma[c] * dist) * geom * ew.reshape(-1)[None, None, :], axis=-1)
        total[c] = np.mean(rho / np.pi * le[c] * np.exp(-sigma[c] * tc) * inner)
    print("block mean", mean, "quadrature", total, "standard error", se, "difference in standard errors", (mean - total) / se)
    assert np.all(se > 0) and np.all(se < 0.05 * total)
    assert np.all(np.abs(mean - total) <= 5 * se)


# ------------------------------------------------------------------------------------------------ 5. the furnace
FURNACE = [
    ("isotropic, nee never", dict(sigma_t=1.0, albedo=1.0), "never"),
    ("hg 0.8, nee always", dict(sigma_t=1.0, albedo=1.0, phase="hg", g=0.8), "always"),
    ("coloured, balance", dict(sigma_t=(0.5, 1.0, 2.0), albedo=1.0), "never"),
]


@pytest.mark.parametrize("name,medium,nee", FURNACE, ids=[f[0] for f in FURNACE])
def test_furnace(name, medium, nee):
    """a null-bounded cube (edge 2: optical thickness about 2) of an albedo-1 medium in a constant environment of radiance 1, nothing else:
    the film's mean is 1 within 5 standard errors, no pixel is NaN or negative — the throughput update, the phase weight, the medium
    branch's roulette and both MIS weights"""
    import ppg_host
    from test_coatings_gpu import _last_iteration_spp
    w = _word(interior=0)
    quads = [(q, 0, -1, w) for q in _outward(_box_quads((-1, -1, -1), (1, 1, 1)), (-1, -1, -1), (1, 1, 1))]
    cam = ppg_host.perspective_camera((0, 0, -6), (0, 0, 0), (0, 1, 0), 30.0, "x", 0.01, 100.0, 16, 16)
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


# ------------------------------------------------------------------------------------------------ 6. guiding survives fog
def test_guiding_survives_fog():
    """the Cornell box in a thin scattering fog the sensor lies in: the render completes, the SD-tree is built, the film's mean lies within
    5 standard errors of the same scene rendered without guiding (bsdfSamplingFraction = 1) and below the fog-free mean"""
    import ppg_host
    from test_coatings_gpu import _last_iteration_spp
    props = dict(budgetType="spp", budget=124, sppPerPass=4, maxDepth=-1, rrDepth=5, seed=8, sampleCombination="discard")
    last = _last_iteration_spp(props["budget"], props["sppPerPass"])
    out = {}
    for key, fog, fraction in (("guided", True, 0.5), ("unguided", True, 1.0), ("clear", False, 0.5)):
        desc = ppg_host.cbox_scene(32, 32)
        if fog:
            desc.media = [dict(sigma_a=0.0001, sigma_s=0.0004, phase="hg", g=0.3)]
            desc.camera_medium = 1
        film, var, info = _render(desc, bsdfSamplingFraction=fraction, **props)
        assert np.isfinite(film).all() and info.is_built and info.n_leaves >= 1
        out[key] = film.reshape(-1, 3).mean(0), np.sqrt((var / last).reshape(-1, 3).sum(0)) / (32 * 32)
    (mg, sg), (mu, su), (mc, _) = out["guided"], out["unguided"], out["clear"]
    print("fog: guided", mg, "+-", sg, "unguided", mu, "+-", su, "clear", mc)
    assert np.all(np.abs(mg - mu) <= 5 * np.sqrt(sg * sg + su * su))
    assert np.all(mg < mc)


# ------------------------------------------------------------------------------------------------ 7. refusals of the device path
def test_the_device_path_refuses_by_code():
    import ppg_host
    e = hip(budgetType="spp", budget=8, sppPerPass=4, maxDepth=6, seed=2)
    desc = ppg_host.cbox_scene(16, 16)
    e.set_scene(desc)
    e.render()
    before = e.read_film().copy()
    # a list sized against another scene: PPG_ERR_INVALID, and the previous scene still renders, bit for bit
    other = ppg_host.cbox_scene(16, 16)
    other.media = [dict(sigma_a=0.1, sigma_s=0.1)]
    other.tri_media = np.full(other.n_triangles + 3, _word(interior=0), np.uint32)
    with pytest.raises(ppg_host.PPGError, match=r"media: tri_media has \d+ entries, the scene \d+ triangles") as err:
        e.set_scene(other)
    assert err.value.code == -1
    e.render()  # (Engine.set_scene has taken the refused list out of the context again)
    assert np.array_equal(e.read_film(), before)
    # between begin and end of a render: PPG_ERR_STATE
    e.begin_render()
    with pytest.raises(ppg_host.PPGError, match="media: not between ppg_begin_render and ppg_end_render") as err:
        e.set_media([dict(sigma_a=0.1, sigma_s=0.1)], camera_medium=1)
    assert err.value.code == -3
    e.end_render()
    # the hook needs a scene that binds a medium
    with pytest.raises(ppg_host.PPGError, match="the scene binds no medium") as err:
        e.debug_medium(R.items_for(0, R.MEDIA[0][1])[:4])
    assert err.value.code == -3
    # a sharded render refuses a scene with media, whichever call comes second
    fog = ppg_host.cbox_scene(16, 16)
    fog.media, fog.camera_medium = [dict(sigma_a=0.0001, sigma_s=0.0004)], 1
    e.set_scene(fog)
    with pytest.raises(ppg_host.PPGError, match="participating media are not supported in a sharded render") as err:
        e.set_shard(0, 2, 8)
    assert err.value.code == -1
    e.set_scene(ppg_host.cbox_scene(16, 16))
    e.set_shard(0, 2, 8)
    with pytest.raises(ppg_host.PPGError, match="participating media are not supported in a sharded render") as err:
        e.set_scene(fog)
    assert err.value.code == -1
    e.close()
