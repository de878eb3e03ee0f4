"""Point, spot and directional emitters on the GPU (include/ppg.h ppg_set_delta_emitters; ppg_device.h delta_sample_direct, ppg_kernels.h
shade_one "Luminaire sampling").  The CPU oracle does not know these emitters, so nothing here is "GPU equals oracle":

  * the film of a direct-light-only scene equals a float64 restatement of every sample (pixel jitter, camera ray, plane hit, shadow segment
    against the occluder, rho/pi * cos * the emitter's sampleDirect value),
  * a point light matches, statistically, a tiny spherical area emitter of the same power — the path the oracle pins — and its own
    unguided render, with bounces and guiding switched on,
  * and the host paths (determinism, sharding, the C++ driver, validation, clearing the list) behave as for any other render."""
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import IMPROVED, ROOT
from test_rfilter_gpu import _rand
from test_rfilter_gpu import _tree_equal

f32 = np.float32
pytestmark = pytest.mark.gpu

W, H = 48, 40
SEED = 19
PROPS = dict(budgetType="spp", budget=16, sppPerPass=16, nee="always", maxDepth=3, seed=SEED)
RHO = 0.5
CAM = (0.0, 0.0, 4.0)                    # looks down -z at the floor z = 0, which fills the view
OCC = (0.25, 0.75, -0.45, 0.05, 0.8)     # x0, x1, y0, y1, z of the black rectangle between light and floor
LIGHT_P = (0.3, -0.2, 1.5)
TILT, CUTOFF, BEAM = math.radians(10), math.radians(25), math.radians(15)
SPOT_AXIS = (-math.sin(TILT) * math.sqrt(0.5), math.sin(TILT) * math.sqrt(0.5), -math.cos(TILT))   # 10 degrees off the normal
DIR_D = (math.sin(math.radians(30)), 0.0, -math.cos(math.radians(30)))   # the direction the light travels in: 30 degrees off the normal


def _frame(axis):
    """rows of a rotation whose last row is `axis`: world -> light frame"""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    s = np.cross(a, (0.0, 1.0, 0.0)); s /= np.linalg.norm(s)
    return np.stack([s, np.cross(a, s), a])


LIGHTS = {
    "point": dict(type="point", intensity=(3.0, 2.0, 1.0), position=LIGHT_P),
    "spot": dict(type="spot", intensity=(3.0, 2.0, 1.0), position=LIGHT_P, to_local=[float(v) for v in _frame(SPOT_AXIS).reshape(-1)],
                 cutoff_angle=CUTOFF, beam_width=BEAM),
    "directional": dict(type="directional", intensity=(3.0, 2.0, 1.0), direction=DIR_D),
}
POINT2 = dict(type="point", intensity=(0.5, 1.0, 2.5), position=(-0.9, 0.6, 1.1))


def hip(**props):
    import ppg_host
    return ppg_host.Engine.hip(**props)


def _scene(lights):
    """one-sided diffuse floor (reflectance 0.5) filling the view, a black rectangle above it, the given delta emitters; nothing else emits"""
    import ppg_host
    x0, x1, y0, y1, z = OCC
    pos = np.array([(-3, -3, 0), (3, -3, 0), (3, 3, 0), (-3, 3, 0), (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)], f32)  # normals +z
    idx = np.array([(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7)], np.uint32)
    cam = ppg_host.scenes.perspective_camera(CAM, (0.0, 0.0, 0.0), (0, 1, 0), 50.0, "x", 0.01, 100.0, W, H)
    return ppg_host.SceneDesc(pos, idx, np.array([0, 0, 1, 1], np.uint32), np.full(4, -1, np.int32),
                              [dict(type=0, reflectance=(RHO, RHO, RHO)), dict(type=0, reflectance=(0.0, 0.0, 0.0))], [], cam, delta_emitters=list(lights))


def _in_occluder(x, y):
    """inside the occluder's rectangle; within a relative 1e-4 of one of its edges"""
    x0, x1, y0, y1, _ = OCC
    ex, ey = 1e-4 * (x1 - x0), 1e-4 * (y1 - y0)
    inside = (x > x0) & (x < x1) & (y > y0) & (y < y1)
    edge = ((np.abs(x - x0) < ex) | (np.abs(x - x1) < ex)) & (y > y0 - ey) & (y < y1 + ey)
    edge |= ((np.abs(y - y0) < ey) | (np.abs(y - y1) < ey)) & (x > x0 - ex) & (x < x1 + ex)
    return inside, edge


def _value(light, p):
    """Emitter::sampleDirect at the floor points p[3, n] in float64: direction to the light wi[3, n], value[n] (a factor of `intensity`),
    falloff[n]"""
    n = p.shape[1]
    if light["type"] == "directional":
        d = np.asarray(light["direction"], np.float64)
        return np.repeat(-d[:, None], n, 1), np.ones(n), np.ones(n)
    d = np.asarray(light["position"], np.float64)[:, None] - p
    dist = np.linalg.norm(d, axis=0)
    wi = d / dist
    fall = np.ones(n)
    if light["type"] == "spot":
        R = np.asarray(light["to_local"], np.float64).reshape(3, 3)
        cos_t = (R @ -wi)[2]
        cut, beam = light["cutoff_angle"], light["beam_width"]
        ramp = (cut - np.arccos(np.clip(cos_t, -1, 1))) / (cut - beam)
        fall = np.where(cos_t <= math.cos(cut), 0.0, np.where(cos_t >= math.cos(beam), 1.0, ramp))
    return wi, fall / dist ** 2, fall


def _restate(desc, light, jitter, spp):
    """per pixel: the mean over `spp` samples of rho/pi * cos(theta) * value * visibility as a factor of the light's intensity (float64
    [H, W]), whether a sample's primary ray or shadow segment grazes an occluder edge, and how many of its samples are lit at full
    strength / shadowed / in the spot's transition zone / outside the cutoff cone.  jitter(sample, dim) -> [W * H] offsets in the pixel."""
    cam = desc.camera
    s2c, c2w = np.asarray(cam["sample_to_camera"], np.float64), np.asarray(cam["camera_to_world"], np.float64)
    pix = np.arange(W * H)
    total, grazing = np.zeros(W * H), np.zeros(W * H, bool)
    counts = {k: np.zeros(W * H, np.int32) for k in ("lit", "shadowed", "transition", "dark")}
    zo = OCC[4]
    for s in range(spp):
        sx, sy = (pix % W) + jitter(s, 0), (pix // W) + jitter(s, 1)
        q = s2c @ np.stack([sx / W, sy / H, np.zeros_like(sx), np.ones_like(sx)])
        d = q[:3] / q[3]
        d = c2w[:3, :3] @ (d / np.linalg.norm(d, axis=0))
        o = c2w[:3, 3:4]
        t_occ = (zo - o[2]) / d[2]
        hit_occ, edge1 = _in_occluder(o[0] + t_occ * d[0], o[1] + t_occ * d[1])   # the primary ray meets the black rectangle first
        p = o + (-o[2] / d[2]) * d
        assert (np.abs(p[0]) < 3).all() and (np.abs(p[1]) < 3).all()               # the floor fills the view
        wi, value, fall = _value(light, p)
        t_sh = zo / wi[2]                                                          # the shadow segment crosses the occluder's plane
        blocked, edge2 = _in_occluder(p[0] + t_sh * wi[0], p[1] + t_sh * wi[1])
        L = np.where(hit_occ | blocked, 0.0, RHO / math.pi * np.maximum(wi[2], 0.0) * value)
        total += L
        grazing |= edge1 | edge2
        floor = ~hit_occ
        counts["lit"] += floor & ~blocked & (fall == 1)
        counts["shadowed"] += floor & blocked & (fall > 0)
        counts["transition"] += floor & ~blocked & (fall > 0) & (fall < 1)
        counts["dark"] += floor & (fall == 0)
    return (total / spp).reshape(H, W), grazing.reshape(H, W), {k: v.reshape(H, W) for k, v in counts.items()}


def _seed_jitter(seed):
    pix = np.arange(W * H, dtype=np.uint32)
    return lambda s, dim: _rand(seed, pix, s, dim).astype(np.float64)


def _peak(light):
    """the unshadowed, unattenuated value right under the light, as a factor of its intensity"""
    return RHO / math.pi * (-DIR_D[2] if light["type"] == "directional" else 1.0 / LIGHT_P[2] ** 2)


def _render(desc, **extra):
    e = hip(**dict(PROPS, **extra))
    e.set_scene(desc)
    e.render()
    film = e.read_film()
    e.close()
    return film


# ---------------------------------------------------------------------------------------------- 1. exact direct light
@pytest.mark.parametrize("env", ["", "PPG_FORCE_BVH"])
@pytest.mark.parametrize("kind", ["point", "spot", "directional"])
def test_direct_light_equals_the_restatement_of_every_sample(monkeypatch, kind, env):
    """|film - want| <= 2e-5 want + 2e-5 peak in every pixel no sample of which grazes an occluder edge: the device chain is about 30
    rounded float32 operations (2e-6 relative), the bound ten times that; the absolute term covers the spot's transition zone, where the
    value falls to zero while the error of acos does not.  Every real defect (a missing 1/pi, the wrong falloff or distance, an MIS weight
    that is not 1) is at percent level."""
    if env:
        monkeypatch.setenv(env, "1")
    light = LIGHTS[kind]
    desc = _scene([light])
    film = _render(desc).astype(np.float64)
    base, grazing, counts = _restate(desc, light, _seed_jitter(SEED), 16)
    want = base[..., None] * np.asarray(light["intensity"], np.float64)
    peak = _peak(light) * np.asarray(light["intensity"], np.float64)
    ok = ~grazing
    print("%s%s: grazing pixels %d of %d" % (kind, " (bvh)" if env else "", grazing.sum(), W * H))
    assert grazing.sum() <= 0.02 * W * H
    err = np.abs(film - want) - (2e-5 * want + 2e-5 * peak)
    worst = np.unravel_index(np.argmax(np.where(ok[..., None], err, -np.inf)), err.shape)
    print("%s: largest |film - want| / bound = %.4f at %s (film %r, want %r)" % (
        kind, (np.abs(film - want) / (2e-5 * want + 2e-5 * peak))[ok].max(), worst, film[worst], want[worst]))
    # the test must bite: whole pixels of every class
    full = {k: int((v == 16).sum()) for k, v in counts.items()}
    print("%s: pixels lit / shadowed / transition / dark: %r" % (kind, full))
    assert full["lit"] >= 20 and full["shadowed"] >= 5
    if kind == "spot":
        assert full["transition"] >= 20 and full["dark"] >= 20
        assert ((counts["transition"] == 16) & ok & (base > 0.05 * _peak(light)) & (base < 0.95 * _peak(light))).sum() >= 10
    assert (film[ok] > 0).any() and (film[ok & (counts["shadowed"] == 16)] == 0).all()
    assert (err[ok] <= 0).all(), np.argwhere((err > 0).any(-1) & ok)[:10]


# ---------------------------------------------------------------------------------------------- 2. nee = never
@pytest.mark.parametrize("kind", ["point", "spot", "directional"])
def test_nee_never_renders_exact_zeros(kind):
    """nothing can hit such a light: without next-event estimation it contributes nothing (the reference's behaviour too)"""
    film = _render(_scene([LIGHTS[kind]]), nee="never")
    assert film.shape == (H, W, 3) and (film == 0).all()


# ---------------------------------------------------------------------------------------------- 3. scene box
def _tree_box(desc):
    e = hip(**PROPS)
    e.set_scene(desc)
    e.render()
    t = e.read_sdtree()
    e.close()
    return t["aabb_min"].astype(np.float64), t["aabb_max"].astype(np.float64)


def test_point_and_spot_positions_enlarge_the_scene_box_and_a_directional_light_does_not():
    far = (10.0, -7.0, 20.0)
    lo0, hi0 = _tree_box(_scene([]))
    assert not ((lo0 <= far) & (far <= hi0)).all()
    for kind in ("point", "spot"):
        lo, hi = _tree_box(_scene([dict(LIGHTS[kind], position=far)]))
        assert ((lo <= far) & (far <= hi)).all(), (kind, lo, hi)
        assert (lo <= lo0).all() and (hi >= hi0).all() and (hi - lo).max() > (hi0 - lo0).max()
        assert lo[2] == lo0[2] and hi[0] >= f32(10.0) and lo[1] == f32(-7.0)
    lo, hi = _tree_box(_scene([LIGHTS["directional"]]))
    assert np.array_equal(lo, lo0) and np.array_equal(hi, hi0)


# ---------------------------------------------------------------------------------------------- 4. unbiased with bounces and guiding
BOX = 556.0
P_LIGHT = (278.0 / BOX, 340.0 / BOX, 100.0 / BOX)   # at least 0.3 from every surface of the unit-size box (the front is open)
R_SPHERE = 0.005
N_SEEDS = 8


def _unit_cbox(lights=(), sphere=False):
    """ppg_host.cbox_scene(64, 48) with its own emitter switched off, scaled by 1 / 556 to unit size.  The scale is what the radius 0.005
    and the 0.3 clearance of this test presuppose: at the box's 556 units a sphere of radius 0.005 subtends sin(alpha) ~ 2e-5 and
    Sphere::sampleDirect's 1 - cos(alpha) is zero in float32, in the oracle-pinned code as in Mitsuba (pdf = inf, the emitter black)."""
    import ppg_host
    d = ppg_host.cbox_scene(64, 48)
    d.positions = (np.asarray(d.positions, np.float64) / BOX).astype(f32)
    d.camera = ppg_host.scenes.perspective_camera((278 / BOX, 273 / BOX, -800 / BOX), (278 / BOX, 273 / BOX, -799 / BOX), (0, 1, 0), 39.3077, "smaller",
                                                  10.0 / BOX, 2800.0 / BOX, 64, 48)
    d.tri_emitter = np.full_like(np.asarray(d.tri_emitter), -1)
    d.emitters = []
    d.delta_emitters = list(lights)
    if sphere:
        d.materials = list(d.materials) + [dict(type=0, reflectance=(0.0, 0.0, 0.0))]
        d.emitters = [dict(radiance=tuple(float(i / (math.pi * R_SPHERE ** 2)) for i in sphere))]
        d.spheres = [dict(center=P_LIGHT, radius=R_SPHERE, material=len(d.materials) - 1, emitter=0)]
    return d


def _clearance(desc, p):
    """smallest distance from p to a triangle of the scene (by its vertices, edges and interior: dense barycentric samples)"""
    pos, idx = np.asarray(desc.positions, np.float64), np.asarray(desc.indices)
    g = np.linspace(0, 1, 41)
    u, v = np.meshgrid(g, g)
    keep = u + v <= 1
    u, v = u[keep], v[keep]
    a, b, c = pos[idx[:, 0]], pos[idx[:, 1]], pos[idx[:, 2]]
    pts = a[:, None] + u[None, :, None] * (b - a)[:, None] + v[None, :, None] * (c - a)[:, None]
    return np.linalg.norm(pts - np.asarray(p), axis=2).min()


def _arm(desc, **extra):
    """films of N_SEEDS renders (127 samples, bounces, the IMPROVED preset) reduced to 8 x 6 block means: [seed, 6, 8] and the image means"""
    import ppg_host
    out = []
    for seed in range(N_SEEDS):
        props = dict(budgetType="spp", budget=127, maxDepth=10, rrDepth=10, strictNormals=1, hideEmitters=1, nee="always", seed=100 + seed, **IMPROVED)
        props.update(extra)
        img = ppg_host.GuidedPathTracer(engine=hip(**props)).render(desc).astype(np.float64).mean(2)
        out.append(img.reshape(6, 8, 8, 8).mean((1, 3)))
    return np.stack(out)


def _compare(name, x, y):
    """|mean1 - mean2| <= 4 sqrt(se1^2 + se2^2) for the whole image and for all but at most two of the 48 blocks (with 14 degrees of
    freedom a true match fails a block about once in a thousand)"""
    def stats(v):
        return v.mean(0), v.std(0, ddof=1) / math.sqrt(len(v))
    (mx, sx), (my, sy) = stats(x.mean((1, 2))), stats(y.mean((1, 2)))
    bound = 4 * math.hypot(sx, sy)
    print("%s: image means %.6g / %.6g, difference %.3g, bound %.3g (%.1f %% of the mean)" % (name, mx, my, abs(mx - my), bound, 100 * bound / mx))
    (bx, ex), (by, ey) = stats(x), stats(y)
    z = np.abs(bx - by) / (4 * np.sqrt(ex ** 2 + ey ** 2))
    print("%s: blocks over their bound: %d of 48 (largest ratio %.2f); median block bound %.1f %% of the block mean" % (
        name, (z > 1).sum(), z.max(), 100 * np.median(4 * np.sqrt(ex ** 2 + ey ** 2) / bx)))
    # the test has power: a 20 % error in the first arm would not pass the whole-image condition
    assert bound < 0.2 * mx, "standard errors too large to see a 20 % error: raise the sample count"
    assert abs(mx - my) <= bound
    assert (z > 1).sum() <= 2


def test_point_light_matches_a_tiny_sphere_emitter_and_its_unguided_render():
    intensity = (1.0, 1.0, 1.0)
    light = dict(type="point", intensity=intensity, position=P_LIGHT)
    a_desc, b_desc = _unit_cbox([light]), _unit_cbox(sphere=intensity)
    assert _clearance(a_desc, P_LIGHT) >= 0.3
    a = _arm(a_desc)
    assert a.mean() > 0 and np.isfinite(a).all()
    b = _arm(b_desc)                                                   # the sphere's finite size biases it by O((r / d)^2) < 1e-3
    c = _arm(a_desc, bsdfSamplingFraction=1.0, bsdfSamplingFractionLoss="none")
    _compare("point light vs sphere emitter", a, b)
    _compare("guided vs unguided", a, c)


# ---------------------------------------------------------------------------------------------- 5. two lights
def test_two_point_lights_add_up():
    """1024 samples of the exact scene with two point lights: the image mean equals the sum of the two single-light restatements (the
    pixel integrals on a 16 x 16 grid per pixel) within four standard errors of the mean over eight seeds"""
    lights = [LIGHTS["point"], POINT2]
    desc = _scene(lights)
    g = (np.arange(16) + 0.5) / 16
    grid = lambda s, dim: np.full(W * H, g[s % 16] if dim == 0 else g[s // 16])  # noqa: E731
    want = sum(_restate(desc, l, grid, 256)[0][..., None] * np.asarray(l["intensity"], np.float64) for l in lights).mean()
    means = np.array([_render(desc, budget=1024, seed=500 + s).astype(np.float64).mean() for s in range(8)])
    se = means.std(ddof=1) / math.sqrt(8)
    print("two lights: render mean %.7g, restatement %.7g, difference %.3g, 4 se %.3g" % (means.mean(), want, abs(means.mean() - want), 4 * se))
    assert 4 * se < 0.01 * want
    assert abs(means.mean() - want) <= 4 * se
    one = _restate(desc, lights[0], grid, 256)[0].mean() * np.mean(lights[0]["intensity"])
    assert abs(one - want) > 40 * se  # (one light alone is far outside the bound)


# ---------------------------------------------------------------------------------------------- 6. host paths
def _lit_cbox(w=64, h=48):
    """the Cornell box with its area light, a point light and a spot: area emitter 0, then the delta emitters"""
    import ppg_host
    d = ppg_host.cbox_scene(w, h)
    d.delta_emitters = [dict(type="point", intensity=(4e4, 3e4, 2e4), position=(150.0, 400.0, 150.0)),
                        dict(type="spot", intensity=(2e5, 2e5, 3e5), position=(400.0, 500.0, 200.0), to_local=[float(v) for v in _frame((-0.2, -1.0, 0.1)).reshape(-1)],
                             cutoff_angle=math.radians(30), beam_width=math.radians(20))]
    return d


GUIDED = dict(budgetType="spp", budget=31, maxDepth=10, rrDepth=10, strictNormals=1, nee="always", seed=23)


def test_render_with_delta_emitters_is_deterministic():
    import ppg_host
    props = dict(GUIDED, **IMPROVED)
    out = []
    for _ in range(2):
        gpt = ppg_host.GuidedPathTracer(engine=hip(**props))
        out.append((gpt.render(_lit_cbox()), gpt.engine.read_sdtree()))
    assert np.array_equal(out[0][0], out[1][0]) and np.isfinite(out[0][0]).all() and out[0][0].mean() > 0
    _tree_equal(out[0][1], out[1][1])
    plain = ppg_host.GuidedPathTracer(engine=hip(**props)).render(ppg_host.cbox_scene(64, 48))
    assert out[0][0].mean() > 1.2 * plain.mean()  # the lights are there


def test_two_shards_in_one_process_equal_the_unsharded_film():
    """every rank gets the same list: two contexts with shards 0 and 1 of 2, their buffers summed as a reducer would, against one context"""
    import torch
    import ppg_host
    from ppg_host.distributed import _view
    dev = torch.device("cuda", 0)
    w, h = 64, 48
    scene = _lit_cbox(w, h)
    props = dict(GUIDED, sppPerPass=1, budget=47)  # iterations of 1, 2, 4, 8 and a final one of 32 passes = two groups of 16
    ref_gpt = ppg_host.GuidedPathTracer(engine=hip(**props))
    ref_img = ref_gpt.render(scene)
    schedule = [it["passes"] for it in ref_gpt.iterations]
    assert schedule == [1, 2, 4, 8, 32]

    def total(views):
        t = views[0].clone()
        for v in views[1:]:
            t += v
        for v in views:
            v.copy_(t)
        torch.cuda.synchronize()

    engines = [hip(**props) for _ in range(2)]
    for r, e in enumerate(engines):
        e.set_scene(scene); e.set_shard(r, 2, 16); e.begin_render()
    n = w * h
    for it, p in enumerate(schedule):
        final = it == len(schedule) - 1
        for e in engines:
            e.set_do_nee(True)  # nee = always (renderSPP, GP:1362)
            e.begin_iteration(final)
        for e in engines:
            e.render_passes_nostat(p)
        if final:
            bufs = [e.final_partials() for e in engines]
            total([_view(torch, b[0], b[1], "<f4", dev) for b in bufs])
            for e in engines:
                e.final_partials_commit()
        else:
            for sel in (0, 1):
                total([_view(torch, e.image_buffers()[sel], 3 * n, "<f4", dev) for e in engines])
            total([_view(torch, e.image_weight_buffer(), n, "<f4", dev) for e in engines])
        for e in engines:
            e.finish_passes()
        if not final:
            bufs = [e.stat_buffers() for e in engines]
            for k in range(2):
                if bufs[0][k][1]:
                    total([_view(torch, b[k][0], b[k][1], "<i8", dev) for b in bufs])
        for e in engines:
            e.build_sdtree(); e.end_iteration()
    for e in engines:
        e.end_render()
        assert np.array_equal(e.read_film(), ref_img)
        _tree_equal(e.read_sdtree(), ref_gpt.engine.read_sdtree())
    assert ref_img.mean() > 0


def test_cpp_driver_equals_python_on_a_scene_with_delta_emitters(tmp_path):
    import ppg_host
    from test_cpp_host import read_pfm
    exe = os.path.join(ROOT, "practical-path-guiding_amd", "bin", "ppg_render")
    path = str(tmp_path / "cbox-lights.ppgs")
    ppg_host.save_scene(_lit_cbox(), path)
    props = dict(budgetType="spp", budget=28, maxDepth=10, rrDepth=10, strictNormals=1, nee="always", seed=4, **{k: v for k, v in IMPROVED.items() if k != "sppPerPass"})
    out = str(tmp_path / "out.pfm")
    args = [exe, "-q", "-o", out] + sum([["-D", "%s=%s" % kv] for kv in props.items()], [])
    r = subprocess.run(args + [path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    back = ppg_host.load_scene_file(path)
    assert len(back.delta_emitters) == 2
    img = ppg_host.GuidedPathTracer(engine=hip(**props)).render(back)
    assert np.array_equal(read_pfm(out), img) and img.mean() > 0
    lightless = ppg_host.GuidedPathTracer(engine=hip(**props)).render(ppg_host.cbox_scene(64, 48))
    assert not np.array_equal(img, lightless)


def test_set_delta_emitters_refuses_bad_values():
    import ppg_host
    from ppg_host.bindings import DeltaEmitter, PPGError
    e = hip(budgetType="spp", budget=4, nee="always")
    nan, inf = float("nan"), float("inf")
    bad = [(dict(LIGHTS["point"], intensity=(1.0, -0.5, 1.0)), "negative intensity"),
           (dict(LIGHTS["point"], intensity=(1.0, nan, 1.0)), "not finite"),
           (dict(LIGHTS["point"], position=(0.0, inf, 0.0)), "not finite"),
           (dict(LIGHTS["spot"], cutoff_angle=nan), "not finite"),
           (dict(LIGHTS["spot"], beam_width=0.0), "beam_width <= cutoff_angle"),
           (dict(LIGHTS["spot"], beam_width=CUTOFF * 1.01), "beam_width <= cutoff_angle"),
           (dict(LIGHTS["spot"], cutoff_angle=math.pi / 2, beam_width=1.0), "cutoff_angle < pi/2"),
           (dict(LIGHTS["spot"], cutoff_angle=2.0, beam_width=1.0), "cutoff_angle < pi/2"),
           (dict(LIGHTS["directional"], direction=(0.0, 0.0, 0.0)), "zero direction"),
           (dict(LIGHTS["directional"], direction=(nan, 0.0, 1.0)), "not finite")]
    for d, msg in bad:
        with pytest.raises(PPGError, match=msg) as ex:
            e.set_delta_emitters([LIGHTS["point"], d])
        assert ex.value.code == -1 and "delta emitter 1" in str(ex.value)
    unknown = DeltaEmitter.from_dict(LIGHTS["point"])
    unknown.type = 3
    with pytest.raises(PPGError, match="unknown type") as ex:
        e.set_delta_emitters([unknown])
    assert ex.value.code == -1
    # a refused list leaves the context's list as it was; the call is refused while a render is open
    e.set_delta_emitters([LIGHTS["point"]])
    with pytest.raises(PPGError):
        e.set_delta_emitters([bad[0][0]])
    e.set_scene(_scene([LIGHTS["point"]]))
    e.begin_render()
    with pytest.raises(PPGError, match="ppg_begin_render") as ex:
        e.set_delta_emitters([])
    assert ex.value.code == -3
    e.end_render()
    e.set_delta_emitters([])
    e.close()


def test_cleared_list_renders_the_lightless_scene_as_a_fresh_context_does():
    import ppg_host
    props = dict(budgetType="spp", budget=12, maxDepth=10, rrDepth=10, strictNormals=1, nee="always", seed=8)
    plain = ppg_host.cbox_scene(48, 40)
    fresh = hip(**props)
    fresh.set_scene(plain)
    fresh.render()
    want = fresh.read_film()
    e = hip(**props)
    e.set_scene(_lit_cbox(48, 40))
    e.render()
    lit = e.read_film()
    assert not np.array_equal(lit, want) and lit.mean() > want.mean()
    e.set_scene(_lit_cbox(48, 40))    # the context kept its list: the same film again
    e.render()
    assert np.array_equal(e.read_film(), lit)
    e.set_delta_emitters([])          # ppg_set_delta_emitters(ctx, NULL, 0), then ppg_set_scene with the lightless copy
    e.set_scene(plain)
    e.render()
    assert np.array_equal(e.read_film(), want)
    g = hip(**props)                  # and through the scene descriptions alone
    g.set_scene(_lit_cbox(48, 40))
    g.render()
    assert np.array_equal(g.read_film(), lit)
    g.set_scene(plain)
    g.render()
    assert np.array_equal(g.read_film(), want)
