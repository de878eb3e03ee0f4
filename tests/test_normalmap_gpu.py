"""Mitsuba's normalmap and null BSDFs on the GPU (include/ppg.h PPG_MAT_NORMALMAP, PPG_BSDF_NULL; csrc: normal_frame, the top kernel family):

  1. the shading frame ray by ray: the hook ppg_debug_shading_frame — fill_isect_tex, then normal_frame or bump_frame, as shade_one calls
     them — against the float64 restatement of tests/normalmap_ref.py, for normal maps and (for the first time) bump maps;
  2. a mirror with a constant normal map tilted 10 degrees: which pixels show an emitter, predicted in float64, and their exact values;
  3. a constant-tilt normal map against a constant-slope bump map of the same tilt;
  4. the null BSDF: closed forms through one and several null surfaces, a null emitter, and a box with a null sheet in mid-air;
  5. the family changes nothing else: a scene that merely holds the two renders the same bits;
  6. ppg_set_scene's refusals on the device build.
The oracle knows none of this: the pins are restatements and closed forms.
"""
import numpy as np
import pytest

from conftest import CBOX_PROPS

import normalmap_ref as R

f32, f64 = np.float32, np.float64
pytestmark = pytest.mark.gpu
W, H = 48, 40


def hip(**props):
    import ppg_host
    return ppg_host.Engine.hip(**props)


# ------------------------------------------------------------------------------------------------ 1. frames, ray by ray
@pytest.fixture(scope="module")
def hook():
    """the hook's records of every case, for the normal map and for the bump map: one context, eight scenes of six triangles"""
    e = hip(**dict(CBOX_PROPS, budget=4))
    out = {}
    for key in ("normal_map", "bump"):
        for case in R.CASES:
            e.set_scene(R.scene(case, key))
            out[key, case] = e.debug_shading_frame(R.rays(case))
    e.close()
    return out


@pytest.mark.parametrize("key", ["normal_map", "bump"])
def test_the_hooks_frames_equal_the_restatement(hook, key):
    """About 3 000 of 4 000 rays hit the three quads (with `vt`, without, with interpolated normals) under four lookups (bilinear and
    nearest, repeat and clamp, uv scales and offsets that leave [0, 1]).  Tolerance: R.ALLOWANCE = 4 x R.FRAME_FIGURE, the largest
    deviation of the float32 numpy restatement from the float64 one over these rays, measured on the CPU by tests/test_normalmap.py —
    normal map 2.62e-6 -> 1.05e-5, bump map 2.74e-6 -> 1.10e-5 (absolute, on the components of unit vectors)."""
    tol = R.ALLOWANCE * R.FRAME_FIGURE[key]
    total = 0
    for case in R.CASES:
        g = hook[key, case]
        ref = R.frames(R.scene(case, key), R.rays(case), f64)
        keep = ref["keep"]
        total += int(keep.sum())
        assert 1.0 - keep.sum() / ref["hit"].sum() <= R.MAX_EXCLUDED
        sure = keep | ~ref["hit"]
        assert np.array_equal(g["material"][sure], ref["tri"][sure])  # (every triangle has its own material; -1: no hit)
        assert np.array_equal(g["prim"][~ref["hit"]], np.full((~ref["hit"]).sum(), -1))
        assert np.all(g["adapted"][keep] == 1) and not g["adapted"][~ref["hit"]].any()
        dev = {w: float(np.abs(g[w][keep].astype(f64) - ref[w][keep]).max()) for w in ("uv", "n", "s", "ps", "pt", "pn")}
        print(key, case, "kept", int(keep.sum()), "hook against float64:", dev, "allowed", tol)
        for w in ("n", "s", "ps", "pt", "pn"):
            assert np.isfinite(g[w]).all() and dev[w] <= tol, (case, w, dev[w], tol)
        assert dev["uv"] <= tol
        if key == "normal_map" and case == "nearest-repeat":  # no flip towards the geometric normal (the bump map has one)
            assert (g["pn"][keep & (ref["tri"] < 4)][:, 2] < 0).any()
        if key == "bump":
            assert np.all(g["pn"][keep & (ref["tri"] < 4)][:, 2] > 0)
    assert total >= 2900


def test_the_hook_without_an_adapter_returns_the_plain_frame():
    import ppg_host
    desc = ppg_host.cbox_scene(16, 12)
    e = hip(**dict(CBOX_PROPS, budget=4))
    e.set_scene(desc)
    rays = np.zeros((64, 8), f32)
    rng = np.random.RandomState(2)
    rays[:, 0:3] = (278.0, 273.0, -800.0)
    d = np.stack([rng.uniform(-0.2, 0.2, 64), rng.uniform(-0.2, 0.2, 64), np.ones(64)], 1)
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 7] = np.inf
    g, h = e.debug_shading_frame(rays), e.debug_intersect(rays)
    e.close()
    assert (g["prim"] >= 0).all() and np.array_equal(g["prim"], h["prim"]) and np.array_equal(g["material"], h["material"])
    assert not g["adapted"].any()
    for a, b in (("n", "n"), ("pn", "n"), ("s", "s"), ("ps", "s")):
        assert np.array_equal(g[a].view(np.uint32), h[b].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 2. a tilted mirror
RADIANCE = {1: (3.0, 2.0, 1.0), -1: (0.5, 1.5, 2.5)}  # the emitter at +x, and its mirror image at -x
SPECULAR = (0.75, 0.5, 0.25)
TILT = np.radians(10.0)
MIRROR_Z, EMITTER_Z = -4.0, -1.0
MIRROR_FOV = 24.0
EMITTER_X, EMITTER_Y = (0.42, 1.82), (-0.95, 0.95)


def mirror_texel(sign):
    n = np.array([sign * np.sin(TILT), 0.0, np.cos(TILT)])
    return ((n + 1.0) / 2.0).astype(f32)


def mirror_scene(sign):
    """Camera at the origin looking down -z at a perfect mirror in the plane z = -4 (texture coordinates (x, y): dpdu = +x) whose constant
    normal map tilts the normal by 10 degrees about y, towards sign * x; two black emitters in the plane z = -1 facing the mirror, outside
    the camera's own view, one the mirror image of the other."""
    import ppg_host
    pos = [[-3, -3, MIRROR_Z], [3, -3, MIRROR_Z], [3, 3, MIRROR_Z], [-3, 3, MIRROR_Z]]
    uv = [[p[0], p[1]] for p in pos]
    idx = [[0, 1, 2], [0, 2, 3]]  # normal +z
    tm, te = [0, 0], [-1, -1]
    for k, side in enumerate((1, -1)):
        x0, x1 = sorted((side * EMITTER_X[0], side * EMITTER_X[1]))
        b = len(pos)
        pos += [[x0, EMITTER_Y[0], EMITTER_Z], [x0, EMITTER_Y[1], EMITTER_Z], [x1, EMITTER_Y[1], EMITTER_Z], [x1, EMITTER_Y[0], EMITTER_Z]]
        uv += [[np.nan, np.nan]] * 4
        idx += [[b, b + 1, b + 2], [b, b + 2, b + 3]]  # normal -z
        tm += [1, 1]
        te += [k, k]
    mats = [dict(type="mirror", reflectance=SPECULAR, normal_map=0), dict(type=0, reflectance=(0.0, 0.0, 0.0))]
    cam = ppg_host.scenes.perspective_camera((0, 0, 0), (0, 0, -1), (0, 1, 0), MIRROR_FOV, "x", 0.01, 100.0, W, H)
    return ppg_host.SceneDesc(np.array(pos, f32), np.array(idx, np.uint32), np.array(tm, np.uint32), np.array(te, np.int32), mats,
                              [dict(radiance=RADIANCE[1]), dict(radiance=RADIANCE[-1])], cam, texcoords=np.array(uv, f32),
                              textures=[dict(rgb=np.broadcast_to(mirror_texel(sign), (2, 2, 3)).copy(), wrap_u="clamp", wrap_v="clamp")])


def predict(desc, sign, grid=5, margin=1e-3):
    """Per pixel, in float64: +1 / -1 = every sample of the pixel sees the emitter at +x / -x in the mirror, 0 = none sees either, 2 =
    boundary.  The pixel's four corners and, because a tilted normal on a flat mirror is not a virtual camera (the image of a pixel edge
    on the emitters' plane is slightly curved: of second order in the pixel's size, ~5e-4 here), a grid x grid lattice over the pixel
    that includes them; a point counts as inside or outside an emitter only by more than `margin`."""
    cam = desc.camera
    s2c, c2w = np.asarray(cam["sample_to_camera"], f64), np.asarray(cam["camera_to_world"], f64)
    t = np.linspace(0.0, 1.0, grid)
    sx = (np.arange(W)[None, :, None, None] + t[None, None, None, :]) / W + np.zeros((H, 1, grid, 1))
    sy = (np.arange(H)[:, None, None, None] + t[None, None, :, None]) / H + np.zeros((1, W, 1, grid))
    near = np.einsum("ij,j...->...i", s2c, np.stack([sx, sy, np.zeros_like(sx), np.ones_like(sx)]))
    dl = near[..., :3] / near[..., 3:4]
    d = np.einsum("ij,...j->...i", c2w[:3, :3], dl / np.linalg.norm(dl, axis=-1, keepdims=True))
    o = c2w[:3, 3]
    p = o + d * ((MIRROR_Z - o[2]) / d[..., 2])[..., None]
    assert np.all(np.abs(p[..., :2]) < 3.0)  # every camera ray meets the mirror
    n = 2.0 * mirror_texel(sign).astype(f64) - 1.0
    n /= np.linalg.norm(n)  # (s, t, n) = (x, y, z) on the mirror
    r = d - 2.0 * (d @ n)[..., None] * n
    assert np.all(r[..., 2] > 0)
    q = p + r * ((EMITTER_Z - p[..., 2]) / r[..., 2])[..., None]
    out = np.full((H, W), 2, int)
    dark = np.ones((H, W), bool)
    for side in (1, -1):
        x0, x1 = sorted((side * EMITTER_X[0], side * EMITTER_X[1]))
        # signed distances to the four edges, positive inside
        dist = np.stack([q[..., 0] - x0, x1 - q[..., 0], q[..., 1] - EMITTER_Y[0], EMITTER_Y[1] - q[..., 1]], -1)
        inside = (dist > margin).all(-1).all((-1, -2))
        beyond = (dist < -margin).all((2, 3)).any(-1)  # all points of the pixel beyond one and the same edge
        out[inside] = side
        dark &= beyond
    out[dark] = 0
    return out


@pytest.fixture(scope="module")
def mirror_renders():
    out = {}
    for depth in (3, -1):
        e = hip(budgetType="spp", budget=12, sppPerPass=4, maxDepth=depth, rrDepth=10, seed=5, sampleCombination="discard")
        for sign in (1, -1):
            e.set_scene(mirror_scene(sign))
            e.render()
            out[depth, sign] = e.read_film().astype(f64)
        e.close()
    return out


@pytest.mark.parametrize("depth", [3, -1], ids=["depth-3", "unbounded"])
def test_a_tilted_mirror_shows_the_emitter_where_predicted(mirror_renders, depth):
    """Lit pixels: radiance x specularReflectance within 1e-5 relative (n equal addends and one division: n 2^-24); dark pixels: exactly
    0.  With the map's x component negated the other emitter shows, in the mirrored pixels: the run that fails when the frame is wrong.
    (depth 3: k_shade; unbounded: k_tail shades the same paths.)"""
    kinds = {sign: predict(mirror_scene(sign), sign) for sign in (1, -1)}
    mirrored = kinds[1][:, ::-1]
    assert np.array_equal(kinds[-1], np.where(mirrored == 2, 2, -mirrored))  # (the scene is its own mirror image)
    for sign in (1, -1):
        kind, img = kinds[sign], mirror_renders[depth, sign]
        lit, boundary = int((kind == sign).sum()), int((kind == 2).sum())
        print("depth", depth, "tilt towards", sign, "lit", lit, "boundary", boundary, "other emitter", int((kind == -sign).sum()), "dark", int((kind == 0).sum()))
        assert lit >= 100 and boundary <= 0.25 * lit
        assert (kind == -sign).sum() == 0  # the other emitter stays out of the picture
        want = np.asarray(RADIANCE[sign], f64) * np.asarray(SPECULAR, f64)
        rel = np.abs(img[kind == sign] / want - 1.0)
        print("largest relative deviation of a lit pixel", rel.max())
        assert rel.max() <= 1e-5
        assert np.all(img[kind == 0] == 0.0)
        assert np.isfinite(img).all()
    # the lit set of the negated map is the mirrored one
    assert np.array_equal(kinds[-1] == -1, (kinds[1] == 1)[:, ::-1])
    a, b = mirror_renders[depth, 1], mirror_renders[depth, -1]
    assert np.array_equal((a > 0).any(2)[kinds[1] != 2], ((b > 0).any(2)[:, ::-1])[kinds[1] != 2])


# ------------------------------------------------------------------------------------------------ 3. against the bump map
def test_a_constant_normal_map_equals_a_constant_slope_bump_map():
    """the textured floor under a constant sky of tests/test_textures.py: the ramp h = 0.8 u tilts the normal by atan(0.8 * 64 / 63 * 0.5)
    about the v axis (bumpmap.cpp:135-160), and the normal map states that very normal.  Under a uniform sky every pixel has the same
    expectation, so the pixels' own spread estimates the error of the image mean; the two means agree within 4 standard errors of the
    bump-mapped render's."""
    from test_textures import _floor_scene
    res = 24
    ramp = np.repeat(np.linspace(0, 1, 64, dtype=f32)[None, :, None], 3, 2).repeat(4, 0) * f32(0.8)
    tex = np.full((2, 2, 3), 0.5, f32)
    bumped = _floor_scene(res, tex, bump=ramp)
    tilt = np.arctan(0.8 * 64 / 63 * 0.5)  # 64 texels over u = 1, 63 steps over h = 0.8; du/dx = 0.5
    # bump_frame's normal in the floor's frame (s = dpdu / |dpdu| = +x, n = +y): turned towards -s
    n = np.array([-np.sin(tilt), 0.0, np.cos(tilt)])
    mapped = _floor_scene(res, tex, bump=ramp)
    del mapped.materials[0]["bump"]
    mapped.materials[0]["normal_map"] = 1
    mapped.textures[1] = dict(rgb=np.broadcast_to(((n + 1) / 2).astype(f32), (2, 2, 3)).copy(), wrap_u="clamp", wrap_v="clamp")
    flat = _floor_scene(res, tex)
    means = {}
    e = hip(budgetType="spp", budget=64, sppPerPass=4, maxDepth=2, rrDepth=10, seed=9, sampleCombination="discard")
    rays = np.array([[0.1, 3.0, 0.2, 0.0, 0.0, -1.0, 0.0, np.inf]], f32)
    frames = {}
    for name, desc in (("bump", bumped), ("normal_map", mapped), ("flat", flat)):
        e.set_scene(desc)
        frames[name] = e.debug_shading_frame(rays)[0]
        e.render()
        img = e.read_film().astype(f64)[..., 0]
        means[name] = img.mean(), img.std(ddof=1) / np.sqrt(img.size)
    e.close()
    print("image means and their standard errors:", means, "frames", {k: v["pn"] for k, v in frames.items()})
    assert np.abs(frames["bump"]["pn"].astype(f64) - frames["normal_map"]["pn"]).max() < 1e-6  # the same normal to begin with
    assert frames["bump"]["adapted"] == 1 and frames["normal_map"]["adapted"] == 1 and frames["flat"]["adapted"] == 0
    (mb, sb), (mn, _), (mf, _) = means["bump"], means["normal_map"], means["flat"]
    assert sb > 0 and abs(mb - mn) <= 4 * sb, (mb, mn, sb)
    lost = (1 - np.cos(tilt)) / 2  # the directions the adapters reject (cosTheta(wo) cosTheta(wo') <= 0)
    assert abs(mn / (0.5 * 2.0 * (1 - lost)) - 1) < 0.01 and mf - mn > 4 * sb  # (the flat floor is brighter: the test can fail)


# ------------------------------------------------------------------------------------------------ 4. null
BACK, FRONT = (3.0, 2.0, 1.0), (0.5, 0.25, 0.125)


def null_scene(k, front_emitter=False, res=(W, H)):
    """Camera at the origin looking down -z at a black emitter of radiance BACK that fills the view, behind k null quads that fill it too
    (front_emitter: the first of them is an emitter of radiance FRONT itself)"""
    import ppg_host
    pos, idx, tm, te = [], [], [], []

    def quad(z, half, material, emitter):
        b = len(pos)
        pos.extend([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]])
        idx.extend([[b, b + 1, b + 2], [b, b + 2, b + 3]])  # normal +z: towards the camera
        tm.extend([material, material]); te.extend([emitter, emitter])
    quad(-5.0, 3.0, 0, 0)
    for j in range(k):
        quad(-1.0 - j, 2.0, 1, 1 if front_emitter and j == 0 else -1)
    mats = [dict(type=0, reflectance=(0.0, 0.0, 0.0)), dict(type="null")]
    ems = [dict(radiance=BACK)] + ([dict(radiance=FRONT)] if front_emitter else [])
    cam = ppg_host.scenes.perspective_camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 30.0, "x", 0.01, 100.0, *res)
    return ppg_host.SceneDesc(np.array(pos, f32), np.array(idx, np.uint32), np.array(tm, np.uint32), np.array(te, np.int32), mats, ems, cam)


def _film(desc, **props):
    e = hip(**dict(dict(budgetType="spp", budget=12, sppPerPass=4, rrDepth=10, seed=4, sampleCombination="discard"), **props))
    e.set_scene(desc)
    e.render()
    img = e.read_film()
    e.close()
    return img


@pytest.mark.parametrize("depth", [3, -1], ids=["depth-3", "unbounded"])
def test_an_emitter_seen_through_a_null_quad_shows_its_radiance_exactly(depth):
    img = _film(null_scene(1), maxDepth=depth)
    assert img.shape == (H, W, 3) and np.all(img == np.asarray(BACK, f32))
    both = _film(null_scene(1, front_emitter=True), maxDepth=depth)
    assert np.all(both == np.asarray(BACK, f32) + np.asarray(FRONT, f32))  # (sums of dyadic numbers: exact)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_null_quads_count_towards_the_depth(k):
    """maxDepth = 2: GP:1917-1921 and 2045-2075 as restated by normalmap_ref.seen_through — a null interaction costs one level"""
    img = _film(null_scene(k, res=(16, 12)), maxDepth=2)
    want = np.asarray(BACK, f32) if R.seen_through(k, 2) else np.zeros(3, f32)
    assert R.seen_through(k, 2) == (k < 2) and np.all(img == want)
    assert np.all(_film(null_scene(k, res=(16, 12)), maxDepth=3) == np.asarray(BACK, f32))


def test_a_null_sheet_in_mid_air_leaves_a_diffuse_box_as_it_is():
    """the Cornell box with and without a null quad hanging in it: the means of the two images agree within 4 standard errors of the
    render without it (per channel, from ppg_read_variance: the variance of the last iteration's samples)"""
    import ppg_host
    from test_coatings_gpu import _last_iteration_spp
    props = dict(budgetType="spp", budget=124, sppPerPass=4, maxDepth=-1, rrDepth=5, seed=8, nee="always", sampleCombination="discard")
    last = _last_iteration_spp(props["budget"], props["sppPerPass"])
    out = {}
    for sheet in (False, True):
        desc = ppg_host.cbox_scene(W, H)
        if sheet:
            b = len(desc.positions)
            quad = np.array([[120, 300, 120], [440, 300, 120], [440, 300, 440], [120, 300, 440]], f32)
            desc.positions = np.concatenate([np.asarray(desc.positions, f32), quad])
            desc.indices = np.concatenate([np.asarray(desc.indices, np.uint32), np.array([[b, b + 1, b + 2], [b, b + 2, b + 3]], np.uint32)])
            desc.tri_material = np.concatenate([np.asarray(desc.tri_material, np.uint32), np.full(2, len(desc.materials), np.uint32)])
            desc.tri_emitter = np.concatenate([np.asarray(desc.tri_emitter, np.int32), np.full(2, -1, np.int32)])
            assert desc.normals is None
            desc.materials = list(desc.materials) + [dict(type="null")]
        e = hip(**props)
        e.set_scene(desc)
        e.render()
        film, var = e.read_film().astype(f64), e.read_variance().astype(f64) / last
        e.close()
        assert np.isfinite(film).all() and np.isfinite(var).all()
        out[sheet] = film.reshape(-1, 3).mean(0), np.sqrt(var.reshape(-1, 3).sum(0)) / (W * H)
    (ma, sa), (mb, sb) = out[False], out[True]
    print("mean without / with the null sheet", ma, mb, "standard error", sa, sb, "difference in standard errors", (mb - ma) / sa)
    assert np.all(ma > 0.01) and np.all(sa < 0.02 * ma)
    assert np.all(np.abs(ma - mb) <= 4 * sa)


# ------------------------------------------------------------------------------------------------ 5. the family changes nothing else
def test_a_scene_that_only_holds_the_two_renders_the_same_bits():
    """in the manner of tests/test_lobes_gpu.py: an unused normal-mapped material and an unused null material send the scene to the top
    kernel family (and switch the look-through code on); film, variance and SD-tree keep their bits"""
    import os
    import ppg_host
    from conftest import IMPROVED
    from test_rfilter_gpu import _tree_equal
    path = os.path.join(os.path.dirname(__file__), "golden", "cbox_16x12_pinhole.ppgs")
    out = []
    for extra in (False, True):
        desc = ppg_host.load_scene_file(path)
        if extra:
            desc.materials = list(desc.materials) + [dict(type=0, reflectance=(0.5, 0.5, 0.5), normal_map=0), dict(type="null")]
            desc.textures = [dict(rgb=R.normal_texels())]
        e = hip(**dict(IMPROVED, budgetType="spp", budget=31, maxDepth=-1, rrDepth=5, seed=11, nee="always"))
        e.set_scene(desc)
        e.render()
        out.append((e.read_film(), e.read_variance(), e.read_sdtree()))
        e.close()
    (fa, va, ta), (fb, vb, tb) = out
    assert np.isfinite(fa).all() and fa.mean() > 0.01
    assert np.array_equal(fa, fb) and np.array_equal(va, vb)
    _tree_equal(ta, tb)


# ------------------------------------------------------------------------------------------------ 6. the refusals
TEX = [dict(rgb=R.normal_texels())]
NULL = dict(type="null")
PLAIN = dict(type=0, reflectance=(0.5, 0.5, 0.5))
COAT = dict(kind="coating", eta=1.5, thickness=1.0, sigma_a=(0.0, 0.0, 0.0), specular=(1.0, 1.0, 1.0))
BLEND = dict(kind="blendbsdf", weight=0.3)
REFUSALS = [  # (name, the material appended last — the one the message names —, what the message says)
    ("flag-without-a-map", dict(PLAIN, _flags=32), "PPG_MAT_NORMALMAP without a normal map"),
    ("flag-with-a-reflectance-bitmap-only", dict(PLAIN, texture=0, _flags=32), "PPG_MAT_NORMALMAP without a normal map"),
    ("null-twosided", dict(NULL, twosided=True), "null cannot be two-sided: only BRDFs can be (twosided.cpp:84-88)"),
    ("null-masked", dict(NULL, opacity=0.5), "a mask around the null BSDF is not supported"),
    ("null-nonlinear", dict(NULL, nonlinear=True), "null takes no flags"),
    ("null-normal-mapped", dict(NULL, normal_map=0), "null takes no flags"),
    ("null-textured", dict(NULL, texture=0), "null reads no bitmap and takes no bump or normal map"),
    ("null-bump-mapped", dict(NULL, bump=0), "null reads no bitmap and takes no bump or normal map"),
    ("null-slot-specular", dict(NULL, specular_texture=0), "texture slot specular: null reads no bitmap"),
    ("null-slot-opacity", dict(NULL, opacity_texture=0), "texture slot opacity: null reads no bitmap"),
    ("null-microfacet", dict(NULL, alpha_v=0.3), "microfacet"),
    ("null-coated", dict(NULL, coating=dict(COAT)), "coating over the null BSDF is not supported"),
    ("null-blended-record", dict(NULL, blend=dict(BLEND, children=[dict(PLAIN), dict(PLAIN)])), "PPG_BSDF_DIFFUSE"),
]


@pytest.fixture(scope="module")
def engine():
    e = hip(**dict(CBOX_PROPS, budget=4))
    yield e
    e.close()


def _scene(last, sphere=False):
    import ppg_host
    desc = ppg_host.cbox_scene(16, 12)
    desc.materials = list(desc.materials) + [dict(last)]
    desc.textures = TEX
    if sphere:
        desc.spheres = [dict(center=(278, 100, 280), radius=50.0, material=len(desc.materials) - 1)]
    return desc


def _renders_a_good_scene(engine):
    engine.set_scene(_scene(dict(PLAIN, normal_map=0)))
    engine.render()
    img = engine.read_film()
    assert np.isfinite(img).all() and img.mean() > 0.01


def _raw_flags(monkeypatch):
    """material dicts cannot state a flag without what it stands for: `_flags` is OR-ed into the record for these cases"""
    from ppg_host.bindings import Material
    plain = Material.from_dict.__func__

    def from_dict(cls, m):
        o = plain(cls, m)
        o.flags |= int(m.get("_flags", 0))
        return o
    monkeypatch.setattr(Material, "from_dict", classmethod(from_dict))


@pytest.mark.parametrize("k", range(len(REFUSALS)), ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_material_and_leave_the_context_usable(engine, monkeypatch, k):
    from ppg_host.bindings import PPGError
    _raw_flags(monkeypatch)
    name, last, says = REFUSALS[k]
    desc = _scene(last)
    with pytest.raises(PPGError) as err:
        engine.set_scene(desc)
    assert err.value.code == -1  # PPG_ERR_INVALID
    assert "material %d" % (len(desc.materials) - 1) in str(err.value) and says in str(err.value), str(err.value)
    _renders_a_good_scene(engine)


def test_refusals_in_blends_and_on_spheres(engine):
    from ppg_host.bindings import PPGError
    cases = [
        (_scene(dict(PLAIN, blend=dict(BLEND, children=[dict(PLAIN), dict(NULL)]))), "a null child is not supported"),
        (_scene(dict(PLAIN, blend=dict(BLEND, children=[dict(PLAIN), dict(PLAIN, normal_map=0)]))), "is masked, two-sided or bump-mapped"),
        (_scene(NULL, sphere=True), "the null BSDF is only supported on triangle meshes (not on spheres, disks or cylinders)"),
        (_scene(dict(PLAIN, normal_map=0), sphere=True), "textured BSDFs are only supported on triangle meshes"),
    ]
    for desc, says in cases:
        with pytest.raises(PPGError) as err:
            engine.set_scene(desc)
        assert err.value.code == -1 and says in str(err.value), str(err.value)
        _renders_a_good_scene(engine)
    desc = _scene(NULL, sphere=True)
    desc.spheres[0]["material"] = 0  # with another material the sphere is taken, the null material beside it
    engine.set_scene(desc)
    engine.render()
    assert np.isfinite(engine.read_film()).all()
