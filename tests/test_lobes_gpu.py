"""The roughdiffuse, difftrans and phong BSDFs on the GPU (include/ppg.h PPG_BSDF_ROUGHDIFFUSE ..; csrc: the lobes kernels, PPG_LOBES):

  * the test hook ppg_debug_bsdf — the render's own mat_eval / mat_pdf / mat_sample — against the float64 restatement of test_lobes.py, each
    case held to 8 x its own float32-against-float64 figure; the reductions to `diffuse` and to a constant weight, bit for bit;
  * a closed form: a diffuse transmitter in front of a constant environment;
  * the lobes family changes nothing else: a scene that merely holds such a material, today's materials through it;
  * renders of a box with the three materials: estimators agree, bookkeeping is intact, and the materials show;
  * the C-ABI's refusals.
"""
import os

import numpy as np
import pytest

from conftest import CBOX_PROPS, IMPROVED
from test_coatings import SMOOTH_COAT
from test_coatings_gpu import LAST_SPP, SPP, _last_iteration_spp
from test_lobes import CASES, MARGIN, MAX_EXCLUDED, PHONG, ROUGH, SHEET, TEXELS, deviations, float32_figures, items, reference
from test_rfilter_gpu import _tree_equal

f32 = np.float32
pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DIFFUSE = dict(type="diffuse", reflectance=ROUGH["reflectance"])


def hip(**props):
    import ppg_host
    return ppg_host.Engine.hip(**props)


def appended(desc, materials, textures=None):
    base = len(desc.materials)
    desc.materials = list(desc.materials) + [dict(m) for m in materials]
    if textures is not None:
        desc.textures = textures
    return base


# ------------------------------------------------------------------------------------------------ 1. the hook against the restatement
@pytest.fixture(scope="module")
def hook():
    import ppg_host
    desc = ppg_host.cbox_scene(16, 12)
    base = appended(desc, CASES.values(), [dict(rgb=TEXELS)])  # on no triangle
    e = hip(**dict(CBOX_PROPS, budget=4))
    e.set_scene(desc)
    out = {}
    for k, name in enumerate(CASES):
        wi, wo, u, uv, _ = items(name)
        out[name] = e.debug_bsdf(base + k, wi, wo, u, uv=uv)
    e.close()
    return out


class _S:
    def __init__(self, g):
        self.wo, self.pdf, self.weight = g["wo"], g["sampled_pdf"], g["weight"]


@pytest.mark.parametrize("name", list(CASES))
def test_hook_equals_the_restatement(hook, name):
    """Bounds: 8 x what the restatement itself loses between float32 and float64 on these very items (test_lobes.py, measured there per
    case), never below 8 x 2^-23: the kernels' operation order differs from numpy's, their exp / log / sincos / atan2 are the library's own,
    and grazing directions cancel.  Items within MARGIN of a branch point — phong's lobe choice |sample.x - w_s|, a rotated phong direction
    at the horizon, roughdiffuse's sine thresholds — are left out; no case may lose more than 1 % of its items to that.
    Measured on an MI355X, largest over the cases: see DESIGN.md "Diffuse-transmission, Oren-Nayar and Phong lobes"."""
    g = hook[name]
    ref = reference(name)
    fig, excluded, _ = float32_figures(name)
    dev = deviations(dict(eval=g["eval"], pdf=g["pdf"], sample=_S(g)), ref)
    floor = 2.0 ** -23
    print(name, "hook vs float64:", dev, "| float32 vs float64:", fig, "| excluded", excluded)
    assert MARGIN == 1e-4 and excluded <= MAX_EXCLUDED == 0.01
    keep, s = ref["keep"], ref["sample"]
    assert np.isfinite(g["eval"]).all() and np.isfinite(g["pdf"]).all() and np.isfinite(g["weight"]).all() and np.isfinite(g["wo"]).all()
    ok = g["weight"].any(1)
    assert np.array_equal(ok[keep], s.weight.any(1)[keep])
    assert not g["delta"].any() and not g["is_null"].any()
    assert np.all(g["eta"] == 1)
    for what in ("eval", "pdf", "weight", "sampled_pdf", "direction"):
        assert dev[what] <= 8 * max(fig[what], floor), (what, dev[what], fig[what])


# ------------------------------------------------------------------------------------------------ 2. reductions at the hook
def test_roughdiffuse_without_roughness_is_diffuse_and_difftrans_weighs_its_transmittance():
    """alpha = 0 in the qualitative model: A = 1, B = 0, so eval = reflectance (INV_PI cos) 1 — the bits of `diffuse` — and so are the density
    and the sampled direction; the weight is eval / pdf = (r x)(1 / x): two roundings around r, 2^-22 relative.  difftrans returns the
    transmittance itself."""
    import ppg_host
    desc = ppg_host.cbox_scene(16, 12)
    base = appended(desc, [dict(ROUGH, alpha=0.0, fast_approx=True), DIFFUSE, SHEET])
    e = hip(**dict(CBOX_PROPS, budget=4))
    e.set_scene(desc)
    wi, wo, u, _, _ = items("roughdiffuse-0.2-fast")
    a, b = e.debug_bsdf(base, wi, wo, u), e.debug_bsdf(base + 1, wi, wo, u)
    wi_t, wo_t, u_t, _, _ = items("difftrans")
    t = e.debug_bsdf(base + 2, wi_t, wo_t, u_t)
    e.close()
    assert b["eval"].any() and b["weight"].any(1).all()
    for what in ("eval", "pdf", "wo", "sampled_pdf"):
        assert np.array_equal(a[what].view(np.uint32), b[what].view(np.uint32)), what
    err = np.abs(a["weight"].astype(np.float64) - b["weight"]) / b["weight"]
    print("weight of roughdiffuse(alpha = 0) against diffuse, largest relative difference:", err.max(), "in 2^-24:", err.max() * 2 ** 24)
    assert err.max() <= 2.0 ** -22
    want = np.broadcast_to(np.asarray(SHEET["reflectance"], f32), t["weight"].shape)
    assert np.array_equal(t["weight"].view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    assert np.all(t["wo"][:, 2] * wi_t[:, 2] < 0) and np.all(t["sampled_pdf"] > 0)


def test_the_edge_cases_of_pow_on_the_device():
    """the library's pow is exp(y log x), which has no answer for two inputs phong meets: sample.y = 0 must put the lobe direction on its
    equator (cos = 0 exactly — from straight above that is the horizon: a failed sample, not one at cos = exp(-80)), and an exponent of 0
    is the uniform lobe, (n + 1) / (2 pi) = 1 / (2 pi)"""
    import ppg_host
    from test_lobes import Lobe
    desc = ppg_host.cbox_scene(16, 12)
    flat = dict(PHONG, exponent=0.0)
    base = appended(desc, [PHONG, flat])
    e = hip(**dict(CBOX_PROPS, budget=4))
    e.set_scene(desc)
    wo = np.array([[0.1, 0.5, 0.7]], np.float64)
    wo = (wo / np.linalg.norm(wo)).astype(f32)
    a = e.debug_bsdf(base, [0, 0, 1], wo, [0.05, 0.0])
    wi = np.array([[0.6, 0.2, 0.5]], np.float64)
    wi = (wi / np.linalg.norm(wi)).astype(f32)
    b = e.debug_bsdf(base + 1, wi, np.repeat(wo, 2, 0), np.array([[0.05, 0.0], [0.05, 0.5]], f32))
    e.close()
    assert a["wo"][0, 2] == 0 and not a["weight"].any() and a["sampled_pdf"][0] == 0
    ref = Lobe(flat)
    assert np.allclose(b["pdf"], float(ref.weight) / (2 * np.pi) + (1 - float(ref.weight)) * wo[0, 2] / np.pi, rtol=1e-6)
    assert np.allclose(b["eval"], ref.eval(wi, np.repeat(wo, 2, 0)), rtol=1e-5)
    assert np.isfinite(b["weight"]).all() and np.isfinite(b["wo"]).all() and b["weight"][1].any()


# ------------------------------------------------------------------------------------------------ 3. the closed form
T = (0.6, 0.4, 0.2)
L = (1.5, 2.0, 0.75)


def sheet_scene(blocked):
    """a difftrans rectangle that fills a 16 x 12 view, under a constant environment; `blocked`: a black wall just behind it, far larger than
    the sheet, so that radiance reaches the camera only from the camera's own side — by reflection, which a transmitter has none of"""
    import ppg_host
    from ppg_host.scenes import SceneDesc, perspective_camera
    quad = lambda s, z: [(-s, -s, z), (s, -s, z), (s, s, z), (-s, s, z)]  # noqa: E731
    pos = quad(4.0, 0.0) + (quad(4e4, 0.01) if blocked else [])
    idx = [(0, 1, 2), (0, 2, 3)] + ([(4, 5, 6), (4, 6, 7)] if blocked else [])
    mats = [dict(type="difftrans", reflectance=T), dict(type="diffuse", reflectance=(0, 0, 0))]
    cam = perspective_camera((0, 0, -5), (0, 0, 0), (0, 1, 0), 40.0, "x", 0.1, 100.0, 16, 12)
    return SceneDesc(np.array(pos, f32), np.array(idx, np.uint32), np.array([0, 0, 1, 1][:len(idx)], np.uint32), np.full(len(idx), -1, np.int32), mats, [], cam,
                     environment=L)


def _sheet_render(blocked, nee):
    e = hip(budgetType="spp", budget=16, maxDepth=2, rrDepth=10, seed=7, nee=nee, bsdfSamplingFraction=1.0, bsdfSamplingFractionLoss="none", sampleCombination="discard")
    e.set_scene(sheet_scene(blocked))
    e.render()
    film = e.read_film()
    e.close()
    return film


def test_a_diffuse_transmitter_in_front_of_a_constant_environment():
    """nee = never, BSDF sampling only, maxDepth = 2: every sample is camera -> sheet -> environment and carries exactly T L — the sample
    weight is the transmittance, no division —, so only the film's float sum rounds: 1e-5 relative.  With a black wall behind the sheet
    the light is on the camera's side only and the sheet renders 0 exactly, with either estimator: it reflects nothing."""
    film = _sheet_render(False, "never")
    want = np.asarray(T, np.float64) * np.asarray(L, np.float64)
    err = np.abs(film / want[None, None] - 1).max()
    print("largest relative deviation from T L:", err)
    assert film.shape == (12, 16, 3) and err <= 1e-5
    for nee in ("never", "always"):
        assert not _sheet_render(True, nee).any()


# ------------------------------------------------------------------------------------------------ 4. the family changes nothing else
def test_a_scene_that_only_holds_a_roughdiffuse_material_renders_the_same_bits():
    import ppg_host
    from test_coatings_gpu import _render
    path = os.path.join(GOLDEN, "cbox_16x12_pinhole.ppgs")
    fa, ta = _render(ppg_host.load_scene_file(path))
    desc = ppg_host.load_scene_file(path)
    appended(desc, [ROUGH])  # on no triangle: the lobes kernels run, and meet no lobe
    fb, tb = _render(desc)
    assert np.isfinite(fa).all() and fa.mean() > 0.01
    assert np.array_equal(fa, fb)
    _tree_equal(ta, tb)


def test_todays_materials_through_the_lobes_kernels_equal_the_blend_kernels():
    from test_blends_gpu import _render, _smooth_box
    fa, ta = _render(_smooth_box(True))
    desc = _smooth_box(True)
    appended(desc, [PHONG])
    fb, tb = _render(desc)
    assert np.isfinite(fa).all() and fa.mean() > 0.01
    assert np.array_equal(fa, fb)
    _tree_equal(ta, tb)


# ------------------------------------------------------------------------------------------------ 5. - 7. renders of a box with the three
W, H = 64, 48
FLOOR = dict(type="roughdiffuse", alpha=0.5)
WALL = dict(type="phong", exponent=40.0, reflectance=(0.4, 0.4, 0.4), specular=(0.3, 0.3, 0.3))
SHADE = dict(type="difftrans", reflectance=(0.6, 0.6, 0.6))


def lobes_box(lobes=True):
    """the Cornell box with the floor a roughdiffuse (full model) of its own white, the back wall a phong and the short box a diffuse
    transmitter (lobes = False: plain diffuse of the same colours)"""
    import ppg_host
    desc = ppg_host.cbox_scene(W, H)
    pos, idx, tm = np.asarray(desc.positions), np.asarray(desc.indices), np.array(desc.tri_material)
    tri = pos[idx]  # [n, 3, 3]
    floor = np.all(tri[:, :, 1] == 0, axis=1) & (tm == 1)  # (the boxes stand on it: "white" alone)
    back = np.all(np.abs(tri[:, :, 2] - 559.20001) < 1e-3, axis=1)
    short = np.zeros(len(tm), bool)
    short[np.nonzero(tm == 0)[0][:12]] = True  # (the first of the two boxes: 165 high)
    assert floor.sum() == 2 and back.sum() == 2 and tri[short][:, :, 1].max() == 165.0 and tri[(tm == 0) & ~short][:, :, 1].max() == 330.0
    white = tuple(desc.materials[1]["reflectance"])
    mats = [dict(FLOOR, reflectance=white), WALL, SHADE]
    if not lobes:
        mats = [dict(type="diffuse", reflectance=m["reflectance"]) for m in mats]
    base = appended(desc, mats)
    tm[floor], tm[back], tm[short] = base, base + 1, base + 2
    desc.tri_material = tm
    return desc


_renders = {}


def box_render(which):
    """film, per-pixel variance of the mean of the last iteration (ppg_read_variance: the variance of that iteration's samples)"""
    if which not in _renders:
        common = dict(budgetType="spp", maxDepth=-1, rrDepth=5, seed=3)
        props = {
            "nee-always": dict(common, budget=SPP - 3, sppPerPass=4, nee="always", sampleCombination="discard"),
            "nee-never": dict(common, budget=SPP - 3, sppPerPass=4, nee="never", sampleCombination="discard"),
            "guided": dict(IMPROVED, **common, budget=SPP, nee="never"),
            "unguided": dict(IMPROVED, **common, budget=SPP, nee="never", bsdfSamplingFraction=1.0, bsdfSamplingFractionLoss="none"),
            "plain": dict(common, budget=SPP - 3, sppPerPass=4, nee="always", sampleCombination="discard"),
        }[which]
        assert _last_iteration_spp(props["budget"], props["sppPerPass"]) == LAST_SPP
        e = hip(**props)
        e.set_scene(lobes_box(which != "plain"))
        e.render()
        film, var = e.read_film(), e.read_variance()
        e.close()
        assert np.isfinite(film).all() and np.isfinite(var).all() and np.all(var >= 0)
        _renders[which] = film.astype(np.float64), var.astype(np.float64) / LAST_SPP
    return _renders[which]


def _mean_and_se(which, rows=slice(None)):
    film, var_of_mean = box_render(which)
    f, v = film[rows].reshape(-1, 3), var_of_mean[rows].reshape(-1, 3)
    return f.mean(0), np.sqrt(v.sum(0)) / len(f)


@pytest.mark.parametrize("pair", [("nee-always", "nee-never"), ("guided", "unguided")], ids=["nee", "guiding"])
def test_estimators_agree_on_a_box_with_the_three(pair):
    """the schedule of tests/test_coatings_gpu.py: 4095 spp (4092 where a pass has 4) with a last iteration of 2048; one standard error of
    the mean image radiance below 1 % of the mean in all four renders, and the means within 4 sigma of each other.
    Measured on an MI355X: DESIGN.md "Diffuse-transmission, Oren-Nayar and Phong lobes"."""
    (ma, sa), (mb, sb) = _mean_and_se(pair[0]), _mean_and_se(pair[1])
    print(pair, "mean", ma, mb, "standard error", sa, sb, "relative", sa / ma, sb / mb, "spp", SPP)
    assert np.all(sa < 0.01 * ma) and np.all(sb < 0.01 * mb)
    assert np.all(np.abs(ma - mb) <= 4 * np.sqrt(sa * sa + sb * sb)), (ma - mb) / np.sqrt(sa * sa + sb * sb)


def test_bookkeeping_of_a_box_with_the_three():
    """the invariants of test_coatings_gpu.test_bookkeeping_of_a_coated_box on this box: samples and rays add up, and with the nearest
    filters every committed vertex carries weight 1 into exactly one leaf"""
    for nee in ("always", "never"):
        e = hip(budgetType="spp", budget=60, maxDepth=-1, rrDepth=5, seed=5, nee=nee)
        e.set_scene(lobes_box()); e.begin_render()
        for p in (1, 2, 4):
            e.begin_iteration(False)
            st = e.render_passes(p)
            t = e.read_sdtree()
            leaf = t["children"][:, 0] == 0
            assert int(round(t["building"]["stat_weight"][leaf].sum())) == st.vertices_committed
            assert st.samples == W * H * 4 * p and st.rays == st.path_length_sum
            e.build_sdtree(); e.end_iteration()
        assert np.isfinite(e.read_film()).all()
        e.end_render()
        e.close()


def test_the_three_show():
    """with plain diffuse in their place the lower rows — the floor and the short box — are another picture: the test that fails when a
    host drops the fields"""
    rows = slice(2 * H // 3, H)
    (ma, sa), (mb, sb) = _mean_and_se("nee-always", rows), _mean_and_se("plain", rows)
    print("lower rows: the three", ma, "plain diffuse", mb, "standard errors", sa, sb)
    assert np.all(np.abs(ma - mb) > 4 * np.sqrt(sa * sa + sb * sb))


# ------------------------------------------------------------------------------------------------ 8. the refusals
BLEND = dict(kind="blendbsdf", weight=0.3)
NAN, INF = float("nan"), float("inf")
REFUSALS = [  # (name, the material appended last — the one the message names —, what the message says)
    ("difftrans-twosided", dict(SHEET, twosided=True), "two-sided"),
    ("phong-black", dict(type="phong", reflectance=0.0, specular=0.0), "luminance 0"),
    ("alpha-negative", dict(ROUGH, alpha=-0.1), "alpha must be finite and not negative"),
    ("alpha-nan", dict(ROUGH, alpha=NAN), "alpha must be finite and not negative"),
    ("exponent-negative", dict(PHONG, exponent=-1.0), "exponent must be finite and not negative"),
    ("exponent-inf", dict(PHONG, exponent=INF), "exponent must be finite and not negative"),
    ("fast-approx-on-diffuse", dict(DIFFUSE, fast_approx=True), "PPG_MAT_FAST_APPROX"),
    ("fast-approx-on-phong", dict(PHONG, fast_approx=True), "PPG_MAT_FAST_APPROX"),
    ("slot-specular-phong", dict(PHONG, specular_texture=0), "texture slot specular"),
    ("slot-alpha-roughdiffuse", dict(ROUGH, alpha_texture=0), "texture slot alpha"),
    ("slot-alpha-phong", dict(PHONG, alpha_texture=0), "texture slot alpha"),
    ("slot-specular-difftrans", dict(SHEET, specular_texture=0), "texture slot specular"),
    ("microfacet-roughdiffuse", dict(ROUGH, alpha_v=0.3), "microfacet"),
    ("microfacet-phong", dict(PHONG, distribution="phong"), "microfacet"),
    ("coating-phong", dict(PHONG, coating=dict(SMOOTH_COAT)), "coating over roughdiffuse, difftrans or phong"),
    ("coating-difftrans", dict(SHEET, coating=dict(SMOOTH_COAT)), "coating over roughdiffuse, difftrans or phong"),
    ("blend-child", dict(type=0, blend=dict(BLEND, children=[dict(DIFFUSE), dict(ROUGH)])), "roughdiffuse, difftrans and phong children"),
    ("blended-record", dict(PHONG, blend=dict(BLEND, children=[dict(DIFFUSE), dict(DIFFUSE)])), "PPG_BSDF_DIFFUSE"),
]


@pytest.fixture(scope="module")
def engine():
    e = hip(**dict(CBOX_PROPS, budget=4))
    yield e
    e.close()


def _scene(last):
    import ppg_host
    desc = ppg_host.cbox_scene(16, 12)
    appended(desc, [last], [dict(rgb=TEXELS)])
    return desc


@pytest.mark.parametrize("k", range(len(REFUSALS)), ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_material_and_leave_the_context_usable(engine, k):
    from ppg_host.bindings import PPGError
    name, last, says = REFUSALS[k]
    desc = _scene(last)
    n = len(desc.materials)
    with pytest.raises(PPGError) as err:
        engine.set_scene(desc)
    assert err.value.code == -1  # PPG_ERR_INVALID
    assert "material %d" % (n - 1) in str(err.value) and says in str(err.value), str(err.value)
    engine.set_scene(_scene(PHONG))
    out = engine.debug_bsdf(n - 1, [0, 0, 1], np.array([[0.3, 0.2, 0.9]], f32), [0.5, 0.5])
    assert out["eval"].any() and np.isfinite(out["eval"]).all()


def test_a_bitmap_on_a_spheres_material_stays_refused(engine):
    from ppg_host.bindings import PPGError
    desc = _scene(dict(ROUGH, texture=0))
    desc.spheres = [dict(center=(278, 100, 280), radius=50.0, material=len(desc.materials) - 1)]
    with pytest.raises(PPGError) as err:
        engine.set_scene(desc)
    assert err.value.code == -1 and "textured BSDFs are only supported on triangle meshes" in str(err.value)
    desc.materials[-1] = dict(ROUGH)  # without the bitmap the sphere takes it
    engine.set_scene(desc)
    engine.render()
    assert np.isfinite(engine.read_film()).all()


def test_an_opacity_bitmap_is_the_one_slot_they_take(engine):
    desc = _scene(dict(SHEET, opacity=0.5, opacity_texture=0))
    engine.set_scene(desc)
    out = engine.debug_bsdf(len(desc.materials) - 1, [0, 0, 1], np.array([[0.3, 0.2, -0.9]], f32), [0.9, 0.5], uv=[0.25, 0.25])
    want = np.asarray(SHEET["reflectance"], np.float64) * TEXELS[0, 0] * (0.9 / np.pi)
    assert np.allclose(out["eval"][0], want, rtol=1e-5)
