"""The blendbsdf / mixturebsdf combinators on the GPU (include/ppg.h ppg_set_blends; csrc: the blend kernels, PPG_BLEND):

  * the test hook ppg_debug_bsdf — the render's own mat_eval / mat_pdf / mat_sample — against the float64 restatement of test_blends.py,
    per case, each held to 8 x its own float32-against-float64 figure;
  * exact reductions through the hook: a weight of 0 or 1, constant or from a bitmap, gives one child's own bits;
  * the blend family changes nothing else: a scene that merely holds a blended material, today's materials through it, an empty list;
  * renders of a box with blended walls: finite, bookkeeping intact, the estimators agree and a blend of two diffuse BSDFs agrees with the
    diffuse BSDF of the mixed reflectance, within the spread the plain-diffuse render itself shows from seed to seed;
  * the C-ABI's refusals.
"""
import os

import numpy as np
import pytest

from conftest import CBOX_PROPS, IMPROVED
from test_blends import (CASES, COPPER, DIFFUSE, GOLD, MARGIN, PLASTIC, ROUGHPLASTIC, SPECS, TEXELS_R, TEXELS_W, blend_lattice, case_id, child_dict,
                         figures)
from test_bsdfs import SMOOTH
from test_coatings import SMOOTH_COAT, deviations
from test_rfilter_gpu import _tree_equal

f32 = np.float32
pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def hip(**props):
    import ppg_host
    return ppg_host.Engine.hip(**props)


def two_texels(a, b):
    """a nearest-filtered bitmap of two texels: `a` where u < 1/2, `b` beyond"""
    return dict(rgb=np.asarray([[a, b]], f32), nearest=True, wrap_u="clamp", wrap_v="clamp")


def with_slices(desc, materials):
    """`materials` appended to desc's own — the children of blended ones stay nested: set_scene appends them —; the slices of roughplastics
    (arrays under `slice`) gathered into desc.rtrans and replaced by their row.  Returns the first new index."""
    rows = [] if getattr(desc, "rtrans", None) is None else [np.asarray(r, f32) for r in desc.rtrans]

    def fix(m):
        m = dict(m)
        if "slice" in m:
            sl = np.asarray(m.pop("slice"), f32)
            for k, r in enumerate(rows):
                if np.array_equal(r, sl):
                    break
            else:
                rows.append(sl)
                k = len(rows) - 1
            m["rtrans"] = k
        if m.get("blend") is not None:
            m["blend"] = dict(m["blend"], children=[fix(c) if isinstance(c, dict) else c for c in m["blend"]["children"]])
        return m
    base = len(desc.materials)
    desc.materials = list(desc.materials) + [fix(m) for m in materials]
    desc.rtrans = np.stack(rows) if rows else None
    return base


W_MAP, R_MAP = 0, 1  # the hook scene's textures


def case_material(case):
    """the material dict of a case of test_blends.py: the blended record with its children nested"""
    name, twosided = case
    spec = SPECS[name]
    kids = []
    for i, c in enumerate(spec["children"]):
        m = child_dict(c)
        if spec.get("reflectance_map") == i:
            m["reflectance"], m["texture"] = tuple(TEXELS_R.mean(0)), R_MAP
        kids.append(m)
    b = dict(kind=spec["kind"], children=kids)
    if spec["kind"] == "mixturebsdf":
        b["weights"] = spec["weights"]
    elif spec.get("weight_map"):
        b["weight"], b["weight_texture"] = 0.5, W_MAP
    else:
        b["weight"] = spec["weight"]
    m = dict(type=0, blend=b)
    if twosided:
        m["twosided"] = True
    return m


# ------------------------------------------------------------------------------------------------ 1. the hook against the restatement
@pytest.fixture(scope="module")
def hook():
    import ppg_host
    desc = ppg_host.cbox_scene(16, 12)
    desc.textures = [two_texels(TEXELS_W[0], TEXELS_W[1]), two_texels(TEXELS_R[0], TEXELS_R[1])]
    base = with_slices(desc, [case_material(c) for c in CASES])
    e = hip(**dict(CBOX_PROPS, budget=4))
    e.set_scene(desc)
    out = {}
    for k, c in enumerate(CASES):
        wi, wo, u, uv = blend_lattice(c[1])
        out[c] = e.debug_bsdf(base + k, wi, wo, u, uv=uv)
    e.close()
    return out


class _S:
    def __init__(self, g):
        self.wo, self.pdf, self.weight, self.delta = g["wo"], g["sampled_pdf"], g["weight"], g["delta"] != 0


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_hook_equals_the_restatement(hook, case):
    """Bounds: 8 x what the restatement itself loses between float32 and float64 on these very items (test_blends.py, per case), never
    below 8 x 2^-23 — the margin of the coating and general-microfacet tests, for their reason: the kernels' operation order differs from
    numpy's, their exp / pow / sincos are the library's own, and grazing directions cancel.
    Measured on an MI355X, largest over the cases — see DESIGN.md "Blends"."""
    g = hook[case]
    ref, fig, excluded = figures(case)
    dev = deviations(dict(eval=g["eval"], pdf=g["pdf"], sample=_S(g)), ref)
    floor = 2.0 ** -23
    print(case_id(case), "hook vs float64:", dev, "| float32 vs float64:", fig, "| excluded", excluded)
    keep, s = ref["keep"], ref["sample"]
    assert np.isfinite(g["eval"]).all() and np.isfinite(g["pdf"]).all() and np.isfinite(g["weight"]).all() and np.isfinite(g["wo"]).all()
    assert MARGIN == 1e-4
    ok = g["weight"].any(1)
    assert np.array_equal(ok[keep], s.weight.any(1)[keep])
    assert np.array_equal((g["delta"] != 0)[keep], s.delta[keep])
    assert not g["is_null"].any()
    assert np.all(g["eta"][keep] == 1)
    for name in ("eval", "pdf", "weight", "sampled_pdf", "direction"):
        assert dev[name] <= 8 * max(fig[name], floor), (name, dev[name], fig[name])


# ------------------------------------------------------------------------------------------------ 2. exact reductions
REDUCTION_PAIRS = [("diffuse-gold", DIFFUSE, GOLD), ("plastic-roughplastic", PLASTIC, ROUGHPLASTIC), ("copper-diffuse", COPPER, DIFFUSE)]


def _ulps(a, b):
    a, b = np.ascontiguousarray(a, f32).view(np.int32).astype(np.int64), np.ascontiguousarray(b, f32).view(np.int32).astype(np.int64)
    return np.abs(np.where(a < 0, -(a & 0x7fffffff), a) - np.where(b < 0, -(b & 0x7fffffff), b))


@pytest.fixture(scope="module")
def reductions():
    """per pair: the hook's output for child 0 and child 1 on their own, and for the blends with w = 0 and w = 1, constant and from a
    two-texel bitmap (0 | 1) at a uv in either half"""
    import ppg_host
    desc = ppg_host.cbox_scene(16, 12)
    desc.textures = [two_texels((0, 0, 0), (1, 1, 1))]
    mats = []
    for _, a, b in REDUCTION_PAIRS:
        mats += [dict(a), dict(b)]
        mats += [dict(type=0, blend=dict(kind="blendbsdf", children=[dict(a), dict(b)], weight=w)) for w in (0.0, 1.0)]
        mats += [dict(type=0, blend=dict(kind="blendbsdf", children=[dict(a), dict(b)], weight=0.5, weight_texture=0))]
    base = with_slices(desc, mats)
    e = hip(**dict(CBOX_PROPS, budget=4))
    e.set_scene(desc)
    wi, wo, u, uv = blend_lattice(False)
    left, right = uv.copy(), uv.copy()
    left[:, 0], right[:, 0] = 0.25, 0.75
    out = {}
    for k, (name, _, _) in enumerate(REDUCTION_PAIRS):
        i = base + 5 * k
        out[name] = dict(child=[e.debug_bsdf(i, wi, wo, u, uv=uv), e.debug_bsdf(i + 1, wi, wo, u, uv=uv)],
                         constant=[e.debug_bsdf(i + 2, wi, wo, u, uv=uv), e.debug_bsdf(i + 3, wi, wo, u, uv=uv)],
                         bitmap=[e.debug_bsdf(i + 4, wi, wo, u, uv=left), e.debug_bsdf(i + 4, wi, wo, u, uv=right)])
    e.close()
    return out


@pytest.mark.parametrize("source", ["constant", "bitmap"])
@pytest.mark.parametrize("name", [p[0] for p in REDUCTION_PAIRS])
def test_a_weight_of_zero_or_one_is_one_child(reductions, name, source):
    r = reductions[name]
    for w in (0, 1):
        child, blend = r["child"][w], r[source][w]
        assert child["eval"].any() or name == "copper-diffuse"
        assert np.array_equal(blend["eval"], child["eval"]) and np.array_equal(blend["pdf"], child["pdf"])
        ok = child["weight"].any(1)  # (what a failed sample leaves in wo and pdf is the leaf's own business; the blend clears it)
        assert np.array_equal(blend["weight"].any(1), ok)
        assert np.array_equal(blend["wo"][ok], child["wo"][ok]) and np.array_equal(blend["delta"][ok], child["delta"][ok])
        assert np.array_equal(blend["sampled_pdf"][ok], child["sampled_pdf"][ok])
        worst = int(_ulps(blend["weight"], child["weight"]).max())
        print(name, source, "w =", w, "sampled weight: largest distance", worst, "ulp")
        assert worst <= 4  # ((a p) / p need not round back to a)
        assert child["weight"].any()


# ------------------------------------------------------------------------------------------------ 3. the family changes nothing else
def _render(desc, **props):
    e = hip(**dict(IMPROVED, budgetType="spp", budget=31, maxDepth=-1, rrDepth=5, seed=11, nee="always", **props))
    e.set_scene(desc)
    e.render()
    out = e.read_film(), e.read_sdtree()
    e.close()
    return out


UNUSED_BLEND = dict(type=0, blend=dict(kind="blendbsdf", children=[dict(DIFFUSE), dict(COPPER)], weight=0.3))


def test_a_scene_that_only_holds_a_blended_material_renders_the_same_bits():
    import ppg_host
    path = os.path.join(GOLDEN, "cbox_16x12_pinhole.ppgs")
    fa, ta = _render(ppg_host.load_scene_file(path))
    desc = ppg_host.load_scene_file(path)
    with_slices(desc, [UNUSED_BLEND])  # on no triangle: the blend kernels run, and meet no blend
    fb, tb = _render(desc)
    assert np.isfinite(fa).all() and fa.mean() > 0.01
    assert np.array_equal(fa, fb)
    _tree_equal(ta, tb)


def _smooth_box(blended):
    """the box's 24 triangles on test_bsdfs.SMOOTH's materials; an unused coat sends it through the coat kernels, an unused blend on top
    of that through the blend kernels"""
    import ppg_host
    desc = ppg_host.cbox_scene(16, 12)
    mats = [dict(m) for _, m in SMOOTH]
    base = with_slices(desc, mats + [dict(GOLD, alpha_v=0.1), dict(DIFFUSE, coating=dict(SMOOTH_COAT)), UNUSED_BLEND if blended else DIFFUSE])
    tm = np.array(desc.tri_material)
    box = np.nonzero(tm == 0)[0]
    assert len(box) == 24
    tm[box] = base + np.arange(24) * len(mats) // 24
    desc.tri_material = tm
    return desc


def test_todays_materials_through_the_blend_kernels_equal_the_coat_kernels():
    fa, ta = _render(_smooth_box(False))
    fb, tb = _render(_smooth_box(True))
    assert np.isfinite(fa).all() and fa.mean() > 0.01
    assert np.array_equal(fa, fb)
    _tree_equal(ta, tb)


def test_a_list_without_a_blend_equals_no_list():
    import ppg_host
    from ppg_host.bindings import Blend
    fa, ta = _render(ppg_host.cbox_scene(16, 12))
    desc = ppg_host.cbox_scene(16, 12)
    desc.blends = [Blend() for _ in desc.materials]  # all of kind 0
    fb, tb = _render(desc)
    desc.blends = []
    fc, tc = _render(desc)
    assert np.array_equal(fa, fb) and np.array_equal(fa, fc)
    _tree_equal(ta, tb)
    _tree_equal(ta, tc)


# ------------------------------------------------------------------------------------------------ 4. renders
W, H = 16, 12
RA, RB, WEIGHT = (0.2, 0.5, 0.8), (0.7, 0.6, 0.1), 0.3


def _box(walls, texcoords=False):
    """the Cornell box with every surface of its first ("white") wall material replaced by `walls`"""
    import ppg_host
    desc = ppg_host.cbox_scene(W, H)
    tm = np.array(desc.tri_material)
    white = np.nonzero(tm == 1)[0]
    assert len(white) > 0
    base = with_slices(desc, [walls])
    tm[white] = base
    desc.tri_material = tm
    if texcoords:  # u runs with x across the box
        pos = np.asarray(desc.positions, f32)
        desc.texcoords = np.stack([pos[:, 0] / f32(556.0), pos[:, 2] / f32(559.2)], 1).astype(f32)
    return desc


def _mixed_reflectance():
    w = f32(WEIGHT)
    return tuple(float(v) for v in (np.asarray(RA, f32) * (f32(1) - w) + np.asarray(RB, f32) * w))


DD_BLEND = dict(type=0, blend=dict(kind="blendbsdf", children=[dict(type="diffuse", reflectance=RA), dict(type="diffuse", reflectance=RB)], weight=WEIGHT))
MIXED_WALLS = dict(type=0, twosided=True, blend=dict(kind="mixturebsdf", children=[dict(DIFFUSE), dict(COPPER), dict(GOLD), dict(ROUGHPLASTIC)],
                                                     weights=(0.5, 0.2, 0.2, 0.3)))
_films = {}


def _film(which, nee, seed):
    key = (which, nee, seed)
    if key not in _films:
        walls = dict(blend=DD_BLEND, constant=dict(type="diffuse", reflectance=_mixed_reflectance()), mixed=MIXED_WALLS)[which]
        e = hip(**dict(IMPROVED, budgetType="spp", budget=31, maxDepth=-1, rrDepth=5, seed=seed, nee=nee))
        e.set_scene(_box(walls))
        e.render()
        _films[key] = e.read_film().astype(np.float64)
        e.close()
    return _films[key]


def _blocks(film):
    return film.reshape(H // 4, 4, W // 4, 4, 3).mean((1, 3))


SEEDS = tuple(range(1, 9))


def _spread(nee):
    """seed-to-seed standard deviation of the plain-diffuse render — of its film mean and of its 4 x 4 blocks — over 8 seeds"""
    films = np.stack([_film("constant", nee, s) for s in SEEDS])
    return films.reshape(len(SEEDS), -1, 3).mean(1).std(0, ddof=1), np.stack([_blocks(f) for f in films]).std(0, ddof=1)


@pytest.mark.parametrize("which", ["blend", "mixed"])
@pytest.mark.parametrize("nee", ["always", "never"])
def test_blended_walls_render_finite_films(which, nee):
    f = _film(which, nee, 1)
    assert np.isfinite(f).all() and np.all(f >= 0) and f.mean() > 0.01


def test_bookkeeping_of_a_blended_box():
    """the invariants of test_gpu_parity.test_full_size_invariants on this scene: samples and rays add up, and with the nearest filters
    every committed vertex carries weight 1 into exactly one leaf"""
    for nee in ("always", "never"):
        e = hip(budgetType="spp", budget=60, maxDepth=-1, rrDepth=5, seed=5, nee=nee)
        e.set_scene(_box(MIXED_WALLS)); e.begin_render()
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


def test_the_two_nee_settings_agree_on_blended_walls():
    """the difference of the two renders against 4 standard errors of that difference, the standard error of either render being the
    seed-to-seed spread of the equivalent plain-diffuse render under the same setting (8 seeds)"""
    (ma, ba), (mn, bn) = _spread("always"), _spread("never")
    fa, fn = _film("blend", "always", 1), _film("blend", "never", 1)
    d, se = fa.reshape(-1, 3).mean(0) - fn.reshape(-1, 3).mean(0), np.sqrt(ma * ma + mn * mn)
    print("film mean: difference", d, "standard error of the difference", se)
    assert np.all(np.abs(d) <= 4 * se)
    db, seb = _blocks(fa) - _blocks(fn), np.sqrt(ba * ba + bn * bn)
    print("4x4 blocks: largest difference / standard error", float((np.abs(db) / seb).max()))
    assert np.all(np.abs(db) <= 4 * seb)


LONG_SPP, LAST_SPP = 4092, 2048  # iterations of 1, 2, 4, .. passes of 4 spp and a last one of 2048 spp


def test_the_two_nee_settings_agree_on_walls_with_delta_children():
    """test_coatings_gpu.test_estimators_agree_on_a_coated_box's method on the four-child mixture (diffuse, copper, gold, roughplastic):
    sampleCombination = discard keeps the last iteration alone, an unbiased estimate whose variance ppg_read_variance reports, and the
    two settings must agree in mean radiance per channel within 4 combined standard errors.  (The 31-spp renders above combine their
    iterations by inverse variance, which is biased at that budget — the plain-diffuse box already differs between the settings by more
    than its seed-to-seed spread of the 8-seed mean —, so they only carry the looser comparison the spread of one render allows.)
    This is where the discrete-measure eval / pdf of the children that were not sampled, and the smooth bit, enter a picture: after a
    delta sample NEE is skipped and the emitter counts in full; were the delta flag, its pdf or the bit wrong the settings would differ."""
    from test_coatings_gpu import _last_iteration_spp
    assert _last_iteration_spp(LONG_SPP, 4) == LAST_SPP
    res = {}
    for nee in ("always", "never"):
        e = hip(budgetType="spp", maxDepth=-1, rrDepth=5, seed=3, budget=LONG_SPP, sppPerPass=4, nee=nee, sampleCombination="discard")
        e.set_scene(_box(MIXED_WALLS))
        e.render()
        film, var = e.read_film().astype(np.float64), e.read_variance().astype(np.float64) / LAST_SPP
        e.close()
        assert np.isfinite(film).all() and np.isfinite(var).all() and np.all(var >= 0)
        res[nee] = film.reshape(-1, 3).mean(0), np.sqrt(var.reshape(-1, 3).sum(0)) / (W * H)
    (ma, sa), (mn, sn) = res["always"], res["never"]
    print("mixture walls: mean", ma, mn, "standard error", sa, sn, "relative", sa / ma, sn / mn)
    assert np.all(np.abs(ma - mn) <= 4 * np.sqrt(sa * sa + sn * sn)), (ma - mn) / np.sqrt(sa * sa + sn * sn)


def test_a_scene_file_with_a_bitmap_weight_reaches_the_kernels(tmp_path):
    """load_scene -> set_scene -> the hook: the mesh keeps its texture coordinates, and at a uv in either half of the loaded weight map the
    blend is one child or the other"""
    import ppg_host
    from test_blends import MESH_VT, NEEDS_UVS, _scene, _write_map
    _write_map(tmp_path)
    dark, bright = '<bsdf type="diffuse"> <rgb name="reflectance" value="0.02"/> </bsdf>', '<bsdf type="diffuse"> <rgb name="reflectance" value="0.9"/> </bsdf>'
    body = MESH_VT % NEEDS_UVS["bitmap-weight"].replace('<bsdf type="diffuse"/>', dark).replace('<bsdf type="conductor"> <string name="material" value="none"/> </bsdf>', bright)
    desc, _, info = ppg_host.load_scene(_scene(tmp_path, body))
    assert not info["warnings"] and desc.texcoords is not None and np.isfinite(np.asarray(desc.texcoords)).any()
    i = len(desc.materials) - 3
    assert desc.materials[i]["blend"]["weight_texture"] == 0 and [desc.materials[c]["reflectance"][0] for c in desc.materials[i]["blend"]["children"]] == [
        float(f32(0.02)), float(f32(0.9))]
    e = hip(**dict(CBOX_PROPS, budget=4))
    e.set_scene(desc)
    wi, wo = np.array([[0, 0, 1]] * 2, f32), np.array([[0.3, 0.2, 0.9]] * 2, f32) / f32(np.sqrt(0.94))
    g = e.debug_bsdf(i, wi, wo, np.full((2, 2), 0.5, f32), uv=np.array([[0.25, 0.5], [0.75, 0.5]], f32))
    e.render()
    film = e.read_film()
    e.close()
    want = np.array([0.02, 0.9], f32)[:, None] * (wo[:, 2:3] / f32(np.pi))
    assert np.allclose(g["eval"], np.repeat(want, 3, 1), rtol=1e-5) and np.isfinite(film).all()


@pytest.mark.parametrize("nee", ["always", "never"])
def test_a_blend_of_two_diffuse_agrees_with_the_mixed_diffuse(nee):
    m, b = _spread(nee)
    fb, fc = _film("blend", nee, 1), _film("constant", nee, 9)  # (a seed outside the eight the spread is measured on)
    d, se = fb.reshape(-1, 3).mean(0) - fc.reshape(-1, 3).mean(0), np.sqrt(2.0) * m
    print(nee, "film mean: difference", d, "standard error of the difference", se)
    assert np.all(np.abs(d) <= 4 * se)
    db, seb = _blocks(fb) - _blocks(fc), np.sqrt(2.0) * b
    print(nee, "4x4 blocks: largest difference / standard error", float((np.abs(db) / seb).max()))
    assert np.all(np.abs(db) <= 4 * seb)


def test_a_bitmap_weight_shows_its_two_children_on_the_two_halves():
    """every white surface a blend of a dark and a bright diffuse BSDF by a two-texel weight map over x: one half of the floor shows the
    one, the other half the other, and exchanging the texels exchanges the halves"""
    means = []
    for texels in (((0, 0, 0), (1, 1, 1)), ((1, 1, 1), (0, 0, 0))):
        walls = dict(type=0, blend=dict(kind="blendbsdf", children=[dict(type="diffuse", reflectance=(0.02, 0.02, 0.02)),
                                                                    dict(type="diffuse", reflectance=(0.9, 0.9, 0.9))], weight=0.5, weight_texture=0))
        desc = _box(walls, texcoords=True)
        desc.textures = [two_texels(*texels)]
        e = hip(**dict(IMPROVED, budgetType="spp", budget=31, maxDepth=-1, rrDepth=5, seed=2, nee="always"))
        e.set_scene(desc)
        e.render()
        f = e.read_film().astype(np.float64)
        e.close()
        assert np.isfinite(f).all()
        floor = f[H - 3:]  # the bottom rows see the floor
        means.append((floor[:, :W // 2 - 2].mean(), floor[:, W // 2 + 2:].mean()))
    print("floor, left and right: texels (0 | 1)", means[0], "texels (1 | 0)", means[1])
    (l0, r0), (l1, r1) = means
    assert max(l0, r0) > 2 * min(l0, r0) and max(l1, r1) > 2 * min(l1, r1)
    assert (l0 > r0) != (l1 > r1)


# ------------------------------------------------------------------------------------------------ 5. the refusals
def _n0():
    import ppg_host
    return len(ppg_host.cbox_scene(16, 12).materials)


def _entry(kind=1, child=(1, 2), weight=(0.5,), tex=0, ensure=0, n=None, reserved=0):
    """a ppg_blend with children given relative to the blended material's own index (which the scene builder adds)"""
    from ppg_host.bindings import Blend
    b = Blend()
    b.kind, b.n = kind, len(child) if n is None else n
    for i, c in enumerate(child):
        b.child[i] = c
    for i, w in enumerate(weight):
        b.weight[i] = w
    b.weight_texture, b.ensure_energy_conservation = tex, ensure
    b._reserved[2] = reserved
    return b


def _refusal_scene(mats, entries, relative=True, **attrs):
    """cbox + `mats` (the first is the blended record) with the ppg_blend `entries` on the first len(entries) of them"""
    import ppg_host
    from ppg_host.bindings import Blend
    desc = ppg_host.cbox_scene(16, 12)
    n0 = len(desc.materials)
    desc.materials = list(desc.materials) + [dict(m) for m in mats]
    blends = [Blend() for _ in desc.materials]
    for k, b in enumerate(entries):
        if relative:
            for i in range(min(b.n, 4)):
                b.child[i] += n0 + k
        blends[n0 + k] = b
    desc.blends = blends
    desc.textures = [two_texels((0, 0, 0), (1, 1, 1))]
    for k, v in attrs.items():
        setattr(desc, k, v)
    return desc, n0


BLENDED = dict(type=0)
D = dict(DIFFUSE)


def _sphere_scene():
    desc, n0 = _refusal_scene([BLENDED, D, D], [_entry(tex=1)])
    desc.spheres = [dict(center=(100.0, 100.0, 100.0), radius=20.0, material=n0)]
    return desc, n0


def _aniso_scene():
    desc, n0 = _refusal_scene([BLENDED, D, dict(GOLD, alpha=0.1, alpha_v=0.3)], [_entry()])
    tm = np.array(desc.tri_material)
    tm[0] = n0
    desc.tri_material = tm
    return desc, n0


REFUSALS = [  # (name, scene, index of the material named relative to the first new one, what the message says)
    ("kind", lambda: _refusal_scene([BLENDED, D, D], [_entry(kind=3)]), 0, "kind"),
    ("blend-three-children", lambda: _refusal_scene([BLENDED, D, D, D], [_entry(child=(1, 2, 3))]), 0, "exactly two"),
    ("mixture-no-child", lambda: _refusal_scene([BLENDED, D], [_entry(kind=2, child=(), weight=(1.0,))]), 0, "1 .. 4"),
    ("mixture-five-children", lambda: _refusal_scene([BLENDED, D], [_entry(kind=2, child=(1, 1, 1, 1), weight=(1, 1, 1, 1), n=5)]), 0, "1 .. 4"),
    ("child-out-of-range", lambda: _refusal_scene([BLENDED, D, D], [_entry(child=(1, 3))]), 0, "out of range"),
    ("child-blended", lambda: _refusal_scene([BLENDED, BLENDED, D, D], [_entry(child=(1, 2)), _entry(child=(1, 2))]), 0, "blends of blends"),
    ("child-coated", lambda: _refusal_scene([BLENDED, dict(D, coating=dict(SMOOTH_COAT)), D], [_entry()]), 0, "coated"),
    ("child-masked", lambda: _refusal_scene([BLENDED, dict(D, opacity=(0.5, 0.5, 0.5)), D], [_entry()]), 0, "masked, two-sided or bump-mapped"),
    ("child-twosided", lambda: _refusal_scene([BLENDED, dict(GOLD, twosided=True), D], [_entry()]), 0, "masked, two-sided or bump-mapped"),
    ("child-twosided-diffuse", lambda: _refusal_scene([BLENDED, D, dict(D, twosided=True)], [_entry()]), 0, "masked, two-sided or bump-mapped"),
    ("child-bumpmapped", lambda: _refusal_scene([BLENDED, dict(D, bump=0), D], [_entry()]), 0, "masked, two-sided or bump-mapped"),
    ("child-dielectric", lambda: _refusal_scene([BLENDED, dict(type="dielectric", eta=1.5), D], [_entry()]), 0, "dielectric"),
    ("child-thindielectric", lambda: _refusal_scene([BLENDED, D, dict(type="thindielectric", eta=1.5)], [_entry()]), 0, "dielectric"),
    ("child-roughdielectric", lambda: _refusal_scene([BLENDED, dict(type="roughdielectric", eta=1.5, alpha=0.2), D], [_entry()]), 0, "dielectric"),
    ("coat-on-the-blend", lambda: _refusal_scene([dict(BLENDED, coating=dict(SMOOTH_COAT)), D, D], [_entry()]), 0, "coating(blendbsdf)"),
    ("reflectance-bitmap-on-the-blend", lambda: _refusal_scene([dict(BLENDED, texture=0), D, D], [_entry()]), 0, "reflectance bitmap"),
    ("specular-slot-on-the-blend", lambda: _refusal_scene([dict(BLENDED, specular_texture=0), D, D], [_entry()]), 0, "specular"),
    ("alpha-slot-on-the-blend", lambda: _refusal_scene([dict(BLENDED, alpha_texture=0), D, D], [_entry()]), 0, "alpha"),
    ("microfacet-entry-on-the-blend", lambda: _refusal_scene([dict(BLENDED, alpha_v=0.2), D, D], [_entry()]), 0, "microfacet"),
    ("record-not-diffuse", lambda: _refusal_scene([dict(GOLD), D, D], [_entry()]), 0, "PPG_BSDF_DIFFUSE"),
    ("weight-negative", lambda: _refusal_scene([BLENDED, D, D], [_entry(weight=(-0.25,))]), 0, "not negative"),
    ("weight-nan", lambda: _refusal_scene([BLENDED, D, D], [_entry(weight=(float("nan"),))]), 0, "finite"),
    ("mixture-weight-negative", lambda: _refusal_scene([BLENDED, D, D], [_entry(kind=2, weight=(0.5, -0.5))]), 0, "not negative"),
    ("mixture-weight-inf", lambda: _refusal_scene([BLENDED, D, D], [_entry(kind=2, weight=(0.5, float("inf")))]), 0, "finite"),
    ("mixture-zero-sum", lambda: _refusal_scene([BLENDED, D, D], [_entry(kind=2, weight=(0.0, 0.0))]), 0, "greater than zero"),
    ("texture-out-of-range", lambda: _refusal_scene([BLENDED, D, D], [_entry(tex=3)]), 0, "weight_texture"),
    ("reserved", lambda: _refusal_scene([BLENDED, D, D], [_entry(kind=0, child=(), weight=(), reserved=7)]), 0, "_reserved"),
    ("sphere-with-a-bitmap", _sphere_scene, 0, "sphere"),
    ("anisotropic-child-without-texcoords", _aniso_scene, 0, "texture coordinates"),
]


@pytest.fixture(scope="module")
def engine():
    e = hip(**dict(CBOX_PROPS, budget=4))
    yield e
    e.close()


@pytest.mark.parametrize("k", range(len(REFUSALS)), ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_material_and_leave_the_context_usable(engine, k):
    from ppg_host.bindings import PPGError
    name, build, which, says = REFUSALS[k]
    desc, n0 = build()
    with pytest.raises(PPGError) as err:
        engine.set_scene(desc)
    assert err.value.code == -1  # PPG_ERR_INVALID
    assert "material %d" % (n0 + which) in str(err.value) and says in str(err.value), str(err.value)
    good, n0 = _refusal_scene([BLENDED, D, dict(COPPER)], [_entry(weight=(0.25,))])
    engine.set_scene(good)
    out = engine.debug_bsdf(n0, [0, 0, 1], np.array([[0.3, 0.2, 0.9]], f32), [0.5, 0.5])
    assert out["eval"].any() and np.isfinite(out["eval"]).all()


def test_list_length_and_state(engine):
    from ppg_host.bindings import Blend, PPGError
    desc, n0 = _refusal_scene([BLENDED, D, D], [_entry()])
    n = len(desc.materials)
    for length in (1, n - 1, n + 1):
        desc.blends = [Blend() for _ in range(length)]
        with pytest.raises(PPGError) as err:
            engine.set_scene(desc)
        assert err.value.code == -1 and "%d entries" % length in str(err.value) and "%d materials" % n in str(err.value)
    desc.blends = []  # n_materials = 0 clears the list
    engine.set_scene(desc)
    engine.begin_render()
    with pytest.raises(PPGError) as err:
        engine.set_blends([Blend() for _ in range(n)])
    assert err.value.code == -3  # PPG_ERR_STATE
    engine.end_render()
    desc, _ = _refusal_scene([BLENDED, D, dict(COPPER)], [_entry()])
    engine.set_scene(desc)
    engine.render()
    assert np.isfinite(engine.read_film()).all()
